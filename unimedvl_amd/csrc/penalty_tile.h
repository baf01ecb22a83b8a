// One 16-column tile of a row of stored logits, recomputed by ONE thread with the bits the lm_head epilogue leaves for it: what the
// kernels that rewrite stored logits between the lm_head call and the step end share (logit_penalty.hip, logit_ngram.hip,
// logit_constrain.hip).
#pragma once
#include "gemm_epilogue.h"

// One 16-column tile of a row, recomputed by ONE thread the way the epilogue's four lane groups do it (gemm_skinny.h: lane group g of a
// row holds columns 4g .. 4g + 3 of the tile): epi_argmax_tile's key maximum - exact, so its order is free - and epi_lse_tile's
// statistics in its order: per group the maximum from -inf and the sum from 0 over the four columns, then groups (g, g ^ 1), then
// (.., g ^ 2), the operands as lane group 0 - the one that stores - sees them.
__device__ __forceinline__ void penalty_tile(const bf16_t* row, int V, int tile, float temp, uint64_t row_key, uint64_t* key_out,
                                             float* lse_out) {
    const int n0 = tile * 16, nend = min(V, n0 + 16);
    float l[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) l[j] = n0 + j < nend ? bf2f(row[n0 + j]) : -INFINITY;
    uint64_t key = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (n0 + j < nend) {
            const float v = temp > 0.f ? epi_gumbel_value(l[j], temp, row_key, n0 + j) : l[j];
            const uint64_t kj = argmax_key(v, n0 + j);
            key = kj > key ? kj : key;
        }
    *key_out = key;
    if (!lse_out) return;
    float y[16], mg[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        mg[g] = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[4 * g + j] = n0 + 4 * g + j < nend ? pick_value(l[4 * g + j], temp) : -INFINITY;
            mg[g] = fmaxf(mg[g], y[4 * g + j]);
        }
    }
    const float mx = fmaxf(fmaxf(mg[0], mg[1]), fmaxf(mg[2], mg[3]));
    const float ref = (mx == -INFINITY) ? 0.f : mx;
    float sg[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        sg[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) sg[g] += __expf(y[4 * g + j] - ref);
    }
    *reinterpret_cast<umv_f32x2*>(lse_out) = (umv_f32x2){mx, (sg[0] + sg[1]) + (sg[2] + sg[3])};
}
