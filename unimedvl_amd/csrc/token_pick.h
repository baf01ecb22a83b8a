// What the two ways of picking the next token share - the stand-alone kernels of token_pick.hip and the lm_head GEMM's epilogue
// (gemm_epilogue.h::epi_argmax_tile): the 64-bit argmax key and the counter-based random stream of the sampler.  One copy, so
// that the key the epilogue writes is the key umv_decode_step_end_argmax reads, and a (seed, step, row, column) names the same
// uniform draw on both paths.
#pragma once
#include "common.h"

// Greedy argmax as a maximum of 64-bit keys (bagel.py:1295-1301: argmax over the bf16 logits):
// (order-preserving image of the logit) << 32 | (0xFFFFFFFF - column) - so that the maximum key is the largest logit and,
// among equal logits, the LOWEST column (torch.argmax's tie rule; NaN ranks highest like torch).
__device__ __forceinline__ uint64_t argmax_key(float v, int n) {
    uint32_t b = __float_as_uint(v == 0.f ? 0.f : v);            // -0 == +0
    uint32_t k = (v != v) ? 0xFFFFFFFFu : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
    return ((uint64_t)k << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)n);
}
__device__ __forceinline__ int64_t argmax_key_column(uint64_t key) { return (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = (uint32_t)__shfl_xor((int)lo, mask, 64);
    hi = (uint32_t)__shfl_xor((int)hi, mask, 64);
    return ((uint64_t)hi << 32) | lo;
}

// The value the token pick orders, without noise, and the y of the token log-probability (include/unimedvl_hip.h): the bf16 logit
// itself in greedy decoding (temp == 0), bf16(logit / T) when sampling - logits / temperature is a bf16 tensor in the reference
// (bagel.py:1297-1299).
__device__ __forceinline__ float pick_value(float logit, float temp) { return temp > 0.f ? rbf(logit / temp) : logit; }

// logprob = y[id] - logsumexp y from the merged statistics: M = max y (exact), S = sum exp(y - M).  (y - M) first: both are bf16
// values, so the difference is exact or nearly so and the one rounding that matters is log's.
__device__ __forceinline__ float logprob_finish(float y_id, float M, float S) { return (y_id - M) - logf(S); }

// The sampler's stream: splitmix64 of (seed, step, row) gives the row key, splitmix64 of (row key + column) the draw - reproducible
// for a given seed, NOT torch's CPU / CUDA stream.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// The three words of a row key: the scalar entries pass (seed, *step, row index), the per-row table (include/unimedvl_hip.h,
// umv_row_sampling) a row's own (seed, draw, stream) - the same function, so equal words name the same draws on either path.
__device__ __forceinline__ uint64_t sample_row_key_of(uint64_t seed, uint64_t step, uint64_t stream) {
    return splitmix64(seed ^ (step * 0xD1B54A32D192ED03ull) ^ (stream << 32));
}
__device__ __forceinline__ uint64_t sample_row_key(uint64_t seed, const int64_t* step_ptr, int m) {
    return sample_row_key_of(seed, step_ptr ? (uint64_t)step_ptr[0] : 0ull, (uint64_t)m);
}
// u = (r + 0.5) 2^-23 with r the top 23 bits of the hash: in [2^-24, 1 - 2^-24], strictly inside (0, 1), and exact in fp32
// (r + 0.5 needs 24 bits), so -ln(u) is a finite, positive Exp(1) draw and a column can only win through its logit - with u = 1
// allowed (round 5) a column won with probability 2^-24 whatever its logit: ~1 % of the draws over a 152 k vocabulary.
__device__ __forceinline__ float sample_uniform(uint64_t row_key, int n) {
    const uint64_t h = splitmix64(row_key + (uint64_t)n);
    return ((float)(h >> 41) + 0.5f) * (1.0f / 8388608.0f);
}

// Truncated sampling (include/unimedvl_hip.h, "truncated sampling"): a class is the set of columns that share one y = pick_value, a
// bf16 value, so at most 65 536 of them.  class_key is the 16-bit order-preserving image of a bf16 value (a logit, or y) -
// argmax_key's, on the upper half of the fp32 word: -0 == +0, every NaN is 0xFFFF, the highest - and class_value its inverse.
__device__ __forceinline__ uint32_t class_key(float y) {
    if (y != y) return 0xFFFFu;
    const uint32_t b = __float_as_uint(y == 0.f ? 0.f : y) >> 16;
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}
__device__ __forceinline__ float class_value(uint32_t key) {
    return __uint_as_float(((key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xFFFFu)) << 16);
}
