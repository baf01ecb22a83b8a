// Classifier-free guidance for text (include/unimedvl_hip.h, "classifier-free guidance for text"): a guided row c of a decode step is
// contrasted with its unconditional row u = pair[c], l' = g (log_softmax l_c - log_softmax l_u) + log_softmax l_u, and replaces l_c in
// memory.  umv_logit_guidance_bf16 sits first behind the lm_head GEMM: it finds the two rows' log-sum-exp from the tile statistics the
// epilogue left (or from tile pairs of its own when that call sampled at a temperature), rewrites the conditional row and then EVERY
// tile's argmax key and softmax statistics to what the epilogue would have left for l' (penalty_tile.h), so that whatever follows
// reads the guided distribution.  umv_guidance_feed, behind the step end, hands the token picked for c to u: both rows are fed it next.
#include "block_reduce.h"
#include "penalty_tile.h"

#define LG_THREADS 256
#define LG_CHUNK UMV_CONSTRAIN_CHUNK      // columns per workgroup: one 16-column tile per thread
static_assert(LG_CHUNK == LG_THREADS * 16, "one tile per thread");

typedef u32x4 __attribute__((may_alias)) lg_u32x4;      // 8 bf16 of a row as one 16-byte access

// The unconditional row of row c under the header's rules, -1 where c is not a guided row: u in [0, M) and not c, u not itself
// pointing at another row, no lower row claiming u.  SCALE: also a usable scale that is not exactly 1 (the stage; the feed pairs
// rows whatever their scale).  The words are uniform over a workgroup wherever this is called with a uniform c.
template <bool SCALE>
__device__ __forceinline__ int lg_partner(const int32_t* __restrict__ pair, const float* __restrict__ scale, int M, int c) {
    const int u = pair[c];
    if (u < 0 || u >= M || u == c) return -1;
    if (SCALE) {
        const float g = scale[c];
        if (!(g >= 0.f) || !(g - g == 0.f) || g == 1.f) return -1;
    }
    const int pu = pair[u];
    if (pu >= 0 && pu < M && pu != u) return -1;
    for (int o = 0; o < c; ++o)
        if (pair[o] == u) return -1;
    return u;
}

// does row r take part - as an active row, or as the unconditional row of one?  Every thread of the workgroup calls it (a barrier).
__device__ __forceinline__ bool lg_takes_part(const int32_t* __restrict__ pair, const float* __restrict__ scale, int M, int r) {
    if (lg_partner<true>(pair, scale, M, r) >= 0) return true;      // (uniform)
    int mine = 0;
    for (int c = threadIdx.x; c < M; c += LG_THREADS)
        if (pair[c] == r && lg_partner<true>(pair, scale, M, c) == r) mine = 1;
    return __syncthreads_or(mine) != 0;
}

// grid (column chunk, row): the temperature-0 tile pairs of the rows that take part, in the epilogue's order (penalty_tile at T = 0)
__global__ __launch_bounds__(LG_THREADS) void guidance_stats_kernel(umv_logit_guidance_args a) {
    const int r = blockIdx.y;
    if (!lg_takes_part(a.pair, a.scale, a.M, r)) return;      // (uniform)
    const int n0 = blockIdx.x * LG_CHUNK + threadIdx.x * 16;
    if (n0 >= a.V) return;
    const int tile = n0 >> 4;
    uint64_t key;
    penalty_tile(a.logits + (int64_t)r * a.ld, a.V, tile, 0.f, 0ull, &key, a.stats + ((int64_t)r * a.n_tiles + tile) * 2);
}

// one workgroup per row: lse[r] = M_r + logf(S_r), row_max[r] = M_r from the row's tile pairs, merged as the step ends merge them
__global__ __launch_bounds__(LG_THREADS) void guidance_merge_kernel(umv_logit_guidance_args a, const float* __restrict__ pairs) {
    __shared__ float smf[LG_THREADS / 64];
    const int r = blockIdx.x;
    if (!lg_takes_part(a.pair, a.scale, a.M, r)) return;      // (uniform)
    const umv_f32x2* st = reinterpret_cast<const umv_f32x2*>(pairs) + (int64_t)r * a.n_tiles;
    float ref, S;
    merge_tile_stats<LG_THREADS>(st, a.n_tiles, smf, ref, S);
    float mx = -INFINITY;                                      // the maximum itself (ref is 0 for a row of -inf only); exact in any order
    for (int c = threadIdx.x; c < a.n_tiles; c += LG_THREADS) mx = fmaxf(mx, st[c].x);
    mx = block_reduce_max(mx, smf);
    if (threadIdx.x == 0) {
        a.lse[r] = __fadd_rn(mx, logf(S));
        a.row_max[r] = mx;
    }
}

// one column of the guided row (the header's "column"): everything in fp32, one rounding per operation
__device__ __forceinline__ bf16_t lg_column(bf16_t bc, bf16_t bu, float lse_c, float lse_u, float g, float floor_c) {
    const float lc = bf2f(bc), lu = bf2f(bu);
    if (lc == -INFINITY || lc < floor_c) return (bf16_t)0xFF80;
    const float cc = __fsub_rn(lc, lse_c);
    if (lu == -INFINITY) return f2bf(cc);
    const float uu = __fsub_rn(lu, lse_u);
    const float d = __fsub_rn(cc, uu);
    return f2bf(__fadd_rn(__fmul_rn(g, d), uu));
}

// grid (column chunk, row): the combine and the tiles
__global__ __launch_bounds__(LG_THREADS) void guidance_combine_kernel(umv_logit_guidance_args a) {
    const int c = blockIdx.y;
    const int u = lg_partner<true>(a.pair, a.scale, a.M, c);
    if (u < 0) return;                                         // not an active row: nothing of it is written (uniform, no barrier here)
    const float mc = a.row_max[c];
    if (mc == -INFINITY) return;                               // a row of -inf (and NaN) only is left as it is
    const int n0 = blockIdx.x * LG_CHUNK + threadIdx.x * 16;
    if (n0 >= a.V) return;
    const int nend = min(a.V, n0 + 16), tile = n0 >> 4;
    const float lse_c = a.lse[c], lse_u = a.lse[u], g = a.scale[c];
    const float floor_c = __fadd_rn(mc, a.log_beta[c]);
    bf16_t* row = a.logits + (int64_t)c * a.ld;
    const bf16_t* urow = a.logits + (int64_t)u * a.ld;
    const bool wide = nend - n0 == 16 && (((reinterpret_cast<uintptr_t>(row + n0) | reinterpret_cast<uintptr_t>(urow + n0)) & 15) == 0);
    if (wide) {
        lg_u32x4 vc[2] = {reinterpret_cast<const lg_u32x4*>(row + n0)[0], reinterpret_cast<const lg_u32x4*>(row + n0)[1]};
        const lg_u32x4 vu[2] = {reinterpret_cast<const lg_u32x4*>(urow + n0)[0], reinterpret_cast<const lg_u32x4*>(urow + n0)[1]};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t lo = lg_column((bf16_t)(vc[h][w] & 0xFFFFu), (bf16_t)(vu[h][w] & 0xFFFFu), lse_c, lse_u, g, floor_c);
                const uint32_t hi = lg_column((bf16_t)(vc[h][w] >> 16), (bf16_t)(vu[h][w] >> 16), lse_c, lse_u, g, floor_c);
                vc[h][w] = lo | (hi << 16);
            }
        reinterpret_cast<lg_u32x4*>(row + n0)[0] = vc[0];
        reinterpret_cast<lg_u32x4*>(row + n0)[1] = vc[1];
    } else {
        for (int n = n0; n < nend; ++n) row[n] = lg_column(row[n], urow[n], lse_c, lse_u, g, floor_c);
    }
    if (!a.argmax_partial) return;
    // the tile as this thread just stored it (its own stores, read back in program order), through the shared recomputation
    const int64_t t = (int64_t)c * a.n_tiles + tile;
    const uint64_t row_key = !(a.temperature > 0.f) ? 0ull : sample_row_key(a.seed, a.step, c);
    uint64_t key;
    penalty_tile(row, a.V, tile, a.temperature, row_key, &key, a.lse_partial ? a.lse_partial + t * 2 : nullptr);
    a.argmax_partial[t] = key;
}

// one thread per row
__global__ __launch_bounds__(UMV_WAVE) void guidance_feed_kernel(const int32_t* __restrict__ pair, int64_t* ids, int64_t* in_ids,
                                                                 int64_t* pred_ids, const int64_t* __restrict__ step_idx, int M,
                                                                 int max_len) {
    const int c = blockIdx.x * UMV_WAVE + threadIdx.x;
    if (c >= M) return;
    const int u = lg_partner<false>(pair, nullptr, M, c);
    if (u < 0) return;
    ids[u] = ids[c];
    const int64_t s = step_idx[c] - 1;
    if (s >= 0 && s < max_len) pred_ids[s * M + u] = pred_ids[s * M + c];
    if (s + 1 >= 0 && s + 1 < max_len) in_ids[(s + 1) * M + u] = in_ids[(s + 1) * M + c];
}

static bool lg_finite(float v) { return v - v == 0.f; }      // false for NaN and +-inf

extern "C" int umv_logit_guidance_bf16(const umv_logit_guidance_args* a, umv_stream_t stream) {
    UMV_CHECK(a && a->logits && a->M >= 0 && a->V > 0 && a->ld >= a->V, UMV_ERR_ARG, "logit_guidance: bad args");
    UMV_CHECK(a->pair && a->scale && a->log_beta && a->lse && a->row_max, UMV_ERR_ARG,
              "logit_guidance: pair, scale, log_beta, lse and row_max are one word per row, none may be NULL");
    UMV_CHECK(lg_finite(a->temperature) && a->temperature >= 0.f, UMV_ERR_ARG, "logit_guidance: temperature (%g) must be >= 0 (0 = greedy)",
              (double)a->temperature);
    UMV_CHECK(a->argmax_partial || !a->lse_partial, UMV_ERR_ARG, "logit_guidance: lse_partial goes with argmax_partial");
    UMV_CHECK(a->n_tiles > 0 && a->V <= (int64_t)a->n_tiles * 16 && a->V > ((int64_t)a->n_tiles - 1) * 16, UMV_ERR_ARG,
              "logit_guidance: V (%d) must be the column count behind the %d tiles", a->V, a->n_tiles);
    // the lm_head call's own statistics are the temperature-0 tile pairs where y = l: greedy, and T = 1 (bf16(l / 1) = l)
    const bool reuse = a->lse_partial && (a->temperature == 0.f || a->temperature == 1.f);
    UMV_CHECK(reuse || a->stats, UMV_ERR_ARG,
              "logit_guidance: without lse_partial at temperature 0 or 1 the call needs stats [M][n_tiles][2] for the tile pairs");
    UMV_CHECK(a->M <= 65535, UMV_ERR_ARG, "logit_guidance: at most 65535 rows per call (got %d)", a->M);
    if (a->M == 0) return UMV_OK;
    const dim3 grid((a->V + LG_CHUNK - 1) / LG_CHUNK, a->M);
    if (!reuse) {
        hipLaunchKernelGGL(guidance_stats_kernel, grid, dim3(LG_THREADS), 0, (hipStream_t)stream, *a);
        UMV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(guidance_merge_kernel, dim3(a->M), dim3(LG_THREADS), 0, (hipStream_t)stream, *a,
                       reuse ? (const float*)a->lse_partial : (const float*)a->stats);
    UMV_LAUNCH_CHECK();
    hipLaunchKernelGGL(guidance_combine_kernel, grid, dim3(LG_THREADS), 0, (hipStream_t)stream, *a);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_guidance_feed(const int32_t* pair, int64_t* ids, int64_t* in_ids, int64_t* pred_ids, const int64_t* step_idx, int M,
                                 int max_len, umv_stream_t stream) {
    UMV_CHECK(pair && ids && in_ids && pred_ids && step_idx && M >= 0 && max_len >= 0, UMV_ERR_ARG,
              "guidance_feed: pair, ids, in_ids, pred_ids and step_idx are needed, M >= 0 and max_len >= 0");
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(guidance_feed_kernel, dim3((M + UMV_WAVE - 1) / UMV_WAVE), dim3(UMV_WAVE), 0, (hipStream_t)stream, pair, ids, in_ids,
                       pred_ids, step_idx, M, max_len);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
