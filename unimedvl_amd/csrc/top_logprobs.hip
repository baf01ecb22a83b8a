// Top-n alternative tokens with their log-probabilities, and the rank of the fed token (include/unimedvl_hip.h, "top-n alternative
// tokens and token ranks"): one workgroup per row, after the step end of a decode step or stand-alone over a logits matrix.
// The selection is the top-k cutoff of truncated sampling (truncation.h) with k = n: it names the class - the columns that share one
// y - that holds the n-th largest value.  One more sweep over the row then gathers the fewer than n columns above that class, the
// lowest columns of the class itself, and counts the columns in front of the fed token.  Everything that decides an id or a rank is
// an integer comparison of class keys and columns; the log-probabilities take (ref, S) merged in the order of the step end that ran.
#include "top_select.h"

// After the step end of a decode step: sample b's step s = step_idx[b] - 1, its fed token ids[b].
__global__ __launch_bounds__(TR_THREADS) void decode_top_logprobs_kernel(const bf16_t* __restrict__ logits, int64_t ldo, int V,
                                                                         const float* __restrict__ lse, int n_tiles, float temperature,
                                                                         const umv_row_sampling* __restrict__ rows, int merge_order,
                                                                         const int64_t* __restrict__ ids, const int64_t* __restrict__ step_idx,
                                                                         const int64_t* __restrict__ forced, int B, int max_len, int n,
                                                                         int32_t* top_ids, float* top_logprobs, int32_t* rank) {
    __shared__ uint32_t hist[TR_BINS];
    __shared__ TruncShared sh;
    __shared__ TopShared ts;
    const int b = blockIdx.x;
    const int64_t s = step_idx[b] - 1;
    if (s < 0 || s >= max_len) return;               // the same in every thread
    const bf16_t* row = logits + (int64_t)b * ldo;
    float temp = temperature;
    bool truncated = merge_order == UMV_TOP_AFTER_TRUNCATED;
    if (rows) {
        temp = row_sampling_temp(rows, b);
        truncated = temp > 0.f && (rows[b].top_k > 0 || rows[b].top_p < 1.f || rows[b].min_p > 0.f);
    }
    const umv_f32x2* st = reinterpret_cast<const umv_f32x2*>(lse) + (int64_t)b * n_tiles;
    float ref, S;
    if (truncated) merge_tile_stats<TR_THREADS>(st, n_tiles, sh.smf, ref, S);
    else merge_tile_stats<TR_THREADS, 256>(st, n_tiles, sh.smf, ref, S);
    const int64_t f = forced ? forced[s * B + b] : -1;
    const int64_t fed = f < V ? ids[b] : -1;         // a forced token outside the vocabulary was never fed: rank 0
    const int64_t at = s * B + b;
    // greedy: y is the logit, so the maximum of the statistics is the row's highest logit (ref == 0 may stand for a row of -inf only)
    const float max_logit = (temp > 0.f || ref == 0.f) ? NAN : ref;
    top_select(row, V, temp, n, fed, ref, S, max_logit, hist, sh, ts, {top_ids + at * n, top_logprobs + at * n, rank + at});
}

// Stand-alone: the statistics of token_logprob_kernel - 1024 threads there, so every thread here sums for two of them, the wave
// trees run per virtual wave and the 16 partials add in that kernel's order: its bits.
__global__ __launch_bounds__(TR_THREADS) void top_logprobs_kernel(const bf16_t* __restrict__ logits, int64_t ld,
                                                                  const int64_t* __restrict__ ids, int V, float temp, int n, int32_t* top_ids,
                                                                  float* top_logprobs, int32_t* rank) {
    __shared__ uint32_t hist[TR_BINS];
    __shared__ TruncShared sh;
    __shared__ TopShared ts;
    const int m = blockIdx.x, t = threadIdx.x;
    const bf16_t* row = logits + (int64_t)m * ld;
    float M = -INFINITY;
    for (int i = t; i < V; i += TR_THREADS) M = fmaxf(M, pick_value(bf2f(row[i]), temp));
    M = block_reduce_max(M, sh.smf);
    const float ref = softmax_ref(M);
    float s0 = 0.f, s1 = 0.f;
    for (int i = t; i < V; i += 2 * TR_THREADS) s0 += expf(pick_value(bf2f(row[i]), temp) - ref);
    for (int i = t + TR_THREADS; i < V; i += 2 * TR_THREADS) s1 += expf(pick_value(bf2f(row[i]), temp) - ref);
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if ((t & 63) == 0) { ts.wsum[t >> 6] = s0; ts.wsum[TR_THREADS / 64 + (t >> 6)] = s1; }
    __syncthreads();
    float S = 0.f;
    for (int i = 0; i < 2 * TR_THREADS / 64; ++i) S += ts.wsum[i];
    top_select(row, V, temp, n, ids[m], ref, S, temp > 0.f ? NAN : M, hist, sh, ts,
               {top_ids + (int64_t)m * n, top_logprobs + (int64_t)m * n, rank + m});
}

static int top_n_ok(const char* who, int n, int V, float temperature, const void* top_ids, const void* top_logprobs, const void* rank) {
    UMV_CHECK(V > 0 && n >= 1 && n <= UMV_TOP_LOGPROBS_MAX && n <= V, UMV_ERR_ARG, "%s: n (%d) must be in [1, %d] and at most V (%d)", who, n,
              UMV_TOP_LOGPROBS_MAX, V);
    UMV_CHECK(top_ids && top_logprobs && rank, UMV_ERR_ARG, "%s: top_ids, top_logprobs and rank must all be set", who);
    UMV_CHECK(temperature >= 0.f, UMV_ERR_ARG, "%s: temperature (%g) must be >= 0 (0 = greedy)", who, (double)temperature);
    return UMV_OK;
}

extern "C" int umv_decode_top_logprobs(const uint16_t* logits, int64_t ldo, int V, const float* lse_partial, int n_tiles, float temperature,
                                       const umv_row_sampling* rows, int merge_order, const int64_t* ids, const int64_t* step_idx,
                                       const int64_t* forced_ids, int B, int max_len, int n, int32_t* top_ids, float* top_logprobs,
                                       int32_t* rank, umv_stream_t stream) {
    if (int rc = top_n_ok("decode_top_logprobs", n, V, temperature, top_ids, top_logprobs, rank)) return rc;
    UMV_CHECK(logits && lse_partial && ids && step_idx && B >= 0 && max_len > 0, UMV_ERR_ARG, "decode_top_logprobs: bad args");
    UMV_CHECK(n_tiles > 0 && V <= n_tiles * 16 && V > (n_tiles - 1) * 16 && ldo >= V, UMV_ERR_ARG,
              "decode_top_logprobs: V (%d) must be the column count behind the %d tiles and ldo (%lld) >= V", V, n_tiles, (long long)ldo);
    UMV_CHECK(merge_order == UMV_TOP_AFTER_LOGPROB || merge_order == UMV_TOP_AFTER_TRUNCATED, UMV_ERR_ARG,
              "decode_top_logprobs: merge_order (%d) names no step end", merge_order);
    UMV_CHECK(((uintptr_t)rows % 16) == 0, UMV_ERR_ARG, "decode_top_logprobs: rows (the per-row sampling table) must be 16-byte aligned");
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_top_logprobs_kernel, dim3(B), dim3(TR_THREADS), 0, (hipStream_t)stream, logits, ldo, V, lse_partial, n_tiles,
                       temperature, rows, merge_order, ids, step_idx, forced_ids, B, max_len, n, top_ids, top_logprobs, rank);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_top_logprobs_bf16(const uint16_t* logits, int64_t ld, const int64_t* ids, int M, int V, float temperature, int n,
                                     int32_t* top_ids, float* top_logprobs, int32_t* rank, umv_stream_t stream) {
    if (int rc = top_n_ok("top_logprobs", n, V, temperature, top_ids, top_logprobs, rank)) return rc;
    UMV_CHECK(logits && ids && M >= 0 && ld >= V, UMV_ERR_ARG, "top_logprobs: bad args");
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(top_logprobs_kernel, dim3(M), dim3(TR_THREADS), 0, (hipStream_t)stream, logits, ld, ids, V, temperature, n, top_ids,
                       top_logprobs, rank);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
