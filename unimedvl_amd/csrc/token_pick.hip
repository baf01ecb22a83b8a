// Next-token picking and the bookkeeping that ends a decode step: argmax and temperature sampling over bf16 logits, the
// step-end kernels (three of them finish the lm_head GEMM's argmax epilogue: plain, with the token's log-probability, and with
// top-k / top-p / min-p), the stand-alone token log-probability, the stand-alone truncated sampler and the step end of a speculative
// greedy step (verify the drafts, commit, roll back, draft again) and the two launches that end a sampled speculative step.
#include "block_reduce.h"
#include "token_pick.h"
#include "truncation.h"
#include <type_traits>
#include "../../include/unimedvl_hip.h"

// ----------------------------------------------------------------------------- argmax (bf16 logits, lowest index wins)
__global__ __launch_bounds__(1024) void argmax_kernel(const bf16_t* __restrict__ logits, int64_t ld, int64_t* __restrict__ out, int V) {
    __shared__ float smax[16];
    __shared__ int sidx[16];
    const int m = blockIdx.x;
    const bf16_t* row = logits + (int64_t)m * ld;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    const int nv = V / 8;
    // one workgroup per row is latency bound (19 dependent round trips for V = 152064): request 8 chunks per thread at a
    // time, then compare in index order (same result as the one-at-a-time loop)
    constexpr int UA = 8;
    for (int c0 = threadIdx.x; c0 < nv; c0 += blockDim.x * UA) {
        bf16x8 v[UA];
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int c = c0 + u * blockDim.x;
            v[u] = c < nv ? ldg_frag(row + c * 8) : zero_frag();
        }
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int c = c0 + u * blockDim.x;
            if (c < nv) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float f = bf2f((bf16_t)v[u][j]);
                    int i = c * 8 + j;
                    if (f > best || (f == best && i < bidx) || (f != f && !(best != best))) { best = f; bidx = i; }
                }
            }
        }
    }
    for (int i = nv * 8 + threadIdx.x; i < V; i += blockDim.x) {
        float f = bf2f(row[i]);
        if (f > best || (f == best && i < bidx)) { best = f; bidx = i; }
    }
    if (block_best_lowest(best, bidx, smax, sidx)) out[m] = bidx;
}

extern "C" int umv_argmax_bf16(const uint16_t* logits, int64_t ld, int64_t* out_ids, int M, int V, umv_stream_t stream) {
    UMV_CHECK(logits && out_ids && V > 0 && (ld % 8) == 0, UMV_ERR_ARG, "argmax: bad args");
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(argmax_kernel, dim3(M), dim3(1024), 0, (hipStream_t)stream, logits, ld, out_ids, V);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- temperature sampling
// bagel.py:1297-1299: probs = softmax(logits / temperature) ; token = multinomial(probs, 1).
// torch draws one sample without replacement as argmax(probs / q), q ~ Exp(1) per element; this kernel
// does the same with the counter-based generator of token_pick.h (the stream the lm_head epilogue's Gumbel-max
// draws from too).  Rounding follows the bf16 tensors of the reference: logits/T -> bf16.
__global__ __launch_bounds__(1024) void sample_kernel(const bf16_t* __restrict__ logits, int64_t ld, int64_t* __restrict__ out, int V,
                                                      float temp, uint64_t seed, const int64_t* __restrict__ step_ptr) {
    __shared__ float smf[16];
    __shared__ int smi[16];
    const int m = blockIdx.x;
    const bf16_t* row = logits + (int64_t)m * ld;
    const uint64_t key = sample_row_key(seed, step_ptr, m);
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < V; i += blockDim.x) mx = fmaxf(mx, rbf(bf2f(row[i]) / temp));
    mx = block_reduce_max(mx, smf);
    float sum = 0.f;
    for (int i = threadIdx.x; i < V; i += blockDim.x) sum += expf(rbf(bf2f(row[i]) / temp) - mx);
    sum = block_reduce_sum(sum, smf);
    float best = -1.f;
    int bidx = 0x7fffffff;
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        const float p = expf(rbf(bf2f(row[i]) / temp) - mx) / sum;   // fp32 probabilities, as autocast's softmax returns them
        const float q = fmaxf(-logf(sample_uniform(key, i)), 5.9604645e-8f);   // Exp(1), q >= 5.9e-8 > 0: a token wins through p / q only
        const float sc = p / q;
        if (sc > best || (sc == best && i < bidx)) { best = sc; bidx = i; }
    }
    __syncthreads();                 // everyone has read the sum out of smf
    if (block_best_lowest(best, bidx, smf, smi)) out[m] = bidx;
}

extern "C" int umv_sample_bf16(const uint16_t* logits, int64_t ld, int64_t* out_ids, int M, int V, float temperature, uint64_t seed,
                               const int64_t* step, umv_stream_t stream) {
    UMV_CHECK(logits && out_ids && V > 0, UMV_ERR_ARG, "sample: bad args");
    UMV_CHECK(temperature > 0.f, UMV_ERR_ARG, "sample: temperature must be > 0 (got %g)", (double)temperature);
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(sample_kernel, dim3(M), dim3(1024), 0, (hipStream_t)stream, logits, ld, out_ids, V, temperature, seed, step);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- end of a decode step
__global__ void decode_advance_kernel(int32_t* slot, int32_t* pos, int32_t* kv_len, int B) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { slot[b] += 1; pos[b] += 1; kv_len[b] += 1; }
}
extern "C" int umv_decode_advance(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, int B, umv_stream_t stream) {
    UMV_CHECK(tok_slot && tok_pos && kv_len, UMV_ERR_ARG, "decode_advance: null pointer");
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_advance_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, tok_slot, tok_pos, kv_len, B);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// Sample b at the end of step s: log the token just predicted (pred_ids[s] = id; in_ids[s + 1] = next, the token the next step is
// fed - bagel.py:1263,1311-1312; next = id unless the token is forced) and bump slot / position / kv_len.
__device__ __forceinline__ void step_end_sample(int32_t* slot, int32_t* pos, int32_t* kv_len, int64_t* in_ids, int64_t* pred_ids, int b,
                                                int64_t id, int64_t next, int64_t s, int B, int max_len) {
    if (s < max_len) pred_ids[s * B + b] = id;
    if (s + 1 < max_len) in_ids[(s + 1) * B + b] = next;
    slot[b] += 1; pos[b] += 1; kv_len[b] += 1;
}

// End of a decode step in ONE launch: step_end_sample for every sample, then the step counter s.
__global__ __launch_bounds__(256) void decode_step_end_kernel(int32_t* slot, int32_t* pos, int32_t* kv_len, const int64_t* ids,
                                                              int64_t* in_ids, int64_t* pred_ids, int64_t* step_idx, int B, int max_len) {
    const int64_t s = step_idx[0];
    for (int b = threadIdx.x; b < B; b += blockDim.x) step_end_sample(slot, pos, kv_len, in_ids, pred_ids, b, ids[b], ids[b], s, B, max_len);
    __syncthreads();                 // everyone has read s
    if (threadIdx.x == 0) step_idx[0] = s + 1;
}
extern "C" int umv_decode_step_end(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const int64_t* ids, int64_t* in_ids,
                                   int64_t* pred_ids, int64_t* step_idx, int B, int max_len, umv_stream_t stream) {
    UMV_CHECK(tok_slot && tok_pos && kv_len && ids && in_ids && pred_ids && step_idx && max_len > 0, UMV_ERR_ARG, "decode_step_end: bad args");
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tok_slot, tok_pos, kv_len, ids, in_ids, pred_ids,
                       step_idx, B, max_len);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- the fused step ends
// One workgroup per sample finishes what the lm_head GEMM epilogue left per 16-column tile - the argmax keys (token_pick.h::argmax_key)
// and, for log-probabilities, the softmax statistics (gemm_epilogue.h::epi_lse_tile) - then does decode_step_end_kernel's bookkeeping
// for its sample.  The step counter is PER SAMPLE - step_idx[b], all equal, read at the top of each kernel - so that no workgroup
// reads a word another workgroup of the same launch writes (rounds 2-3 shared step_idx[0] behind a relaxed ticket; correct on this
// hardware, not by the memory model).  The pieces take the workgroup's thread count T as a template parameter.
struct StepEnd {                 // what every fused step end reads and writes
    int32_t *slot, *pos, *kv_len;
    int64_t *ids, *in_ids, *pred_ids, *step_idx;
    int B, max_len;
};

// A thread's share of the maximum of a sample's n_tiles keys.
template <int T>
__device__ __forceinline__ uint64_t strided_max_key(const uint64_t* __restrict__ row, int n_tiles) {
    uint64_t best = 0;
    constexpr int UA = 8;      // all loads of a thread in flight together: one round trip for up to 8 T tiles per pass
    for (int c0 = threadIdx.x; c0 < n_tiles; c0 += T * UA) {
        uint64_t v[UA];
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int c = c0 + u * T;
            v[u] = c < n_tiles ? row[c] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < UA; ++u) best = v[u] > best ? v[u] : best;
    }
    return best;
}

// (the merge of a sample's per-tile softmax statistics: block_reduce.h::merge_tile_stats, shared with top_logprobs.hip)

// Thread 0's tail for sample b at step s, id the pick.  The token the next step is fed is the forced one where there is one inside
// the vocabulary (a forced token outside it is never fed: the pick is, with a NaN log-probability).  Row s of lp.out / co.cut_y /
// co.n_kept - each optional - takes that token's log-probability from the merged (ref, S) and the row's cutoff; then the bookkeeping
// and the sample's own step counter.  (e by value: taken by reference, the truncated kernel came out with 36 bytes of scratch reserved.)
struct StepLogprob {             // the sample's logits row of V columns, the temperature, the merged statistics; out: [max_len, B]
    const bf16_t* row = nullptr;
    int V = 0;
    float temp = 0.f, ref = 0.f, S = 0.f;
    float* out = nullptr;
};
struct StepCutoff {              // the row's cutoff value and kept-column count; cut_y / n_kept: [max_len, B]
    float cut = 0.f;
    uint32_t kept = 0u;
    float* cut_y = nullptr;
    int32_t* n_kept = nullptr;
};
__device__ __forceinline__ void step_end_finish(const StepEnd e, int b, int64_t s, int64_t id, const int64_t* __restrict__ forced = nullptr,
                                                const StepLogprob lp = {}, const StepCutoff co = {}) {
    const int64_t f = (forced && s < e.max_len) ? forced[s * e.B + b] : -1;
    const int64_t next = (f >= 0 && f < lp.V) ? f : id;
    e.ids[b] = next;
    if (s < e.max_len) {
        if (lp.out) lp.out[s * e.B + b] = f < lp.V ? logprob_finish(pick_value(bf2f(lp.row[next]), lp.temp), lp.ref, lp.S) : NAN;
        if (co.cut_y) co.cut_y[s * e.B + b] = co.cut;
        if (co.n_kept) co.n_kept[s * e.B + b] = (int32_t)co.kept;
    }
    step_end_sample(e.slot, e.pos, e.kv_len, e.in_ids, e.pred_ids, b, id, next, s, e.B, e.max_len);
    e.step_idx[b] = s + 1;
}

// Greedy (or untruncated sampled) pick + end of step in one launch.
__global__ __launch_bounds__(256) void decode_step_end_argmax_kernel(StepEnd e, const uint64_t* __restrict__ part, int n_tiles) {
    __shared__ uint64_t sm[4];
    const int b = blockIdx.x;
    const int64_t s = e.step_idx[b];
    const uint64_t best = block_max_u64<256, false>(strided_max_key<256>(part + (int64_t)b * n_tiles, n_tiles), sm);
    if (threadIdx.x == 0) step_end_finish(e, b, s, argmax_key_column(best));
}

// The same, plus the log-probability of the token the next step is fed - the pick, or the forced token
// (include/unimedvl_hip.h, token log-probabilities).
__global__ __launch_bounds__(256) void decode_step_end_logprob_kernel(StepEnd e, const uint64_t* __restrict__ part,
                                                                      const float* __restrict__ lse, int n_tiles,
                                                                      const bf16_t* __restrict__ logits, int64_t ldo, int V, float temp,
                                                                      const int64_t* __restrict__ forced, float* logprob) {
    __shared__ uint64_t sm[4];
    __shared__ float smf[4];
    const int b = blockIdx.x;
    const int64_t s = e.step_idx[b];
    const uint64_t best = block_max_u64<256, false>(strided_max_key<256>(part + (int64_t)b * n_tiles, n_tiles), sm);
    float ref, S;
    merge_tile_stats<256>(reinterpret_cast<const umv_f32x2*>(lse) + (int64_t)b * n_tiles, n_tiles, smf, ref, S);
    if (threadIdx.x == 0) step_end_finish(e, b, s, argmax_key_column(best), forced, {logits + (int64_t)b * ldo, V, temp, ref, S, logprob});
}

// The host side the fused entries share.  rest: the entry's own required arguments.
static int step_end_args_ok(const char* who, const StepEnd& e, const uint64_t* argmax_partial, int n_tiles, bool rest) {
    UMV_CHECK(e.slot && e.pos && e.kv_len && argmax_partial && e.ids && e.in_ids && e.pred_ids && e.step_idx && rest && e.max_len > 0 &&
                  n_tiles > 0,
              UMV_ERR_ARG, "%s: bad args", who);
    return UMV_OK;
}
static int tile_columns_ok(const char* who, int V, int n_tiles, int64_t ldo) {
    UMV_CHECK(V > 0 && V <= n_tiles * 16 && V > (n_tiles - 1) * 16 && ldo >= V, UMV_ERR_ARG,
              "%s: V (%d) must be the column count behind the %d tiles and ldo (%lld) >= V", who, V, n_tiles, (long long)ldo);
    return UMV_OK;
}

extern "C" int umv_decode_step_end_argmax(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial, int n_tiles,
                                          int64_t* ids, int64_t* in_ids, int64_t* pred_ids, int64_t* step_idx, int B,
                                          int max_len, umv_stream_t stream) {
    const StepEnd e{tok_slot, tok_pos, kv_len, ids, in_ids, pred_ids, step_idx, B, max_len};
    if (int rc = step_end_args_ok("decode_step_end_argmax", e, argmax_partial, n_tiles, true)) return rc;
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_argmax_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, e, argmax_partial, n_tiles);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_decode_step_end_logprob(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial,
                                           const float* lse_partial, int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                                           int64_t* step_idx, const uint16_t* logits, int64_t ldo, int V, float temperature,
                                           const int64_t* forced_ids, float* logprob, int B, int max_len, umv_stream_t stream) {
    const StepEnd e{tok_slot, tok_pos, kv_len, ids, in_ids, pred_ids, step_idx, B, max_len};
    if (int rc = step_end_args_ok("decode_step_end_logprob", e, argmax_partial, n_tiles, lse_partial && logits && logprob)) return rc;
    if (int rc = tile_columns_ok("decode_step_end_logprob", V, n_tiles, ldo)) return rc;
    UMV_CHECK(temperature >= 0.f, UMV_ERR_ARG, "decode_step_end_logprob: temperature (%g) must be >= 0 (0 = greedy)", (double)temperature);
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_logprob_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, e, argmax_partial, lse_partial, n_tiles,
                       logits, ldo, V, temperature, forced_ids, logprob);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- token log-probabilities (include/unimedvl_hip.h)
// The stand-alone form: one workgroup per row of bf16 logits, the definition of merge_tile_stats from the logits themselves - the maximum of y
// (exact), then the sum of exp(y - M) thread-strided in column order, the wave tree, the waves in order.
__global__ __launch_bounds__(1024) void token_logprob_kernel(const bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ ids,
                                                             float* __restrict__ out, int V, float temp) {
    __shared__ float smf[16];
    const int m = blockIdx.x;
    const bf16_t* row = logits + (int64_t)m * ld;
    float M = -INFINITY;
    for (int i = threadIdx.x; i < V; i += blockDim.x) M = fmaxf(M, pick_value(bf2f(row[i]), temp));
    M = block_reduce_max(M, smf);
    const float ref = softmax_ref(M);
    float S = 0.f;
    for (int i = threadIdx.x; i < V; i += blockDim.x) S += expf(pick_value(bf2f(row[i]), temp) - ref);
    S = block_reduce_sum(S, smf);
    if (threadIdx.x == 0) {
        const int64_t id = ids[m];
        out[m] = (id >= 0 && id < V) ? logprob_finish(pick_value(bf2f(row[id]), temp), ref, S) : NAN;
    }
}
extern "C" int umv_token_logprob_bf16(const uint16_t* logits, int64_t ld, const int64_t* ids, float* out, int M, int V, float temperature,
                                      umv_stream_t stream) {
    UMV_CHECK(logits && ids && out && V > 0 && M >= 0 && ld >= V, UMV_ERR_ARG, "token_logprob: bad args");
    UMV_CHECK(temperature >= 0.f, UMV_ERR_ARG, "token_logprob: temperature (%g) must be >= 0 (0 = greedy)", (double)temperature);
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(token_logprob_kernel, dim3(M), dim3(1024), 0, (hipStream_t)stream, logits, ld, ids, out, V, temperature);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- truncated sampling (include/unimedvl_hip.h)
// The cutoff of a row and the Gumbel maximum over what it keeps: truncation.h.
__global__ __launch_bounds__(TR_THREADS) void sample_truncated_kernel(const bf16_t* __restrict__ logits, int64_t ld, int64_t* __restrict__ out,
                                                                      int V, float temp, uint64_t seed, const int64_t* __restrict__ step_ptr,
                                                                      int top_k, float top_p, float min_p, float* __restrict__ cut_y,
                                                                      int32_t* __restrict__ n_kept) {
    __shared__ uint32_t hist[TR_BINS];
    __shared__ TruncShared sh;
    const int m = blockIdx.x;
    const bf16_t* row = logits + (int64_t)m * ld;
    float cut;
    uint32_t floor_key, kept;
    truncation_cutoff(row, V, temp, top_k, top_p, min_p, hist, sh, cut, floor_key, kept);
    const uint64_t best = kept_gumbel_max(row, V, temp, sample_row_key(seed, step_ptr, m), floor_key, sh);
    if (threadIdx.x == 0) {
        out[m] = argmax_key_column(best);
        if (cut_y) cut_y[m] = cut;
        if (n_kept) n_kept[m] = (int32_t)kept;
    }
}

static int truncation_args_ok(const char* who, float temperature, int top_k, float top_p, float min_p) {
    UMV_CHECK(temperature > 0.f, UMV_ERR_ARG, "%s: temperature must be > 0 (got %g)", who, (double)temperature);
    UMV_CHECK(top_k >= 0, UMV_ERR_ARG, "%s: top_k must be >= 0 (0 = off; got %d)", who, top_k);
    UMV_CHECK(top_p > 0.f && top_p <= 1.f, UMV_ERR_ARG, "%s: top_p must be in (0, 1] (1 = off; got %g)", who, (double)top_p);
    UMV_CHECK(min_p >= 0.f && min_p < 1.f, UMV_ERR_ARG, "%s: min_p must be in [0, 1) (0 = off; got %g)", who, (double)min_p);
    UMV_CHECK(top_k > 0 || top_p < 1.f || min_p > 0.f, UMV_ERR_ARG, "%s: no filter is on - the untruncated sampler is another entry", who);
    return UMV_OK;
}

extern "C" int umv_sample_truncated_bf16(const uint16_t* logits, int64_t ld, int64_t* out_ids, int M, int V, float temperature, uint64_t seed,
                                         const int64_t* step, int top_k, float top_p, float min_p, float* cut_y, int32_t* n_kept,
                                         umv_stream_t stream) {
    UMV_CHECK(logits && out_ids && V > 0 && M >= 0 && ld >= V, UMV_ERR_ARG, "sample_truncated: bad args");
    if (int rc = truncation_args_ok("sample_truncated", temperature, top_k, top_p, min_p)) return rc;
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(sample_truncated_kernel, dim3(M), dim3(TR_THREADS), 0, (hipStream_t)stream, logits, ld, out_ids, V, temperature, seed,
                       step, top_k, top_p, min_p, cut_y, n_kept);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// The step end of a truncated sampling step: decode_step_end_logprob_kernel whose pick is the lm_head epilogue's only if that
// column survived the filters - then the argmax over the kept set under the same noise IS that column - and the Gumbel maximum over
// the kept columns otherwise.  A kernel of its own for the 128 KiB of LDS the cutoff takes.
__global__ __launch_bounds__(TR_THREADS) void decode_step_end_truncated_kernel(
    StepEnd e, const uint64_t* __restrict__ part, const float* __restrict__ lse, int n_tiles, const bf16_t* __restrict__ logits, int64_t ldo,
    int V, float temp, uint64_t seed, int top_k, float top_p, float min_p, const int64_t* __restrict__ forced, float* logprob, float* cut_y,
    int32_t* n_kept) {
    __shared__ uint32_t hist[TR_BINS];
    __shared__ TruncShared sh;
    const int b = blockIdx.x;
    const int64_t s = e.step_idx[b];
    const bf16_t* row = logits + (int64_t)b * ldo;
    float cut;
    uint32_t floor_key, kept;
    truncation_cutoff(row, V, temp, top_k, top_p, min_p, hist, sh, cut, floor_key, kept);
    // the untruncated pick: the maximum of the sample's per-tile keys, in every thread
    uint64_t best = block_max_u64<TR_THREADS, true>(strided_max_key<TR_THREADS>(part + (int64_t)b * n_tiles, n_tiles), sh.wbest);
    const int64_t fused = argmax_key_column(best);
    const bool fused_kept = fused >= 0 && fused < V && class_key(bf2f(row[fused])) >= floor_key;     // the same in every thread
    __syncthreads();                 // wbest has been read
    if (!fused_kept) best = kept_gumbel_max(row, V, temp, sample_row_key(seed, e.step_idx + b, b), floor_key, sh);
    float ref = 0.f, S = 0.f;
    if (logprob) merge_tile_stats<TR_THREADS>(reinterpret_cast<const umv_f32x2*>(lse) + (int64_t)b * n_tiles, n_tiles, sh.smf, ref, S);
    if (threadIdx.x == 0) step_end_finish(e, b, s, argmax_key_column(best), forced, {row, V, temp, ref, S, logprob}, {cut, kept, cut_y, n_kept});
}

extern "C" int umv_decode_step_end_truncated(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial,
                                             const float* lse_partial, int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                                             int64_t* step_idx, const uint16_t* logits, int64_t ldo, int V, float temperature,
                                             const int64_t* forced_ids, float* logprob, int B, int max_len, uint64_t seed, int top_k,
                                             float top_p, float min_p, float* cut_y, int32_t* n_kept, umv_stream_t stream) {
    const StepEnd e{tok_slot, tok_pos, kv_len, ids, in_ids, pred_ids, step_idx, B, max_len};
    if (int rc = step_end_args_ok("decode_step_end_truncated", e, argmax_partial, n_tiles, logits && B >= 0)) return rc;
    UMV_CHECK((logprob != nullptr) == (lse_partial != nullptr), UMV_ERR_ARG,
              "decode_step_end_truncated: logprob and lse_partial go together (both or neither)");
    if (int rc = tile_columns_ok("decode_step_end_truncated", V, n_tiles, ldo)) return rc;
    if (int rc = truncation_args_ok("decode_step_end_truncated", temperature, top_k, top_p, min_p)) return rc;
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_truncated_kernel, dim3(B), dim3(TR_THREADS), 0, (hipStream_t)stream, e, argmax_partial, lse_partial,
                       n_tiles, logits, ldo, V, temperature, seed, top_k, top_p, min_p, forced_ids, logprob, cut_y, n_kept);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- per-row sampling parameters (include/unimedvl_hip.h)
// The step end of a step whose rows carry their own sampler (umv_row_sampling): per workgroup - uniformly - either
// decode_step_end_truncated_kernel's path with the row's temperature, filters and (seed, draw, stream), or the key maximum of
// decode_step_end_logprob_kernel (a greedy row, or a sampled one with no filter on), its statistics merged in that kernel's 256-thread
// order.  Thread 0 then advances the row's own draw counter: the one word of the table this launch writes, read by nobody else in it.
// The kernel is a template on what ends it, so that there is one copy of the pick: E = StepEnd is the step end just described (row b is
// sample b); E = PickOnly is umv_decode_pick_rows - the same pick, row b's outputs at entry b of picks / logprob / cut_y / n_kept, the
// pick's own log-probability, and nothing else written: no bookkeeping, no draw.
struct PickOnly {
    int64_t* picks;
};
template <class E>
__global__ __launch_bounds__(TR_THREADS) void decode_step_end_rows_kernel(E e, const uint64_t* __restrict__ part,
                                                                          const float* __restrict__ lse, int n_tiles,
                                                                          const bf16_t* __restrict__ logits, int64_t ldo, int V,
                                                                          umv_row_sampling* rows, const int64_t* __restrict__ forced,
                                                                          float* logprob, float* cut_y, int32_t* n_kept) {
    __shared__ uint32_t hist[TR_BINS];
    __shared__ TruncShared sh;
    constexpr bool STEP_END = std::is_same<E, StepEnd>::value;
    const int b = blockIdx.x;
    int64_t s = 0;
    if constexpr (STEP_END) s = e.step_idx[b];
    const bf16_t* row = logits + (int64_t)b * ldo;
    const float temp = row_sampling_temp(rows, b);
    const int top_k = rows[b].top_k;
    const float top_p = rows[b].top_p, min_p = rows[b].min_p;
    const int64_t draw = rows[b].draw;
    const bool truncated = temp > 0.f && (top_k > 0 || top_p < 1.f || min_p > 0.f);       // the same in every thread
    float cut = -INFINITY;
    uint32_t floor_key = 0u, kept = (uint32_t)V;
    if (truncated) truncation_cutoff(row, V, temp, top_k, top_p, min_p, hist, sh, cut, floor_key, kept);
    uint64_t best = block_max_u64<TR_THREADS, true>(strided_max_key<TR_THREADS>(part + (int64_t)b * n_tiles, n_tiles), sh.wbest);
    if (truncated) {
        const int64_t fused = argmax_key_column(best);
        const bool fused_kept = fused >= 0 && fused < V && class_key(bf2f(row[fused])) >= floor_key;
        __syncthreads();                 // wbest has been read
        if (!fused_kept)
            best = kept_gumbel_max(row, V, temp, sample_row_key_of(rows[b].seed, (uint64_t)draw, (uint64_t)rows[b].stream), floor_key, sh);
    }
    float ref = 0.f, S = 0.f;
    if (logprob) {
        const umv_f32x2* st = reinterpret_cast<const umv_f32x2*>(lse) + (int64_t)b * n_tiles;
        if (truncated) merge_tile_stats<TR_THREADS>(st, n_tiles, sh.smf, ref, S);
        else merge_tile_stats<TR_THREADS, 256>(st, n_tiles, sh.smf, ref, S);
    }
    if constexpr (STEP_END) {
        if (threadIdx.x == 0) {
            step_end_finish(e, b, s, argmax_key_column(best), forced, {row, V, temp, ref, S, logprob}, {cut, kept, cut_y, n_kept});
            rows[b].draw = draw + 1;
        }
    } else if (threadIdx.x == 0) {
        const int64_t id = argmax_key_column(best);
        e.picks[b] = id;
        if (logprob) logprob[b] = (id >= 0 && id < V) ? logprob_finish(pick_value(bf2f(row[id]), temp), ref, S) : NAN;
        if (cut_y) cut_y[b] = cut;
        if (n_kept) n_kept[b] = (int32_t)kept;
    }
}

extern "C" int umv_decode_step_end_rows(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial,
                                        const float* lse_partial, int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                                        int64_t* step_idx, const uint16_t* logits, int64_t ldo, int V, const int64_t* forced_ids,
                                        float* logprob, int B, int max_len, umv_row_sampling* rows, float* cut_y, int32_t* n_kept,
                                        umv_stream_t stream) {
    const StepEnd e{tok_slot, tok_pos, kv_len, ids, in_ids, pred_ids, step_idx, B, max_len};
    if (int rc = step_end_args_ok("decode_step_end_rows", e, argmax_partial, n_tiles, logits && B >= 0)) return rc;
    UMV_CHECK(rows && ((uintptr_t)rows % 16) == 0, UMV_ERR_ARG, "decode_step_end_rows: rows (the per-row sampling table) must be set and "
              "16-byte aligned");
    UMV_CHECK((logprob != nullptr) == (lse_partial != nullptr), UMV_ERR_ARG,
              "decode_step_end_rows: logprob and lse_partial go together (both or neither)");
    if (int rc = tile_columns_ok("decode_step_end_rows", V, n_tiles, ldo)) return rc;
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_rows_kernel<StepEnd>, dim3(B), dim3(TR_THREADS), 0, (hipStream_t)stream, e, argmax_partial, lse_partial,
                       n_tiles, logits, ldo, V, rows, forced_ids, logprob, cut_y, n_kept);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- speculative greedy decode (include/unimedvl_hip.h)
// The step end of a step that verified k drafts per sample: steps 1-8 of the header, one workgroup per sample.  The picks are the
// key maxima of decode_step_end_argmax_kernel, one row after the other; the sample's bookkeeping is thread 0's; the prompt lookup
// scans the candidate starts thread-strided and takes the largest through the same key maximum.
__device__ __forceinline__ bool spec_token_ok(int64_t t, int V) { return t >= 0 && t < V; }

// One body for two kernels, a template on the arguments: umv_spec_step_args is the greedy step end (the picks are the key maxima);
// umv_spec_rows_step_args is umv_decode_step_end_speculative_rows (ROWS) - the picks are read from r.picks, step 9 advances the draw
// counters of the sample's table rows and the emitted tokens take their rows' log-probabilities.
__device__ __forceinline__ const umv_spec_step_args& spec_step_of(const umv_spec_step_args& x) { return x; }
__device__ __forceinline__ const umv_spec_step_args& spec_step_of(const umv_spec_rows_step_args& x) { return x.step; }
template <class Args>
__global__ __launch_bounds__(256) void decode_step_end_speculative_kernel(Args r) {
    constexpr bool ROWS = std::is_same<Args, umv_spec_rows_step_args>::value;
    const umv_spec_step_args& a = spec_step_of(r);
    __shared__ uint64_t sm[4];
    __shared__ int64_t pick[64];
    __shared__ int32_t s_hist_len, s_n_out;
    const int b = blockIdx.x, k = a.k, r0 = b * (k + 1);
    int32_t* hist = a.hist + (int64_t)b * a.hist_ld;
    if constexpr (ROWS) {
        if (!a.draft_only && (int)threadIdx.x <= k) pick[threadIdx.x] = r.picks[r0 + threadIdx.x];
        __syncthreads();                 // pick[0..k] is written
    } else if (!a.draft_only) {
        for (int j = 0; j <= k; ++j) {
            const uint64_t best = block_max_u64<256, true>(strided_max_key<256>(a.argmax_partial + (int64_t)(r0 + j) * a.n_tiles, a.n_tiles), sm);
            if (threadIdx.x == 0) pick[j] = argmax_key_column(best);
            __syncthreads();             // sm is free again, pick[j] is written
        }
    }
    if (threadIdx.x == 0) {
        int32_t hl = a.hist_len[b], n_out = a.n_out[b];
        hl = hl < 0 ? 0 : hl > a.hist_ld ? (int32_t)a.hist_ld : hl;      // nothing is read or written outside the row
        if (!a.draft_only) {
            const int nd = a.n_draft[b];
            int n = 0;
            while (n < nd && n < k && a.ids[r0 + n + 1] == pick[n]) ++n;
            const int64_t lim = a.limit[b] < a.out_ld ? (int64_t)a.limit[b] : a.out_ld;
            const int m = (n_out < 0 || lim - n_out <= 0) ? 0 : lim - n_out < n + 1 ? (int)(lim - n_out) : n + 1;
            for (int i = 0; i < m; ++i) {
                a.out_ids[(int64_t)b * a.out_ld + n_out + i] = pick[i];
                if (hl < a.hist_ld) hist[hl++] = (int32_t)pick[i];
                if constexpr (ROWS)
                    if (r.out_logprobs) r.out_logprobs[(int64_t)b * a.out_ld + n_out + i] = r.row_logprob[r0 + i];
            }
            if constexpr (ROWS) {
                if (m > 0) {             // the draws: row j of the next step is the sample's token n_out + m + j
                    const int64_t d0 = r.rows[r0].draw;
                    for (int j = 0; j <= k; ++j) r.rows[r0 + j].draw = d0 + m + j;
                }
            }
            n_out += m;
            a.n_out[b] = n_out;
            a.hist_len[b] = hl;
            a.kv_len[b] += m;
            a.tok_slot[r0] += m;
            a.tok_pos[r0] += m;
            if (m > 0) a.ids[r0] = pick[m - 1];
            a.stats[b * 3 + 0] += 1;
            a.stats[b * 3 + 1] += nd;
            a.stats[b * 3 + 2] += n;
        }
        s_hist_len = hl;
        s_n_out = n_out;
    }
    __syncthreads();                     // the appended history is visible to the workgroup
    const int32_t hl = s_hist_len, n_out = s_n_out;
    const bool use_pred = a.predicted && a.pred_len[b] > 0;
    int64_t start = -1;                  // the index of hist the drafts are read from; the same in every thread
    if (!use_pred) {
        for (int g = a.ngram_max; g >= a.ngram_min && start < 0; --g) {
            if (hl <= g) continue;
            const int32_t* suf = hist + hl - g;
            uint64_t found = 0;          // 1 + the largest matching start of this thread
            for (int i = threadIdx.x; i < hl - g; i += 256) {
                bool eq = true;
                for (int t = 0; t < g && eq; ++t) eq = suf[t] >= 0 && hist[i + t] == suf[t];
                if (eq) found = (uint64_t)i + 1;
            }
            found = block_max_u64<256, true>(found, sm);
            __syncthreads();             // sm is free again
            if (found) start = (int64_t)found - 1 + g;
        }
    }
    if (threadIdx.x == 0) {
        const int64_t t0 = a.ids[r0];
        const int32_t slot0 = a.tok_slot[r0], pos0 = a.tok_pos[r0];
        int nd = 0;
        bool open = true;                // drafts stop at the first index or entry that is out of range
        for (int j = 1; j <= k; ++j) {
            int64_t d = -1;
            if (open && use_pred) {
                const int64_t at = (int64_t)n_out + j - 1;
                if (at < a.pred_len[b] && at < a.pred_ld) d = a.predicted[(int64_t)b * a.pred_ld + at];
            } else if (open && start >= 0) {
                const int64_t at = start + j - 1;
                if (at < hl) d = hist[at];
            }
            open = open && spec_token_ok(d, a.V);
            if (open) ++nd;
            a.ids[r0 + j] = open ? d : t0;
            a.tok_slot[r0 + j] = slot0 + j;
            a.tok_pos[r0 + j] = pos0 + j;
        }
        a.n_draft[b] = nd;
    }
}

// What the two entries check alike.  keys: the entry reads argmax_partial (unless draft_only).
static int spec_step_args_ok(const char* who, const umv_spec_step_args* a, bool keys) {
    UMV_CHECK(a->k >= 1 && a->B >= 0 && (int64_t)a->B * (a->k + 1) <= 64, UMV_ERR_ARG,
              "%s: k (%d) must be >= 1 and B * (k + 1) (%d x %d) at most 64 rows", who, a->k, a->B, a->k + 1);
    UMV_CHECK(a->ngram_min >= 1 && a->ngram_min <= a->ngram_max, UMV_ERR_ARG, "%s: 1 <= ngram_min (%d) <= ngram_max (%d)", who,
              a->ngram_min, a->ngram_max);
    UMV_CHECK(a->tok_slot && a->tok_pos && a->kv_len && a->ids && a->out_ids && a->n_out && a->limit && a->n_draft && a->hist &&
                  a->hist_len && a->stats && (!keys || a->argmax_partial || a->draft_only) && a->out_ld > 0 && a->hist_ld > 0,
              UMV_ERR_ARG, "%s: null pointer", who);
    UMV_CHECK((a->predicted != nullptr) == (a->pred_len != nullptr) && (!a->predicted || a->pred_ld > 0), UMV_ERR_ARG,
              "%s: predicted and pred_len go together", who);
    UMV_CHECK(a->n_tiles > 0, UMV_ERR_ARG, "%s: n_tiles must be > 0", who);
    return tile_columns_ok(who, a->V, a->n_tiles, a->V);
}

extern "C" int umv_decode_step_end_speculative(const umv_spec_step_args* a, umv_stream_t stream) {
    UMV_CHECK(a, UMV_ERR_ARG, "decode_step_end_speculative: null args");
    if (int rc = spec_step_args_ok("decode_step_end_speculative", a, true)) return rc;
    if (a->B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_speculative_kernel<umv_spec_step_args>, dim3(a->B), dim3(256), 0, (hipStream_t)stream, *a);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- speculative decode with sampling (include/unimedvl_hip.h)
// Two launches end a sampled speculative step: every row's pick with its own sampler (decode_step_end_rows_kernel<PickOnly>, the T
// workgroups sweeping their rows in parallel), then the commit per sample (decode_step_end_speculative_kernel on the rows arguments).
extern "C" int umv_decode_pick_rows(const uint64_t* argmax_partial, const float* lse_partial, int n_tiles, const uint16_t* logits, int64_t ldo,
                                    int V, const umv_row_sampling* rows, int T, int64_t* picks, float* logprob, float* cut_y, int32_t* n_kept,
                                    umv_stream_t stream) {
    UMV_CHECK(argmax_partial && logits && picks && n_tiles > 0 && T >= 0, UMV_ERR_ARG, "decode_pick_rows: bad args");
    UMV_CHECK(T <= 64, UMV_ERR_ARG, "decode_pick_rows: at most 64 rows (got %d)", T);
    UMV_CHECK(rows && ((uintptr_t)rows % 16) == 0, UMV_ERR_ARG, "decode_pick_rows: rows (the per-row sampling table) must be set and "
              "16-byte aligned");
    UMV_CHECK((logprob != nullptr) == (lse_partial != nullptr), UMV_ERR_ARG,
              "decode_pick_rows: logprob and lse_partial go together (both or neither)");
    if (int rc = tile_columns_ok("decode_pick_rows", V, n_tiles, ldo)) return rc;
    if (T == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_rows_kernel<PickOnly>, dim3(T), dim3(TR_THREADS), 0, (hipStream_t)stream, PickOnly{picks},
                       argmax_partial, lse_partial, n_tiles, logits, ldo, V, const_cast<umv_row_sampling*>(rows), (const int64_t*)nullptr,
                       logprob, cut_y, n_kept);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_decode_step_end_speculative_rows(const umv_spec_rows_step_args* a, umv_stream_t stream) {
    UMV_CHECK(a, UMV_ERR_ARG, "decode_step_end_speculative_rows: null args");
    if (int rc = spec_step_args_ok("decode_step_end_speculative_rows", &a->step, false)) return rc;
    UMV_CHECK(a->picks || a->step.draft_only, UMV_ERR_ARG, "decode_step_end_speculative_rows: picks must be set");
    UMV_CHECK(a->rows && ((uintptr_t)a->rows % 16) == 0, UMV_ERR_ARG, "decode_step_end_speculative_rows: rows (the per-row sampling table) "
              "must be set and 16-byte aligned");
    UMV_CHECK((a->row_logprob != nullptr) == (a->out_logprobs != nullptr), UMV_ERR_ARG,
              "decode_step_end_speculative_rows: row_logprob and out_logprobs go together (both or neither)");
    if (a->step.B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_speculative_kernel<umv_spec_rows_step_args>, dim3(a->step.B), dim3(256), 0, (hipStream_t)stream, *a);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
