// Next-token picking and the bookkeeping that ends a decode step: argmax and temperature sampling over bf16 logits, the
// step-end kernels (two of them finish the lm_head GEMM's argmax epilogue, one with the token's log-probability) and the stand-alone
// token log-probability.
#include "block_reduce.h"
#include "token_pick.h"
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

// The maximum of a sample's n_tiles keys, complete in thread 0 of a 256-thread workgroup; sm: one word per wave.
__device__ __forceinline__ uint64_t block_max_key(const uint64_t* __restrict__ row, int n_tiles, uint64_t* sm) {
    uint64_t best = 0;
    constexpr int UA = 8;      // all loads of a thread in flight together: one round trip for up to 2048 tiles per pass
    for (int c0 = threadIdx.x; c0 < n_tiles; c0 += 256 * UA) {
        uint64_t v[UA];
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int c = c0 + u * 256;
            v[u] = c < n_tiles ? row[c] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < UA; ++u) best = v[u] > best ? v[u] : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ob = shfl_xor_u64(best, o);
        best = ob > best ? ob : best;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) best = sm[w] > best ? sm[w] : best;
    return best;
}

// Greedy pick + end of step in one launch: one workgroup per sample takes the maximum of the per-tile keys the lm_head GEMM
// epilogue left (token_pick.h::argmax_key), then does decode_step_end_kernel's bookkeeping for its sample.  The step counter
// is PER SAMPLE - step_idx[b], all equal - so that no workgroup reads a word another workgroup of the same launch writes
// (rounds 2-3 shared step_idx[0] behind a relaxed ticket; correct on this hardware, not by the memory model).
__global__ __launch_bounds__(256) void decode_step_end_argmax_kernel(int32_t* slot, int32_t* pos, int32_t* kv_len,
                                                                     const uint64_t* __restrict__ part, int n_tiles, int64_t* ids,
                                                                     int64_t* in_ids, int64_t* pred_ids, int64_t* step_idx,
                                                                     int B, int max_len) {
    __shared__ uint64_t sm[4];
    const int b = blockIdx.x;
    const int64_t s = step_idx[b];
    const uint64_t best = block_max_key(part + (int64_t)b * n_tiles, n_tiles, sm);
    if (threadIdx.x == 0) {
        const int64_t id = argmax_key_column(best);
        ids[b] = id;
        step_end_sample(slot, pos, kv_len, in_ids, pred_ids, b, id, id, s, B, max_len);
        step_idx[b] = s + 1;
    }
}
extern "C" int umv_decode_step_end_argmax(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial, int n_tiles,
                                          int64_t* ids, int64_t* in_ids, int64_t* pred_ids, int64_t* step_idx, int B,
                                          int max_len, umv_stream_t stream) {
    UMV_CHECK(tok_slot && tok_pos && kv_len && argmax_partial && ids && in_ids && pred_ids && step_idx && max_len > 0 && n_tiles > 0,
              UMV_ERR_ARG, "decode_step_end_argmax: bad args");
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_argmax_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, tok_slot, tok_pos, kv_len, argmax_partial,
                       n_tiles, ids, in_ids, pred_ids, step_idx, B, max_len);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- token log-probabilities (include/unimedvl_hip.h)
// decode_step_end_argmax_kernel that also merges the sample's per-tile softmax statistics (gemm_epilogue.h::epi_lse_tile) and
// writes the log-probability of the token the next step is fed - the pick, or the forced token.  Two passes over the 8 n_tiles
// bytes (L2 resident: the GEMM has just written them): M = max m_t, then S = sum s_t exp(m_t - M) about that maximum, each
// thread-strided, then the wave tree, then waves 0..3 in order (block_reduce.h) - a fixed order, so a sample's bits do not depend
// on the batch it sits in.  A tile of -inf only is (-inf, 0) and adds 0 * exp(-inf) = 0; a NaN s_t makes S NaN.
__global__ __launch_bounds__(256) void decode_step_end_logprob_kernel(int32_t* slot, int32_t* pos, int32_t* kv_len,
                                                                      const uint64_t* __restrict__ part, const float* __restrict__ lse,
                                                                      int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                                                                      int64_t* step_idx, const bf16_t* __restrict__ logits, int64_t ldo, int V,
                                                                      float temp, const int64_t* __restrict__ forced, float* logprob, int B,
                                                                      int max_len) {
    __shared__ uint64_t sm[4];
    __shared__ float smf[4];
    const int b = blockIdx.x;
    const int64_t s = step_idx[b];
    const uint64_t best = block_max_key(part + (int64_t)b * n_tiles, n_tiles, sm);
    const umv_f32x2* st = reinterpret_cast<const umv_f32x2*>(lse) + (int64_t)b * n_tiles;
    float M = -INFINITY;
    for (int c = threadIdx.x; c < n_tiles; c += 256) M = fmaxf(M, st[c].x);
    M = block_reduce_max(M, smf);
    const float ref = (M == -INFINITY) ? 0.f : M;
    float S = 0.f;
    for (int c = threadIdx.x; c < n_tiles; c += 256) {
        const umv_f32x2 v = st[c];
        S += v.y * expf(v.x - ref);
    }
    S = block_reduce_sum(S, smf);
    if (threadIdx.x == 0) {
        const int64_t id = argmax_key_column(best);
        const int64_t f = (forced && s < max_len) ? forced[s * B + b] : -1;
        const int64_t next = (f >= 0 && f < V) ? f : id;      // a forced token outside the vocabulary is never fed: the pick is, with a NaN
        ids[b] = next;
        if (s < max_len)
            logprob[s * B + b] = f < V ? logprob_finish(pick_value(bf2f(logits[(int64_t)b * ldo + next]), temp), ref, S) : NAN;
        step_end_sample(slot, pos, kv_len, in_ids, pred_ids, b, id, next, s, B, max_len);
        step_idx[b] = s + 1;
    }
}
extern "C" int umv_decode_step_end_logprob(int32_t* tok_slot, int32_t* tok_pos, int32_t* kv_len, const uint64_t* argmax_partial,
                                           const float* lse_partial, int n_tiles, int64_t* ids, int64_t* in_ids, int64_t* pred_ids,
                                           int64_t* step_idx, const uint16_t* logits, int64_t ldo, int V, float temperature,
                                           const int64_t* forced_ids, float* logprob, int B, int max_len, umv_stream_t stream) {
    UMV_CHECK(tok_slot && tok_pos && kv_len && argmax_partial && lse_partial && ids && in_ids && pred_ids && step_idx && logits && logprob &&
                  max_len > 0 && n_tiles > 0,
              UMV_ERR_ARG, "decode_step_end_logprob: bad args");
    UMV_CHECK(V > 0 && V <= n_tiles * 16 && V > (n_tiles - 1) * 16 && ldo >= V, UMV_ERR_ARG,
              "decode_step_end_logprob: V (%d) must be the column count behind the %d tiles and ldo (%lld) >= V", V, n_tiles, (long long)ldo);
    UMV_CHECK(temperature >= 0.f, UMV_ERR_ARG, "decode_step_end_logprob: temperature (%g) must be >= 0 (0 = greedy)", (double)temperature);
    if (B == 0) return UMV_OK;
    hipLaunchKernelGGL(decode_step_end_logprob_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, tok_slot, tok_pos, kv_len, argmax_partial,
                       lse_partial, n_tiles, ids, in_ids, pred_ids, step_idx, logits, ldo, V, temperature, forced_ids, logprob, B, max_len);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// The stand-alone form: one workgroup per row of bf16 logits, the same definition from the logits themselves - the maximum of y
// (exact), then the sum of exp(y - M) thread-strided in column order, the wave tree, the waves in order.
__global__ __launch_bounds__(1024) void token_logprob_kernel(const bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ ids,
                                                             float* __restrict__ out, int V, float temp) {
    __shared__ float smf[16];
    const int m = blockIdx.x;
    const bf16_t* row = logits + (int64_t)m * ld;
    float M = -INFINITY;
    for (int i = threadIdx.x; i < V; i += blockDim.x) M = fmaxf(M, pick_value(bf2f(row[i]), temp));
    M = block_reduce_max(M, smf);
    const float ref = (M == -INFINITY) ? 0.f : M;
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
