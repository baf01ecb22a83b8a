// Workgroup reductions of the row kernels (norm.hip, token_pick.hip, image_head.hip): wave_sum / wave_max of common.h, then one LDS
// exchange between the waves.  Every thread of the workgroup must call them.
#pragma once
#include "common.h"
#include "token_pick.h"         // shfl_xor_u64

// sum / max over the blockDim.x / 64 waves, in wave order; sm: one float per wave.  The leading barrier makes `sm` reusable
// from one call to the next.
__device__ __forceinline__ float block_reduce_sum(float v, float* sm) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += sm[w];
    return r;
}
__device__ __forceinline__ float block_reduce_max(float v, float* sm) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, sm[w]);
    return r;
}

// The point a sum of exponentials is taken about, given its maximum M: M itself, and 0 for a row of -inf only - every term is then
// exp(-inf - 0) = 0, not exp(-inf + inf) = NaN.
__device__ __forceinline__ float softmax_ref(float M) { return (M == -INFINITY) ? 0.f : M; }

// The merge of a sample's per-tile softmax statistics (m_t, s_t) into (ref, S), in every thread: M = max m_t, ref = softmax_ref(M),
// S = sum s_t exp(m_t - ref).  Two passes over the 8 n_tiles bytes (L2 resident: the GEMM has just written them), each thread-strided
// by T, then the wave tree, then the waves in order - a fixed order for a given T, so a sample's bits do not depend on the batch it
// sits in.  A tile of -inf only is (-inf, 0) and adds 0 * exp(-inf) = 0; a NaN s_t makes S NaN.  smf: one float per wave.
// TA < T: only the first TA threads take tiles, in TA's order - the other waves add +0 behind them, so a workgroup of T threads gets
// the bits a workgroup of TA threads gets (the per-row step end and the top-n kernel run the 256-thread kernels' merge in their 512
// threads).  Used by the step ends of token_pick.hip and by top_logprobs.hip, which must merge in the order the step end did.
template <int T, int TA = T>
__device__ __forceinline__ void merge_tile_stats(const umv_f32x2* __restrict__ st, int n_tiles, float* smf, float& ref, float& S) {
    const int c_first = (TA == T || (int)threadIdx.x < TA) ? (int)threadIdx.x : n_tiles;
    float M = -INFINITY;
    for (int c = c_first; c < n_tiles; c += TA) M = fmaxf(M, st[c].x);
    M = block_reduce_max(M, smf);
    ref = softmax_ref(M);
    S = 0.f;
    for (int c = c_first; c < n_tiles; c += TA) {
        const umv_f32x2 v = st[c];
        S += v.y * expf(v.x - ref);
    }
    S = block_reduce_sum(S, smf);
}

// The maximum of a 64-bit value (an argmax key, token_pick.h) over a workgroup of T threads: complete in every thread (ALL) or in
// thread 0 only.  sm: one word per wave, not in use by anything before this call; an ALL caller that reuses it puts a barrier behind.
template <int T, bool ALL>
__device__ __forceinline__ uint64_t block_max_u64(uint64_t best, uint64_t* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ob = shfl_xor_u64(best, o);
        best = ob > best ? ob : best;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
    __syncthreads();
    if (ALL || threadIdx.x == 0)
        for (int w = ALL ? 0 : 1; w < T / 64; ++w) best = sm[w] > best ? sm[w] : best;
    return best;
}

// The sum of a 256-thread workgroup as (p0 + p1) + (p2 + p3): the fixed order of the decode norms, whose results must not
// depend on which of them a row went through.  part: four floats, written once per kernel.
__device__ __forceinline__ float four_wave_sum(float v, float* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// The largest value of the workgroup and, among equal values, its LOWEST index.  True in the one thread (thread 0) whose
// (best, bidx) is the result.  smv / smi: one entry per wave, not in use by anything before this call (a caller that reuses
// them puts a barrier in front).
__device__ __forceinline__ bool block_best_lowest(float& best_io, int& bidx_io, float* smv, int* smi) {
    float best = best_io;
    int bidx = bidx_io;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ob = __shfl_xor(best, o, 64);
        int oi = __shfl_xor(bidx, o, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { smv[threadIdx.x >> 6] = best; smi[threadIdx.x >> 6] = bidx; }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
        if (smv[w] > best || (smv[w] == best && smi[w] < bidx)) { best = smv[w]; bidx = smi[w]; }
    best_io = best;
    bidx_io = bidx;
    return true;
}
