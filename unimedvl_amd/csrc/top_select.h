// The selection body of the top-n kernels (top_logprobs.hip) and of the beam search candidates (beam.hip): one copy, so that a beam's
// candidate list is a row's top-n list bit for bit.
#pragma once
#include "block_reduce.h"
#include "token_pick.h"
#include "truncation.h"
#include "../../include/unimedvl_hip.h"

constexpr int TOPN = UMV_TOP_LOGPROBS_MAX;
static_assert(TOPN * TR_THREADS <= TR_BINS, "the per-thread candidate lists reuse the histogram's LDS");

struct TopShared {
    uint64_t key[TOPN];                      // the n selected columns as (class_key(y) << 32 | ~column), unsorted above the class
    uint32_t wmin[2][TR_THREADS / 64];       // per wave: lowest candidate column of a round (two rounds in flight)
    uint32_t wcnt[TR_THREADS / 64];          // per wave: columns in front of the fed token
    uint32_t n_above;                        // columns above the cutoff class
    float wsum[2 * TR_THREADS / 64];         // the stand-alone sum's 16 wave partials
};

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t b = (uint32_t)__shfl_xor((int)v, o, 64);
        v = b < v ? b : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_add_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// What a row's workgroup writes: n ids, n log-probabilities, one rank.
struct TopOut {
    int32_t* ids;
    float* logprobs;
    int32_t* rank;
};

// The row's n best columns by (y descending, column ascending) and the rank of column `fed` (outside [0, V): rank 0), from (ref, S).
// Every thread of the workgroup calls it with the same arguments.  hist: TR_BINS words of LDS.  max_logit: the row's highest logit
// where the caller knows it (a greedy row: the maximum of its statistics), NaN where not - the cutoff then looks for it itself.
__device__ __forceinline__ void top_select(const bf16_t* __restrict__ row, int V, float temp, int n, int64_t fed, float ref, float S,
                                           float max_logit, uint32_t* hist, TruncShared& sh, TopShared& ts, const TopOut o) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (S != S) {                        // a NaN logit: the same in every thread
        if (t < n) { o.ids[t] = -1; o.logprobs[t] = NAN; }
        if (t == 0) o.rank[0] = 0;
        return;
    }
    float cut;
    uint32_t floor_key, kept;
    if (max_logit == max_logit) truncation_cutoff<true>(row, V, temp, n, 1.f, 0.f, hist, sh, cut, floor_key, kept, class_key(max_logit));
    else truncation_cutoff(row, V, temp, n, 1.f, 0.f, hist, sh, cut, floor_key, kept);
    const uint32_t ycut = class_key(cut);                // the class of the n-th largest y
    const bool fed_ok = fed >= 0 && fed < V;
    const uint32_t yfed = fed_ok ? class_key(pick_value(bf2f(row[fed]), temp)) : 0xFFFFFFFFu;
    const uint32_t cfed = fed_ok ? (uint32_t)fed : 0u;
    if (t == 0) ts.n_above = 0u;
    if (t < TOPN) ts.key[t] = 0xFFFFFFFFull;             // column 0 until selected: nothing below indexes the row from an unset word
    __syncthreads();                     // the cutoff is done with hist; n_above is zero
    // a thread meets its columns in ascending order, so the first n of the class it meets are its n lowest: list entry i of thread t
    // is hist[i * TR_THREADS + t]
    uint32_t mine = 0u, before = 0u;
    for_each_column(row, V, [&](int c, float x) {
        const uint32_t ky = class_key(pick_value(x, temp));
        before += (ky > yfed || (ky == yfed && (uint32_t)c < cfed)) ? 1u : 0u;
        if (ky > ycut) {
            const uint32_t slot = atomicAdd(&ts.n_above, 1u);        // fewer than n by the cutoff's definition; their order is settled below
            if (slot < (uint32_t)n) ts.key[slot] = ((uint64_t)ky << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c);
        } else if (ky == ycut && mine < (uint32_t)n) {
            hist[mine * TR_THREADS + t] = (uint32_t)c;
            ++mine;
        }
    });
    before = wave_add_u32(before);
    if (lane == 0) ts.wcnt[w] = before;
    __syncthreads();
    const uint32_t na = ts.n_above < (uint32_t)n ? ts.n_above : (uint32_t)n;
    // the class's lowest columns, one per round: the minimum over the heads of the threads' lists
    uint32_t ptr = 0u, head = mine ? hist[t] : 0xFFFFFFFFu;
    for (uint32_t r = na; r < (uint32_t)n; ++r) {
        const uint32_t wm = wave_min_u32(head);
        if (lane == 0) ts.wmin[r & 1][w] = wm;
        __syncthreads();
        uint32_t g = ts.wmin[r & 1][0];
#pragma unroll
        for (int i = 1; i < TR_THREADS / 64; ++i) g = ts.wmin[r & 1][i] < g ? ts.wmin[r & 1][i] : g;
        if (head == g && g != 0xFFFFFFFFu) {             // its owner: columns are distinct
            ts.key[r] = ((uint64_t)ycut << 32) | (uint64_t)(0xFFFFFFFFu - g);
            ++ptr;
            head = ptr < mine ? hist[ptr * TR_THREADS + t] : 0xFFFFFFFFu;
        }
    }
    __syncthreads();
    if (t < n) {
        // entries above the class take the place their key has among them (keys are distinct); the class's are in order already
        const uint64_t k = ts.key[t];
        uint32_t pos = (uint32_t)t;
        if ((uint32_t)t < na) {
            pos = 0u;
            for (uint32_t i = 0; i < na; ++i) pos += ts.key[i] > k ? 1u : 0u;
        }
        const int64_t col = argmax_key_column(k);
        o.ids[pos] = (int32_t)col;
        o.logprobs[pos] = logprob_finish(pick_value(bf2f(row[col]), temp), ref, S);
    }
    if (t == 0) {
        uint32_t total = 0u;
        for (int i = 0; i < TR_THREADS / 64; ++i) total += ts.wcnt[i];
        o.rank[0] = fed_ok ? (int32_t)(total + 1u) : 0;
    }
}
