// Constrained decoding (include/unimedvl_hip.h, "token automata"): a row in state s of a token automaton may only be fed one of the
// tokens of s's edges.  umv_logit_constrain_bf16 sits where the penalty kernel sits - between the lm_head GEMM and the step end - with
// the opposite sparsity: a handful of columns of a masked row keep their bits, every other one becomes -inf, and EVERY tile's argmax
// key and softmax statistics are rewritten to what the lm_head epilogue would have left for the masked logits (penalty_tile.h), so that
// whichever step end follows reads the restricted distribution.  umv_constraint_advance moves the rows' state words along the edges of
// the tokens the step end left to be fed next; it is the only writer of those words.
#include "penalty_tile.h"

#define LC_THREADS 256
#define LC_CHUNK UMV_CONSTRAIN_CHUNK      // columns per workgroup: one 16-column tile per thread
static_assert(LC_CHUNK == LC_THREADS * 16, "one tile per thread");

typedef u32x4 __attribute__((may_alias)) lc_u32x4;      // 8 bf16 of a row as one 16-byte access (the tile is read back as bf16_t)

// first index in [lo, hi) whose token is >= v (the edges of a state are sorted)
__device__ __forceinline__ int lc_lower_bound(const int32_t* __restrict__ tok, int lo, int hi, int64_t v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)tok[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// state s's edge range, held inside [0, n_edges] whatever the table says (the contents are the caller's; nothing is read outside it)
__device__ __forceinline__ void lc_edge_range(const umv_token_automaton& t, int s, int* e0, int* e1) {
    const int lo = max(0, min(t.row_ptr[s], t.n_edges));
    *e0 = lo;
    *e1 = max(lo, min(t.row_ptr[s + 1], t.n_edges));
}

// grid (column chunk, row).  ROWS: the temperature and the sampling key of row b come from a.rows[b] (per-row sampling parameters).
template <bool ROWS>
__global__ __launch_bounds__(LC_THREADS) void logit_constrain_kernel(umv_logit_constrain_args a) {
    __shared__ uint32_t s_allowed[LC_CHUNK / 32];        // bit n - c0: column n is an edge token of the row's state
    const int b = blockIdx.y;
    const int s = a.state[b];
    if (s < 0 || s >= a.automaton.n_states) return;      // a free row: nothing of it is written (uniform: before any barrier)
    const int c0 = blockIdx.x * LC_CHUNK, c1 = min(a.V, c0 + LC_CHUNK);
    if (threadIdx.x < LC_CHUNK / 32) s_allowed[threadIdx.x] = 0u;
    __syncthreads();
    int e0, e1;
    lc_edge_range(a.automaton, s, &e0, &e1);
    const int32_t* __restrict__ tok = a.automaton.edge_token;
    const int lo = lc_lower_bound(tok, e0, e1, c0), hi = lc_lower_bound(tok, lo, e1, c1);
    for (int e = lo + threadIdx.x; e < hi; e += LC_THREADS) {
        const uint32_t n = (uint32_t)(tok[e] - c0);
        if (n < (uint32_t)(c1 - c0)) atomicOr(&s_allowed[n >> 5], 1u << (n & 31));      // (the range check holds for sorted edges)
    }
    __syncthreads();
    // ---- this thread's tile
    const int n0 = c0 + threadIdx.x * 16;
    if (n0 >= a.V) return;
    const int nend = min(a.V, n0 + 16), tile = n0 >> 4;
    const uint32_t allowed = (s_allowed[threadIdx.x >> 1] >> ((threadIdx.x & 1) * 16)) & 0xFFFFu;
    bf16_t* row = a.logits + (int64_t)b * a.ld;
    const bf16_t ninf = 0xFF80;
    const bool wide = nend - n0 == 16 && ((reinterpret_cast<uintptr_t>(row + n0) & 15) == 0);
    const int64_t t = (int64_t)b * a.n_tiles + tile;
    if (allowed == 0u) {
        // no load: the logits are the constant -inf, the statistics (-inf, 0) and - sampled or not, -inf plus noise is -inf - the key
        // the maximum of argmax_key(-inf, n) over the valid columns: that of the lowest one
        if (wide) {
            const lc_u32x4 v = {0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u};
            reinterpret_cast<lc_u32x4*>(row + n0)[0] = v;
            reinterpret_cast<lc_u32x4*>(row + n0)[1] = v;
        } else {
            for (int n = n0; n < nend; ++n) row[n] = ninf;
        }
        if (!a.argmax_partial) return;
        a.argmax_partial[t] = argmax_key(-INFINITY, n0);
        if (a.lse_partial) *reinterpret_cast<umv_f32x2*>(a.lse_partial + t * 2) = (umv_f32x2){-INFINITY, 0.f};
        return;
    }
    if (wide) {
        lc_u32x4 v[2] = {reinterpret_cast<const lc_u32x4*>(row + n0)[0], reinterpret_cast<const lc_u32x4*>(row + n0)[1]};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t two = (allowed >> (8 * h + 2 * w)) & 3u;
                const uint32_t keep = ((two & 1u) ? 0x0000FFFFu : 0u) | ((two & 2u) ? 0xFFFF0000u : 0u);
                v[h][w] = (v[h][w] & keep) | (0xFF80FF80u & ~keep);
            }
        reinterpret_cast<lc_u32x4*>(row + n0)[0] = v[0];
        reinterpret_cast<lc_u32x4*>(row + n0)[1] = v[1];
    } else {
        for (int n = n0; n < nend; ++n)
            if (!((allowed >> (n - n0)) & 1u)) row[n] = ninf;
    }
    if (!a.argmax_partial) return;
    // the tile as this thread just stored it (its own stores, read back in program order), through the shared recomputation
    const float temp = ROWS ? row_sampling_temp(a.rows, b) : a.temperature;
    const uint64_t row_key = !(temp > 0.f) ? 0ull : ROWS ? row_sampling_key(a.rows, b) : sample_row_key(a.seed, a.step, b);
    uint64_t key;
    penalty_tile(row, a.V, tile, temp, row_key, &key, a.lse_partial ? a.lse_partial + t * 2 : nullptr);
    a.argmax_partial[t] = key;
}

// one thread per row
__global__ __launch_bounds__(UMV_WAVE) void constraint_advance_kernel(umv_token_automaton t, int32_t* __restrict__ state,
                                                                      const int64_t* __restrict__ ids, int M) {
    const int b = blockIdx.x * UMV_WAVE + threadIdx.x;
    if (b >= M) return;
    const int s = state[b];
    if (s < 0 || s >= t.n_states) return;
    int e0, e1;
    lc_edge_range(t, s, &e0, &e1);
    const int64_t id = ids[b];
    const int e = lc_lower_bound(t.edge_token, e0, e1, id);
    state[b] = (e < e1 && (int64_t)t.edge_token[e] == id) ? t.edge_next[e] : UMV_CONSTRAINT_LEFT;
}

static bool lc_finite(float v) { return v - v == 0.f; }      // false for NaN and +-inf

static bool lc_automaton_ok(const umv_token_automaton* t) {
    return t && t->row_ptr && t->n_states > 0 && t->n_edges >= 0 && (t->n_edges == 0 || (t->edge_token && t->edge_next));
}

extern "C" int umv_logit_constrain_bf16(const umv_logit_constrain_args* a, umv_stream_t stream) {
    UMV_CHECK(a && a->logits && a->M >= 0 && a->V > 0 && a->ld >= a->V, UMV_ERR_ARG, "logit_constrain: bad args");
    UMV_CHECK(lc_automaton_ok(&a->automaton) && a->state, UMV_ERR_ARG,
              "logit_constrain: the automaton needs row_ptr, n_states > 0, n_edges >= 0 and its edge arrays, and the rows their state words");
    UMV_CHECK(lc_finite(a->temperature) && a->temperature >= 0.f, UMV_ERR_ARG, "logit_constrain: temperature (%g) must be >= 0 (0 = greedy)",
              (double)a->temperature);
    UMV_CHECK(a->argmax_partial || !a->lse_partial, UMV_ERR_ARG, "logit_constrain: lse_partial goes with argmax_partial");
    if (a->argmax_partial)
        UMV_CHECK(a->V <= a->n_tiles * 16 && a->V > (a->n_tiles - 1) * 16, UMV_ERR_ARG,
                  "logit_constrain: V (%d) must be the column count behind the %d tiles", a->V, a->n_tiles);
    UMV_CHECK(!a->rows || a->temperature == 0.f, UMV_ERR_ARG,
              "logit_constrain: with rows (the per-row sampling table) the scalar temperature must be neutral (0)");
    UMV_CHECK(((uintptr_t)a->rows % 16) == 0, UMV_ERR_ARG, "logit_constrain: rows must be 16-byte aligned");
    UMV_CHECK(a->M <= 65535, UMV_ERR_ARG, "logit_constrain: at most 65535 rows per call (got %d)", a->M);
    if (a->M == 0) return UMV_OK;
    const dim3 grid((a->V + LC_CHUNK - 1) / LC_CHUNK, a->M);
    if (a->rows)
        hipLaunchKernelGGL(logit_constrain_kernel<true>, grid, dim3(LC_THREADS), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(logit_constrain_kernel<false>, grid, dim3(LC_THREADS), 0, (hipStream_t)stream, *a);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_constraint_advance(const umv_token_automaton* t, int32_t* state, const int64_t* ids, int M, umv_stream_t stream) {
    UMV_CHECK(lc_automaton_ok(t) && state && ids && M >= 0, UMV_ERR_ARG,
              "constraint_advance: the automaton needs row_ptr, n_states > 0, n_edges >= 0 and its edge arrays; state and ids one word per row");
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(constraint_advance_kernel, dim3((M + UMV_WAVE - 1) / UMV_WAVE), dim3(UMV_WAVE), 0, (hipStream_t)stream, *t, state, ids, M);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
