// no_repeat_ngram_size on the stored bf16 logits of a decode step (include/unimedvl_hip.h, "no-repeat n-grams"): one small kernel
// between the lm_head GEMM (and the penalty kernel) and the step end.  Every row owns an ordered int32 history; the kernel appends the
// token the step is fed, finds every earlier occurrence of the history's last n - 1 tokens, stores -inf to the column of the token
// that followed it, and recomputes the per-tile argmax keys and softmax statistics of only the tiles it touched - with the functions
// the lm_head epilogue itself calls (penalty_tile.h), so that every step end reads what the GEMM would have left for the banned logits.
#include "penalty_tile.h"

#define LN_THREADS 256

// Does the n-gram that starts at hist[i] open with the suffix (n - 1 tokens, all of them inside the vocabulary)?  Integer compares only;
// a separator or an out-of-range entry equals no suffix token.
__device__ __forceinline__ bool ngram_prefix_matches(const int32_t* __restrict__ hist, const int32_t* suffix, int i, int n) {
    for (int j = 0; j < n - 1; ++j)
        if (hist[i + j] != suffix[j]) return false;
    return true;
}

// One workgroup per row.  ROWS: the temperature and the sampling key of row b come from a.rows[b] (per-row sampling parameters).
template <bool ROWS>
__global__ __launch_bounds__(LN_THREADS) void logit_ngram_ban_kernel(umv_ngram_ban_args a) {
    __shared__ int s_len;
    __shared__ int32_t s_suffix[UMV_NGRAM_MAX];
    const int b = blockIdx.x;
    int32_t* hist = a.hist + (int64_t)b * a.hist_ld;
    // ---- record: the token this step is fed, the start token and forced tokens included
    if (threadIdx.x == 0) {
        int len = a.hist_len[b];
        if (len >= 0) {
            if ((int64_t)len >= a.hist_ld) {
                len = UMV_NGRAM_FULL;              // no room: the row is off from now on, nothing is written at or beyond hist_ld
            } else {
                const int64_t id = a.ids[b];
                hist[len] = (id >= 0 && id <= 0x7FFFFFFFll) ? (int32_t)id : -1;      // (what is no column matches nothing)
                ++len;
            }
            a.hist_len[b] = len;
        }
        s_len = len;
    }
    __threadfence_block();
    __syncthreads();                 // thread 0's history store is visible to the workgroup
    const int L = s_len;
    const int n = a.row_n ? a.row_n[b] : a.n;
    if (L < 0 || n < 1 || n > UMV_NGRAM_MAX || L < n) return;      // off, recorded only, or too short (uniform: before any barrier)
    // ---- the suffix h[L - n + 1 .. L): a token of it outside the vocabulary matches nothing, so the row bans nothing
    if ((int)threadIdx.x < n - 1) s_suffix[threadIdx.x] = hist[L - n + 1 + threadIdx.x];
    __syncthreads();
    for (int j = 0; j < n - 1; ++j)
        if (s_suffix[j] < 0 || s_suffix[j] >= a.V) return;         // (uniform)
    bf16_t* row = a.logits + (int64_t)b * a.ld;
    const bf16_t ninf = 0xFF80;
    // ---- ban: the candidate starts 0 .. L - n, thread-strided; every match stores -inf to its follower's column
    for (int i = threadIdx.x; i <= L - n; i += LN_THREADS) {
        if (!ngram_prefix_matches(hist, s_suffix, i, n)) continue;
        const int32_t f = hist[i + n - 1];
        if (f >= 0 && f < a.V) row[f] = ninf;       // two matches with one follower store the same bits
    }
    if (!a.argmax_partial) return;
    // ---- tiles: the banned columns were stored by other threads - possibly other waves - of this workgroup: a workgroup-scope fence
    // and the barrier order ALL of the row's stores before the loads below; then the same scan again, each match recomputing its
    // follower's tile (matches that share a tile store the same bits)
    __threadfence_block();
    __syncthreads();
    const float temp = ROWS ? row_sampling_temp(a.rows, b) : a.temperature;
    const uint64_t row_key = !(temp > 0.f) ? 0ull : ROWS ? row_sampling_key(a.rows, b) : sample_row_key(a.seed, a.step, b);
    for (int i = threadIdx.x; i <= L - n; i += LN_THREADS) {
        if (!ngram_prefix_matches(hist, s_suffix, i, n)) continue;
        const int32_t f = hist[i + n - 1];
        if (f < 0 || f >= a.V) continue;
        const int tile = f >> 4;
        const int64_t t = (int64_t)b * a.n_tiles + tile;
        uint64_t key;
        penalty_tile(row, a.V, tile, temp, row_key, &key, a.lse_partial ? a.lse_partial + t * 2 : nullptr);
        a.argmax_partial[t] = key;
    }
}

static bool ln_finite(float v) { return v - v == 0.f; }      // false for NaN and +-inf

extern "C" int umv_logit_ngram_ban_bf16(const umv_ngram_ban_args* a, umv_stream_t stream) {
    UMV_CHECK(a && a->logits && a->M >= 0 && a->V > 0 && a->ld >= a->V, UMV_ERR_ARG, "logit_ngram_ban: bad args");
    UMV_CHECK(a->ids && a->hist && a->hist_len && a->hist_ld >= 1, UMV_ERR_ARG,
              "logit_ngram_ban: ids, hist and hist_len are needed, and hist_ld >= 1 (got %lld)", (long long)a->hist_ld);
    UMV_CHECK(a->n >= 0 && a->n <= UMV_NGRAM_MAX, UMV_ERR_ARG, "logit_ngram_ban: n (%d) must be in [0, %d] (0 = record only)", a->n,
              UMV_NGRAM_MAX);
    UMV_CHECK(ln_finite(a->temperature) && a->temperature >= 0.f, UMV_ERR_ARG, "logit_ngram_ban: temperature (%g) must be >= 0 (0 = greedy)",
              (double)a->temperature);
    UMV_CHECK(a->argmax_partial || !a->lse_partial, UMV_ERR_ARG, "logit_ngram_ban: lse_partial goes with argmax_partial");
    if (a->argmax_partial)
        UMV_CHECK(a->V <= a->n_tiles * 16 && a->V > (a->n_tiles - 1) * 16, UMV_ERR_ARG,
                  "logit_ngram_ban: V (%d) must be the column count behind the %d tiles", a->V, a->n_tiles);
    UMV_CHECK(!a->rows || a->temperature == 0.f, UMV_ERR_ARG,
              "logit_ngram_ban: with rows (the per-row sampling table) the scalar temperature must be neutral (0)");
    UMV_CHECK(((uintptr_t)a->rows % 16) == 0, UMV_ERR_ARG, "logit_ngram_ban: rows must be 16-byte aligned");
    if (a->M == 0) return UMV_OK;
    if (a->rows)
        hipLaunchKernelGGL(logit_ngram_ban_kernel<true>, dim3(a->M), dim3(LN_THREADS), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(logit_ngram_ban_kernel<false>, dim3(a->M), dim3(LN_THREADS), 0, (hipStream_t)stream, *a);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
