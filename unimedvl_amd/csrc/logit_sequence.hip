// bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens on the stored bf16 logits of a decode step
// (include/unimedvl_hip.h, "banned sequences"): one small kernel behind the lm_head GEMM, the penalty kernel and the n-gram ban, before
// the constraint mask and the step end.  Every row owns a count and the last 15 tokens it was fed; the kernel records the token the step
// is fed, walks a static table of token sequences, stores -inf to the last token's column of every entry that is active and whose
// first m - 1 tokens are the row's last m - 1, and recomputes the per-tile argmax keys and softmax statistics of only the tiles it
// touched - with the functions the lm_head epilogue itself calls (penalty_tile.h).  logit_ngram.hip's structure.  The beam
// instantiation owns no state: a row's count is its step number + 1 and its tail a short walk over the search's back-pointers.
#include "penalty_tile.h"

#define LS_THREADS 256
#define LS_TAIL (UMV_SEQ_MAX - 1)

// a fed token as a history word: what is no int32 column matches nothing
__device__ __forceinline__ int32_t seq_history_word(int64_t id) { return (id >= 0 && id <= 0x7FFFFFFFll) ? (int32_t)id : -1; }

// The column entry s bans for a row with `count` tokens fed and the tail `tail` (LDS, most recent last), or -1.  Integer compares only.
__device__ __forceinline__ int sequence_entry_bans(const umv_sequence_ban_args& a, int s, int count, int row_min, const int32_t* tail) {
    const int32_t until = a.seq_until[s];
    const int limit = until == UMV_SEQ_ROW ? row_min : until;       // (row_min is 0 where there is none: never active)
    if (until < UMV_SEQ_ROW || (until != 0 && count > limit)) return -1;
    const int p0 = a.seq_ptr[s], m = a.seq_ptr[s + 1] - p0;
    if (m < 1 || m > UMV_SEQ_MAX || p0 < 0 || p0 > a.n_tok - m || m - 1 > count) return -1;
    for (int j = 0; j < m - 1; ++j) {
        const int32_t h = tail[LS_TAIL - (m - 1) + j];
        if (h < 0 || h >= a.V || h != a.seq_tok[p0 + j]) return -1;
    }
    const int32_t col = a.seq_tok[p0 + m - 1];
    return (col >= 0 && col < a.V) ? col : -1;
}

// One workgroup per row.  ROWS: the temperature and the sampling key of row b come from a.rows[b] (per-row sampling parameters).
// BEAM: the row is beam b % K of request b / K; its history comes from the back-pointers and nothing is recorded.
template <bool ROWS, bool BEAM>
__global__ __launch_bounds__(LS_THREADS) void logit_sequence_ban_kernel(umv_sequence_ban_args a) {
    __shared__ int s_count;
    __shared__ int32_t s_tail[LS_TAIL];
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int count;
        if (BEAM) {
            const int64_t t = a.step_idx[b];
            for (int j = 0; j < LS_TAIL; ++j) s_tail[j] = -1;
            if (t < 0 || t >= a.max_len) {
                count = -1;                                         // no step of this search: the row bans nothing
            } else {
                count = (int)t + 1;
                const int need = a.max_m - 1;                       // tokens the longest entry compares (<= LS_TAIL)
                const int base = b - b % a.K;
                int beam = b % a.K;
                if (need >= 1) s_tail[LS_TAIL - 1] = seq_history_word(a.ids[b]);
                for (int d = 1; d < need; ++d) {
                    const int pos = (int)t - d;                     // the history index of this token: 0 is the start token
                    if (pos < 0) break;
                    if (pos == 0) {
                        s_tail[LS_TAIL - 1 - d] = seq_history_word(a.start_ids[b / a.K]);
                        break;
                    }
                    beam = a.beam_parent[(int64_t)pos * a.M + base + beam];
                    if (beam < 0 || beam >= a.K) break;             // no beam of this request: the walk ends
                    s_tail[LS_TAIL - 1 - d] = a.beam_tok[(int64_t)(pos - 1) * a.M + base + beam];
                }
            }
        } else {
            // ---- record: the token this step is fed, the start token and forced tokens included
            int32_t* tail = a.tail + (int64_t)b * LS_TAIL;
            count = a.count[b];
            if (count >= 0) {
                for (int j = 0; j < LS_TAIL - 1; ++j) s_tail[j] = tail[j + 1];
                s_tail[LS_TAIL - 1] = seq_history_word(a.ids[b]);
                for (int j = 0; j < LS_TAIL; ++j) tail[j] = s_tail[j];
                if (count < 0x7FFFFFFF) ++count;
                a.count[b] = count;
            }
        }
        s_count = count;
    }
    __syncthreads();                 // thread 0's LDS words are visible to the workgroup
    const int count = s_count;
    if (count < 0 || a.S == 0) return;                              // off, or recorded only (uniform: before any barrier)
    const int row_min = a.row_min ? a.row_min[b] : 0;
    bf16_t* row = a.logits + (int64_t)b * a.ld;
    const bf16_t ninf = 0xFF80;
    // ---- ban: the entries thread-strided; every match stores -inf to its last token's column
    for (int s = threadIdx.x; s < a.S; s += LS_THREADS) {
        const int col = sequence_entry_bans(a, s, count, row_min, s_tail);
        if (col >= 0) row[col] = ninf;              // two entries with one column store the same bits
    }
    if (!a.argmax_partial) return;
    // ---- tiles: the banned columns were stored by other threads - possibly other waves - of this workgroup: a workgroup-scope fence
    // and the barrier order ALL of the row's stores before the loads below; then the same scan again, each match recomputing its
    // column's tile (matches that share a tile store the same bits)
    __threadfence_block();
    __syncthreads();
    const float temp = ROWS ? row_sampling_temp(a.rows, b) : a.temperature;
    const uint64_t row_key = !(temp > 0.f) ? 0ull : ROWS ? row_sampling_key(a.rows, b) : sample_row_key(a.seed, a.step, b);
    for (int s = threadIdx.x; s < a.S; s += LS_THREADS) {
        const int col = sequence_entry_bans(a, s, count, row_min, s_tail);
        if (col < 0) continue;
        const int tile = col >> 4;
        const int64_t t = (int64_t)b * a.n_tiles + tile;
        uint64_t key;
        penalty_tile(row, a.V, tile, temp, row_key, &key, a.lse_partial ? a.lse_partial + t * 2 : nullptr);
        a.argmax_partial[t] = key;
    }
}

static bool ls_finite(float v) { return v - v == 0.f; }      // false for NaN and +-inf

extern "C" int umv_logit_sequence_ban_bf16(const umv_sequence_ban_args* a, umv_stream_t stream) {
    UMV_CHECK(a && a->logits && a->M >= 0 && a->V > 0 && a->ld >= a->V, UMV_ERR_ARG, "logit_sequence_ban: bad args");
    UMV_CHECK(a->S >= 0 && a->S <= UMV_SEQ_ENTRIES_MAX, UMV_ERR_ARG, "logit_sequence_ban: S (%d) must be in [0, %d]", a->S,
              UMV_SEQ_ENTRIES_MAX);
    UMV_CHECK(a->S == 0 || (a->seq_ptr && a->seq_tok && a->seq_until), UMV_ERR_ARG,
              "logit_sequence_ban: seq_ptr, seq_tok and seq_until are needed with S > 0");
    UMV_CHECK(a->n_tok >= a->S && (int64_t)a->n_tok <= (int64_t)a->S * UMV_SEQ_MAX, UMV_ERR_ARG,
              "logit_sequence_ban: n_tok (%d) must be in [S, S * %d] (S = %d)", a->n_tok, UMV_SEQ_MAX, a->S);
    UMV_CHECK(a->max_m >= (a->S ? 1 : 0) && a->max_m <= UMV_SEQ_MAX, UMV_ERR_ARG,
              "logit_sequence_ban: max_m (%d) must be the longest entry's length, at most %d", a->max_m, UMV_SEQ_MAX);
    UMV_CHECK(a->ids, UMV_ERR_ARG, "logit_sequence_ban: ids are needed");
    if (a->K == 0) {
        UMV_CHECK(a->tail && a->count, UMV_ERR_ARG, "logit_sequence_ban: the plain form needs tail and count");
    } else {
        UMV_CHECK(a->K >= 1 && a->K <= UMV_BEAM_K_MAX, UMV_ERR_ARG, "logit_sequence_ban: K (%d) must be in [1, %d] (0 = the plain form)",
                  a->K, UMV_BEAM_K_MAX);
        UMV_CHECK(a->beam_tok && a->beam_parent && a->step_idx && a->start_ids, UMV_ERR_ARG,
                  "logit_sequence_ban: the beam form needs beam_tok, beam_parent, step_idx and start_ids");
        UMV_CHECK(a->M % a->K == 0 && a->max_len >= 1, UMV_ERR_ARG,
                  "logit_sequence_ban: the beam form needs M (%d) a multiple of K (%d) and max_len (%d) >= 1", a->M, a->K, a->max_len);
        UMV_CHECK(!a->rows, UMV_ERR_ARG, "logit_sequence_ban: the beam form is greedy, rows must be NULL");
    }
    UMV_CHECK(ls_finite(a->temperature) && a->temperature >= 0.f, UMV_ERR_ARG,
              "logit_sequence_ban: temperature (%g) must be >= 0 (0 = greedy)", (double)a->temperature);
    UMV_CHECK(a->argmax_partial || !a->lse_partial, UMV_ERR_ARG, "logit_sequence_ban: lse_partial goes with argmax_partial");
    if (a->argmax_partial)
        UMV_CHECK(a->V <= a->n_tiles * 16 && a->V > (a->n_tiles - 1) * 16, UMV_ERR_ARG,
                  "logit_sequence_ban: V (%d) must be the column count behind the %d tiles", a->V, a->n_tiles);
    UMV_CHECK(!a->rows || a->temperature == 0.f, UMV_ERR_ARG,
              "logit_sequence_ban: with rows (the per-row sampling table) the scalar temperature must be neutral (0)");
    UMV_CHECK(((uintptr_t)a->rows % 16) == 0, UMV_ERR_ARG, "logit_sequence_ban: rows must be 16-byte aligned");
    if (a->M == 0) return UMV_OK;
    if (a->K)
        hipLaunchKernelGGL((logit_sequence_ban_kernel<false, true>), dim3(a->M), dim3(LS_THREADS), 0, (hipStream_t)stream, *a);
    else if (a->rows)
        hipLaunchKernelGGL((logit_sequence_ban_kernel<true, false>), dim3(a->M), dim3(LS_THREADS), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL((logit_sequence_ban_kernel<false, false>), dim3(a->M), dim3(LS_THREADS), 0, (hipStream_t)stream, *a);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
