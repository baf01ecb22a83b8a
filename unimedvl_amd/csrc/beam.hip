// Beam search decode (include/unimedvl_hip.h, "beam search decode"): the three launches that end a step of K beams per request.
//   umv_beam_candidates  every row's 2K best columns with their log-probabilities: the top-n selection body (top_select.h), the
//                        statistics merged in the greedy step end's order - a row's candidate list is its top-n list bit for bit.
//   umv_beam_step_end    one workgroup per request: order the candidates, walk them, keep the finished list, decide "done", write the
//                        next live beams with their back-pointers, advance the counters, rewrite the request's K page-table rows and
//                        leave one (source page, destination page, tokens) copy per row.
//   umv_beam_kv_copy     grid (chunk, layer, row): the partially filled page of a row that changed its parent, K [tokens][hd] and
//                        V^T [hd][tokens] per kv head, 16 bytes per access.
#include "top_select.h"

// ----------------------------------------------------------------------------- candidates
__global__ __launch_bounds__(TR_THREADS) void beam_candidates_kernel(const bf16_t* __restrict__ logits, int64_t ldo, int V,
                                                                     const float* __restrict__ lse, int n_tiles, int n, int32_t* cand_ids,
                                                                     float* cand_lp, int32_t* rank) {
    __shared__ uint32_t hist[TR_BINS];
    __shared__ TruncShared sh;
    __shared__ TopShared ts;
    const int r = blockIdx.x;
    const bf16_t* row = logits + (int64_t)r * ldo;
    float ref, S;
    merge_tile_stats<TR_THREADS, 256>(reinterpret_cast<const umv_f32x2*>(lse) + (int64_t)r * n_tiles, n_tiles, sh.smf, ref, S);
    // greedy: the maximum of the statistics is the row's highest logit (ref == 0 may stand for a row of -inf only); no fed token
    top_select(row, V, 0.f, n, -1, ref, S, ref == 0.f ? NAN : ref, hist, sh, ts, {cand_ids + (int64_t)r * n, cand_lp + (int64_t)r * n, rank + r});
}

extern "C" int umv_beam_candidates(const uint16_t* logits, int64_t ldo, int V, const float* lse_partial, int n_tiles, int R, int n,
                                   int32_t* cand_ids, float* cand_lp, int32_t* rank, umv_stream_t stream) {
    UMV_CHECK(logits && lse_partial && cand_ids && cand_lp && rank && R >= 0, UMV_ERR_ARG, "beam_candidates: bad args");
    UMV_CHECK(n >= 2 && n <= UMV_TOP_LOGPROBS_MAX && (n & 1) == 0 && V > n, UMV_ERR_ARG,
              "beam_candidates: n (%d) must be 2K with 1 <= K <= %d, and V (%d) > n", n, UMV_BEAM_K_MAX, V);
    UMV_CHECK(n_tiles > 0 && V <= n_tiles * 16 && V > (n_tiles - 1) * 16 && ldo >= V, UMV_ERR_ARG,
              "beam_candidates: V (%d) must be the column count behind the %d tiles and ldo (%lld) >= V", V, n_tiles, (long long)ldo);
    if (R == 0) return UMV_OK;
    hipLaunchKernelGGL(beam_candidates_kernel, dim3(R), dim3(TR_THREADS), 0, (hipStream_t)stream, logits, ldo, V, lse_partial, n_tiles, n,
                       cand_ids, cand_lp, rank);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- step end
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_CAND = 2 * UMV_BEAM_K_MAX * UMV_BEAM_K_MAX;                      // candidates of a request: K lists of 2K
constexpr int BEAM_TABLE_PASSES = UMV_BEAM_TABLE_ENTRIES / BEAM_THREADS;              // full-page entries a thread carries over the barrier
static_assert(BEAM_CAND <= BEAM_THREADS, "one candidate per thread");
static_assert(UMV_BEAM_K_MAX * 4 <= BEAM_THREADS && UMV_BEAM_TABLE_ENTRIES % BEAM_THREADS == 0, "finished list and table by thread");

struct BeamShared {
    float total[BEAM_CAND], lp[BEAM_CAND];           // per candidate (beam * 2K + place in the beam's list)
    int32_t tok[BEAM_CAND];                          // -1: not a candidate
    int32_t ord[BEAM_CAND];                          // ord[r]: the candidate at place r of the request's order
    uint32_t n_cand;
    float fin_f[UMV_BEAM_K_MAX][4];                  // the finished list (score, total, last log-probability, -)
    int32_t fin_i[UMV_BEAM_K_MAX][4];                //                   (step, parent beam, last token, sequence number)
    int32_t n_fin, n_ever, done;
    int32_t live_tok[UMV_BEAM_K_MAX], live_parent[UMV_BEAM_K_MAX];
    float live_total[UMV_BEAM_K_MAX], live_lp[UMV_BEAM_K_MAX];
};

// Offer a finished hypothesis to the list: appended while there is room; a full list replaces its worst entry - lowest score, the
// latest among equals - only for a strictly better one.
__device__ __forceinline__ void beam_offer(BeamShared& sh, int K, float score, float total, float lp, int t, int parent, int tok) {
    int slot;
    if (sh.n_fin < K) {
        slot = sh.n_fin++;
    } else {
        slot = 0;
        for (int i = 1; i < K; ++i)
            if (sh.fin_f[i][0] < sh.fin_f[slot][0] || (sh.fin_f[i][0] == sh.fin_f[slot][0] && sh.fin_i[i][3] > sh.fin_i[slot][3])) slot = i;
        if (!(score > sh.fin_f[slot][0])) return;
    }
    sh.fin_f[slot][0] = score; sh.fin_f[slot][1] = total; sh.fin_f[slot][2] = lp; sh.fin_f[slot][3] = 0.f;
    sh.fin_i[slot][0] = t; sh.fin_i[slot][1] = parent; sh.fin_i[slot][2] = tok; sh.fin_i[slot][3] = sh.n_ever++;
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_step_end_kernel(const umv_beam_step_args a) {
    __shared__ BeamShared sh;
    const int b = blockIdx.x, t_ = threadIdx.x, K = a.K, n = 2 * a.K, R = a.B * a.K;
    const int row0 = b * K;
    int32_t* hdr = a.hdr + 4 * b;
    if (hdr[2]) return;                                  // a done request: no word is written (the same in every thread)
    const int64_t t = a.step_idx[row0];
    if (t < 0 || t >= a.max_len) return;
    const int L = a.tok_slot[row0] + 1;                  // the request's committed length after this step
    // ---- 1. the candidates with their totals; a beam at -inf contributes nothing
    bool valid = false;
    if (t_ < K * n) {
        const int row = row0 + t_ / n;
        const float s = a.scores[row];
        const int32_t id = a.cand_ids[(int64_t)row * n + t_ % n];
        const float lp = a.cand_lp[(int64_t)row * n + t_ % n];
        const float total = s + lp;
        valid = s > -INFINITY && id >= 0 && total == total;
        sh.total[t_] = total; sh.lp[t_] = lp; sh.tok[t_] = valid ? id : -1;
    }
    if (t_ < K * 4) {
        reinterpret_cast<float*>(sh.fin_f)[t_] = a.fin_f[(int64_t)row0 * 4 + t_];
        reinterpret_cast<int32_t*>(sh.fin_i)[t_] = a.fin_i[(int64_t)row0 * 4 + t_];
    }
    if (t_ == 0) { sh.n_cand = 0u; sh.n_fin = hdr[0]; sh.n_ever = hdr[1]; sh.done = 0; }
    __syncthreads();
    // ---- 2. the order: total descending, beam ascending, place in the beam's list ascending (the thread index is (beam, place))
    if (valid) {
        const float mine = sh.total[t_];
        int r = 0;
        for (int j = 0; j < K * n; ++j) r += (sh.tok[j] >= 0 && (sh.total[j] > mine || (sh.total[j] == mine && j < t_))) ? 1 : 0;
        sh.ord[r] = t_;
        atomicAdd(&sh.n_cand, 1u);
    }
    __syncthreads();
    // ---- 3.-5. walk, finished list, done: a few tens of dependent LDS steps, one thread
    if (t_ == 0) {
        const int nc = (int)sh.n_cand;
        const bool last = t + 1 == a.max_len;
        const float norm = a.len_norm[t];
        int nl = 0;
        for (int r = 0; r < nc; ++r) {
            const int c = sh.ord[r];
            const int tok = sh.tok[c];
            const bool is_end = tok == a.end_token_id;
            if (r < K && (is_end || last)) beam_offer(sh, K, sh.total[c] / norm, sh.total[c], sh.lp[c], (int)t, c / n, tok);
            if (!is_end && nl < K) {
                sh.live_tok[nl] = tok; sh.live_parent[nl] = c / n; sh.live_total[nl] = sh.total[c]; sh.live_lp[nl] = sh.lp[c];
                ++nl;
            }
            if (nl == K && r >= K - 1) break;
        }
        for (; nl < K; ++nl) {                           // fewer than K candidates in all (NaN rows): dead successors
            sh.live_tok[nl] = 0; sh.live_parent[nl] = nl; sh.live_total[nl] = -INFINITY; sh.live_lp[nl] = -INFINITY;
        }
        const bool full = sh.n_fin == K;
        bool done = full;
        if (full && !a.early_stopping) {
            float worst = sh.fin_f[0][0];
            for (int i = 1; i < K; ++i) worst = sh.fin_f[i][0] < worst ? sh.fin_f[i][0] : worst;
            done = worst >= sh.live_total[0] / norm;
        }
        sh.done = done ? 1 : 0;
    }
    __syncthreads();
    const bool done_now = sh.done != 0;
    // ---- the KV plan: read every word of the request's table rows that changes, barrier, then write
    const int j0 = a.j0[b], Lp = L >> 8, rem = L & 255;
    int nfull = Lp - j0;                                 // full private pages; never past the fork's horizon or the table row
    nfull = nfull > a.n_own ? a.n_own : nfull;
    nfull = nfull > a.table_stride - j0 ? a.table_stride - j0 : nfull;
    nfull = (nfull < 0 || j0 < 0) ? 0 : nfull;
    const int n_entries = done_now ? 0 : K * nfull;      // (the host keeps K * n_own within UMV_BEAM_TABLE_ENTRIES)
    int32_t carry[BEAM_TABLE_PASSES];
#pragma unroll
    for (int i = 0; i < BEAM_TABLE_PASSES; ++i) {
        const int e = t_ + i * BEAM_THREADS;
        carry[i] = 0;
        if (e < n_entries) carry[i] = a.table[(int64_t)(row0 + sh.live_parent[e / nfull]) * a.table_stride + j0 + e % nfull];
    }
    int32_t cp_src = 0, cp_dst = 0, cp_tokens = 0;
    if (t_ < K && !done_now) {
        const int p = sh.live_parent[t_], q = Lp - j0;
        if (rem != 0 && p != t_ && j0 >= 0 && q >= 0 && q < a.n_own && Lp < a.table_stride) {
            const int32_t cur = a.table[(int64_t)(row0 + t_) * a.table_stride + Lp];
            const int32_t* pair = a.own + ((int64_t)(row0 + t_) * a.n_own + q) * 2;
            cp_src = a.table[(int64_t)(row0 + p) * a.table_stride + Lp];
            cp_dst = pair[0] == cur ? pair[1] : pair[0];
            cp_tokens = (rem + 7) & ~7;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < BEAM_TABLE_PASSES; ++i) {
        const int e = t_ + i * BEAM_THREADS;
        if (e < n_entries) a.table[(int64_t)(row0 + e / nfull) * a.table_stride + j0 + e % nfull] = carry[i];
    }
    // ---- the rows' words
    if (t_ < K) {
        const int row = row0 + t_;
        if (cp_tokens) a.table[(int64_t)row * a.table_stride + Lp] = cp_dst;
        reinterpret_cast<u32x4*>(a.copies)[row] = (u32x4){(uint32_t)cp_src, (uint32_t)cp_dst, (uint32_t)cp_tokens, 0u};
        a.ids[row] = sh.live_tok[t_];
        a.beam_tok[t * R + row] = sh.live_tok[t_];
        a.beam_parent[t * R + row] = sh.live_parent[t_];
        a.beam_lp[t * R + row] = sh.live_lp[t_];
        a.scores[row] = sh.live_total[t_];
        a.tok_slot[row] += 1; a.tok_pos[row] += 1; a.kv_len[row] += 1;
        a.step_idx[row] = t + 1;
    }
    if (t_ < K * 4) {
        a.fin_f[(int64_t)row0 * 4 + t_] = reinterpret_cast<float*>(sh.fin_f)[t_];
        a.fin_i[(int64_t)row0 * 4 + t_] = reinterpret_cast<int32_t*>(sh.fin_i)[t_];
    }
    if (t_ == 0) reinterpret_cast<u32x4*>(hdr)[0] = (u32x4){(uint32_t)sh.n_fin, (uint32_t)sh.n_ever, (uint32_t)sh.done, 0u};
}

extern "C" int umv_beam_step_end(const umv_beam_step_args* a, umv_stream_t stream) {
    UMV_CHECK(a, UMV_ERR_ARG, "beam_step_end: null args");
    UMV_CHECK(a->tok_slot && a->tok_pos && a->kv_len && a->ids && a->step_idx && a->cand_ids && a->cand_lp && a->scores && a->beam_tok &&
                  a->beam_parent && a->beam_lp && a->fin_f && a->fin_i && a->hdr && a->len_norm && a->table && a->own && a->j0 && a->copies,
              UMV_ERR_ARG, "beam_step_end: null pointer");
    UMV_CHECK(a->B >= 0 && a->K >= 1 && a->K <= UMV_BEAM_K_MAX && a->max_len > 0, UMV_ERR_ARG,
              "beam_step_end: K (%d) must be in [1, %d], B (%d) >= 0, max_len (%d) > 0", a->K, UMV_BEAM_K_MAX, a->B, a->max_len);
    UMV_CHECK(a->table_stride > 0 && a->n_own > 0 && (int64_t)a->K * a->n_own <= UMV_BEAM_TABLE_ENTRIES, UMV_ERR_ARG,
              "beam_step_end: table_stride (%d) and n_own (%d) must be positive and K * n_own at most %d", a->table_stride, a->n_own,
              UMV_BEAM_TABLE_ENTRIES);
    UMV_CHECK(((uintptr_t)a->copies % 16) == 0 && ((uintptr_t)a->hdr % 16) == 0, UMV_ERR_ARG, "beam_step_end: copies and hdr must be 16-byte aligned");
    if (a->B == 0) return UMV_OK;
    hipLaunchKernelGGL(beam_step_end_kernel, dim3(a->B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, *a);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- KV copy
// 16-byte units of one (row, layer): per kv head tokens * hd / 8 contiguous units of K, then hd rows of tokens / 8 units of V^T.
__global__ __launch_bounds__(256) void beam_kv_copy_kernel(const int32_t* __restrict__ copies, const void* const* __restrict__ pools, int nkv,
                                                           int hd, int npages) {
    const u32x4 c = reinterpret_cast<const u32x4*>(copies)[blockIdx.z];
    const int tokens = (int)c[2];
    if (tokens <= 0) return;                             // nothing to copy: the same in every thread
    if (c[0] >= (uint32_t)npages || c[1] >= (uint32_t)npages || c[0] == c[1] || tokens > UMV_KV_PAGE || (tokens & 7)) return;
    const int64_t page_units = (int64_t)nkv * UMV_KV_PAGE * hd / 8;
    const u32x4* __restrict__ ks = reinterpret_cast<const u32x4*>(pools[2 * blockIdx.y]) + (int64_t)c[0] * page_units;
    const u32x4* __restrict__ vs = reinterpret_cast<const u32x4*>(pools[2 * blockIdx.y + 1]) + (int64_t)c[0] * page_units;
    u32x4* __restrict__ kd = reinterpret_cast<u32x4*>(const_cast<void*>(pools[2 * blockIdx.y])) + (int64_t)c[1] * page_units;
    u32x4* __restrict__ vd = reinterpret_cast<u32x4*>(const_cast<void*>(pools[2 * blockIdx.y + 1])) + (int64_t)c[1] * page_units;
    const int ku = tokens * hd / 8, vu = tokens / 8;
    const int total_k = nkv * ku, total = total_k + nkv * hd * vu;
    for (int u = blockIdx.x * 256 + threadIdx.x; u < total; u += gridDim.x * 256) {
        if (u < total_k) {
            const int idx = (u / ku) * (UMV_KV_PAGE * hd / 8) + u % ku;
            kd[idx] = ks[idx];
        } else {
            const int w = u - total_k;
            const int idx = (w / vu) * (UMV_KV_PAGE / 8) + w % vu;
            vd[idx] = vs[idx];
        }
    }
}

extern "C" int umv_beam_kv_copy(const int32_t* copies, const void* const* pools, int R, int layers, int nkv, int hd, int npages, int chunks,
                                umv_stream_t stream) {
    UMV_CHECK(copies && pools && R >= 0 && layers > 0 && nkv > 0 && hd > 0 && (hd % 8) == 0 && npages > 0, UMV_ERR_ARG,
              "beam_kv_copy: bad args (hd = %d must be a multiple of 8)", hd);
    UMV_CHECK(chunks >= 1 && chunks <= 64 && R <= 65535 && layers <= 65535, UMV_ERR_ARG, "beam_kv_copy: chunks (%d) must be in [1, 64]", chunks);
    UMV_CHECK(((uintptr_t)copies % 16) == 0, UMV_ERR_ARG, "beam_kv_copy: copies must be 16-byte aligned");
    if (R == 0) return UMV_OK;
    hipLaunchKernelGGL(beam_kv_copy_kernel, dim3(chunks, layers, R), dim3(256), 0, (hipStream_t)stream, copies, pools, nkv, hd, npages);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
