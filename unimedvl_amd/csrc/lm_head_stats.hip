// The prefill-time scorer's two kernels (include/unimedvl_hip.h, "token log-probabilities of given rows"):
//   * umv_lm_head_stats_bf16: the lm_head GEMM on the 8-wave MFMA tile of gemm_tiled.h - its frame and k-loop as they are - ending in
//     gemm_epilogue.h::epi_wave_tile_stats instead of a store epilogue: per row and 16-column tile the softmax statistics (m_t, s_t)
//     and, per row, the one logit the row is scored against.  No logits are written: 76 KB of statistics per row at V = 152 064 where
//     the logits are 304 KB, and no second pass over them.
//   * umv_token_logprob_from_stats: one workgroup per row merges the tiles in decode_step_end_logprob_kernel's order and finishes
//     with its function - the same statistics and y give that kernel's bits.
// Two tile shapes with x staged in full lines - 256(n) x 128(m) x 32 (the plain call's 368) and, from 1024 rows, 256 x 256 x 32 (its
// 366): N is the vocabulary, so any row count fills the chip, and few rows waste MFMA work, not bytes.  Every output is one accumulator chain over k in ascending 32-wide steps, as in
// every other kernel of the family: the logit behind the statistics is the bf16 value the plain call stores, whatever tile that takes.
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "block_reduce.h"
#include "gemm_epilogue.h"
#include "gemm_internal.h"
#include "gemm_tiled.h"
#include "token_pick.h"

template <int WN, int WM, int TN, int TM, int KTS, int NBUF, int SCHED>
__global__ __launch_bounds__(WN * WM * 64) void gemm_tiled_stats_kernel(umv_gemm_args a, int KT, int NTT, int mblocks, int nblocks, int gn,
                                                                        int ms, const int64_t* __restrict__ ids, float* __restrict__ lse,
                                                                        float* __restrict__ target_y) {
    using Cf = TiledCfg<WN, WM, TN, TM, KTS, NBUF, SCHED>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    TilePos p;      // the frame of gemm_tiled_kernel, without split-K
    p.lane = tid & 63;
    p.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    p.wn = p.wave % WN, p.wm = p.wave / WN;
    int mblk, nblk;
    umv_tile_order(mblocks, nblocks, gn, ms, (int)blockIdx.x, mblk, nblk);
    p.m0 = mblk * Cf::BM;
    p.nt_blk = nblk * (Cf::BN / 16);
    bf16_t* bias_lds = reinterpret_cast<bf16_t*>(smem + Cf::STAGE_BYTES);
    umv_bias_to_lds<Cf::BN, Cf::NW * 64>(a, bias_lds, p.nt_blk, tid);      // (the first barrier of the main loop orders it before the epilogue)
    p.kt0 = 0, p.kt1 = KT, p.KTL = KT;
    p.nsteps = (KT + KTS - 1) / KTS;

    f32x4 acc[TN][TM];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (SCHED == 3) tiled_loop_full_line<Cf>(a, smem, p, KT, NTT, acc);
    else if constexpr (SCHED == 1) tiled_loop_interleaved<Cf>(a, smem, p, KT, NTT, acc);
    else tiled_loop_plain<Cf>(a, smem, p, KT, NTT, acc);

    // compile-time accumulator indices (a runtime-indexed acc[][] would be demoted to scratch); the staging buffers are not reused
    epi_wave_tile_stats<TN, TM>(acc, p.lane, p.m0 + p.wm * TM * 16, a.M, a.N, p.nt_blk + p.wn * TN, NTT,
                                (a.epilogue & UMV_EPI_BIAS) ? bias_lds + p.wn * TN * 16 : nullptr, ids, lse, target_y);
}

// 8 waves as WN x WM, each TN x TM MFMA tiles, k-steps of 32, x staged in full lines
template <int WN, int WM, int TN, int TM>
static int launch_stats(const umv_gemm_args& a, const int64_t* ids, float* lse_partial, float* target_y, hipStream_t s) {
    using Cf = TiledCfg<WN, WM, TN, TM, 1, 4, 3>;
    const auto kernel = &gemm_tiled_stats_kernel<WN, WM, TN, TM, 1, 4, 3>;
    static bool attr_set[UMV_MAX_DEVICES] = {};
    if (umv_first_on_device(attr_set)) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, Cf::LDS_BYTES);
    }
    const int KT = (a.K + 31) / 32, NTT = (a.N + 15) / 16;
    const int mblocks = (a.M + Cf::BM - 1) / Cf::BM, nblocks = (a.N + Cf::BN - 1) / Cf::BN;
    hipLaunchKernelGGL(kernel, dim3(mblocks * nblocks), dim3(Cf::NW * 64), Cf::LDS_BYTES, s, a, KT, NTT, mblocks, nblocks, UMV_TILE_GN,
                       umv_tile_superblock(mblocks, Cf::BM, a.K), ids, lse_partial, target_y);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// Rows from which the 256 x 256 tile takes the call (below: 256(n) x 128(m)).  Measured on MI355X at the lm_head of the 14B model
// (152 064 x 3584; profiles/score_prefill_bench.json): 260 rows 0.489 ms with 256 x 128 against 0.556 with 256 x 256; two 1024-row
// passes and one of 8 rows 2.66 ms against 2.43.  Same MFMAs on the same operands in the same k order: the bits do not depend on it.
constexpr int STATS_TILE256_MIN_ROWS = 1024;

extern "C" int umv_lm_head_stats_bf16(const umv_gemm_args* ap, const int64_t* ids, float* lse_partial, float* target_y, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "lm_head_stats: null args");
    const umv_gemm_args a = *ap;      // (a.out may be NULL: nothing is stored there)
    UMV_CHECK(a.x && a.wp && ids && lse_partial && target_y, UMV_ERR_ARG, "lm_head_stats: null pointer (x, wp, ids, lse_partial and target_y are required)");
    if (const int rc = umv_gemm_check_args(a, "lm_head_stats", 8)) return rc;
    UMV_CHECK(!a.row_idx && !a.residual && a.k_splits <= 1 && !a.norm_w && (a.tile_rows == 0 || a.tile_rows == 16) &&
                  !(a.epilogue & ~UMV_EPI_BIAS) && !a.argmax_partial && a.sample_temperature == 0.f,
              UMV_ERR_UNSUPPORTED, "lm_head_stats: a plain lm_head call on the 16-row bf16 image (optional bias; no row_idx / residual / "
              "split-K / fused norm / other epilogue flags / argmax_partial / sample_temperature - the statistics and the target logit go "
              "to the arguments behind the struct)");
    if (a.M == 0) return UMV_OK;
    static const int tile = umv_env_int("UMV_LM_HEAD_STATS_TILE", 0);      // tuning only: 256 = the 256 x 256 tile at every row count, 128 = never
    if (tile == 256 || (tile != 128 && a.M >= STATS_TILE256_MIN_ROWS)) return launch_stats<2, 4, 8, 4>(a, ids, lse_partial, target_y, (hipStream_t)stream);
    return launch_stats<4, 2, 4, 4>(a, ids, lse_partial, target_y, (hipStream_t)stream);
}

// The finish: decode_step_end_logprob_kernel's merge and last line for a row whose y[id] the GEMM left in target_y.
__global__ __launch_bounds__(256) void token_logprob_from_stats_kernel(const float* __restrict__ lse, int n_tiles, const float* __restrict__ target_y,
                                                                       const int64_t* __restrict__ ids, int V, float* __restrict__ out) {
    __shared__ float smf[4];
    const int m = blockIdx.x;
    float ref, S;
    merge_tile_stats<256>(reinterpret_cast<const umv_f32x2*>(lse) + (int64_t)m * n_tiles, n_tiles, smf, ref, S);
    if (threadIdx.x == 0) {
        const int64_t id = ids[m];
        out[m] = (id >= 0 && id < V) ? logprob_finish(target_y[m], ref, S) : NAN;
    }
}

extern "C" int umv_token_logprob_from_stats(const float* lse_partial, int n_tiles, const float* target_y, const int64_t* ids, int V, float* out,
                                            int M, umv_stream_t stream) {
    UMV_CHECK(lse_partial && target_y && ids && out && M >= 0 && n_tiles > 0, UMV_ERR_ARG, "token_logprob_from_stats: bad args");
    UMV_CHECK(V > 0 && V <= n_tiles * 16 && V > (n_tiles - 1) * 16, UMV_ERR_ARG,
              "token_logprob_from_stats: V (%d) must be the column count behind the %d tiles", V, n_tiles);
    if (M == 0) return UMV_OK;
    hipLaunchKernelGGL(token_logprob_from_stats_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, lse_partial, n_tiles, target_y, ids, V, out);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
