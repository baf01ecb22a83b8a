// MXFP4 weights on the MFMA-tiled path (M > 64, gfx950): the tiled GEMM that reads the MXFP4 image of pack.hip directly, so that an fp4
// linear needs no bf16 image of its dequantised weights W' for prefill, the flow passes and the 65..128-row decode step.
//
// Workgroup = WN(n) x WM(m) waves; a wave owns NP tile PAIRS (2 NP n-tiles of 16) x TM row tiles of 16.
//   * Everything arrives by LDS-DMA (global_load_lds), nothing passes through VGPRs on its way in, and the 4-bit codes are what is
//     staged: a quarter of the LDS bytes of a bf16 W tile.  One 1-KiB wave piece of the image is two n-tiles x two k halves of a 64-k
//     unit, already in MFMA A-fragment lane order, the pair's 64 scale bytes beside it, NW - 1 units ahead.  After the ds_read,
//     v_cvt_scalef32_pk_bf16_fp4 turns a lane's 16 bytes into its four bf16 fragments (cvt_fp4x8 / e8m0_scale of quant.h, as
//     SkMxfp4::frags does).
//   * x (BM rows x 64 k = 16 KiB per unit) : a 1-KiB piece gathers 16 rows x 64 bytes with per-lane addresses and lands in B-fragment
//     order, 3 slots, one barrier per unit; every fragment read is a lane-linear ds_read_b128.
//   * v_mfma_f32_16x16x32_bf16, one accumulator chain per output over k in ascending 32-wide steps, epilogue of gemm_epilogue.h: the
//     operands, the order and the roundings of the tiled bf16 family on the bf16 image of W' - results are bit-identical to
//     umv_gemm_bf16(x, pack(W')) for every M > 64, split-K partials included.
// Per 64-k unit a wave issues 2 TM + 2 NP fragment reads for 4 NP TM MFMAs (the bf16 tiles: TN + TM reads for TN TM MFMAs per 32 k),
// and the reads of one k half are in flight while the MFMAs of the other run.
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "gemm_epilogue.h"
#include "gemm_internal.h"
#include "quant.h"

// NX / NW = slots of the x / W rings (NX - 1 units of x, NW - 1 units of codes + scales in flight)
template <int WN, int WM, int NP, int TM, int NX_, int NW>
struct T4Cfg {
    static constexpr int NWV = WN * WM;                      // waves per workgroup
    static constexpr int TN = 2 * NP, BM = WM * TM * 16;
    static constexpr int PPB = WN * NP;                     // tile pairs per workgroup
    static constexpr int SPW = PPB / NWV;              // ... staged per wave
    static constexpr int XT = 2 * WM * TM;                  // 1 KiB x fragment tiles per unit: [k half][row tile]
    static constexpr int XPW = XT / NWV;               // ... staged per wave
    static constexpr int NX = NX_;
    static constexpr int XSLOT = XT * 1024;
    static constexpr int WSLOT = PPB * (1024 + 256);        // PPB code KiB, then PPB x 64 lanes x 4 scale bytes
    static constexpr int WBASE = NX * XSLOT;
    static constexpr int STAGE_BYTES = WBASE + NW * WSLOT;
    static constexpr int EPI_BYTES = NWV * TN * TM * 512;
    static constexpr int LDS_BYTES = STAGE_BYTES > EPI_BYTES ? STAGE_BYTES : EPI_BYTES;
    static constexpr int PX = XPW, PW = 2 * SPW;            // LDS-DMA pieces per wave and unit
    static constexpr int WAIT = PW + (NX - 2) * (PX + PW);  // pieces a wave has issued behind its pieces of x(t) when it enters unit t
    static_assert(XT % NWV == 0 && PPB % NWV == 0 && NX >= 3 && NW > NX, "even split of the pieces over the waves; W at least as far ahead as x");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// Pipeline (everything arrives by LDS-DMA, so the counted waits are exact; units past the end of the K range re-fetch the last one - in
// bounds, never read - so that every wave issues the same pieces at every step).  enter(t), between the two k halves of unit t-1:
//     s_waitcnt vmcnt(WAIT)        my pieces of x(t) have landed, and W(t), issued NW - NX steps before them; what was issued behind them may fly
//     s_waitcnt lgkmcnt(0)         my fragment reads of x(t-1) are complete
//     s_barrier                    everyone's pieces of x(t) / W(t) landed AND everyone finished reading unit t-1, whose slots
//     issue x(t+NX-1), W(t+NW-1)   the pieces these slots take (the other wave of the SIMD has the matrix pipe meanwhile)
//     ds_read codes + scales of W(t) and the x fragments of its first k half      (in flight during the MFMAs of the second half of t-1)
// and at the head of unit t: ds_read the x fragments of the second half (in flight during the MFMAs of the first),
// v_cvt_scalef32_pk_bf16_fp4 -> 4 NP A fragments.
template <int WN, int WM, int NP, int TM, int NX_, int NW>
__global__ __launch_bounds__(WN * WM * 64) void gemm_mxfp4t_kernel(umv_gemm_args a, int KT, int KT8, int NTT, int NPT, int mblocks,
                                                                   int nblocks, int gn, int ms, int ksplit) {
    using Cf = T4Cfg<WN, WM, NP, TM, NX_, NW>;
    constexpr int TN = Cf::TN, BM = Cf::BM, XPW = Cf::XPW, NX = Cf::NX, PPB = Cf::PPB, SPW = Cf::SPW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave % WN, wm = wave / WN;
    const int r = lane & 15, g = lane >> 4;
    int mblk, nblk;
    umv_tile_order(mblocks, nblocks, gn, ms, (int)blockIdx.x, mblk, nblk);
    const int m0 = mblk * BM;
    const int nt_base = 2 * (nblk * PPB + wn * NP);  // this wave's first n-tile
    // split-K (ksplit = k-tiles of 32 per split, 0 = none): blockIdx.y owns k-tiles [kt0, kt1) - the ranges of umv_gemm_bf16's 65..128-row tile
    const int kt0 = ksplit ? min(KT, (int)blockIdx.y * ksplit) : 0;
    const int kt1 = ksplit ? min(KT, kt0 + ksplit) : KT;
    const int u0 = kt0 >> 1, u1 = (kt1 + 1) >> 1;    // the 64-k units that hold them; a half outside [kt0, kt1) is skipped

    // ---- W: codes C[p][kt8][lane][16 B], scales S[p][kt8][r][4 B] behind them (pack.hip); wave w stages pairs w * SPW .. of the workgroup's PPB
    const uint8_t* img = reinterpret_cast<const uint8_t*>(a.wp);
    const uint8_t* wbase[SPW];
    const uint8_t* sbase[SPW];
#pragma unroll
    for (int i = 0; i < SPW; ++i) {
        const int pg = nblk * PPB + wave * SPW + i;
        const int p = pg < NPT ? pg : 0;             // pairs past the end re-read pair 0; their columns are never stored
        wbase[i] = img + ((int64_t)p * KT8 * 64 + lane) * 16;
        sbase[i] = img + (int64_t)NPT * KT8 * 1024 + ((int64_t)p * KT8 * 16 + r) * 4;      // the four quarter waves fetch the same 64 bytes
    }
    // ---- x: tile f = wave * XPW + i is row tile f >> 1, k half f & 1 (the two half lines of a row are requested back to back); a lane
    // brings row r, 16 bytes at k = g * 8 of its k-tile, so the KiB lands in B-fragment order
    const bf16_t* xsrc[XPW];
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
        const int f = wave * XPW + i;
        const int m = m0 + (f >> 1) * 16 + r;
        const int mm = m < a.M ? m : a.M - 1;        // rows past M are clamped (their outputs are masked)
        const int64_t row = a.row_idx ? (int64_t)a.row_idx[mm] : (int64_t)mm;
        xsrc[i] = a.x + row * a.ldx + g * 8;
    }
    // G(t) = the pieces issued behind the barrier of enter(t): x(t+NX-1) into the slot of x(t-1), then W(t+NW-1) into the slot of W(t-1).
    // A unit past the K range re-fetches the last one; so does a k-tile past K (its half is skipped).
    auto stage_x = [&](int t) {
        const int u = t + NX - 1, uu = u < u1 ? u : u1 - 1;
        char* dst = smem + ((u - u0) % NX) * Cf::XSLOT;
#pragma unroll
        for (int i = 0; i < XPW; ++i) {
            const int f = wave * XPW + i;
            const int kt = min(2 * uu + (f & 1), KT - 1);
            __builtin_amdgcn_global_load_lds((const void*)(xsrc[i] + (int64_t)kt * 32), (umv_lds_ptr_t)(dst + ((f & 1) * (WM * TM) + (f >> 1)) * 1024), 16,
                                             0, 0);
        }
    };
    auto stage_w = [&](int t) {
        const int u = t + NW - 1, uu = u < u1 ? u : u1 - 1;
        char* dst = smem + Cf::WBASE + ((u - u0) % NW) * Cf::WSLOT;
#pragma unroll
        for (int i = 0; i < SPW; ++i) {
            const int sp = wave * SPW + i;
            __builtin_amdgcn_global_load_lds((const void*)(wbase[i] + (int64_t)uu * 1024), (umv_lds_ptr_t)(dst + sp * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)(sbase[i] + (int64_t)uu * 64), (umv_lds_ptr_t)(dst + PPB * 1024 + sp * 256), 4, 0, 0);
        }
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (u0 < u1) {                                   // (an empty K range of a split: zeros)
        u32x4 q[NP];
        uint32_t sc[NP];
        bf16x8 xf[2][TM];
        auto enter = [&](int u) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Cf::WAIT) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            UMV_BARRIER();
            stage_x(u);
            stage_w(u);
            const char* wb = smem + Cf::WBASE + ((u - u0) % NW) * Cf::WSLOT + (wn * NP) * 1024;
            const char* xb = smem + ((u - u0) % NX) * Cf::XSLOT + (wm * TM) * 1024 + lane * 16;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                q[i] = *reinterpret_cast<const u32x4*>(wb + i * 1024 + lane * 16);
                sc[i] = *reinterpret_cast<const uint32_t*>(wb + (PPB - wn * NP) * 1024 + (wn * NP + i) * 256 + lane * 4);
            }
#pragma unroll
            for (int j = 0; j < TM; ++j) xf[0][j] = *reinterpret_cast<const bf16x8*>(xb + j * 1024);
            __builtin_amdgcn_sched_barrier(0);
        };
        // prologue: W(0) .. W(NW-2) and x(0) .. x(NX-2) in the order the groups G(-NW+1) .. G(-1) would have issued them - every x(t)
        // behind W(t+NW-NX)
        static_for<0, NW - 1>([&](auto T) {
            constexpr int tt = decltype(T)::value;
            if constexpr (tt >= NW - NX) stage_x(u0 - (NW - 1) + tt);
            stage_w(u0 - (NW - 1) + tt);
        });
        enter(u0);
        for (int u = u0; u < u1; ++u) {
            const char* xb = smem + ((u - u0) % NX) * Cf::XSLOT + (WM * TM + wm * TM) * 1024 + lane * 16;
#pragma unroll
            for (int j = 0; j < TM; ++j) xf[1][j] = *reinterpret_cast<const bf16x8*>(xb + j * 1024);
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 wf[2][TN];
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                wf[0][2 * i] = cvt_fp4x8(q[i].x, e8m0_scale(sc[i] & 0xFFu));
                wf[1][2 * i] = cvt_fp4x8(q[i].y, e8m0_scale((sc[i] >> 8) & 0xFFu));
                wf[0][2 * i + 1] = cvt_fp4x8(q[i].z, e8m0_scale((sc[i] >> 16) & 0xFFu));
                wf[1][2 * i + 1] = cvt_fp4x8(q[i].w, e8m0_scale(sc[i] >> 24));
            }
            if (2 * u >= kt0) {                      // uniform: the first / last unit of a K range may hold one k-tile of it
#pragma unroll
                for (int j = 0; j < TM; ++j)
#pragma unroll
                    for (int t = 0; t < TN; ++t) acc[t][j] = mfma16(wf[0][t], xf[0][j], acc[t][j]);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (u + 1 < u1) enter(u + 1);
            if (2 * u + 1 < kt1) {
#pragma unroll
                for (int j = 0; j < TM; ++j)
#pragma unroll
                    for (int t = 0; t < TN; ++t) acc[t][j] = mfma16(wf[1][t], xf[1][j], acc[t][j]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the surplus pieces: the epilogue reuses the staging area
    }
    UMV_BARRIER();

    // ---- epilogue (gemm_epilogue.h), as gemm_tiled_kernel: bf16 outputs leave through LDS as whole rows, fp32 outputs directly
    EpiCtx e{a.bias, a.residual, a.ldr, a.out, a.ldo, a.N, a.epilogue};
    if (ksplit) {   // partial sums: fp32, no bias / activation / residual (umv_qkv_post / umv_residual_rmsnorm_bf16 finish the row)
        e.out = reinterpret_cast<float*>(a.out) + (int64_t)blockIdx.y * a.split_stride;
        e.flags = UMV_EPI_OUT_F32;
    }
    const int m_wave0 = m0 + wm * TM * 16;
    if (e.flags & UMV_EPI_OUT_F32) epi_wave_tile_direct<TN, TM>(e, acc, lane, m_wave0, a.M, a.row_idx, nt_base, NTT);
    else epi_wave_tile_lds<TN, TM>(e, acc, smem + wave * (TN * TM * 512), lane, m_wave0, a.M, a.row_idx, nt_base, NTT);
}

template <int WN, int WM, int NP, int TM, int NX_, int NW>
static int launch_mxfp4t(const umv_gemm_args& a, hipStream_t s) {
    using Cf = T4Cfg<WN, WM, NP, TM, NX_, NW>;
    constexpr int BM = Cf::BM;
    static bool attr_set[UMV_MAX_DEVICES] = {};
    if (umv_first_on_device(attr_set))
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_mxfp4t_kernel<WN, WM, NP, TM, NX_, NW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            Cf::LDS_BYTES);
    const int KT = a.K / 32, KT8 = (a.K + 63) / 64, NTT = (a.N + 15) / 16, NPT = (NTT + 1) / 2;
    const int mblocks = (a.M + BM - 1) / BM, nblocks = (NPT + Cf::PPB - 1) / Cf::PPB;
    const int splits = a.k_splits > 1 ? a.k_splits : 1;
    const int ksplit = splits > 1 ? (KT + splits - 1) / splits : 0;     // k-tiles per split: umv_gemm_bf16's ranges (its split-K tile steps by one k-tile)
    hipLaunchKernelGGL((gemm_mxfp4t_kernel<WN, WM, NP, TM, NX_, NW>), dim3(mblocks * nblocks, splits), dim3(Cf::NWV * 64), Cf::LDS_BYTES, s, a, KT,
                       KT8, NTT, NPT, mblocks, nblocks, UMV_TILE_GN, umv_tile_superblock(mblocks, BM, a.K), ksplit);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_gemm_mxfp4t(const umv_gemm_args* ap, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm_mxfp4t: null args");
    umv_gemm_args a = *ap;
    UMV_CHECK(a.x && a.wp && a.out, UMV_ERR_ARG, "gemm_mxfp4t: null pointer (x, wp and out are required)");
    UMV_CHECK(!a.w_scale, UMV_ERR_ARG, "gemm_mxfp4t: w_scale must be NULL (the block scales are part of the MXFP4 image)");
    if (const int rc = umv_gemm_check_args(a, "gemm_mxfp4t", 32)) return rc;
    UMV_CHECK(a.M > 64, UMV_ERR_UNSUPPORTED, "gemm_mxfp4t: the tiled MXFP4 kernel takes M > 64; use the weight-streaming kernel "
              "umv_gemm_mxfp4w for M=%d", a.M);
    UMV_CHECK(!a.norm_w, UMV_ERR_UNSUPPORTED, "gemm_mxfp4t: no fused norm (a decode prologue, M <= 16: umv_gemm_bf16 on a bf16 image)");
    UMV_CHECK(a.tile_rows == 0 || a.tile_rows == 16, UMV_ERR_UNSUPPORTED, "gemm_mxfp4t: no th-row tiles (a bf16 decode layout: umv_gemm_bf16)");
    UMV_CHECK(!a.argmax_partial, UMV_ERR_UNSUPPORTED, "gemm_mxfp4t: no argmax_partial (lm_head stays e4m3: umv_gemm_fp8w)");
    UMV_CHECK(a.k_splits <= 1 || (a.M <= 128 && !(a.epilogue & UMV_EPI_SWIGLU) && a.split_stride > 0 && a.k_splits <= 64),
              UMV_ERR_UNSUPPORTED, "gemm_mxfp4t: split-K (k_splits=%d) is a decode mode: M <= 128, no SwiGLU, split_stride > 0, k_splits <= 64",
              a.k_splits);
    hipStream_t s = (hipStream_t)stream;
    // Every wave owns 64 x 64 (two pairs x four row tiles) and a SIMD holds two of them: a wave that issues LDS-DMA pieces or converts is
    // off the matrix pipe, and with one wave per SIMD (128 x 64 per wave was tried) nothing fills the gap.  Few rows (the 65..128-row decode
    // step, short prefills): 128 x 128, 2 x 2 waves, 78 KiB of LDS - two workgroups per CU.  More rows: 256(n) x 128, 4 x 2 waves.
    const int NPT = ((a.N + 15) / 16 + 1) / 2;
    const long wg256 = (long)((a.M + 127) / 128) * ((NPT + 7) / 8);
    if (a.M <= 128 || wg256 < 256) return launch_mxfp4t<2, 2, 2, 4, 3, 6>(a, s);
    return launch_mxfp4t<4, 2, 2, 4, 3, 4>(a, s);
}
