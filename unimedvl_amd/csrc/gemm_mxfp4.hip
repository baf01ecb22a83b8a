// MXFP4 weights for the decode GEMMs (gfx950): e2m1 codes with one E8M0 power-of-two scale per 32 consecutive k of a row (format and
// image: pack.hip, which makes it).  The decode kernel is the weight-streaming body (gemm_skinny.h) with the MXFP4 policy: the codes
// become bf16 in registers (v_cvt_scalef32_pk_bf16_fp4) and feed the same v_mfma_f32_16x16x32_bf16 with the same operands in the same
// k order as gemm_skinny_kernel on the bf16 image of W': for K % 512 == 0 and no split-K the results are bit-identical.
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "gemm_skinny.h"

// ----------------------------------------------------------------------------- decode GEMM (M <= 64)
// A workgroup owns NP tile PAIRS (NT = 2 NP n-tiles): at 4 bits x is the larger stream (M = 8: 16 B of x per k against 8.5 B of one
// 16-row tile), so each x fragment - staged once per wave slice as full 128-byte lines (XL) - feeds 2 NP tiles.  Split-K (a.k_splits)
// over blockIdx.y as in the other decode kernels.
template <int MB, int NP, int U, int XL = 0>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny4_kernel(umv_gemm_args a, int KT8, int NTT, int NPT) {
    gemm_skinny_body<SkMxfp4<NP>, MB, U, true, 0, XL>(a, KT8, NTT, NPT);
}

template <int MB, int NP, int U>
static int launch_skinny4(const umv_gemm_args& a, int KT8, int NTT, int NPT, hipStream_t s) {
    return launch_skinny_body<MB, 2 * NP, U, 2, 0>([](auto XL) { return &gemm_skinny4_kernel<MB, NP, U, decltype(XL)::value>; }, a, KT8,
                                                   NTT, s, KT8, NTT, NPT);
}

// U = super-tiles per chunk (double buffered): 1, or 2 for one pair.  Row tiles beyond one keep fewer pairs per workgroup: with
// MB = 4 and 2 pairs the registers spill
template <int NP>
static int launch_skinny4_m(const umv_gemm_args& a, int KT8, int NTT, int NPT, hipStream_t s) {
    if (a.M <= 16) return launch_skinny4<1, NP, NP == 1 ? 2 : 1>(a, KT8, NTT, NPT, s);
    if (a.M <= 32) return launch_skinny4<2, NP < 2 ? NP : 2, 1>(a, KT8, NTT, NPT, s);
    return launch_skinny4<4, 1, 1>(a, KT8, NTT, NPT, s);
}

extern "C" int umv_gemm_mxfp4w(const umv_gemm_args* ap, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm_mxfp4w: null args");
    umv_gemm_args a = *ap;
    UMV_CHECK(a.x && a.wp && a.out, UMV_ERR_ARG, "gemm_mxfp4w: null pointer (x, wp and out are required)");
    UMV_CHECK(!a.w_scale, UMV_ERR_ARG, "gemm_mxfp4w: w_scale must be NULL (the block scales are part of the MXFP4 image)");
    if (const int rc = umv_gemm_check_args(a, "gemm_mxfp4w", 32)) return rc;
    if (const int rc = umv_gemm_check_decode(a, "gemm_mxfp4w", "MXFP4", "the bf16 image of the dequantised weights with umv_gemm_bf16", false, false))
        return rc;
    if (a.M == 0) return UMV_OK;
    hipStream_t s = (hipStream_t)stream;
    const int KT8 = (a.K + 63) / 64, NTT = (a.N + 15) / 16, NPT = (NTT + 1) / 2;
    // tile pairs per workgroup: UMV_MXFP4_NP = 1 | 2 | 4 replaces the policy below (A/B only)
    static const int np_env = umv_env_int("UMV_MXFP4_NP", 0);
    int np = np_env;
    if (np != 1 && np != 2 && np != 4) np = (a.k_splits > 1 || NPT >= 512) ? 2 : 1;
    if (np == 4) return launch_skinny4_m<4>(a, KT8, NTT, NPT, s);
    if (np == 2) return launch_skinny4_m<2>(a, KT8, NTT, NPT, s);
    return launch_skinny4_m<1>(a, KT8, NTT, NPT, s);
}
