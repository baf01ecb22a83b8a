// The exact 13-bit image of bf16 weights for the decode GEMMs (gfx950); format and packer: include/unimedvl_hip.h, pack.hip.  The kernel
// is the weight-streaming body (gemm_skinny.h) with the SkZ13 policy: the planes become the bf16 A-fragments in registers and feed the
// same v_mfma_f32_16x16x32_bf16 with the same operands over the same K slices in the same k order as gemm_skinny_kernel on the bf16
// image, so the results are that kernel's bits for every M, K split and epilogue.
//
// A (tile pair, 512-k block) that holds a weight the format cannot code is flagged in the image.  A workgroup ORs the flags of its
// pairs over its K range first; if any is set the WHOLE workgroup runs the bf16 body on the bf16 image (a.wp) instead - one
// workgroup-uniform branch around two complete bodies, nothing conditional among the loads.
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "gemm_skinny.h"

// One text for the two kernels: gemm_skinny13_kernel, and gemm_skinny13_rows_kernel - the lm_head call with a per-row sampling table
// (umv_gemm_z13w_rows, ROWS of gemm_skinny.h; the kernel without ROWS gets a NULL table it never reads).  (A macro, not a shared __device__ function: with the arguments taken by reference there the
// existing kernels came out with other scalar registers.)
#define UMV_SKINNY13_KERNEL(NAME, ROWS, ROWS_ARG, ROWS_USE)                                                                                                 \
    template <int MB, int NP, int U, int XL = 0>                                                                                        \
    __global__ __launch_bounds__(SK_WAVES * 64) void NAME(umv_gemm_args a, const uint8_t* z13, int KT8, int NTT, int NPT ROWS_ARG) {   \
        /* the workgroup's K range in 512-k blocks: SkBf16's split over 32-k tiles */                                                   \
        const int KT = 2 * KT8, nsplit = a.k_splits > 1 ? a.k_splits : 1;                                                               \
        const int kts = (KT + nsplit - 1) / nsplit;                                                                                     \
        const int ks0 = (int)blockIdx.y * kts, ks1 = min(KT, ks0 + kts);                                                                \
        uint64_t any = 0;                                                                                                               \
        if (ks1 > ks0) {                                                                                                                \
            const int b0 = ks0 >> 4, b1 = (ks1 + 15) >> 4;              /* < 64 blocks: K <= 32768 */                                   \
            const uint64_t range = (b1 - b0 >= 64 ? ~0ull : ((1ull << (b1 - b0)) - 1ull)) << b0;                                        \
            const uint64_t* flags = reinterpret_cast<const uint64_t*>(z13);                                                             \
            _Pragma("unroll") for (int i = 0; i < NP; ++i) {                                                                            \
                const int p = (int)blockIdx.x * NP + i;                                                                                 \
                if (p < NPT) any |= flags[2 * p] & range;          /* 16-byte head entries: flags, then the base the body reads */     \
            }                                                                                                                           \
        }                                                                                                                               \
        if (any != 0) {                                                                                                                 \
            gemm_skinny_body<SkBf16<2 * NP>, MB, 2 * U, true, 0, XL, ROWS>(a, KT, NTT, 0 ROWS_USE);                                     \
        } else {                                                                                                                        \
            a.wp = reinterpret_cast<const uint16_t*>(z13);                                                                              \
            gemm_skinny_body<SkZ13<NP>, MB, U, true, 0, XL, ROWS>(a, KT8, NTT, NPT ROWS_USE);                                           \
        }                                                                                                                               \
    }
#define UMV_COMMA ,
UMV_SKINNY13_KERNEL(gemm_skinny13_kernel, false, , )
UMV_SKINNY13_KERNEL(gemm_skinny13_rows_kernel, true, UMV_COMMA const umv_row_sampling* rows, UMV_COMMA rows)
#undef UMV_COMMA
#undef UMV_SKINNY13_KERNEL

template <int MB, int NP, int U>
static int launch_skinny13(const umv_gemm_args& a, const uint8_t* z13, int KT8, int NTT, int NPT, hipStream_t s) {
    return launch_skinny_body<MB, 2 * NP, U, 2, 0>([](auto XL) { return &gemm_skinny13_kernel<MB, NP, U, decltype(XL)::value>; }, a, KT8,
                                                   NTT, s, z13, KT8, NTT, NPT);
}
template <int MB, int NP, int U>
static int launch_skinny13_rows(const umv_gemm_args& a, const uint8_t* z13, int KT8, int NTT, int NPT, hipStream_t s,
                                const umv_row_sampling* rows) {
    return launch_skinny_body<MB, 2 * NP, U, 2, 0>([](auto XL) { return &gemm_skinny13_rows_kernel<MB, NP, U, decltype(XL)::value>; }, a, KT8,
                                                   NTT, s, z13, KT8, NTT, NPT, rows);
}

// rows: the per-row sampling table of umv_gemm_z13w_rows (checked there), NULL for umv_gemm_z13w
static int gemm_z13w(const umv_gemm_args* ap, const void* z13, const umv_row_sampling* rows, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm_z13w: null args");
    umv_gemm_args a = *ap;
    UMV_CHECK(a.x && a.wp && a.out && z13, UMV_ERR_ARG, "gemm_z13w: null pointer (x, wp = the bf16 image, out and z13 are required)");
    UMV_CHECK(!a.w_scale, UMV_ERR_ARG, "gemm_z13w: w_scale must be NULL");
    if (const int rc = umv_gemm_check_args(a, "gemm_z13w", 32)) return rc;
    UMV_CHECK((a.K % 64) == 0 && a.K <= 32768, UMV_ERR_UNSUPPORTED, "gemm_z13w: K (%d) must be a multiple of 64 and <= 32768", a.K);
    if (const int rc = umv_gemm_check_decode(a, "gemm_z13w", "13-bit", "umv_gemm_bf16", true, true)) return rc;
    UMV_CHECK(((uintptr_t)z13 % 256) == 0, UMV_ERR_ARG, "gemm_z13w: the 13-bit image must be 256-byte aligned");
    if (a.M == 0) return UMV_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* z = reinterpret_cast<const uint8_t*>(z13);
    const int KT8 = a.K / 64, NTT = (a.N + 15) / 16, NPT = (NTT + 1) / 2;
    // (row tiles, tile pairs, 64-k units per chunk).  The bits do not depend on the grouping, so this need not be umv_gemm_bf16's
    // dispatch, and it is not everywhere: a workgroup takes whole PAIRS, so where the bf16 kernel runs one n-tile per workgroup
    // (no split, N < 16384, no SwiGLU) this one has half the workgroups, and at 33..64 rows it takes one pair where the bf16 kernel
    // takes four tiles.  Measured are the decode forms at 8, 16 and 32 rows - SwiGLU gate/up <1,1,2> / <2,2,1>, split-K <1,2,1> /
    // <2,2,1>, lm_head with keys <1,1,2> / <2,2,1> - and the engine routes here the ones that won (ops._route:
    // not gate/up and lm_head at 9..16 rows, where <1,1,2> with two-piece x staging holds 151 registers and ties); the other forms
    // are served for the contract's sake.
    if (a.k_splits > 1) {
        if (a.M <= 16) return launch_skinny13<1, 2, 1>(a, z, KT8, NTT, NPT, s);
        if (a.M <= 32) return launch_skinny13<2, 2, 1>(a, z, KT8, NTT, NPT, s);
        return launch_skinny13<4, 1, 1>(a, z, KT8, NTT, NPT, s);
    }
    const bool two = (a.epilogue & UMV_EPI_SWIGLU) || NTT >= 1024;
    if (rows) {    // the lm_head call with a per-row table: the shapes below, instantiated with the per-row epilogue
        if (a.M <= 16) return launch_skinny13_rows<1, 1, 2>(a, z, KT8, NTT, NPT, s, rows);
        if (a.M <= 32)
            return two ? launch_skinny13_rows<2, 2, 1>(a, z, KT8, NTT, NPT, s, rows) : launch_skinny13_rows<2, 1, 2>(a, z, KT8, NTT, NPT, s, rows);
        return launch_skinny13_rows<4, 1, 1>(a, z, KT8, NTT, NPT, s, rows);
    }
    if (a.M <= 16) return launch_skinny13<1, 1, 2>(a, z, KT8, NTT, NPT, s);
    if (a.M <= 32) return two ? launch_skinny13<2, 2, 1>(a, z, KT8, NTT, NPT, s) : launch_skinny13<2, 1, 2>(a, z, KT8, NTT, NPT, s);
    // 33..64 rows of a wide-N GEMM: umv_gemm_bf16 runs these on an MFMA tile with ONE accumulator chain over K, not the 8-wave K
    // slices - other bits, and faster than streaming at these rows.  They stay on that kernel and the bf16 image.  (This mirrors
    // umv_gemm_bf16's DEFAULT policy: under its tuning variables UMV_GEMM_M64_TILED=0 / UMV_GEMM_SKINNY_MAX that call is still
    // umv_gemm_bf16's own, but the streamed call below is then not what umv_gemm_bf16 would run - see the contract in the header.)
    if (two && !a.argmax_partial && a.K >= 1024) return umv_gemm_bf16(&a, stream);
    return launch_skinny13<4, 1, 1>(a, z, KT8, NTT, NPT, s);
}

extern "C" int umv_gemm_z13w(const umv_gemm_args* ap, const void* z13, umv_stream_t stream) { return gemm_z13w(ap, z13, nullptr, stream); }
extern "C" int umv_gemm_z13w_rows(const umv_gemm_args* ap, const void* z13, const umv_row_sampling* rows, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm_z13w_rows: null args");
    if (const int rc = umv_gemm_check_rows(*ap, rows, "gemm_z13w_rows")) return rc;
    return gemm_z13w(ap, z13, rows, stream);
}
