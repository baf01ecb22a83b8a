// GEMM family for libunimedvl_hip (gfx950).  out[m,n] = epi(sum_k x[m,k] W[n,k]).
//
// W is pre-tiled (umv_pack_weight_bf16) into MFMA A-fragment order so that one
// wavefront instruction fetches a whole 16(n) x 32(k) tile as 1 KiB contiguous:
//   P[nt][kt][lane][8],  lane = g*16 + r,  element j  <->  W[nt*16 + r][kt*32 + g*8 + j]
// With W as the A operand and x^T as the B operand of v_mfma_f32_16x16x32_bf16 the
// accumulator of lane (r,g) holds out[m = r][n = g*4 + reg]: four consecutive n per
// lane, i.e. one 8-byte bf16x4 store per 16x16 tile.
//
// This file has the entry points (umv_gemm_bf16, umv_gemm_fp8w), the tile policy (umv_gemm_tile_config) and the dispatch of
//   * gemm_skinny  (M <= 64, decode / MoT text rows): HBM-bound weight streaming, the body in gemm_skinny.h; its bf16 and
//     e4m3 kernels (gemm_skinny_kernel, gemm_skinny8_kernel) are here;
//   * gemm_tiled   (M > 64, prefill / ViT / diffusion, and the 33..128-row decode tiles): the 8-wave MFMA tiles of gemm_tiled.h
//     (W fragments from the packed stream, x staged through LDS) and the 4-wave tiles of gemm_w4.hip.
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "gemm_epilogue.h"
#include "gemm_internal.h"
#include "gemm_skinny.h"
#include "gemm_tiled.h"
#include <string.h>
#include <stdlib.h>

// ----------------------------------------------------------------------------- skinny (M <= 64): gemm_skinny.h
template <int MB, int NT, int U, bool DB, int NORM, int XL = 0>   // NORM: 0 = off, 8 / 16 = fused RMSNorm keeping that many x rows
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny_kernel(umv_gemm_args a, int KT, int NTT) {
    gemm_skinny_body<SkBf16<NT>, MB, U, DB, NORM, XL>(a, KT, NTT, 0);
}
// the lm_head call with a per-row sampling table (umv_gemm_bf16_rows): the same body, the epilogue's keys and statistics per row
template <int MB, int NT, int U, bool DB, int XL = 0>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny_rows_kernel(umv_gemm_args a, int KT, int NTT, const umv_row_sampling* rows) {
    gemm_skinny_body<SkBf16<NT>, MB, U, DB, 0, XL, true>(a, KT, NTT, 0, rows);
}

template <int MB, int NT, int U, bool DB, int NORM>
static int launch_skinny(const umv_gemm_args& a, int KT, int NTT, hipStream_t s) {
    return launch_skinny_body<MB, NT, U, 1, NORM>([](auto XL) { return &gemm_skinny_kernel<MB, NT, U, DB, NORM, decltype(XL)::value>; }, a, KT,
                                                  NTT, s, KT, NTT);
}
template <int MB, int NT, int U, bool DB>
static int launch_skinny_rows(const umv_gemm_args& a, int KT, int NTT, hipStream_t s, const umv_row_sampling* rows) {
    return launch_skinny_body<MB, NT, U, 1, 0>([](auto XL) { return &gemm_skinny_rows_kernel<MB, NT, U, DB, decltype(XL)::value>; }, a, KT, NTT,
                                               s, KT, NTT, rows);
}

// ----------------------------------------------------------------------------- fp8 weights (decode, BASELINE.json configs[4])
// Weight-only e4m3 (OCP) with one power-of-two scale per output channel (an E8M0 exponent, as in the MX
// formats): W' = q * 2^e is exactly representable in bf16, so streaming q and converting in registers
// (v_cvt_scalef32_pk_bf16_fp8: two elements per instruction, the channel scale rides along for free) feeds the
// SAME bf16 MFMAs with the SAME operands as the bf16 kernel on W'.  Decode reads half the bytes; prefill /
// diffusion keep using the bf16 image of W' on the tiled kernel, and both paths agree bit for bit.
//   image: P8[nt][kt8][lane][16 B], lane = g*16 + r; bytes 0..7  <-> W[nt*16 + r][kt8*64 +      g*8 + j]
//                                                    bytes 8..15 <-> W[nt*16 + r][kt8*64 + 32 + g*8 + j]
//   scale: f32 [ntt*16] in packed row order (SwiGLU images interleave gate / up 16-row tiles like the bf16 one)
// The weight-streaming body over the e4m3 image (64-k units); for K % 512 == 0 its 8-wave K slices - and so the fp32 sums - are those
// of gemm_skinny_kernel on W'.  x costs as much L2->L1 traffic as the e4m3 weights at NT = 1 (M = 8 rows x 2 B vs 16 rows x 1 B per k)
// and is what holds this kernel below the HBM rate: down_proj 18.2 us with these x loads, 12.8 us with x from a constant
// (tools/skinny_bench.py; rotating the K order per workgroup or pre-packing x in fragment order did not help).
template <int MB, int NT, int U, int XL = 0>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny8_kernel(umv_gemm_args a, int KT8, int NTT) {
    gemm_skinny_body<SkE4m3<NT>, MB, U, true, 0, XL>(a, KT8, NTT, 0);
}
template <int MB, int NT, int U, int XL = 0>      // the lm_head call with a per-row sampling table (umv_gemm_fp8w_rows)
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny8_rows_kernel(umv_gemm_args a, int KT8, int NTT, const umv_row_sampling* rows) {
    gemm_skinny_body<SkE4m3<NT>, MB, U, true, 0, XL, true>(a, KT8, NTT, 0, rows);
}

template <int MB, int NT, int U>
static int launch_skinny8(const umv_gemm_args& a, int KT8, int NTT, hipStream_t s) {
    return launch_skinny_body<MB, NT, U, 2, 0>([](auto XL) { return &gemm_skinny8_kernel<MB, NT, U, decltype(XL)::value>; }, a, KT8, NTT, s,
                                               KT8, NTT);
}
template <int MB, int NT, int U>
static int launch_skinny8_rows(const umv_gemm_args& a, int KT8, int NTT, hipStream_t s, const umv_row_sampling* rows) {
    return launch_skinny_body<MB, NT, U, 2, 0>([](auto XL) { return &gemm_skinny8_rows_kernel<MB, NT, U, decltype(XL)::value>; }, a, KT8, NTT, s,
                                               KT8, NTT, rows);
}

// rows: the per-row sampling table of umv_gemm_fp8w_rows (checked there), NULL for umv_gemm_fp8w
static int gemm_fp8w(const umv_gemm_args* ap, const umv_row_sampling* rows, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm_fp8w: null args");
    umv_gemm_args a = *ap;
    UMV_CHECK(a.x && a.wp && a.out && a.w_scale, UMV_ERR_ARG, "gemm_fp8w: null pointer (x, wp, out and w_scale are required)");
    if (const int rc = umv_gemm_check_args(a, "gemm_fp8w", 8)) return rc;
    if (const int rc = umv_gemm_check_decode(a, "gemm_fp8w", "e4m3", "the bf16 image of the dequantised weights with umv_gemm_bf16", true, false))
        return rc;
    if (a.M == 0) return UMV_OK;
    hipStream_t s = (hipStream_t)stream;
    const int KT8 = (a.K + 63) / 64, NTT = (a.N + 15) / 16;
    if (a.k_splits > 1) {   // split-K decode mode: see umv_gemm_bf16
        if (a.M <= 16) return launch_skinny8<1, 4, 1>(a, KT8, NTT, s);
        if (a.M <= 32) return launch_skinny8<2, 4, 1>(a, KT8, NTT, s);
        return launch_skinny8<4, 4, 1>(a, KT8, NTT, s);
    }
    const bool two = (a.epilogue & UMV_EPI_SWIGLU) || NTT >= 1024;
    if (rows) {    // the lm_head call with a per-row table: the shapes below, instantiated with the per-row epilogue
        if (a.M <= 16) return two ? launch_skinny8_rows<1, 2, 2>(a, KT8, NTT, s, rows) : launch_skinny8_rows<1, 1, 8>(a, KT8, NTT, s, rows);
        if (a.M <= 32) return two ? launch_skinny8_rows<2, 4, 1>(a, KT8, NTT, s, rows) : launch_skinny8_rows<2, 1, 4>(a, KT8, NTT, s, rows);
        return two ? launch_skinny8_rows<4, 4, 1>(a, KT8, NTT, s, rows) : launch_skinny8_rows<4, 1, 2>(a, KT8, NTT, s, rows);
    }
    // (NT, U) from a sweep on MI355X at M = 8 (tools/skinny_bench.py, FP8=1): gate/up 25.5 us with <2,2> (110 VGPRs, two
    // workgroups per CU) vs 33.9 <2,4>, 27.9 <4,1>; down_proj 18.2 us with <1,8> vs 23.7 for NT = 2 (only 112 workgroups)
    if (a.M <= 16) return two ? launch_skinny8<1, 2, 2>(a, KT8, NTT, s) : launch_skinny8<1, 1, 8>(a, KT8, NTT, s);
    static const int nt4 = umv_env_int("UMV_GEMM_SKINNY_NT", 4) == 2 ? 0 : 1;   // as in umv_gemm_bf16: 4 n-tiles per workgroup on the wide-N GEMMs at M > 16 (UMV_GEMM_SKINNY_NT=2 reverts)
    if (two && nt4) return a.M <= 32 ? launch_skinny8<2, 4, 1>(a, KT8, NTT, s) : launch_skinny8<4, 4, 1>(a, KT8, NTT, s);
    if (a.M <= 32) return two ? launch_skinny8<2, 2, 2>(a, KT8, NTT, s) : launch_skinny8<2, 1, 4>(a, KT8, NTT, s);
    return two ? launch_skinny8<4, 2, 1>(a, KT8, NTT, s) : launch_skinny8<4, 1, 2>(a, KT8, NTT, s);
}

extern "C" int umv_gemm_fp8w(const umv_gemm_args* ap, umv_stream_t stream) { return gemm_fp8w(ap, nullptr, stream); }
extern "C" int umv_gemm_fp8w_rows(const umv_gemm_args* ap, const umv_row_sampling* rows, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm_fp8w_rows: null args");
    if (const int rc = umv_gemm_check_rows(*ap, rows, "gemm_fp8w_rows")) return rc;
    return gemm_fp8w(ap, rows, stream);
}

// ----------------------------------------------------------------------------- tiled (M > 64): gemm_tiled.h
// the epilogue form of a tiled call: >= 0 = gemm_epilogue.h's lean form for this flag combination, -1 = the general one
// (UMV_GEMM_LEAN_EPI=0: always the general one - A/B, tuning only; results are bit-identical)
int umv_gemm_lean_epilogue(const umv_gemm_args& a) {
    static const int on = umv_env_int("UMV_GEMM_LEAN_EPI", 1);
    return on ? epi_lean_kind(a) : -1;
}

template <int WN, int WM, int TN, int TM, int KTS, int NBUF, int SCHED = 0>
static int launch_tiled(const umv_gemm_args& a, int KT, int NTT, hipStream_t s) {
    using Cf = TiledCfg<WN, WM, TN, TM, KTS, NBUF, SCHED>;
    constexpr int lds = Cf::LDS_BYTES;      // staging buffers + the tile's bias + a spare KiB per surplus staging slot
    static bool attr_set[UMV_MAX_DEVICES] = {};
    if (umv_first_on_device(attr_set)) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_tiled_kernel<WN, WM, TN, TM, KTS, NBUF, SCHED>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    }
    const int mblocks = (a.M + Cf::BM - 1) / Cf::BM, nblocks = (a.N + Cf::BN - 1) / Cf::BN;
    const int splits = a.k_splits > 1 ? a.k_splits : 1;
    const int ksplit = splits > 1 ? ((KT + splits - 1) / splits + KTS - 1) / KTS * KTS : 0;    // whole k-steps per split
    hipLaunchKernelGGL((gemm_tiled_kernel<WN, WM, TN, TM, KTS, NBUF, SCHED>), dim3(mblocks * nblocks, splits), dim3(WN * WM * 64), lds, s, a,
                       KT, NTT, mblocks, nblocks, UMV_TILE_GN, ksplit, umv_tile_superblock(mblocks, Cf::BM, a.K), umv_gemm_lean_epilogue(a));
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// Tile choice from measurements on MI355X (tools/gemm_bench.py, profiles/r01_gemm_tiles_auto.txt).  The 256x256x32
// 4-buffer tile with the interleaved schedule wins whenever it yields >= ~144 workgroups (885-1120 TF/s on the
// prefill / flow / ViT shapes); below that the 256(n) x 128(m) interleaved tile (M ~ 2048: 920-1020 TF/s), then
// 128 x 128 with two workgroups per CU (M ~ 1024: 560-680), then 128(n) x 64(m).
// UMV_GEMM_TILE=<256|266|258|268|384|288|129|130|270|64> overrides (tuning only).
// Exported so that tests can assert which kernel a shape is sent to (returns 0 for M <= 64: weight-streaming kernels).
// compute units of the current device (256 on MI355X; 256 as well when no device answers - the policy is also queried on hosts without one)
static int umv_cu_count() {
    static const int n = [] {
        int d = 0, v = 0;
        if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) return 256;
        return v;
    }();
    return n;
}

extern "C" int umv_gemm_tile_config(int M, int N, int K) {
    static const int force = umv_env_int("UMV_GEMM_TILE", 0);
    if (force) return force;
    if (M <= 64) return 0;
    const long wg256 = (long)((M + 255) / 256) * ((N + 255) / 256);
    const long wg128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    const long wg258 = (long)((M + 127) / 128) * ((N + 255) / 256);
    if (K < 1024) return 64;              // short K: the 4-buffer prologue does not amortise
    if (wg256 >= 144 && (N <= 8192 || M <= 1024)) {   // (wide N: many n-blocks either way, 256 x 256 wins or ties - 2064 x 37888: 602 vs 606 us -
                                                      // except at few rows: a single image's guided flow pass, 512 x 37888 x 3584, is 296 tiles = two
                                                      // rounds of 256 x 256 against two rounds of the smaller 384 x 128: 231 -> 206 us)
        // N = 1152 (SigLIP out / fc2) is 4.5 tiles of 256: 10 % padding and 160 tiles for 256 CUs.  As 3 x 384 columns by 128 rows
        // it is 192 tiles of 3/4 the work: rounds x tile area decides (out 46.7 -> 37.3 us, fc2 103.8 -> 89.9, fc1 (N = 4304: 544
        // tiles = 2.1 rounds against 768 = 3 rounds of 3/4) 120.3 -> 111.7; the fused q/k/v GEMM, N = 3456, stays on
        // 256 x 256: 76 vs 95 us)
        const long cus = umv_cu_count(), t384 = (long)((M + 127) / 128) * ((N + 383) / 384);
        const long c266 = (wg256 + cus - 1) / cus * 65536, c384 = (t384 + cus - 1) / cus * 49152;
        // 288 x 128 (round 3): N = 1152 / 4608 = 4 / 16 x 288 columns give exactly 256 tiles at 8192 / 2048 rows where 384 x 128 fills
        // 192 of the 256 CUs.  Its 18 MFMAs per k-step carry the same per-step overhead as the bigger tiles' 24 - 32 (about 0.8 of
        // their rate per unit of tile area), so it has to win by more than that: out-proj 38.4 -> 34.8 us, fc2 91.9 -> 85.4, the
        // flow passes' q/k/v GEMM (2048 x 4608 x 3584) 80.2 -> 73.8
        if (N % 288 == 0) {
            const long t288 = (long)((M + 127) / 128) * (N / 288), c288 = (t288 + cus - 1) / cus * 36864;
            if (c288 * 6 < c384 * 5 && c288 * 6 < c266 * 5) return 288;
        }
        // few rows on a wide N (the 8 x 34-token question prefill: 272 x 37888 is 297 tiles of 384 x 128 = two rounds for 1.16 rounds of
        // work): 256 x 128 tiles at ~1.15x the cost per unit of area (444 tiles = two rounds of two thirds the size): 154 -> 134 us
        // (profiles/r04_m272_tiles.txt); the same rule sends the 65..128-row decode gate/up GEMM to 148 tiles of 256 x 128 instead of 99 of
        // 384 x 128: 128 samples 7.80 -> 7.47 ms per step, 96: 7.07 -> 6.76, 72: 6.50 -> 6.17 (profiles/r04_fewrow_tile.txt)
        const long c268 = (wg258 + cus - 1) / cus * 32768 * 115 / 100;
        static const int fewrow = umv_env_int("UMV_GEMM_FEWROW", 1);      // UMV_GEMM_FEWROW=0: without this rule (A/B, tuning only)
        if (fewrow && M <= 512 && c268 < c384 && c268 < c266) return 268;
        if (c384 * 10 < c266 * 9) return 384;
    }
    if (wg256 >= 144) return 266;
    if (wg258 >= 140) return 268;
    if (wg128 >= 128) return 270;
    return 64;
}

// rows: the per-row sampling table of umv_gemm_bf16_rows (checked there), NULL for umv_gemm_bf16
static int gemm_bf16(const umv_gemm_args* ap, const umv_row_sampling* rows, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm: null args");
    umv_gemm_args a = *ap;
    UMV_CHECK(a.x && a.wp && a.out, UMV_ERR_ARG, "gemm: null pointer");
    if (const int rc = umv_gemm_check_args(a, "gemm", 8)) return rc;
    UMV_CHECK(!a.norm_w || (a.M <= 16 && a.K <= SK_WAVES * SK_XMAX * 32), UMV_ERR_UNSUPPORTED,
              "gemm: fused RMSNorm needs M <= 16 and K <= %d (got M=%d K=%d)", SK_WAVES * SK_XMAX * 32, a.M, a.K);
    UMV_CHECK(a.k_splits <= 1 || (a.M <= 128 && !a.norm_w && !(a.epilogue & UMV_EPI_SWIGLU) && a.tile_rows % 16 == 0 && a.split_stride > 0),
              UMV_ERR_UNSUPPORTED, "gemm: split-K (k_splits=%d) is a decode mode: M <= 128, 16-row image, no SwiGLU / fused norm, "
              "split_stride > 0", a.k_splits);
    UMV_CHECK(a.k_splits <= 64, UMV_ERR_ARG, "gemm: k_splits %d > 64", a.k_splits);
    UMV_CHECK(!a.argmax_partial || (a.M <= 64 && a.k_splits <= 1 && !a.row_idx && !a.norm_w && (a.tile_rows == 0 || a.tile_rows == 16) &&
                                    !(a.epilogue & (UMV_EPI_SWIGLU | UMV_EPI_OUT_F32))),
              UMV_ERR_UNSUPPORTED, "gemm: argmax_partial is an epilogue of the decode lm_head GEMM (M <= 64, 16-row image, bf16 out, "
              "no SwiGLU / split-K / row_idx / fused norm)");
    UMV_CHECK(a.sample_temperature >= 0.f && (a.sample_temperature == 0.f || a.argmax_partial), UMV_ERR_ARG,
              "gemm: sample_temperature (%g) is a mode of the argmax_partial epilogue and must be >= 0", (double)a.sample_temperature);
    if (a.M == 0) return UMV_OK;
    hipStream_t s = (hipStream_t)stream;
    const int KT = (a.K + 31) / 32;
    const int TH = a.tile_rows > 0 ? a.tile_rows : 16;
    UMV_CHECK(TH <= 16, UMV_ERR_ARG, "gemm: tile_rows %d > 16", TH);
    UMV_CHECK(TH == 16 || (a.M <= 64 && !(a.epilogue & UMV_EPI_SWIGLU)), UMV_ERR_UNSUPPORTED,
              "gemm: %d-row packed tiles are a decode-only layout (M <= 64, no SwiGLU)", TH);
    const int NTT = (a.N + TH - 1) / TH;
    static const int skinny_max = umv_env_int("UMV_GEMM_SKINNY_MAX", 64);   // tuning only: UMV_GEMM_SKINNY_MAX=<M> (rows up to which the weight-streaming kernel is used)
    static const int sk_tiled_min = umv_env_int("UMV_SPLITK_TILED_MIN", 65);   // tuning only: UMV_SPLITK_TILED_MIN=<rows from which split-K runs on the tiled kernel>
    static const int sk_xl = umv_env_int("UMV_SPLITK_TILED_XL", 1);          // UMV_SPLITK_TILED_XL=0: the half-line staging of the 65..128-row split-K tile (A/B, tuning only; bit-identical;
    if (a.k_splits > 1 && (a.M > 64 || a.M >= sk_tiled_min) && TH == 16) {  // 65..128 rows: the 128 x 128 tile (two workgroups per CU) over k_splits K ranges, fp32 partials
        if (sk_xl) return launch_tiled<2, 2, 4, 4, 1, 4, 3>(a, KT, NTT, s);
        return launch_tiled<2, 2, 4, 4, 1, 4, 1>(a, KT, NTT, s);
    }
    if (a.k_splits > 1) {
        // split-K decode GEMM: 4 n-tiles per workgroup share every x fragment (x re-reads from L2 drop 4x against the
        // one-tile workgroups), the K range is cut k_splits ways to keep >= 256 workgroups, partial sums go to fp32
        // (two n-tiles per workgroup at M <= 8 - twice the workgroups, 216-224 is less than one per CU - measured 3.199 vs
        // 3.176 ms per step: no)
        if (a.M <= 16) return launch_skinny<1, 4, 2, true, 0>(a, KT, NTT, s);
        if (a.M <= 32) {
            static const int v32 = umv_env_int("UMV_SKINNY_M32", 0);    // tuning only: UMV_SKINNY_M32=<0|1|2>
            if (v32 == 1) return launch_skinny<2, 4, 1, true, 0>(a, KT, NTT, s);
            if (v32 == 2) return launch_skinny<2, 2, 2, true, 0>(a, KT, NTT, s);
            return launch_skinny<2, 4, 2, true, 0>(a, KT, NTT, s);
        }
        // (33..64 rows on a tiled kernel over the K ranges - 128 x 64 full-line or UMV_SPLITK_TILED_MIN=33 - measured 6.25 / 6.45 ms per
        // 64-sample step against 5.41: the weight-streaming kernel stays)
        return launch_skinny<4, 4, 1, true, 0>(a, KT, NTT, s);
    }
    if (rows) {    // the lm_head call with a per-row sampling table (M <= 64, 16-row image, no split - checked above): the default
        // policy's shapes below, instantiated with the per-row epilogue.  The bits of a GEMM do not depend on the grouping.
        const bool two = NTT >= 1024;
        if (a.M <= 16) return two ? launch_skinny_rows<1, 2, 4, true>(a, KT, NTT, s, rows) : launch_skinny_rows<1, 1, 8, true>(a, KT, NTT, s, rows);
        if (a.M <= 32) return two ? launch_skinny_rows<2, 4, 2, true>(a, KT, NTT, s, rows) : launch_skinny_rows<2, 1, 4, false>(a, KT, NTT, s, rows);
        return two ? launch_skinny_rows<4, 4, 1, true>(a, KT, NTT, s, rows) : launch_skinny_rows<4, 1, 4, false>(a, KT, NTT, s, rows);
    }
    if (a.M <= 64 && (a.M <= skinny_max || TH != 16)) {
        const bool two = (a.epilogue & UMV_EPI_SWIGLU) || NTT >= 1024;
        if (a.M <= 16) {
            if (a.norm_w && a.M <= 8) return two ? launch_skinny<1, 2, 4, true, 8>(a, KT, NTT, s) : launch_skinny<1, 1, 8, true, 8>(a, KT, NTT, s);
            if (a.norm_w) return two ? launch_skinny<1, 2, 4, true, 16>(a, KT, NTT, s) : launch_skinny<1, 1, 8, true, 16>(a, KT, NTT, s);
            return two ? launch_skinny<1, 2, 4, true, 0>(a, KT, NTT, s) : launch_skinny<1, 1, 8, true, 0>(a, KT, NTT, s);
        }
        // M > 16: every workgroup re-reads all of x from L2, so wide-N GEMMs take 4 n-tiles per workgroup (x : weight bytes
        // = M : 64); UMV_GEMM_SKINNY_NT=2 restores the 2-tile kernels (tuning only)
        static const int nt4_env = umv_env_int("UMV_GEMM_SKINNY_NT", 4), nt4 = nt4_env == 2 ? 0 : nt4_env == 8 ? 8 : 1;
        // (the 128 x 64 full-line tile at 17..32 rows: 32 samples 3.99 -> 4.09 ms per step, 24: 3.80 -> 3.92, 17: 3.62 -> 3.74 - the
        // weight-streaming kernel keeps these rows; profiles/r04_midbatch_xline.txt)
        if (two && nt4 == 8 && TH == 16 && a.M <= 32) return launch_skinny<2, 8, 1, true, 0>(a, KT, NTT, s);
        if (two && nt4 && TH == 16 && a.M <= 32) {
            static const int v32 = umv_env_int("UMV_SKINNY_M32", 0);
            if (v32 == 1) return launch_skinny<2, 4, 1, true, 0>(a, KT, NTT, s);
            if (v32 == 2) return launch_skinny<2, 2, 2, true, 0>(a, KT, NTT, s);
            return launch_skinny<2, 4, 2, true, 0>(a, KT, NTT, s);
        }
        // 33..64 rows on the wide-N GEMMs: the LDS-staged tile 128(n) x 64(m) x 64 reads x once per 128 columns instead of once
        // per 64 and streams gate/up in 73 us against 84 for the 4-tile skinny kernel (tools/stream_tile_bench.py 64); at
        // <= 32 rows the skinny kernel wins (60 vs 64-66 us).  Not with the argmax epilogue (skinny kernels only).
        static const int m64 = umv_env_int("UMV_GEMM_M64_TILED", 2);
        // UMV_GEMM_M64_TILED=2 (default): the same tile with k-steps of 32 and x staged in full 128-byte lines (SCHED = 3, 48 KiB, 3 WG/CU):
        // bit-identical, 64-sample decode step 5.65 -> 5.42 ms, 40 samples 4.82 -> 4.60 ms; 1 = the 64-wide k-step tile, 0 = skinny
        if (two && TH == 16 && m64 == 2 && a.M > 32 && !a.argmax_partial && !a.norm_w && a.K >= 1024) return launch_tiled<4, 1, 2, 4, 1, 4, 3>(a, KT, NTT, s);
        if (two && TH == 16 && m64 && a.M > 32 && !a.argmax_partial && !a.norm_w && a.K >= 1024) return launch_tiled<4, 1, 2, 4, 2, 3>(a, KT, NTT, s);
        if (two && nt4 && TH == 16) return launch_skinny<4, 4, 1, true, 0>(a, KT, NTT, s);
        if (a.M <= 32) return two ? launch_skinny<2, 2, 4, false, 0>(a, KT, NTT, s) : launch_skinny<2, 1, 4, false, 0>(a, KT, NTT, s);
        return two ? launch_skinny<4, 2, 2, false, 0>(a, KT, NTT, s) : launch_skinny<4, 1, 4, false, 0>(a, KT, NTT, s);
    }
    int cfg = umv_gemm_tile_config(a.M, a.N, a.K);
    // SwiGLU pairs the gate / up tiles (2p, 2p + 1) INSIDE a wave's column range: the 288-column tile gives a wave 9 tiles, its pairs
    // would straddle two waves.  (The policy can pick 288 for N = 2 I = k * 288; the model's 37888 is not one of those.)
    if ((a.epilogue & UMV_EPI_SWIGLU) && cfg == 288) cfg = 384;
    {   // the staging variant of the interleaved tiles: full-line x staging (SCHED = 3) unless UMV_GEMM_XLINE=0 (A/B, tuning only).
        // Bit-identical results; end to end on MI355X (tools/stage_profile.py, same box): text-to-image 1530 -> 1443 ms per batch of 4,
        // prefill of 8 images 131.7 -> 130.7 ms, ViT tower 12.70 -> 12.50 ms.  (A 20-launch microbenchmark from a cold chip shows the
        // opposite sign, -2..-8 %: the variant pays a longer prologue and wins only at the clocks a sustained load runs at.)
        static const int xline = umv_env_int("UMV_GEMM_XLINE", 1);      // (the 288-column tile with full-line staging: measured, not adopted)
        if (xline) cfg = cfg == 266 ? 366 : cfg == 268 ? 368 : cfg == 384 ? 484 : cfg == 270 ? 370 : cfg;
    }
    {   // round 5: the 4-wave tiles with the accumulators in AGPRs (gemm_w4.hip) take over the 8-wave tiles of the same shape: bit-identical
        // results (same MFMAs, operands and k order).  Sustained loops on MI355X (profiles/r05_w4_policy.txt): gate/up 2048 x 37888 x 3584
        // 458 -> 408 us (1.21 -> 1.36 PF), 8208 rows 1790 -> 1602 us (1.39 PF), down 2048 x 3584 x 18944 254 -> 205 us (1.36 PF), o_proj
        // 8208 x 3584 x 3584 182 -> 169 us; end to end text-to-image 1387 -> 1315 ms per batch of 4, prefill of 8 images 123.1 -> 116.5 ms.
        // At short K (SigLIP, K = 1152) they first LOST - q/k/v 67.8 -> 80.6 us, tower 11.6 -> 12.3 ms - because the general epilogue's
        // 35 k cycles per tile ran on four waves instead of eight; with the lean epilogue (gemm_epilogue.h) they win there too: q/k/v
        // 64.5 -> 59.9 us, fc1 84.9 -> 80.0 us, tower 10.66 -> 10.50 ms at 8 images and 38.0 -> 37.3 ms at 32 (20-repetition runs, twice;
        // profiles/r05_lean_epilogue.txt).  So: every K.  UMV_GEMM_W4=0: the 8-wave tiles everywhere, 3: the 4-wave tiles only at
        // K >= 2048 (the rule before the lean epilogue) - A/B, tuning only.
        static const int w4 = umv_env_int("UMV_GEMM_W4", 1);
        const int c4 = cfg == 366 ? 466 : cfg == 368 ? 468 : cfg == 484 ? 4384 : 0;
        if (w4 && c4 && (w4 != 3 || a.K >= 2048) && umv_gemm_w4_can_take(a, KT, NTT)) return umv_gemm_w4_launch(a, KT, NTT, c4, s);
    }
    // every tile configuration, once, with its shape: <waves n, waves m, MFMA tiles n, m per wave, k-tiles per step, LDS buffers, SCHED>
    switch (cfg) {
    case 466: case 468: case 4384: case 94661: case 94662: return umv_gemm_w4_launch(a, KT, NTT, cfg, s);   // the 4-wave tiles, forced (gemm_w4.hip)
    // experimental weight-streaming shapes of the tiled kernel for 16 < M <= 128 (tuning only, UMV_GEMM_TILE + UMV_GEMM_SKINNY_MAX)
    case 332: return launch_tiled<4, 1, 2, 2, 4, 3>(a, KT, NTT, s);      // 128(n) x 32(m) x 128, 3 buffers (120 KiB), 4 waves
    case 333: return launch_tiled<4, 1, 2, 2, 2, 4>(a, KT, NTT, s);      // 128(n) x 32(m) x 64, 4 buffers (80 KiB)
    case 335: return launch_tiled<4, 1, 2, 2, 2, 3>(a, KT, NTT, s);      // 128(n) x 32(m) x 64, 3 buffers (60 KiB, 2 WG/CU)
    case 364: return launch_tiled<4, 1, 2, 4, 2, 3>(a, KT, NTT, s);      // 128(n) x 64(m) x 64, 3 buffers (72 KiB)
    case 3128: return launch_tiled<4, 1, 2, 8, 2, 3>(a, KT, NTT, s);     // 128(n) x 128(m) x 64, 3 buffers (96 KiB)
    // the plain loop
    case 256: return launch_tiled<2, 4, 8, 4, 1, 4>(a, KT, NTT, s);      // 256x256x32, 4 buffers (128 KiB)
    case 258: return launch_tiled<4, 2, 4, 4, 1, 4>(a, KT, NTT, s);      // 256(n)x128(m)x32, 8 waves as 4x2 (96 KiB)
    case 129: return launch_tiled<2, 2, 4, 4, 2, 2>(a, KT, NTT, s);      // 128x128x64, 2 buffers (64 KiB, 2 WG/CU)
    case 130: return launch_tiled<2, 2, 4, 4, 1, 4>(a, KT, NTT, s);      // 128x128x32, 4 buffers (64 KiB, 2 WG/CU)
    // MFMA / ds_read interleaved by hand, x staged in half lines (SCHED = 1)
    case 266: return launch_tiled<2, 4, 8, 4, 1, 4, 1>(a, KT, NTT, s);   // 256x256x32, 4 buffers
    case 268: return launch_tiled<4, 2, 4, 4, 1, 4, 1>(a, KT, NTT, s);   // 256(n)x128(m)x32, 8 waves as 4x2
    case 384: return launch_tiled<4, 2, 6, 4, 1, 4, 1>(a, KT, NTT, s);   // 384(n)x128(m)x32, 8 waves of 96 x 64: N = 1152 = 3 x 384 without padding
    case 270: return launch_tiled<2, 2, 4, 4, 1, 4, 1>(a, KT, NTT, s);   // 128x128x32, 4 waves, 4 buffers (64 KiB, 2 WG/CU)
    case 288: return launch_tiled<2, 4, 9, 2, 1, 4, 1>(a, KT, NTT, s);   // 288(n)x128(m)x32: N = 1152 / 4608 = 4 / 16 x 288 -> 256 tiles at 8192 / 2048 rows
    // 266 / 268 / 384 / 270 with the x operand staged in full 128-byte lines (SCHED = 3)
    case 366: return launch_tiled<2, 4, 8, 4, 1, 4, 3>(a, KT, NTT, s);
    case 368: return launch_tiled<4, 2, 4, 4, 1, 4, 3>(a, KT, NTT, s);
    case 484: return launch_tiled<4, 2, 6, 4, 1, 4, 3>(a, KT, NTT, s);
    case 370: return launch_tiled<2, 2, 4, 4, 1, 4, 3>(a, KT, NTT, s);
    default: return launch_tiled<2, 2, 4, 2, 2, 3>(a, KT, NTT, s);       // 64: 128(n) x 64(m) x 64, 3 buffers (72 KiB)
    }
}

extern "C" int umv_gemm_bf16(const umv_gemm_args* ap, umv_stream_t stream) { return gemm_bf16(ap, nullptr, stream); }
extern "C" int umv_gemm_bf16_rows(const umv_gemm_args* ap, const umv_row_sampling* rows, umv_stream_t stream) {
    UMV_CHECK(ap != nullptr, UMV_ERR_ARG, "gemm_bf16_rows: null args");
    if (const int rc = umv_gemm_check_rows(*ap, rows, "gemm_bf16_rows")) return rc;
    return gemm_bf16(ap, rows, stream);
}
