// MXFP4 weights for the decode GEMMs (gfx950): e2m1 codes with one E8M0 power-of-two scale per 32 consecutive k of a row.
//
// Format (include/unimedvl_hip.h): s = 2^e, e the smallest integer with 6 * 2^e >= max|W[block]| (6 = the largest e2m1 value, so
// nothing is clipped), clamped to [-127, 127], e = 0 for an all-zero block; q = rne_e2m1(W / s) with the sign kept (a negative value
// that rounds to zero is code 8, -0); W' = q * s is exact in bf16.  The decode kernel converts the codes to bf16 in registers with
// v_cvt_scalef32_pk_bf16_fp4 and feeds the same v_mfma_f32_16x16x32_bf16 with the same operands in the same k order as
// gemm_skinny_kernel on the bf16 image of W': for K % 512 == 0 and no split-K the results are bit-identical.
//
// Image (one buffer, NP = ceil(ceil(N/16) / 2) pairs of 16-row tiles, KT8 = ceil(K/64)):
//   codes  C[p][kt8][lane = g*16 + r][16 B]   bytes  0..3  <-> tile 2p,   row r, k = kt8*64 +      g*8 + j  (nibble j of the 4 bytes,
//                                             bytes  4..7  <-> tile 2p,   row r, k = kt8*64 + 32 + g*8 + j   low nibble first)
//                                             bytes  8..11 <-> tile 2p+1, row r, k = kt8*64 +      g*8 + j
//                                             bytes 12..15 <-> tile 2p+1, row r, k = kt8*64 + 32 + g*8 + j
//   scales S[p][kt8][r][4 B] at byte NP*KT8*1024: E8M0 of (tile 2p, k block 2*kt8), (2p, 2*kt8+1), (2p+1, 2*kt8), (2p+1, 2*kt8+1)
// One lane load of 16 B covers two n-tiles x 64 k: a wave's unit of work along k is 64, as for the e4m3 image, so the 8-wave K
// partition is the bf16 kernel's.  Padding rows / k are zero codes with scale byte 127.  SwiGLU images interleave the gate and up
// 16-row tiles like the bf16 one, so a pair is (gate tile t, up tile t).
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "gemm_epilogue.h"
#include "gemm_internal.h"

#define SK4_WAVES 8

// E8M0 byte -> the f32 scale operand of v_cvt_scalef32_*: 2^(b - 127); b = 0 is the subnormal 2^-127
__device__ __forceinline__ float e8m0_scale(uint32_t b) { return __uint_as_float(b ? b << 23 : 0x00400000u); }

// 8 e2m1 codes (low nibble first) x one scale -> 8 bf16 (exact)
__device__ __forceinline__ bf16x8 cvt_fp4x8(uint32_t q, float scale) {
    union { bf16x2_hw h[4]; bf16x8 v; } a;
    a.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0);
    a.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1);
    a.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2);
    a.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3);
    return a.v;
}

// E8M0 byte of a block from the bf16 bits of its largest magnitude (bits & 0x7FFF; the order of the bit patterns is the order of
// the values).  amax = 1.m * 2^(E-127): 6 * 2^e >= amax  <=>  e >= E - 129 when 1.m <= 1.5 (m <= 0x40), else e >= E - 128.
__device__ __forceinline__ uint32_t mxfp4_scale_byte(uint32_t amax_bits) {
    if (amax_bits == 0) return 127u;
    const int E = (int)(amax_bits >> 7), m = (int)(amax_bits & 0x7F);
    int e = E == 0 ? -127 : ((m <= 0x40) ? E - 129 : E - 128);      // bf16 subnormals: e <= -129, clamped
    e = e < -127 ? -127 : (e > 127 ? 127 : e);
    return (uint32_t)(e + 127);
}

// |v| / 2^e (exact where it matters: at and above the first threshold 0.25) -> e2m1 code by round to nearest even, sign kept
__device__ __forceinline__ uint32_t e2m1_code(uint16_t h, int e) {
    const float a = ldexpf(fabsf(bf2f(h)), -e);
    uint32_t c;
    if (a <= 0.25f) c = 0;            // ties go to the even code: 0.25 -> 0, 0.75 -> 1 (code 2), 1.25 -> 1, 1.75 -> 2, 2.5 -> 2,
    else if (a < 0.75f) c = 1;        // 3.5 -> 4, 5 -> 4
    else if (a <= 1.25f) c = 2;
    else if (a < 1.75f) c = 3;
    else if (a <= 2.5f) c = 4;
    else if (a < 3.5f) c = 5;
    else if (a <= 5.0f) c = 6;
    else c = 7;
    return c | ((uint32_t)(h >> 15) << 3);
}

// One workgroup (256 threads) per tile pair: block scales into LDS and the image, then the codes (+ optional W' in bf16, converted
// by the decode kernel's instruction).  LDS: 32 rows x 2*KT8 scale bytes.
__global__ __launch_bounds__(256) void quantize_pack_mxfp4_kernel(const bf16_t* __restrict__ w, const bf16_t* __restrict__ w2,
                                                                  uint8_t* __restrict__ img, bf16_t* __restrict__ deq,
                                                                  bf16_t* __restrict__ deq2, int rows, int K, int KT8, int NTT, int NP) {
    extern __shared__ uint8_t sexp[];       // [2 tiles][16 rows][2*KT8]
    const int p = blockIdx.x, tid = threadIdx.x;
    const bool inter = w2 != nullptr;
    const int KB = 2 * KT8;
    // which source row a (tile of this pair, row) is, or -1
    auto src_row = [&](int i, int r, const bf16_t*& src, bf16_t*& dq) -> int {
        const int t = 2 * p + i;
        src = (inter && (t & 1)) ? w2 : w;
        dq = (inter && (t & 1)) ? deq2 : deq;
        const int n = (inter ? (t >> 1) : t) * 16 + r;
        return (t < NTT && n < rows) ? n : -1;
    };
    uint8_t* scales = img + (int64_t)NP * KT8 * 1024;
    for (int idx = tid; idx < 32 * KB; idx += 256) {      // one thread per (tile, row, 32-k block)
        const int kb = idx % KB, rr = idx / KB, i = rr >> 4, r = rr & 15;
        const bf16_t* src;
        bf16_t* dq;
        const int n = src_row(i, r, src, dq);
        uint32_t amax = 0;
        if (n >= 0 && kb * 32 < K) {
            const u32x4* q = reinterpret_cast<const u32x4*>(src + (int64_t)n * K + kb * 32);    // K % 32 == 0: 64 aligned bytes
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const u32x4 x = q[v];
                const uint32_t wd[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) amax = max(amax, max(wd[j] & 0x7FFFu, (wd[j] >> 16) & 0x7FFFu));
            }
        }
        const uint32_t sb = mxfp4_scale_byte(amax);
        sexp[rr * KB + kb] = (uint8_t)sb;
        scales[((int64_t)p * KT8 + (kb >> 1)) * 64 + r * 4 + i * 2 + (kb & 1)] = (uint8_t)sb;
    }
    __syncthreads();
    for (int idx = tid; idx < KT8 * 64; idx += 256) {      // one thread per (kt8, lane) 16-byte group
        const int lane = idx & 63, kt8 = idx >> 6;
        const int r = lane & 15, g = lane >> 4;
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bf16_t* src;
            bf16_t* dq;
            const int n = src_row(i, r, src, dq);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kb = kt8 * 2 + h;
                const int k0 = kb * 32 + g * 8;
                const uint32_t sb = sexp[(i * 16 + r) * KB + kb];
                uint32_t word = 0;
                if (n >= 0 && k0 < K) {
                    const u32x4 x = *reinterpret_cast<const u32x4*>(src + (int64_t)n * K + k0);
                    const uint32_t wd[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        word |= e2m1_code((uint16_t)(wd[j] & 0xFFFFu), (int)sb - 127) << (8 * j);
                        word |= e2m1_code((uint16_t)(wd[j] >> 16), (int)sb - 127) << (8 * j + 4);
                    }
                    if (dq) {
                        const bf16x8 d = cvt_fp4x8(word, e8m0_scale(sb));
                        *reinterpret_cast<bf16x8*>(dq + (int64_t)n * K + k0) = d;
                    }
                }
                o[2 * i + h] = word;
            }
        }
        *reinterpret_cast<u32x4*>(img + (((int64_t)p * KT8 + kt8) * 64 + lane) * 16) = (u32x4){o[0], o[1], o[2], o[3]};
    }
}

extern "C" size_t umv_packed_weight_mxfp4_bytes(int N, int K) {
    if (N <= 0 || K <= 0) return 0;
    const size_t np = ((size_t)(N + 15) / 16 + 1) / 2, kt8 = (size_t)(K + 63) / 64;
    return np * kt8 * (1024 + 64);
}

extern "C" int umv_quantize_pack_weight_mxfp4(const uint16_t* w, const uint16_t* w_up, uint8_t* packed4, uint16_t* deq,
                                              uint16_t* deq_up, int rows, int K, umv_stream_t stream) {
    UMV_CHECK(w && packed4 && rows > 0 && K > 0, UMV_ERR_ARG, "quantize_pack_weight_mxfp4: bad args");
    UMV_CHECK((K % 32) == 0 && K <= 65536, UMV_ERR_ARG, "quantize_pack_weight_mxfp4: K (%d) must be a multiple of 32 (the block) and <= 65536",
              K);
    UMV_CHECK(!w_up || (rows % 16) == 0, UMV_ERR_ARG, "quantize_pack_weight_mxfp4: SwiGLU image needs I %% 16 == 0 (I=%d)", rows);
    UMV_CHECK(!(deq_up && !w_up), UMV_ERR_ARG, "quantize_pack_weight_mxfp4: deq_up without w_up");
    UMV_CHECK(((uintptr_t)w | (uintptr_t)w_up | (uintptr_t)deq | (uintptr_t)deq_up | (uintptr_t)packed4) % 16 == 0, UMV_ERR_ARG,
              "quantize_pack_weight_mxfp4: every buffer must be 16-byte aligned");
    const int NTT = (w_up ? 2 : 1) * ((rows + 15) / 16), NP = (NTT + 1) / 2, KT8 = (K + 63) / 64;
    const size_t lds = (size_t)32 * 2 * KT8;
    hipLaunchKernelGGL(quantize_pack_mxfp4_kernel, dim3(NP), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)w, (const bf16_t*)w_up,
                       packed4, (bf16_t*)deq, (bf16_t*)deq_up, rows, K, KT8, NTT, NP);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- decode GEMM (M <= 64)
// gemm_skinny8_kernel over the MXFP4 image: 8 waves split K in contiguous slices of 64-wide super-tiles, LDS reduce in wave order,
// the same epilogue.  A workgroup owns NP tile PAIRS (NT = 2 NP n-tiles): at 4 bits x is the larger stream (M = 8: 16 B of x per k
// against 8.5 B of one 16-row tile), so each x fragment - staged once per wave slice as full 128-byte lines (XL, as in the e4m3
// kernel) - feeds 2 NP tiles.  Split-K (a.k_splits) over blockIdx.y as in the other decode kernels.
template <int MB, int NP, int U, int XL = 0>
struct SkBuf4 {
    u32x4 w[U][NP];
    uint32_t s[U][NP];
    bf16x8 x[U][2][MB];
    u32x4 xp[XL ? U : 1][XL == 1 ? 1 : (XL ? 2 * MB : 1)];
};

template <int MB, int NP, int U, int XL = 0>
__global__ __launch_bounds__(SK4_WAVES * 64) void gemm_skinny4_kernel(umv_gemm_args a, int KT8, int NTT, int NPT) {
    constexpr int NT = 2 * NP;
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int p0 = blockIdx.x * NP, nt0 = 2 * p0;
    const uint8_t* img = reinterpret_cast<const uint8_t*>(a.wp);
    const uint8_t* scales = img + (int64_t)NPT * KT8 * 1024;

    const bf16_t* xrow[MB];
    bool xvalid[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        int m = mb * 16 + r;
        xvalid[mb] = m < a.M;
        int64_t row = xvalid[mb] ? (a.row_idx ? (int64_t)a.row_idx[m] : (int64_t)m) : 0;
        xrow[mb] = a.x + row * a.ldx;
    }
    f32x4 acc[NT][MB];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[t][mb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nsplit = a.k_splits > 1 ? a.k_splits : 1;
    const int kts = (KT8 + nsplit - 1) / nsplit;
    const int ks0 = (int)blockIdx.y * kts, ks1 = min(KT8, ks0 + kts);
    const int kt_per = (max(0, ks1 - ks0) + SK4_WAVES - 1) / SK4_WAVES;
    const int kt_begin = ks0 + wave * kt_per;
    const int kt_end = min(ks1, kt_begin + kt_per);
    const int nk = max(0, kt_end - kt_begin);
    const int nchunks = (nk + U - 1) / U;
    const uint8_t* wbase[NP];
    const uint8_t* sbase[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = (p0 + i) < NPT ? p0 + i : 0;          // pairs past the end re-read pair 0; their columns are never stored
        wbase[i] = img + ((int64_t)p * KT8 * 64 + lane) * 16;
        sbase[i] = scales + ((int64_t)p * KT8 * 16 + r) * 4;
    }
    static_assert(XL != 1 || MB == 1, "one-piece staging serves one 16-row tile of at most 8 valid rows");
    constexpr int XLP = XL == 1 ? 1 : 2 * MB;
    const int xchunk = (lane & 7) ^ ((lane >> 3) & 7);
    const bf16_t* xprow[XL ? XLP : 1];
    bool xpvalid[XL ? XLP : 1];
    if constexpr (XL != 0) {
#pragma unroll
        for (int q = 0; q < XLP; ++q) {
            const int m = q * 8 + (lane >> 3);
            xpvalid[q] = m < a.M;
            const int64_t row = xpvalid[q] ? (a.row_idx ? (int64_t)a.row_idx[m] : (int64_t)m) : 0;
            xprow[q] = a.x + row * a.ldx + xchunk * 8;
        }
    }
    char* xstage = reinterpret_cast<char*>(red) + wave * (U * XLP * 1024);
    auto load_chunk = [&](int c, SkBuf4<MB, NP, U, XL>& b) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kt = kt_begin + c * U + u;
            const bool ok = kt < kt_end;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                b.w[u][i] = ok ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase[i] + (int64_t)kt * 1024)) : (u32x4){0u, 0u, 0u, 0u};
                b.s[u][i] = ok ? *reinterpret_cast<const uint32_t*>(sbase[i] + (int64_t)kt * 64) : 0x7F7F7F7Fu;
            }
            if constexpr (XL != 0) {
                const int k = kt * 64 + xchunk * 8;
#pragma unroll
                for (int q = 0; q < XLP; ++q)
                    b.xp[u][q] = (ok && xpvalid[q] && k < a.K) ? *reinterpret_cast<const u32x4*>(xprow[q] + (int64_t)kt * 64) : (u32x4){0u, 0u, 0u, 0u};
            } else
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = kt * 64 + h * 32 + g * 8;
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) b.x[u][h][mb] = (ok && xvalid[mb] && k < a.K) ? ldg_frag(xrow[mb] + k) : zero_frag();
            }
        }
    };
    auto consume = [&](SkBuf4<MB, NP, U, XL>& b) {
        if constexpr (XL != 0) {       // pieces -> the wave's own LDS KiBs (row-major, XOR-swizzled by the row) -> B fragments
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < XLP; ++q) *reinterpret_cast<u32x4*>(xstage + (u * XLP + q) * 1024 + lane * 16) = b.xp[u][q];
            const int rr = XL == 1 ? (r & 7) : r;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
                        b.x[u][h][mb] = *reinterpret_cast<const bf16x8*>(xstage + u * (XLP * 1024) + (mb * 16 + rr) * 128 + (((h * 4 + g) ^ (rr & 7)) << 4));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bf16x8 wf[2][NT];      // [k half][tile]
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const uint32_t s = b.s[u][i];
                wf[0][2 * i] = cvt_fp4x8(b.w[u][i].x, e8m0_scale(s & 0xFFu));
                wf[1][2 * i] = cvt_fp4x8(b.w[u][i].y, e8m0_scale((s >> 8) & 0xFFu));
                wf[0][2 * i + 1] = cvt_fp4x8(b.w[u][i].z, e8m0_scale((s >> 16) & 0xFFu));
                wf[1][2 * i + 1] = cvt_fp4x8(b.w[u][i].w, e8m0_scale(s >> 24));
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[t][mb] = mfma16(wf[h][t], b.x[u][h][mb], acc[t][mb]);
        }
    };
    SkBuf4<MB, NP, U, XL> b0, b1;
    if (nchunks > 0) load_chunk(0, b0);
    for (int c = 0; c < nchunks; c += 2) {
        if (c + 1 < nchunks) load_chunk(c + 1, b1);
        consume(b0);
        if (c + 1 < nchunks) {
            if (c + 2 < nchunks) load_chunk(c + 2, b0);
            consume(b1);
        }
    }
    if constexpr (XL != 0) __syncthreads();      // the reduction buffer overlays the waves' x staging KiBs
    skinny16_reduce_epilogue<SK4_WAVES, NT, MB>(a, red, acc, tid, lane, wave, nt0, NTT, nsplit);
}

template <int MB, int NP, int U, int XL>
static int launch_skinny4_v(const umv_gemm_args& a, int KT8, int NTT, int NPT, hipStream_t s) {
    const int blocks = (NPT + NP - 1) / NP;
    size_t lds = (size_t)SK4_WAVES * 2 * NP * MB * 4 * 64 * sizeof(float);
    if (XL != 0) {
        const size_t xl = (size_t)SK4_WAVES * U * (XL == 1 ? 1 : 2 * MB) * 1024;
        if (xl > lds) lds = xl;
    }
    static bool attr_set[UMV_MAX_DEVICES] = {};
    if (lds > 64 * 1024 && umv_first_on_device(attr_set))
        hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_skinny4_kernel<MB, NP, U, XL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((gemm_skinny4_kernel<MB, NP, U, XL>), dim3(blocks, a.k_splits > 1 ? a.k_splits : 1), dim3(SK4_WAVES * 64), lds, s, a,
                       KT8, NTT, NPT);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

template <int MB, int NP, int U>
static int launch_skinny4(const umv_gemm_args& a, int KT8, int NTT, int NPT, hipStream_t s) {
    const bool lines = (a.ldx % 64) == 0 && ((uintptr_t)a.x % 128) == 0;      // rows start on a 128-byte boundary
    if (lines) {
        if constexpr (MB == 1) {
            if (a.M <= 8) return launch_skinny4_v<MB, NP, U, 1>(a, KT8, NTT, NPT, s);
        }
        return launch_skinny4_v<MB, NP, U, 2>(a, KT8, NTT, NPT, s);
    }
    return launch_skinny4_v<MB, NP, U, 0>(a, KT8, NTT, NPT, s);
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
    UMV_CHECK(a.M >= 0 && a.N > 0 && a.K > 0, UMV_ERR_ARG, "gemm_mxfp4w: bad shape M=%d N=%d K=%d", a.M, a.N, a.K);
    UMV_CHECK(a.M <= 64, UMV_ERR_UNSUPPORTED, "gemm_mxfp4w: the MXFP4 image is the decode (M <= 64) layout; use the bf16 image of the "
              "dequantised weights with umv_gemm_bf16 for M=%d", a.M);
    UMV_CHECK((a.K % 32) == 0 && (a.ldx % 8) == 0, UMV_ERR_ARG, "gemm_mxfp4w: K (%d) must be a multiple of 32 and ldx (%lld) of 8", a.K,
              (long long)a.ldx);
    UMV_CHECK(!(a.epilogue & UMV_EPI_BIAS) || a.bias, UMV_ERR_ARG, "gemm_mxfp4w: BIAS without bias pointer");
    UMV_CHECK(!(a.epilogue & UMV_EPI_RESIDUAL) || a.residual, UMV_ERR_ARG, "gemm_mxfp4w: RESIDUAL without residual pointer");
    UMV_CHECK(!(a.epilogue & UMV_EPI_SWIGLU) || (a.N % 32) == 0, UMV_ERR_ARG, "gemm_mxfp4w: SWIGLU needs N %% 32 == 0");
    UMV_CHECK(!a.norm_w && (a.tile_rows == 0 || a.tile_rows == 16), UMV_ERR_UNSUPPORTED, "gemm_mxfp4w: no fused norm / th-row tiles");
    UMV_CHECK(!a.argmax_partial, UMV_ERR_UNSUPPORTED, "gemm_mxfp4w: no argmax_partial (lm_head stays e4m3: umv_gemm_fp8w)");
    UMV_CHECK(a.k_splits <= 1 || (!(a.epilogue & UMV_EPI_SWIGLU) && a.split_stride > 0 && a.k_splits <= 64), UMV_ERR_UNSUPPORTED,
              "gemm_mxfp4w: split-K (k_splits=%d) needs no SwiGLU, split_stride > 0, k_splits <= 64", a.k_splits);
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
