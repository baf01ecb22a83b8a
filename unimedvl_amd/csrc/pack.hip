// Weight images of libunimedvl_hip (gfx950): everything that turns a checkpoint tensor into what the GEMM kernels stream.
//
//   bf16   P[n/16][k/32][lane = g*16 + r][8]: element j of lane (r, g) is W[nt*16 + r][kt*32 + g*8 + j] - MFMA A-fragment order, one
//          wavefront instruction fetches a 16(n) x 32(k) tile as 1 KiB contiguous (umv_pack_weight_bf16; SwiGLU: gate / up tiles
//          interleaved, umv_pack_weight_swiglu_bf16); Q[n/th][k/32][g][r < th][8] = the same with th-row tiles for the decode GEMM
//   e4m3   P8[n/16][k/64][lane][16 B] + one power-of-two fp32 scale per output channel (umv_quantize_pack_weight_fp8), and the
//          K = 128 image of the scaled fp8 MFMA made from it (umv_repack_weight_fp8_mfma)
//   MXFP4  C[pair of 16-row tiles][k/64][lane][16 B] e2m1 codes, then E8M0 scales per 32 k (umv_quantize_pack_weight_mxfp4)
//   z13    the bf16 image without loss at 13 bits per weight: flags and bases per tile pair, then R[pair][k/64][3328 B]
//          (umv_pack_weight_z13)
//
// This file and the headers it includes (with PACK_LAYOUT_VERSION) are what unimedvl_amd/packstore.py stamps its on-disk cache of
// packed images with: an edit here invalidates the cache, an edit of a GEMM / attention / vision kernel does not.
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "quant.h"
#include <stdlib.h>

// ----------------------------------------------------------------------------- bf16 images
__global__ void pack_weight_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ p, int N, int K, int NTT,
                                   int KT, int interleave_I, const bf16_t* __restrict__ w2) {
    // one thread per 8-element group of the packed image
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = (int64_t)NTT * KT * 64;
    if (gid >= total) return;
    int lane = (int)(gid & 63);
    int64_t tile = gid >> 6;
    int kt = (int)(tile % KT);
    int nt = (int)(tile / KT);
    int r = lane & 15, g = lane >> 4;
    int k = kt * 32 + g * 8;
    const bf16_t* src = w;
    int n;
    if (interleave_I > 0) {  // swiglu: even tiles gate, odd tiles up
        int t = nt >> 1;
        n = t * 16 + r;
        src = (nt & 1) ? w2 : w;
        if (n >= interleave_I) n = -1;
    } else {
        n = nt * 16 + r;
        if (n >= N) n = -1;
    }
    bf16_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (n >= 0 && k + j < K) ? src[(int64_t)n * K + k + j] : (bf16_t)0;
    u32x4 o;
    o.x = v[0] | ((uint32_t)v[1] << 16);
    o.y = v[2] | ((uint32_t)v[3] << 16);
    o.z = v[4] | ((uint32_t)v[5] << 16);
    o.w = v[6] | ((uint32_t)v[7] << 16);
    *reinterpret_cast<u32x4*>(p + gid * 8) = o;
}

// Re-tile a standard packed image (16-row tiles) into `th`-row tiles for the decode GEMM:
//   Q[n/th][k/32][g][r < th][k%8]   (th <= 16; th == 16 is the standard image)
// With th = N / 256 (e.g. 14 rows for N = 3584) the skinny GEMM gets exactly one tile per CU.
__global__ void repack_rows_kernel(const bf16_t* __restrict__ p16, bf16_t* __restrict__ q, int N, int KT, int th, int64_t total) {
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one 8-element group per thread
    if (gid >= total) return;
    const int r = (int)(gid % th);
    const int g = (int)((gid / th) % 4);
    const int kt = (int)((gid / (4 * th)) % KT);
    const int64_t nt = gid / ((int64_t)4 * th * KT);
    const int64_t n = nt * th + r;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (n < N) v = *reinterpret_cast<const u32x4*>(p16 + (((n >> 4) * KT + kt) * 64 + g * 16 + (n & 15)) * 8);
    *reinterpret_cast<u32x4*>(q + gid * 8) = v;
}

extern "C" size_t umv_repacked_weight_elems(int N, int K, int th) {
    size_t nt = ((size_t)N + th - 1) / th, kt = (size_t)(K + 31) / 32;
    return nt * kt * 4 * th * 8;
}

extern "C" int umv_repack_weight_rows_bf16(const uint16_t* packed16, uint16_t* out, int N, int K, int th, umv_stream_t stream) {
    UMV_CHECK(packed16 && out && N > 0 && K > 0 && th >= 1 && th <= 16, UMV_ERR_ARG, "repack_weight_rows: bad args (th=%d)", th);
    const int KT = (K + 31) / 32;
    const int64_t total = (int64_t)((N + th - 1) / th) * KT * 4 * th;
    hipLaunchKernelGGL(repack_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, packed16, out, N,
                       KT, th, total);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" size_t umv_packed_weight_elems(int N, int K) {
    size_t ntt = (size_t)(N + 15) / 16, kt = (size_t)(K + 31) / 32;
    return ntt * kt * 512;
}

extern "C" int umv_pack_weight_bf16(const uint16_t* w, uint16_t* packed, int N, int K, umv_stream_t stream) {
    UMV_CHECK(w && packed && N > 0 && K > 0, UMV_ERR_ARG, "pack_weight: bad args");
    int NTT = (N + 15) / 16, KT = (K + 31) / 32;
    int64_t total = (int64_t)NTT * KT * 64;
    int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, packed, N, K, NTT, KT, 0,
                       (const bf16_t*)nullptr);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_pack_weight_swiglu_bf16(const uint16_t* gate, const uint16_t* up, uint16_t* packed, int I, int K,
                                           umv_stream_t stream) {
    UMV_CHECK(gate && up && packed && I > 0 && K > 0, UMV_ERR_ARG, "pack_weight_swiglu: bad args");
    int NTT = 2 * ((I + 15) / 16), KT = (K + 31) / 32;
    int64_t total = (int64_t)NTT * KT * 64;
    int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, gate, packed, 2 * I, K, NTT,
                       KT, I, up);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- e4m3 images
// smallest power of two s with 448 * s >= amax (448 = 0.875 * 2^9 is the largest finite e4m3 value)
__device__ __forceinline__ float fp8_pow2_scale(float amax) {
    if (!(amax > 0.f)) return 1.0f;
    int ea;
    float ma = frexpf(amax, &ea);   // amax = ma * 2^ea, ma in [0.5, 1)
    return ldexpf(1.0f, ma <= 0.875f ? ea - 9 : ea - 8);
}

// One workgroup (256 threads) per packed 16-row tile: row maxima -> scales -> e4m3 image (+ optional W' in bf16).
__global__ __launch_bounds__(256) void quantize_pack_fp8_kernel(const bf16_t* __restrict__ w, const bf16_t* __restrict__ w2,
                                                                uint8_t* __restrict__ p8, float* __restrict__ scale,
                                                                bf16_t* __restrict__ deq, bf16_t* __restrict__ deq2, int rows,
                                                                int K, int KT8) {
    __shared__ float smax[16][17];
    __shared__ float sscale[16];
    const int nt = blockIdx.x, tid = threadIdx.x;
    const bool inter = w2 != nullptr;
    const bf16_t* src = (inter && (nt & 1)) ? w2 : w;
    bf16_t* dq = (inter && (nt & 1)) ? deq2 : deq;
    const int row0 = (inter ? (nt >> 1) : nt) * 16;
    {   // 16 threads per row
        const int r = tid >> 4, c = tid & 15;
        float m = 0.f;
        if (row0 + r < rows)
            for (int k = c; k < K; k += 16) m = fmaxf(m, fabsf(bf2f(src[(int64_t)(row0 + r) * K + k])));
        smax[r][c] = m;
    }
    __syncthreads();
    if (tid < 16) {
        float m = 0.f;
        for (int c = 0; c < 16; ++c) m = fmaxf(m, smax[tid][c]);
        const float s = fp8_pow2_scale(m);
        sscale[tid] = s;
        scale[nt * 16 + tid] = s;
    }
    __syncthreads();
    // one thread per (kt8, lane) 16-byte group
    for (int idx = tid; idx < KT8 * 64; idx += 256) {
        const int lane = idx & 63, kt8 = idx >> 6;
        const int r = lane & 15, g = lane >> 4;
        const bool rowok = row0 + r < rows;
        const float inv = 1.0f / sscale[r];   // exact: a power of two
        uint32_t o[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k0 = kt8 * 64 + h * 32 + g * 8;
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = (rowok && k0 + j < K) ? bf2f(src[(int64_t)(row0 + r) * K + k0 + j]) * inv : 0.f;
            int lo = 0, hi = 0;
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
            o[2 * h] = (uint32_t)lo;
            o[2 * h + 1] = (uint32_t)hi;
            if (dq && rowok) {
                u32x4 qq = {(uint32_t)lo, (uint32_t)hi, 0u, 0u};
                bf16x8 d, unused;
                cvt_fp8x16(qq, sscale[r], d, unused);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (k0 + j < K) dq[(int64_t)(row0 + r) * K + k0 + j] = (bf16_t)d[j];
            }
        }
        u32x4 v = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<u32x4*>(p8 + ((int64_t)nt * KT8 * 64 + idx) * 16) = v;
    }
}

extern "C" size_t umv_packed_weight_fp8_bytes(int N, int K) {
    return ((size_t)(N + 15) / 16) * ((size_t)(K + 63) / 64) * 1024;
}

extern "C" int umv_quantize_pack_weight_fp8(const uint16_t* w, const uint16_t* w_up, uint8_t* packed8, float* scale,
                                            uint16_t* deq, uint16_t* deq_up, int rows, int K, umv_stream_t stream) {
    UMV_CHECK(w && packed8 && scale && rows > 0 && K > 0, UMV_ERR_ARG, "quantize_pack_weight_fp8: bad args");
    UMV_CHECK(!w_up || (rows % 16) == 0, UMV_ERR_ARG, "quantize_pack_weight_fp8: SwiGLU image needs I %% 16 == 0 (I=%d)", rows);
    UMV_CHECK(!(deq_up && !w_up), UMV_ERR_ARG, "quantize_pack_weight_fp8: deq_up without w_up");
    const int ntt = (w_up ? 2 : 1) * ((rows + 15) / 16), KT8 = (K + 63) / 64;
    hipLaunchKernelGGL(quantize_pack_fp8_kernel, dim3(ntt), dim3(256), 0, (hipStream_t)stream, w, w_up, packed8, scale, deq, deq_up,
                       rows, K, KT8);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}


// ----------------------------------------------------------------------------- weight image for the MFMA
// from the decode image P8[nt][k/64][lane = g*16 + r][16 B: (k%64)/32 * 8 + k%8]; one thread per 8-byte piece
__global__ void repack_fp8_mfma_kernel(const uint8_t* __restrict__ p8, uint8_t* __restrict__ out, int KT8, int KT128, int64_t total) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // ((nt*KT128 + kt)*2 + h)*64 + lane)*2 + half
    if (gid >= total) return;
    const int half = (int)(gid & 1);
    const int lane = (int)((gid >> 1) & 63);
    const int h = (int)((gid >> 7) & 1);
    const int64_t tile = gid >> 8;
    const int kt = (int)(tile % KT128);
    const int64_t nt = tile / KT128;
    const int r = lane & 15, g = lane >> 4;
    const int k0 = kt * 128 + g * 32 + h * 16 + half * 8;
    const int kt8 = k0 >> 6, rem = k0 & 63;
    u32x2 v = {0u, 0u};
    if (kt8 < KT8) v = *reinterpret_cast<const u32x2*>(p8 + ((nt * KT8 + kt8) * 64 + ((rem & 31) >> 3) * 16 + r) * 16 + (rem >> 5) * 8);
    *reinterpret_cast<u32x2*>(out + gid * 8) = v;
}

extern "C" size_t umv_packed_weight_fp8_mfma_bytes(int N, int K) {
    return ((size_t)(N + 15) / 16) * ((size_t)(K + 127) / 128) * 2048;
}

extern "C" int umv_repack_weight_fp8_mfma(const uint8_t* packed8, uint8_t* out, int N, int K, umv_stream_t stream) {
    UMV_CHECK(packed8 && out && N > 0 && K > 0, UMV_ERR_ARG, "repack_weight_fp8_mfma: bad args");
    const int KT8 = (K + 63) / 64, KT128 = (K + 127) / 128;
    const int64_t total = (int64_t)((N + 15) / 16) * KT128 * 2 * 64 * 2;
    hipLaunchKernelGGL(repack_fp8_mfma_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, packed8, out,
                       KT8, KT128, total);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- MXFP4 images
// e2m1 codes with one E8M0 power-of-two scale per 32 consecutive k of a row (decode GEMM: gemm_mxfp4.hip).
// Format (include/unimedvl_hip.h): s = 2^e, e the smallest integer with 6 * 2^e >= max|W[block]| (6 = the largest e2m1 value, so
// nothing is clipped), clamped to [-127, 127], e = 0 for an all-zero block; q = rne_e2m1(W / s) with the sign kept (a negative value
// that rounds to zero is code 8, -0); W' = q * s is exact in bf16.
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
//
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

// ----------------------------------------------------------------------------- the exact 13-bit image ("z13")
// bf16 weights without loss at 13 bits each (decode GEMM: gemm_z13.hip; format: include/unimedvl_hip.h).  Made from the packed bf16
// image, which stays resident as the fallback of flagged blocks: lane (r, g) of record (pair p, unit u) holds the 32 weights of the
// bf16 image's fragments (tile 2p + tt, k-tile 2u + h), fragment number f = 2*tt + h.
//   base[p]  = the largest exponent field below 255 among the pair's rows (rows at or beyond N do not count)
//   code     = base - field, codable when field != 255 and code <= 30; anything else is written as code 0 and, in a row below N,
//              flags its (pair, 512-k block)
#define Z13_RECORD 3328
static inline size_t z13_head_bytes_host(size_t NPT) { return (NPT * 16 + 255) / 256 * 256; }

__global__ __launch_bounds__(256) void z13_base_kernel(const bf16_t* __restrict__ p16, unsigned long long* __restrict__ head, int N, int KT,
                                                       int NTT) {
    __shared__ uint32_t smax[256];
    const int p = blockIdx.x, tid = threadIdx.x;
    uint32_t m = 0;
    for (int tt = 0; tt < 2; ++tt) {
        const int nt = 2 * p + tt;
        if (nt >= NTT) continue;
        for (int64_t idx = tid; idx < (int64_t)KT * 64; idx += 256) {       // one 8-element group per step
            const int lane = (int)(idx & 63);
            if (nt * 16 + (lane & 15) >= N) continue;
            const u32x4 v = *reinterpret_cast<const u32x4*>(p16 + ((int64_t)nt * KT * 64 + idx) * 8);
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t f0 = (wd[j] >> 7) & 0xFFu, f1 = (wd[j] >> 23) & 0xFFu;
                if (f0 != 255u) m = max(m, f0);
                if (f1 != 255u) m = max(m, f1);
            }
        }
    }
    smax[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) smax[tid] = max(smax[tid], smax[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {              // the pair's 16-byte head entry: flags (the encode kernel ORs into them), base, zeros
        head[2 * p] = 0;
        head[2 * p + 1] = smax[0];
    }
}

// one thread per (pair, unit, lane); z13_base_kernel has zeroed the flags
__global__ __launch_bounds__(256) void z13_encode_kernel(const bf16_t* __restrict__ p16, uint8_t* __restrict__ img, int N, int KT8, int NTT,
                                                         int NPT, int64_t total) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int lane = (int)(gid & 63);
    const int u = (int)((gid >> 6) % KT8);
    const int p = (int)((gid >> 6) / KT8);
    const int KT = 2 * KT8;
    const uint32_t base = img[(int64_t)p * 16 + 8];
    uint32_t sm[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, nib[4] = {0u, 0u, 0u, 0u}, top = 0u;
    bool flag = false;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int nt = 2 * p + tt;
        if (nt >= NTT) continue;                                   // the missing tile of a ragged pair: zeros
        const bool counts = nt * 16 + (lane & 15) < N;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(p16 + (((int64_t)nt * KT + 2 * u + h) * 64 + lane) * 8);
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
            const int f = 2 * tt + h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t w = (wd[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
                const uint32_t field = (w >> 7) & 0xFFu;
                const bool codable = field != 255u && base >= field && base - field <= 30u;
                const uint32_t code = codable ? base - field : 0u;
                flag = flag || (counts && !codable);
                const int byte = ((j & 1) << 1) | ((j >> 1) & 1), q = j >> 2;
                sm[tt][2 * h + (j >> 2)] |= (((w >> 8) & 0x80u) | (w & 0x7Fu)) << (8 * (j & 3));
                nib[f] |= (code & 15u) << (8 * byte + 4 * q);
                top |= (code >> 4) << (8 * byte + 2 * f + q);
            }
        }
    }
    uint8_t* rec = img + ((int64_t)NPT * 16 + 255) / 256 * 256 + ((int64_t)p * KT8 + u) * Z13_RECORD;
    *reinterpret_cast<u32x4*>(rec + lane * 16) = (u32x4){sm[0][0], sm[0][1], sm[0][2], sm[0][3]};
    *reinterpret_cast<u32x4*>(rec + 1024 + lane * 16) = (u32x4){sm[1][0], sm[1][1], sm[1][2], sm[1][3]};
    *reinterpret_cast<u32x4*>(rec + 2048 + lane * 16) = (u32x4){nib[0], nib[1], nib[2], nib[3]};
    *reinterpret_cast<uint32_t*>(rec + 3072 + lane * 4) = top;
    if (flag) atomicOr(reinterpret_cast<unsigned long long*>(img) + 2 * p, 1ull << (u >> 3));
}

extern "C" size_t umv_packed_weight_z13_bytes(int N, int K) {
    if (N <= 0 || K <= 0) return 0;
    const size_t np = ((size_t)(N + 15) / 16 + 1) / 2, kt8 = (size_t)(K + 63) / 64;
    return z13_head_bytes_host(np) + np * kt8 * Z13_RECORD;
}

extern "C" int umv_pack_weight_z13(const uint16_t* packed16, uint8_t* z13, int N, int K, umv_stream_t stream) {
    UMV_CHECK(packed16 && z13 && N > 0 && K > 0, UMV_ERR_ARG, "pack_weight_z13: bad args");
    UMV_CHECK((K % 64) == 0 && K <= 32768, UMV_ERR_ARG, "pack_weight_z13: K (%d) must be a multiple of 64 and <= 32768", K);
    UMV_CHECK(((uintptr_t)packed16 % 16) == 0 && ((uintptr_t)z13 % 256) == 0, UMV_ERR_ARG,
              "pack_weight_z13: the bf16 image must be 16-byte and the 13-bit image 256-byte aligned");
    const int NTT = (N + 15) / 16, NPT = (NTT + 1) / 2, KT8 = K / 64;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(z13_base_kernel, dim3(NPT), dim3(256), 0, s, (const bf16_t*)packed16,
                       reinterpret_cast<unsigned long long*>(z13), N, 2 * KT8, NTT);
    UMV_LAUNCH_CHECK();
    const int64_t total = (int64_t)NPT * KT8 * 64;
    hipLaunchKernelGGL(z13_encode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const bf16_t*)packed16, z13, N, KT8, NTT,
                       NPT, total);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
