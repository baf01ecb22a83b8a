// Weight-streaming decode GEMM of libunimedvl_hip (gfx950), M <= 64: one kernel body for the three weight images.  Internal to csrc/.
//
// out[m, n] = epi(sum_k x[m, k] W[n, k]), HBM-bound.  One workgroup = NT n-tiles x all of K (or of one K split); its 8 waves take
// contiguous K slices and reduce through LDS (deterministic, no atomics).  Weight bytes go straight from HBM to VGPRs (no LDS round
// trip: each byte is used once) and become the A operand of v_mfma_f32_16x16x32_bf16, x^T the B operand: the accumulator of lane
// (r, g) holds out[m = r][n = g*4 + reg].  Each wave keeps U weight units per n-tile in flight and, when DB, prefetches the next chunk
// while the MFMAs of the current one issue.
//
// A format policy says what a lane loads per weight UNIT along k and how a unit becomes bf16 A-fragments; the body does the rest:
//   SkBf16<NT>    bf16 image, unit = one 32-k tile (KH = 1 k half); th-row tiles; the fused RMSNorm prologue (NORM)
//   SkE4m3<NT>    e4m3 image + one power-of-two scale per row, unit = 64 k (KH = 2): 16 B per lane and n-tile -> two fragments
//   SkMxfp4<NP>   MXFP4 codes + E8M0 block scales, unit = 64 k: 16 B + 4 scale bytes per lane and tile PAIR -> four fragments
//   SkZ13<NP>     the exact 13-bit image of bf16 weights (sign + mantissa bytes, 5-bit exponent codes below a per-pair base), unit =
//                 64 k: 52 B per lane and tile pair -> four fragments; HALVES: the K slices are cut in 32-k halves, so they are SkBf16's
//                 for every K and every split (a half outside the slice decodes to zeros)
// (the images: pack.hip).  The MFMAs of a chunk issue in the order (u, k half, tile, mb) and every accumulator takes its k in ascending
// order, so on the same K slices (K % 512 == 0, no split-K) the three images of the same W' give the same bits.
//
// NORM fuses Qwen2RMSNorm (modeling_qwen2.py:89-94) of the x rows into the prologue: RMSNorm(x) * norm_w is staged once per workgroup
// into LDS in B-fragment order, with the reference's two bf16 roundings, and the MFMAs read x from there.
#pragma once
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "gemm_epilogue.h"
#include "gemm_internal.h"
#include "quant.h"

#define SK_WAVES 8
#define SK_XMAX 16   // NORM: K <= 8*16*32 = 4096

// ----------------------------------------------------------------------------- format policies
// Built by every lane for the workgroup's first n-tile nt0 (KT = units along K, NTT = n-tiles, NPT = MXFP4 tile pairs): load()
// fetches one unit (zeros where !ok), frags() turns it into the A-fragments wf[k half][n-tile].  TH = rows per n-tile.
template <int NT_>
struct SkBf16 {       // tile (nt, kt) holds [g][r < TH][8]: TH = a.tile_rows (16 standard); lanes r >= TH of the exact-partition copies carry no row
    static constexpr int NT = NT_, KH = 1;
    static constexpr bool HALVES = false;
    struct Unit { bf16x8 w[NT]; };
    int TH, tile_elems;
    bool rowlane;
    const bf16_t* wbase[NT];
    __device__ __forceinline__ SkBf16(const umv_gemm_args& a, int KT, int NTT, int, int nt0, int lane) {
        const int r = lane & 15, g = lane >> 4;
        TH = a.tile_rows > 0 ? a.tile_rows : 16;
        tile_elems = 4 * TH * 8;
        rowlane = r < TH;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool tv = (nt0 + t) < NTT;
            wbase[t] = a.wp + ((int64_t)(tv ? nt0 + t : 0) * KT) * tile_elems + (g * TH + (rowlane ? r : 0)) * 8;
        }
    }
    __device__ __forceinline__ void load(Unit& b, int kt, bool ok) const {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            b.w[t] = (ok && rowlane) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wbase[t] + (int64_t)kt * tile_elems)) : zero_frag();
    }
    __device__ __forceinline__ void frags(const Unit& b, bf16x8 (&wf)[KH][NT]) const {
#pragma unroll
        for (int t = 0; t < NT; ++t) wf[0][t] = b.w[t];
    }
};

template <int NT_>
struct SkE4m3 {       // P8[nt][kt8][lane][16 B] (bytes 0..7: k half 0, 8..15: k half 1) + one f32 scale per row in packed order
    static constexpr int NT = NT_, KH = 2, TH = 16;
    static constexpr bool HALVES = false;
    struct Unit { u32x4 w[NT]; };
    const uint8_t* wbase[NT];
    float wscale[NT];
    __device__ __forceinline__ SkE4m3(const umv_gemm_args& a, int KT8, int NTT, int, int nt0, int lane) {
        const uint8_t* wq = reinterpret_cast<const uint8_t*>(a.wp);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool tv = (nt0 + t) < NTT;
            const int nt = tv ? nt0 + t : 0;
            wbase[t] = wq + ((int64_t)nt * KT8 * 64 + lane) * 16;
            wscale[t] = a.w_scale[nt * 16 + (lane & 15)];
        }
    }
    __device__ __forceinline__ void load(Unit& b, int kt, bool ok) const {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            b.w[t] = ok ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase[t] + (int64_t)kt * 1024)) : (u32x4){0u, 0u, 0u, 0u};
    }
    __device__ __forceinline__ void frags(const Unit& b, bf16x8 (&wf)[KH][NT]) const {
#pragma unroll
        for (int t = 0; t < NT; ++t) cvt_fp8x16(b.w[t], wscale[t], wf[0][t], wf[1][t]);
    }
};

template <int NP>
struct SkMxfp4 {      // codes C[p][kt8][lane][16 B] of tile pairs (4 B per (tile, k half)), then scales S[p][kt8][r][4 B]
    static constexpr int NT = 2 * NP, KH = 2, TH = 16;
    static constexpr bool HALVES = false;
    struct Unit { u32x4 w[NP]; uint32_t s[NP]; };
    const uint8_t* wbase[NP];
    const uint8_t* sbase[NP];
    __device__ __forceinline__ SkMxfp4(const umv_gemm_args& a, int KT8, int, int NPT, int, int lane) {
        const uint8_t* img = reinterpret_cast<const uint8_t*>(a.wp);
        const uint8_t* scales = img + (int64_t)NPT * KT8 * 1024;
        const int p0 = blockIdx.x * NP;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = (p0 + i) < NPT ? p0 + i : 0;          // pairs past the end re-read pair 0; their columns are never stored
            wbase[i] = img + ((int64_t)p * KT8 * 64 + lane) * 16;
            sbase[i] = scales + ((int64_t)p * KT8 * 16 + (lane & 15)) * 4;
        }
    }
    __device__ __forceinline__ void load(Unit& b, int kt, bool ok) const {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            b.w[i] = ok ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase[i] + (int64_t)kt * 1024)) : (u32x4){0u, 0u, 0u, 0u};
            b.s[i] = ok ? *reinterpret_cast<const uint32_t*>(sbase[i] + (int64_t)kt * 64) : 0x7F7F7F7Fu;
        }
    }
    __device__ __forceinline__ void frags(const Unit& b, bf16x8 (&wf)[KH][NT]) const {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t s = b.s[i];
            wf[0][2 * i] = cvt_fp4x8(b.w[i].x, e8m0_scale(s & 0xFFu));
            wf[1][2 * i] = cvt_fp4x8(b.w[i].y, e8m0_scale((s >> 8) & 0xFFu));
            wf[0][2 * i + 1] = cvt_fp4x8(b.w[i].z, e8m0_scale((s >> 16) & 0xFFu));
            wf[1][2 * i + 1] = cvt_fp4x8(b.w[i].w, e8m0_scale(s >> 24));
        }
    }
};

// The 13-bit image (include/unimedvl_hip.h, pack.hip): per (tile pair, 64 k) one 3328-byte record - two sign/mantissa planes (tile 2p,
// 2p + 1: 16 B per lane, k half 0 then 1), the low-nibble plane of the exponent codes (16 B per lane, dword f = fragment 2*tile + k half)
// and their top-bit plane (4 B per lane).  bf16 bits of a weight = s << 15 | (base - code) << 7 | m.  Per fragment the codes are first
// gathered to one byte each (qa: weights 0..3, qb: 4..7, in the byte order 0, 2, 1, 3 so that a packed 16-bit operation sees the two
// weights of an output dword), then per output dword: code -> (base - code) << 7 (v_pk_mad_u16 by -128), the s:m7 byte to both bytes of
// its half (v_perm_b32), one bit-select.  A k half outside the wave's slice takes the constants (0, 0, all ones) and decodes to zeros
// whatever its bytes are: no extra VALU.
typedef __attribute__((ext_vector_type(2))) unsigned short umv_u16x2;
__device__ __forceinline__ uint32_t z13_pk_mad(uint32_t q, uint32_t mul, uint32_t add) {
    const umv_u16x2 r = __builtin_bit_cast(umv_u16x2, q) * __builtin_bit_cast(umv_u16x2, mul) + __builtin_bit_cast(umv_u16x2, add);
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t z13_pk_shr8(uint32_t q) {
    const umv_u16x2 r = __builtin_bit_cast(umv_u16x2, q) >> (umv_u16x2){8, 8};
    return __builtin_bit_cast(uint32_t, r);
}
// E = fragment number 2*tile + k half (where its top bits sit in t); sm0 / sm1 = the 8 s:m7 bytes, n = the 8 low nibbles
template <int E>
__device__ __forceinline__ bf16x8 z13_frag(uint32_t sm0, uint32_t sm1, uint32_t n, uint32_t t, uint32_t mul, uint32_t base7, uint32_t emask) {
    constexpr int EA = 2 * E, EB = 2 * E + 1;
    const uint32_t ta = EA < 4 ? t << (4 - EA) : t >> (EA - 4), tb = EB < 4 ? t << (4 - EB) : t >> (EB - 4);
    const uint32_t qa = (ta & 0x10101010u) | (n & 0x0F0F0F0Fu), qb = (tb & 0x10101010u) | ((n >> 4) & 0x0F0F0F0Fu);
    const uint32_t e[4] = {z13_pk_mad(qa, mul, base7), z13_pk_mad(z13_pk_shr8(qa), mul, base7), z13_pk_mad(qb, mul, base7),
                           z13_pk_mad(z13_pk_shr8(qb), mul, base7)};
    const uint32_t p[4] = {__builtin_amdgcn_perm(sm0, sm0, 0x01010000u), __builtin_amdgcn_perm(sm0, sm0, 0x03030202u),
                           __builtin_amdgcn_perm(sm1, sm1, 0x01010000u), __builtin_amdgcn_perm(sm1, sm1, 0x03030202u)};
    u32x4 o;
    o.x = (e[0] & emask) | (p[0] & ~emask);
    o.y = (e[1] & emask) | (p[1] & ~emask);
    o.z = (e[2] & emask) | (p[2] & ~emask);
    o.w = (e[3] & emask) | (p[3] & ~emask);
    return __builtin_bit_cast(bf16x8, o);
}

#define Z13_RECORD 3328
// bytes before the records: one 16-byte entry per pair (flags u64, base u8, 7 zero bytes), rounded up to 256
__host__ __device__ __forceinline__ int64_t z13_head_bytes(int NPT) { return ((int64_t)NPT * 16 + 255) / 256 * 256; }

template <int NP>
struct SkZ13 {        // head H[NPT][16 B] = (flags u64, base u8, 0...), then (256-aligned) records R[p][kt8][3328 B]; a.wp = the image
    static constexpr int NT = 2 * NP, KH = 2, TH = 16;
    static constexpr bool HALVES = true;
    struct Unit { u32x4 sm[NP][2]; u32x4 n[NP]; uint32_t t[NP]; };
    const uint8_t* rec[NP];      // wave-uniform: the pair's records
    uint32_t base7[NP];          // (base << 7) in both halves
    uint32_t lane16, lane4;
    __device__ __forceinline__ SkZ13(const umv_gemm_args& a, int KT8, int, int NPT, int, int lane) {
        const uint8_t* img = reinterpret_cast<const uint8_t*>(a.wp);
        const int p0 = blockIdx.x * NP;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = (p0 + i) < NPT ? p0 + i : 0;          // pairs past the end re-read pair 0; their columns are never stored
            rec[i] = img + z13_head_bytes(NPT) + (int64_t)p * KT8 * Z13_RECORD;
            const uint32_t b = reinterpret_cast<const uint32_t*>(img)[4 * p + 2] & 0xFFu;   // next to the flags the kernel has just read
            base7[i] = (b << 7) * 0x10001u;
        }
        lane16 = (uint32_t)lane * 16u;
        lane4 = 3072u + (uint32_t)lane * 4u;
    }
    __device__ __forceinline__ void load(Unit& b, int kt, bool ok) const {
        const int ktu = __builtin_amdgcn_readfirstlane(kt);      // a wave's unit: scalar base + lane offset addressing
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint8_t* r = rec[i] + (int64_t)ktu * Z13_RECORD;
            const u32x4 z = {0u, 0u, 0u, 0u};
            b.sm[i][0] = ok ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(r + lane16)) : z;
            b.sm[i][1] = ok ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(r + 1024 + lane16)) : z;
            b.n[i] = ok ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(r + 2048 + lane16)) : z;
            b.t[i] = ok ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(r + lane4)) : 0u;
        }
    }
    // v0 / v1: k half 0 / 1 of the unit lies inside the wave's slice (wave-uniform)
    __device__ __forceinline__ void frags(const Unit& b, bf16x8 (&wf)[KH][NT], bool in0, bool in1) const {
        const bool v0 = __builtin_amdgcn_readfirstlane((int)in0) != 0, v1 = __builtin_amdgcn_readfirstlane((int)in1) != 0;   // constants in SGPRs
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t mul0 = v0 ? 0xFF80FF80u : 0u, mul1 = v1 ? 0xFF80FF80u : 0u;
            const uint32_t b0 = v0 ? base7[i] : 0u, b1 = v1 ? base7[i] : 0u;
            const uint32_t m0 = v0 ? 0x7F807F80u : 0xFFFFFFFFu, m1 = v1 ? 0x7F807F80u : 0xFFFFFFFFu;
            wf[0][2 * i] = z13_frag<0>(b.sm[i][0].x, b.sm[i][0].y, b.n[i].x, b.t[i], mul0, b0, m0);
            wf[1][2 * i] = z13_frag<1>(b.sm[i][0].z, b.sm[i][0].w, b.n[i].y, b.t[i], mul1, b1, m1);
            wf[0][2 * i + 1] = z13_frag<2>(b.sm[i][1].x, b.sm[i][1].y, b.n[i].z, b.t[i], mul0, b0, m0);
            wf[1][2 * i + 1] = z13_frag<3>(b.sm[i][1].z, b.sm[i][1].w, b.n[i].w, b.t[i], mul1, b1, m1);
        }
    }
};

// ----------------------------------------------------------------------------- reduction and epilogue
// Every wave parks its NT x MB accumulator fragments in `red` ([NW waves][NT*MB][64] f32x4), the sums run in wave order 0..NW-1, then
// bias / activation / residual / SwiGLU (with the argmax / sampling keys of the lm_head) or, for split-K (nsplit > 1), the raw fp32
// partial sums of split blockIdx.y.  Tiles of TH rows (TH < 16: the exact-partition bf16 images).  The caller has made `red` free (no
// wave still reads its x staging there).  ROWS: the lm_head keys and statistics take every row's temperature and sampling key from the
// per-row table `rows` (include/unimedvl_hip.h, umv_row_sampling; a kernel argument of its own behind umv_gemm_args) - instantiations of
// their own (gemm.hip, gemm_z13.hip: the shapes an lm_head call reaches), so that no other kernel's code, arguments or registers move.
template <int NW, int NT, int MB, bool ROWS = false>
__device__ __forceinline__ void skinny16_reduce_epilogue(const umv_gemm_args& a, float* red, const f32x4 (&acc)[NT][MB], int tid,
                                                         int lane, int wave, int nt0, int NTT, int nsplit, int TH,
                                                         const umv_row_sampling* __restrict__ rows = nullptr) {
    constexpr int E4 = NT * MB;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) reinterpret_cast<f32x4*>(red)[(wave * E4 + t * MB + mb) * 64 + lane] = acc[t][mb];
    __syncthreads();
    EpiCtx e{a.bias, a.residual, a.ldr, a.out, a.ldo, a.N, a.epilogue};
    if (nsplit > 1) {   // partial sums: fp32, no bias / activation / residual (the consumer kernel finishes the row)
        e.out = reinterpret_cast<float*>(a.out) + (int64_t)blockIdx.y * a.split_stride;
        e.flags = UMV_EPI_OUT_F32;
    }
    if (a.epilogue & UMV_EPI_SWIGLU) {
        // tiles come in (gate, up) pairs; NT is even
        for (int idx = tid; idx < (NT / 2) * MB * 64; idx += NW * 64) {
            int l = idx & 63;
            int f = idx >> 6;  // pair*MB + mb
            int pair = f / MB, mb = f % MB;
            f32x4 sg = {0, 0, 0, 0}, su = {0, 0, 0, 0};
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                sg += reinterpret_cast<f32x4*>(red)[(w * E4 + (2 * pair) * MB + mb) * 64 + l];
                su += reinterpret_cast<f32x4*>(red)[(w * E4 + (2 * pair + 1) * MB + mb) * 64 + l];
            }
            int m = mb * 16 + (l & 15);
            int ntile = nt0 + 2 * pair;
            if (m < a.M && ntile < NTT) {
                int64_t orow = a.row_idx ? (int64_t)a.row_idx[m] : (int64_t)m;
                int c0 = (ntile >> 1) * 16 + (l >> 4) * 4;
                float gg[4] = {sg.x, sg.y, sg.z, sg.w}, uu[4] = {su.x, su.y, su.z, su.w};
                epi_swiglu4(e, orow, c0, a.N / 2, gg, uu);
            }
        }
    } else {
        for (int idx = tid; idx < E4 * 64; idx += NW * 64) {
            int l = idx & 63;
            int f = idx >> 6;  // t*MB + mb
            int t = f / MB, mb = f % MB;
            f32x4 s = {0, 0, 0, 0};
#pragma unroll
            for (int w = 0; w < NW; ++w) s += reinterpret_cast<f32x4*>(red)[(w * E4 + f) * 64 + l];
            int m = mb * 16 + (l & 15);
            int n0 = (nt0 + t) * TH + (l >> 4) * 4;
            int nend = min(a.N, (nt0 + t) * TH + TH);            // rows of this tile stop at TH
            const bool valid = m < a.M && n0 < nend;
            float fin[4] = {0.f, 0.f, 0.f, 0.f};
            if (valid) {
                int64_t orow = a.row_idx ? (int64_t)a.row_idx[m] : (int64_t)m;
                EpiCtx et = e;
                et.N = nend;
                epi_store4(et, orow, n0, s.x, s.y, s.z, s.w, fin);
            }
            if constexpr (ROWS) {
                if (a.argmax_partial && nt0 + t < NTT) {   // wave-uniform; row m's own temperature and (seed, draw, stream): a greedy and
                    // a sampled row may sit in one fragment - the branch on temp is per lane, the shuffles are everyone's
                    const float temp = valid ? row_sampling_temp(rows, m) : 0.f;
                    epi_argmax_tile_keyed(a.argmax_partial, NTT, m, nt0 + t, l, valid, n0, nend, fin, temp,
                                          [&] { return row_sampling_key(rows, m); });
                    if (a.lse_partial) epi_lse_tile(a.lse_partial, NTT, m, nt0 + t, l, valid, n0, nend, fin, temp);
                }
            } else if (a.argmax_partial && nt0 + t < NTT) { // wave-uniform: greedy argmax rides on the lm_head epilogue
                epi_argmax_tile(a.argmax_partial, NTT, m, nt0 + t, l, valid, n0, nend, fin, a.sample_temperature, a.sample_seed, a.sample_step);
                if (a.lse_partial) epi_lse_tile(a.lse_partial, NTT, m, nt0 + t, l, valid, n0, nend, fin, a.sample_temperature);   // and the softmax statistics
            }
        }
    }
}

// ----------------------------------------------------------------------------- the body
// XL (round 4): x reaches the MFMAs in FULL 128-byte lines (64 k of a row).  The plain form loads x in fragment shape - per wave
// instruction 16 rows x 64 bytes, half a line per row - and every workgroup re-reads all of x through L2 -> L1 (at 8 rows that is half
// the bf16 weight bytes, at 32 rows twice them).  Here a wave loads one line of 8 rows per instruction (lane L: row L >> 3, chunk
// (L & 7) ^ (L >> 3)), parks the piece in its own KiB of LDS (lane-linear ds_write_b128: the image is row-major, XOR-swizzled by the
// row) and reads the B fragments of the line's two k halves back conflict free (lane (r, g), k half h: chunk (4h + g) ^ (r & 7) of
// row r) - the tiled kernel's full-line staging (SCHED = 3) without the DMA.  Same operands, same MFMAs, same order: bit-identical to
// the plain form.  XL = 2: two pieces per 16-row tile; XL = 1 (M <= 8): one piece, rows 8..15 of a fragment re-read rows 0..7 (their
// output columns are never stored).  Needs whole lines per chunk.
template <class F, int MB, int U, int XL>
struct SkBuf {
    typename F::Unit w[U];
    bf16x8 x[U][F::KH][MB];
    u32x4 xp[XL ? U * F::KH / 2 : 1][XL == 1 ? 1 : (XL ? 2 * MB : 1)];     // XL: the x pieces of the chunk's lines on their way to LDS
};

template <class F, int MB, int U, bool DB, int NORM, int XL, bool ROWS = false>   // NORM: 0 = off, 8 / 16 = fused RMSNorm keeping that many x rows
__device__ __forceinline__ void gemm_skinny_body(const umv_gemm_args& a, int KT, int NTT, int NPT, const umv_row_sampling* rows = nullptr) {
    constexpr int NT = F::NT, KH = F::KH;
    extern __shared__ __attribute__((aligned(16))) float red[];  // [SK_WAVES][NT*MB*4][64] (+ norm partials and x) / XL staging
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nt0 = blockIdx.x * NT;

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

    // split-K (a.k_splits > 1): blockIdx.y owns the units [ks0, ks1) and stores raw fp32 partial sums
    // HALVES: the same cut in 32-k halves [g_begin, g_end) - SkBf16's slices - and the units that hold them
    const int nsplit = a.k_splits > 1 ? a.k_splits : 1;
    constexpr int SG = F::HALVES ? KH : 1;                          // slice granules per unit
    const int KTG = KT * SG;
    const int kts = (KTG + nsplit - 1) / nsplit;
    const int ks0 = (int)blockIdx.y * kts, ks1 = min(KTG, ks0 + kts);
    const int kt_per = (max(0, ks1 - ks0) + SK_WAVES - 1) / SK_WAVES;
    const int g_begin = ks0 + wave * kt_per;
    const int g_end = min(ks1, g_begin + kt_per);
    const int kt_begin = g_begin / SG;
    const int kt_end = g_end > g_begin ? (g_end + SG - 1) / SG : kt_begin;
    // XL works on whole lines: a slice that starts inside one (a bf16 slice on an odd k-tile) starts at the line's first unit, with
    // that unit's weights masked to zero - an MFMA that adds exact zeros (the x it multiplies is the neighbour wave's, finite).
    // PRECONDITION of "bit-identical to the plain form": x is finite.  Where x holds Inf / NaN in the neighbour's k-tile the masked
    // product is 0 * Inf = NaN and this wave's partial sum becomes NaN where the plain form's would not (the row's final result is
    // Inf / NaN either way - the neighbour's own product sees the same value; only WHICH of the two non-finite values differs).
    constexpr int UPL = 2 / KH;                                      // units per line
    const int kt_lo = XL != 0 ? (kt_begin & -UPL) : kt_begin;
    const int nk = max(0, kt_end - kt_lo);
    const int nchunks = (nk + U - 1) / U;
    const F f(a, KT, NTT, NPT, nt0, lane);
    static_assert(!XL || ((U * KH) % 2 == 0 && NORM == 0), "full-line x staging: whole lines per chunk, no fused norm");
    static_assert(!F::HALVES || NORM == 0, "half-unit slices: no fused norm");
    static_assert(XL != 1 || MB == 1, "one-piece staging serves one 16-row tile of at most 8 valid rows");
    constexpr int XLN = U * KH / 2, XLP = XL == 1 ? 1 : 2 * MB;     // lines per chunk, pieces per line
    // XL: this lane's row of each 8-row piece and its 16-byte chunk of the line
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
    char* xstage = reinterpret_cast<char*>(red) + wave * (XLN * XLP * 1024);      // XL: this wave's own staging KiBs
    auto load_chunk = [&](int c, SkBuf<F, MB, U, XL>& b) {
        if constexpr (XL != 0) {
#pragma unroll
            for (int ln = 0; ln < XLN; ++ln) {
                const int kt = kt_lo + c * U + ln * UPL;
                const int k = kt * (32 * KH) + xchunk * 8;
#pragma unroll
                for (int q = 0; q < XLP; ++q)
                    b.xp[ln][q] = (kt < kt_end && xpvalid[q] && k < a.K) ? *reinterpret_cast<const u32x4*>(xprow[q] + (int64_t)kt * (32 * KH))
                                                                         : (u32x4){0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kt = kt_lo + c * U + u;
            const bool ok = kt >= kt_begin && kt < kt_end;
            f.load(b.w[u], kt, ok);
            if (!NORM && XL == 0) {
#pragma unroll
                for (int h = 0; h < KH; ++h) {
                    const int k = kt * (32 * KH) + h * 32 + g * 8;
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) b.x[u][h][mb] = (ok && xvalid[mb] && k < a.K) ? ldg_frag(xrow[mb] + k) : zero_frag();
                }
            }
        }
    };
    SkBuf<F, MB, U, XL> b0, b1;
    if (nchunks > 0) load_chunk(0, b0);

    constexpr int MP = NORM ? NORM : 8;          // NORM: x rows kept
    bf16_t* xl = reinterpret_cast<bf16_t*>(red + SK_WAVES * NT * MB * 4 * 64 + SK_WAVES * 16);
    if constexpr (NORM != 0) {
        static_assert(!NORM || MB == 1, "fused RMSNorm supports M <= 16");
        // Stage RMSNorm(x) * norm_w ONCE per workgroup into LDS, already in MFMA B-fragment order:
        // slot (kt, g, r) holds the 8 bf16 of row r at k = kt*32 + g*8.
        float* part = red + SK_WAVES * NT * MB * 4 * 64;   // [SK_WAVES][16]
        const int rr = tid & (MP - 1);
        constexpr int sh = MP == 8 ? 3 : 4;        // log2(MP)
        constexpr int XS = MP;                     // 16-byte groups per thread: (4096/32) * 4 * MP / 512
        const int nslots = KT * 4 * MP;
        const bool rowok = rr < a.M;
        const bf16_t* xr = a.x + (rowok ? (a.row_idx ? (int64_t)a.row_idx[rr] : (int64_t)rr) : 0) * a.ldx;
        // ONE batch of loads per phase: a loop of dependent L2 round trips (7 per pass at K = 3584) costs ~10 us per
        // workgroup, a batch about one round trip.  Phase 1: x -> registers -> row sums of squares, raw x parked in LDS.
        {
            bf16x8 xv[XS];
#pragma unroll
            for (int i = 0; i < XS; ++i) {
                const int sidx = tid + i * SK_WAVES * 64;
                const int k = (sidx >> (sh + 2)) * 32 + ((sidx >> sh) & 3) * 8;
                xv[i] = (sidx < nslots && k < a.K && rowok) ? ldg_frag(xr + k) : zero_frag();
            }
            float ss = 0.f;
#pragma unroll
            for (int i = 0; i < XS; ++i) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float fv = bf2f((bf16_t)xv[i][j]);
                    ss += fv * fv;
                }
                const int sidx = tid + i * SK_WAVES * 64;
                if (sidx < nslots) *reinterpret_cast<bf16x8*>(xl + (int64_t)sidx * 8) = xv[i];
            }
            // lanes sharing a row: lane & (MP-1)
            if (MP == 8) ss += __shfl_xor(ss, 8, 64);
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            if (lane < MP) part[wave * 16 + lane] = ss;
        }
        // phase 2: norm_w batch (in flight across the barrier), then normalise the thread's own slots in place
        bf16x8 wv[XS];
#pragma unroll
        for (int i = 0; i < XS; ++i) {
            const int sidx = tid + i * SK_WAVES * 64;
            const int k = (sidx >> (sh + 2)) * 32 + ((sidx >> sh) & 3) * 8;
            wv[i] = (sidx < nslots && k < a.K) ? ldg_frag(a.norm_w + k) : zero_frag();
        }
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < SK_WAVES; ++w) tot += part[w * 16 + rr];
        const float rstd = rsqrt_ieee(tot / (float)a.K + a.norm_eps);
#pragma unroll
        for (int i = 0; i < XS; ++i) {
            const int sidx = tid + i * SK_WAVES * 64;
            if (sidx < nslots) {
                bf16x8 v = *reinterpret_cast<const bf16x8*>(xl + (int64_t)sidx * 8), o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(bf2f((bf16_t)wv[i][j]) * rbf(bf2f((bf16_t)v[j]) * rstd));   // two roundings
                *reinterpret_cast<bf16x8*>(xl + (int64_t)sidx * 8) = o;
            }
        }
        __syncthreads();
    }
    // the MFMAs of chunk c.  XL: its pieces go through the wave's LDS KiBs first and come back as the B fragments (LDS operations of
    // one wave execute in order and nobody else touches these bytes: no barrier)
    auto consume = [&](SkBuf<F, MB, U, XL>& b, int c) {
        if constexpr (NORM != 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kt = min(kt_begin + c * U + u, KT - 1);
                bf16x8 xf = *reinterpret_cast<const bf16x8*>(xl + ((int64_t)(kt * 4 + g) * MP + (r & (MP - 1))) * 8);
                bf16x8 wf[KH][NT];
                f.frags(b.w[u], wf);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t][0] = mfma16(wf[0][t], xf, acc[t][0]);
            }
        } else {
            if constexpr (XL != 0) {
#pragma unroll
                for (int ln = 0; ln < XLN; ++ln)
#pragma unroll
                    for (int q = 0; q < XLP; ++q) *reinterpret_cast<u32x4*>(xstage + (ln * XLP + q) * 1024 + lane * 16) = b.xp[ln][q];
                const int rr = XL == 1 ? (r & 7) : r;
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int h = 0; h < KH; ++h)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) {
                            const int j = u * KH + h;        // k half j of the chunk: line j >> 1, its half j & 1
                            b.x[u][h][mb] = *reinterpret_cast<const bf16x8*>(xstage + (j >> 1) * (XLP * 1024) + (mb * 16 + rr) * 128 +
                                                                             ((((j & 1) * 4 + g) ^ (rr & 7)) << 4));
                        }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bf16x8 wf[KH][NT];
                if constexpr (F::HALVES) {
                    const int g0 = (kt_lo + c * U + u) * SG;
                    f.frags(b.w[u], wf, g0 >= g_begin && g0 < g_end, g0 + 1 >= g_begin && g0 + 1 < g_end);
                } else {
                    f.frags(b.w[u], wf);
                }
#pragma unroll
                for (int h = 0; h < KH; ++h)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) acc[t][mb] = mfma16(wf[h][t], b.x[u][h][mb], acc[t][mb]);
            }
        }
    };
    for (int c = 0; c < nchunks; c += 2) {
        if (DB && c + 1 < nchunks) load_chunk(c + 1, b1);
        consume(b0, c);
        if (c + 1 < nchunks) {
            if (!DB) load_chunk(c + 1, b1);
            if (c + 2 < nchunks && DB) load_chunk(c + 2, b0);
            consume(b1, c + 1);
            if (c + 2 < nchunks && !DB) load_chunk(c + 2, b0);
        }
    }
    if constexpr (XL != 0) __syncthreads();      // the reduction buffer overlays the waves' x staging KiBs: everyone has left the main loop
    skinny16_reduce_epilogue<SK_WAVES, NT, MB, ROWS>(a, red, acc, tid, lane, wave, nt0, NTT, nsplit, f.TH, rows);
}

// ----------------------------------------------------------------------------- launcher
// full-line x staging: 2 (default) = always, 1 = above 8 rows only, 0 = never (UMV_SKINNY_XL, A/B only).
// Measured on MI355X (tools/skinny_bench.py, us, plain -> XL; profiles/r04_skinny_xl.txt): 32 rows qkv 21.3 -> 16.4, o 13.0 -> 9.9,
// gate/up 59.3 -> 53.3, down 51.0 -> 34.8 (configs[3] decode step 4.445 -> 4.099 ms, 7199 -> 7807 tokens/s); 16 rows 14.3 -> 11.9 /
// 9.0 -> 8.1 / 48.5 -> 47.2 / 33.5 -> 27.9.  At 8 rows the two-piece form costs gate/up its second resident workgroup (125 -> 142
// registers: 42.4 -> 45.4 us), the ONE-piece form (rows 0..7 only, 124 registers) wins: gate/up 42.5 -> 41.4 (6.57 TB/s), down
// 26.0 -> 24.7, qkv 11.4 -> 9.2, headline step 3.161 -> 3.111 ms.
static int skinny_xl() {
    static const int v = umv_env_int("UMV_SKINNY_XL", 2);
    return v;
}

// One (MB, NT, U) configuration of a format with KH k halves per unit: kernel(XL) = its __global__ entry for x staging XL, args = the
// entry's arguments after the umv_gemm_args (KT = units along K, NTT = n-tiles).  XL takes x rows that start on a 128-byte boundary,
// so that a line is one cache line (any K, any split).
template <int MB, int NT, int U, int KH, int NORM, class Kernel, class... Args>
static int launch_skinny_body(Kernel kernel, const umv_gemm_args& a, int KT, int NTT, hipStream_t s, Args... args) {
    size_t lds = (size_t)SK_WAVES * NT * MB * 4 * 64 * sizeof(float);
    if (NORM) lds += SK_WAVES * 16 * sizeof(float) + (size_t)KT * 4 * NORM * 16;
    auto go = [&](auto XLV) {
        constexpr int XL = decltype(XLV)::value;
        const void* fn = reinterpret_cast<const void*>(kernel(XLV));
        const size_t xl = (size_t)SK_WAVES * (U * KH / 2) * (XL == 1 ? 1 : 2 * MB) * 1024;
        const size_t bytes = XL != 0 && xl > lds ? xl : lds;
        static bool attr_set[UMV_MAX_DEVICES] = {};
        if (bytes > 64 * 1024 && umv_first_on_device(attr_set)) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        umv_gemm_args ka = a;
        void* argv[] = {&ka, &args...};
        (void)hipLaunchKernel(fn, dim3((NTT + NT - 1) / NT, a.k_splits > 1 ? a.k_splits : 1), dim3(SK_WAVES * 64), argv, bytes, s);   // (error: UMV_LAUNCH_CHECK)
        UMV_LAUNCH_CHECK();
        return UMV_OK;
    };
    if constexpr (NORM == 0 && (U * KH) % 2 == 0) {
        const int mode = skinny_xl();
        if (mode && (mode > 1 || a.M > 8) && (a.ldx % 64) == 0 && ((uintptr_t)a.x % 128) == 0) {
            if constexpr (MB == 1) {
                if (a.M <= 8) return go(std::integral_constant<int, 1>{});
            }
            return go(std::integral_constant<int, 2>{});
        }
    }
    return go(std::integral_constant<int, 0>{});
}
