// VAE (FLUX autoencoder) convolutions: NHWC implicit GEMMs on MFMA - the im2col gather kernel and the input-stationary 3x3 kernel -
// and their dispatch.  From gemm_internal.h: the zero page and the LDS pointer type of the LDS-DMA pieces.
#include "gemm_internal.h"

// ----------------------------------------------------------------------------- VAE: implicit-GEMM convolution
// NHWC bf16 activations.  out[b,oy,ox,co] = bias[co] + sum_{ky,kx,ci} in[b,iy,ix,ci] * W[co][ky][kx][ci]
// is the GEMM  out[m = pixel][n = co] = sum_k x[m][k] Wp[n][k]  with k = (ky*ks+kx)*Cin + ci,
// so it reuses the packed-weight MFMA tile of gemm.hip: W is the A operand streamed from the
// packed image, the im2col row fragment (8 consecutive ci of one tap = 16 contiguous bytes,
// Cin % 8 == 0) is gathered straight into the LDS B-fragment image - no im2col buffer.
// mode 0: stride 1, pad (ks-1)/2 (autoencoder.py:76,78,138,167,214,238)
// mode 1: nearest 2x upsample fused into the gather (Upsample, autoencoder.py:116-118)
// mode 2: stride 2 after F.pad(0,1,0,1), no other padding (Downsample, autoencoder.py:104-107)
struct ConvGeom {
    int B, Cin, Hin, Win, Cout, Hout, Wout, ks, mode;
};

// ----------------------------------------------------------------------------- the epilogue of the gather kernel
// 4 consecutive bf16 as floats: one 8-byte load (packed), or element by element with the index clamped to the n_valid that exist
__device__ __forceinline__ void conv_load4(const bf16_t* p, bool packed, int n_valid, float (&f)[4]) {
    if (packed) {
        const u32x2 pk = *reinterpret_cast<const u32x2*>(p);
        f[0] = __uint_as_float(pk.x << 16); f[1] = __uint_as_float(pk.x & 0xFFFF0000u);
        f[2] = __uint_as_float(pk.y << 16); f[3] = __uint_as_float(pk.y & 0xFFFF0000u);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) f[q] = bf2f(p[min(q, n_valid - 1)]);
    }
}
// One lane's four consecutive output channels of one pixel (lane (r, g) of an MFMA tile: pixel r, channels n0 = 16 * tile + 4 g ..):
// + bias -> bf16 ; (+ residual -> bf16).  o: the offset of that pixel's channel n0 in `residual` and `out`, b4: the bias of the four
// channels.  full: the four channels exist and bias / residual / out are 8-byte aligned (Cout % 4 == 0 makes every such address
// aligned) - 8-byte accesses; otherwise the n_valid = Cout - n0 channels that exist, one by one.
// conv3x3_patch_kernel does NOT end in this function: with it (full = true, so no scalar path) the kernel measured 0.7 - 0.9 % slower
// on the 1024 x 1024 decode in three runs against the parent, cause not found (profiles/vision_split.txt, section 5), so it keeps its
// own always-packed copy.
__device__ __forceinline__ void conv_epilogue4(const f32x4& acc, const bf16_t* bias, const float (&b4)[4], const bf16_t* residual, bf16_t* out,
                                               int64_t o, bool full, int n_valid) {
    const float v[4] = {acc.x, acc.y, acc.z, acc.w};
    float r4[4] = {0.f, 0.f, 0.f, 0.f}, f[4];
    if (residual) conv_load4(residual + o, full, n_valid, r4);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f[q] = rbf(bias ? v[q] + b4[q] : v[q] + 0.f);
        if (residual) f[q] = rbf(f[q] + r4[q]);
    }
    if (full) {
        u32x2 pk;
        pk.x = pack2bf(f[0], f[1]);
        pk.y = pack2bf(f[2], f[3]);
        *reinterpret_cast<u32x2*>(out + o) = pk;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < n_valid) out[o + q] = f2bf(f[q]);
    }
}

// Same pipeline as gemm_tiled_kernel (gemm_tiled.h): WN x WM waves of TN x TM MFMA tiles, k-step KTS*32, NBUF LDS
// buffers filled by LDS-DMA with counted vmcnt and one raw barrier per step.  W tiles are straight 1 KiB copies
// of the packed image; an x tile is the im2col fragment gathered per lane (tap / channel decode per k, zero page
// for padding, upsampled or strided source coordinates by mode).  The step loop is a second copy of tiled_loop_plain's on
// purpose: calling one shared loop from both changed the compiled GEMM kernels (profiles/vision_split.txt, section 3).
template <int WN, int WM, int TN, int TM, int KTS, int NBUF>
__global__ __launch_bounds__(WN * WM * 64) void conv_tiled_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp,
                                                                  const bf16_t* __restrict__ bias, const bf16_t* __restrict__ residual,
                                                                  bf16_t* __restrict__ out, ConvGeom geo, int KT, int NTT, int mblocks) {
    constexpr int NW = WN * WM;
    constexpr int BN = WN * TN * 16, BM = WM * TM * 16;
    constexpr int WTILES = BN / 16 * KTS, XTILES = BM / 16 * KTS;
    constexpr int TPW = (WTILES + XTILES) / NW;
    static_assert((WTILES + XTILES) % NW == 0, "staging tiles must divide evenly over the waves");
    constexpr int BUF = (WTILES + XTILES) * 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int wn = wave % WN, wm = wave / WN;
    const int mblk = blockIdx.x % mblocks;
    const int nblk = blockIdx.x / mblocks;
    const int m0 = mblk * BM;
    const int nt_blk = nblk * (BN / 16);
    const int nt_base = nt_blk + wn * TN;
    const int M = geo.B * geo.Hout * geo.Wout;
    const int K = geo.ks * geo.ks * geo.Cin;
    const int nsteps = (KT + KTS - 1) / KTS;

    // per staged tile: either a W tile (pointer) or an x tile (this lane's output pixel)
    const bf16_t* wsrc[TPW];
    bool wvalid[TPW];
    int pb[TPW], poy[TPW], pox[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int f = wave * TPW + i;
        wsrc[i] = nullptr; wvalid[i] = false; pb[i] = poy[i] = pox[i] = 0;
        if (f < WTILES) {
            const int tl = f / KTS, kk = f % KTS;
            const int nt = nt_blk + tl;
            wvalid[i] = nt < NTT;
            wsrc[i] = wp + ((int64_t)(wvalid[i] ? nt : 0) * KT + kk) * 512 + lane * 8;
        } else {
            const int tl = (f - WTILES) / KTS;
            int m = m0 + tl * 16 + r;
            m = m < M ? m : M - 1;
            pb[i] = m / (geo.Hout * geo.Wout);
            const int rem = m % (geo.Hout * geo.Wout);
            poy[i] = rem / geo.Wout;
            pox[i] = rem % geo.Wout;
        }
    }
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(umv_zero_page);
    const bool cin32 = (geo.Cin & 31) == 0;
    auto stage = [&](int step, int buf) {
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int f = wave * TPW + i;
            const bf16_t* p = zero;
            if (f < WTILES) {
                const int kt = step * KTS + f % KTS;
                if (wvalid[i] && kt < KT) p = wsrc[i] + (int64_t)step * (KTS * 512);
            } else {
                const int kt = step * KTS + (f - WTILES) % KTS;
                const int k = kt * 32 + g * 8;
                if (k < K) {
                    // Cin % 32 == 0 (every conv of the VAE but conv_in): a 32-wide k-tile lies inside one filter tap, so the tap and
                    // its (ky, kx) are wave-uniform - scalar divisions instead of ~60 VALU instructions per staged piece
                    int tap, ci;
                    if (cin32) {
                        const int tu = __builtin_amdgcn_readfirstlane((kt * 32) / geo.Cin);
                        tap = tu;
                        ci = k - tu * geo.Cin;
                    } else {
                        tap = k / geo.Cin;
                        ci = k - tap * geo.Cin;
                    }
                    const int ky = tap / geo.ks, kx = tap - ky * geo.ks;
                    int iy, ix;
                    bool ok;
                    if (geo.mode == 0) {
                        const int pad = (geo.ks - 1) >> 1;
                        iy = poy[i] + ky - pad; ix = pox[i] + kx - pad;
                        ok = iy >= 0 && iy < geo.Hin && ix >= 0 && ix < geo.Win;
                    } else if (geo.mode == 1) {
                        iy = poy[i] + ky - 1; ix = pox[i] + kx - 1;        // coordinates in the 2x upsampled image
                        ok = iy >= 0 && iy < 2 * geo.Hin && ix >= 0 && ix < 2 * geo.Win;
                        iy >>= 1; ix >>= 1;
                    } else {
                        iy = 2 * poy[i] + ky; ix = 2 * pox[i] + kx;        // zero pad on the bottom / right only
                        ok = iy < geo.Hin && ix < geo.Win;
                    }
                    if (ok) p = x + (((int64_t)pb[i] * geo.Hin + iy) * geo.Win + ix) * geo.Cin + ci;
                }
            }
            char* dst = smem + buf * BUF + f * 1024;
            __builtin_amdgcn_global_load_lds((const void*)p, (umv_lds_ptr_t)dst, 16, 0, 0);
        }
    };
    f32x4 acc[TN][TM];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < NBUF - 1; ++p)
        if (p < nsteps) stage(p, p);
    for (int step = 0; step < nsteps; ++step) {
        const int cur = step % NBUF;
        const int ahead = min(NBUF - 2, nsteps - 1 - step);
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * TPW) : "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        UMV_BARRIER();
        if (step + NBUF - 1 < nsteps) stage(step + NBUF - 1, (step + NBUF - 1) % NBUF);
        const char* wb = smem + cur * BUF;
        const char* xb = wb + WTILES * 1024;
#pragma unroll
        for (int kk = 0; kk < KTS; ++kk) {
            bf16x8 wf[TN], xf[TM];
#pragma unroll
            for (int t = 0; t < TN; ++t) wf[t] = *reinterpret_cast<const bf16x8*>(wb + ((wn * TN + t) * KTS + kk) * 1024 + lane * 16);
#pragma unroll
            for (int j = 0; j < TM; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(xb + ((wm * TM + j) * KTS + kk) * 1024 + lane * 16);
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
                for (int j = 0; j < TM; ++j) acc[t][j] = mfma16(wf[t], xf[j], acc[t][j]);
        }
    }
    // epilogue: 4 consecutive output channels per lane, the bias once per channel group
    const bool vec4 = (geo.Cout & 3) == 0 && ((reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(out)) & 7) == 0;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const int n0 = (nt_base + t) * 16 + g * 4;
        if (n0 >= geo.Cout) continue;
        const bool full = vec4 && n0 + 3 < geo.Cout;
        float b4[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) conv_load4(bias + n0, full, geo.Cout - n0, b4);
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = m0 + (wm * TM + j) * 16 + r;
            if (m >= M) continue;
            const int64_t o = (int64_t)m * geo.Cout + n0;
            conv_epilogue4(acc[t][j], bias, b4, residual, out, o, full, geo.Cout - n0);
        }
    }
}

// ----------------------------------------------------------------------------- VAE: 3x3 convolution, input-stationary
// conv_tiled_kernel gathers the im2col fragment of every filter tap from global memory: each input pixel goes through the
// texture-address path NINE times, 16 bytes per lane from a different pixel row each (16 half cache lines per wave instruction).
// At 128-512 channels that path, not the matrix pipe, sets the pace: 768 address cycles against 544 MFMA cycles per k-step on
// a CU, 190-260 TFLOP/s on the decoder's 3x3 convolutions (profiles/r03_vae4_kernel_stats_by_grid.csv).
// Here the INPUT stays put: a workgroup owns a 16 x 16 output tile and 128 output channels; for every 64-channel slice of the
// input it brings the 18 x 18 pixel patch (halo included) into LDS ONCE - 40.5 KiB, pixel-major, 128 bytes per pixel with the
// 16-byte channel octets XOR-swizzled by the pixel index - and all nine taps read their MFMA B fragments from that patch at
// shifted pixel positions (16 consecutive pixels of a patch row per 16-lane row: conflict-free ds_read_b128).  Only the weights
// stream per tap (16 KiB = 8 n-tiles x 2 k-tiles, straight copies of the packed image, 3-deep ring).  Per (slice, tap) step a
// wave issues exactly three LDS-DMA pieces (two weight tiles + one piece of the NEXT slice's patch or a dummy), so the counted
// vmcnt waits see a uniform queue; one raw barrier per step.  Same MFMA operands in the same k order (tap-major, channel-minor
// inside a 64-channel slice... the k order is (slice, tap, channel) instead of (tap, channel): another fp32 summation order,
// same bf16 rounding points (bias, residual) as conv_tiled_kernel.
// MODE 1 = the nearest-2x upsample of Upsample.forward (autoencoder.py:116-118) fused in: the 16 x 16 OUTPUT tile reads a 10 x 10
// patch of the half-resolution input (output pixel (oy, ox), tap (dy, dx) -> input ((oy + dy - 1) >> 1, (ox + dx - 1) >> 1); lanes
// that share an input pixel read the same LDS address: a broadcast, not a conflict).
#define CP_TW 16
#define CP_TH 16
#define CP_WBUF 16384                                // 8 n-tiles x 2 k-tiles
template <int MODE> struct CpGeo {
    static constexpr int PW = MODE == 1 ? CP_TW / 2 + 2 : CP_TW + 2;
    static constexpr int PH = MODE == 1 ? CP_TH / 2 + 2 : CP_TH + 2;
    static constexpr int PIX = PW * PH;                                      // 324 / 100 patch pixels
    static constexpr int PATCH_BYTES = (PIX * 128 + 1023) / 1024 * 1024;     // 41 / 13 DMA pieces of 1 KiB
    static constexpr int PIECES = PATCH_BYTES / 1024;
    static constexpr int LDS = 2 * PATCH_BYTES + 3 * CP_WBUF + 1024;
};

template <int MODE>
__global__ __launch_bounds__(512) void conv3x3_patch_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp,
                                                            const bf16_t* __restrict__ bias, const bf16_t* __restrict__ residual,
                                                            bf16_t* __restrict__ out, int B, int H, int W, int Cin, int Cout, int KT,
                                                            int NTT, int tiles_x, int tiles_y) {
    // H, W: OUTPUT size (MODE 1: the input is H/2 x W/2)
    constexpr int CP_PW = CpGeo<MODE>::PW, CP_PIX = CpGeo<MODE>::PIX, CP_PATCH_BYTES = CpGeo<MODE>::PATCH_BYTES, CP_PATCH_PIECES = CpGeo<MODE>::PIECES;
    const int Hi = MODE == 1 ? H / 2 : H, Wi = MODE == 1 ? W / 2 : W;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* patch = smem;                               // 2 buffers
    char* wbuf = smem + 2 * CP_PATCH_BYTES;           // 3 buffers
    char* dummy = wbuf + 3 * CP_WBUF;                 // 1 KiB sink of the padding pieces
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int wn = wave & 1, wm = wave >> 1;          // 2 (n) x 4 (m) waves of 64 channels x 64 pixels (4 tile rows)
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y; bid /= tiles_y;
    const int b = bid % B;
    const int nblk = bid / B;
    const int ox0 = tx * CP_TW, oy0 = ty * CP_TH;
    const int nt_blk = nblk * 8;
    const int nslices = Cin / 64;
    const int nsteps = nslices * 9;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(umv_zero_page);
    const bf16_t* xb = x + (int64_t)b * Hi * Wi * Cin;
    const int iy0 = MODE == 1 ? oy0 / 2 - 1 : oy0 - 1, ix0 = MODE == 1 ? ox0 / 2 - 1 : ox0 - 1;     // input coordinates of patch pixel (0, 0)

    // ---- LDS-DMA pieces of a step: W tiles f = wave*2 + {0,1} (n-tile f/2.. : tile index t = f >> 1?  8 n-tiles x 2 k-tiles = 16 pieces)
    auto stage_w = [&](int step, int buf) {
        const int slice = step / 9, tap = step - slice * 9;
        const int kt0 = (tap * Cin + slice * 64) >> 5;            // k-tile of the packed image: k = tap*Cin + ci
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = wave * 2 + i;                           // piece = (n-tile f >> 1, k-tile f & 1)
            const int nt = nt_blk + (f >> 1);
            const bf16_t* p = nt < NTT ? wp + ((int64_t)nt * KT + kt0 + (f & 1)) * 512 + lane * 8 : zero;
            __builtin_amdgcn_global_load_lds((const void*)p, (umv_lds_ptr_t)(wbuf + buf * CP_WBUF + f * 1024), 16, 0, 0);
        }
    };
    // piece q (0..40) of the patch of `slice`: 64 consecutive 16-byte slots s = q*64 + lane = pixel*8 + pos; the slot holds channel
    // octet pos ^ (pixel & 7) of that pixel (the swizzle is applied on the SOURCE side: the LDS image of a DMA is lane-linear)
    auto stage_patch_piece = [&](int slice, int q, int buf) {
        const int sidx = q * 64 + lane;
        const int pix = sidx >> 3, pos = sidx & 7;
        const int py = pix / CP_PW, px = pix - py * CP_PW;
        const int iy = iy0 + py, ix = ix0 + px;
        const int oct = pos ^ (pix & 7);
        const bool ok = pix < CP_PIX && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
        const bf16_t* p = ok ? xb + ((int64_t)iy * Wi + ix) * Cin + slice * 64 + oct * 8 : zero;
        __builtin_amdgcn_global_load_lds((const void*)p, (umv_lds_ptr_t)(patch + buf * CP_PATCH_BYTES + q * 1024), 16, 0, 0);
    };
    // the third piece of step (slice, tap): a piece of the NEXT slice's patch during taps 0..5 - into the buffer the PREVIOUS
    // slice used, which every wave has left by then - else a dummy
    auto stage_third = [&](int slice, int tap) {
        const int q = tap * 8 + wave;                              // 6 taps x 8 waves = 48 >= 41 (13) pieces
        if (tap < 6 && q < CP_PATCH_PIECES && slice + 1 < nslices) stage_patch_piece(slice + 1, q, (slice + 1) & 1);
        else __builtin_amdgcn_global_load_lds((const void*)zero, (umv_lds_ptr_t)dummy, 16, 0, 0);
    };

    // ---- prologue: patch of slice 0 (all 41 pieces, 5-6 per wave), then W(0), W(1) with a dummy behind each: the queue of a
    //      wave then looks like the steady state (per step: two weight pieces for step + 2, then one third piece)
    for (int q = wave; q < CP_PATCH_PIECES; q += 8) stage_patch_piece(0, q, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stage_w(0, 0);
    __builtin_amdgcn_global_load_lds((const void*)zero, (umv_lds_ptr_t)dummy, 16, 0, 0);
    stage_w(1, 1);
    __builtin_amdgcn_global_load_lds((const void*)zero, (umv_lds_ptr_t)dummy, 16, 0, 0);

    f32x4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int step = 0; step < nsteps; ++step) {
        // W(step) was issued two steps ago; behind it in the queue: that step's third piece, W(step + 1) and its third piece = 4
        // pieces that may still be in flight (the patch of a slice is issued during taps 0..5 of the slice before: long landed)
        if (step + 1 < nsteps) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        UMV_BARRIER();
        const int slice = step / 9, tap = step - slice * 9;
        if (step + 2 < nsteps) stage_w(step + 2, (step + 2) % 3);
        else {      // (keep three pieces per step to the end)
            __builtin_amdgcn_global_load_lds((const void*)zero, (umv_lds_ptr_t)dummy, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)zero, (umv_lds_ptr_t)dummy, 16, 0, 0);
        }
        stage_third(slice, tap);
        const int dy = tap / 3, dx = tap - dy * 3;
        const char* wb = wbuf + (step % 3) * CP_WBUF;
        const char* pb = patch + (slice & 1) * CP_PATCH_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 wf[4], xf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) wf[t] = *reinterpret_cast<const bf16x8*>(wb + (((wn * 4 + t) * 2 + kk) * 1024) + lane * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // patch pixel of output (tile row wm*4+j, column r) at this tap
                const int pix = MODE == 1 ? ((wm * 4 + j + dy + 1) >> 1) * CP_PW + ((r + dx + 1) >> 1) : (wm * 4 + j + dy) * CP_PW + r + dx;
                xf[j] = *reinterpret_cast<const bf16x8*>(pb + pix * 128 + (((kk * 4 + g) ^ (pix & 7)) << 4));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t][j] = mfma16(wf[t], xf[j], acc[t][j]);
        }
    }
    // ---- epilogue: + bias -> bf16 ; (+ residual -> bf16); lane (r, g) of tile (t, j) holds pixel column r, channels n0..n0+3
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n0 = (nt_blk + wn * 4 + t) * 16 + g * 4;
        if (n0 >= Cout) continue;
        float b4[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
            const u32x2 pk = *reinterpret_cast<const u32x2*>(bias + n0);
            b4[0] = __uint_as_float(pk.x << 16); b4[1] = __uint_as_float(pk.x & 0xFFFF0000u);
            b4[2] = __uint_as_float(pk.y << 16); b4[3] = __uint_as_float(pk.y & 0xFFFF0000u);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oy = oy0 + wm * 4 + j, ox = ox0 + r;
            if (oy >= H || ox >= W) continue;
            const int64_t m = ((int64_t)b * H + oy) * W + ox;
            const float v[4] = {acc[t][j].x, acc[t][j].y, acc[t][j].z, acc[t][j].w};
            float r4[4] = {0.f, 0.f, 0.f, 0.f};
            if (residual) {
                const u32x2 pk = *reinterpret_cast<const u32x2*>(residual + m * Cout + n0);
                r4[0] = __uint_as_float(pk.x << 16); r4[1] = __uint_as_float(pk.x & 0xFFFF0000u);
                r4[2] = __uint_as_float(pk.y << 16); r4[3] = __uint_as_float(pk.y & 0xFFFF0000u);
            }
            float f[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f[q] = rbf(bias ? v[q] + b4[q] : v[q] + 0.f);
                if (residual) f[q] = rbf(f[q] + r4[q]);
            }
            u32x2 pk;
            pk.x = pack2bf(f[0], f[1]);
            pk.y = pack2bf(f[2], f[3]);
            *reinterpret_cast<u32x2*>(out + m * Cout + n0) = pk;
        }
    }
}

template <int MODE>
static int launch_conv_patch(const bf16_t* x, const bf16_t* wp, const bf16_t* bias, const bf16_t* residual, bf16_t* out, int B, int H, int W,
                             int Cin, int Cout, int KT, int NTT, hipStream_t s) {
    constexpr int CP_LDS = CpGeo<MODE>::LDS;
    static bool attr_set[UMV_MAX_DEVICES] = {};
    if (umv_first_on_device(attr_set)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_patch_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CP_LDS);
        UMV_CHECK(e == hipSuccess, UMV_ERR_LAUNCH, "conv3x3_patch: cannot reserve %d bytes of LDS", (int)CP_LDS);
    }
    const int tiles_x = (W + CP_TW - 1) / CP_TW, tiles_y = (H + CP_TH - 1) / CP_TH, nblocks = (Cout + 127) / 128;
    hipLaunchKernelGGL(conv3x3_patch_kernel<MODE>, dim3(tiles_x * tiles_y * B * nblocks), dim3(512), CP_LDS, s, x, wp, bias, residual, out, B, H, W, Cin,
                       Cout, KT, NTT, tiles_x, tiles_y);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

template <int WN, int WM, int TN, int TM, int KTS, int NBUF>
static int launch_conv(const bf16_t* x, const bf16_t* wp, const bf16_t* bias, const bf16_t* residual, bf16_t* out, const ConvGeom& geo,
                       int KT, int NTT, hipStream_t s) {
    constexpr int BN = WN * TN * 16, BM = WM * TM * 16;
    constexpr size_t lds = (size_t)NBUF * (BN / 16 * KTS + BM / 16 * KTS) * 1024;
    static_assert(lds <= 160 * 1024, "LDS budget");
    static bool attr_set[UMV_MAX_DEVICES] = {};
    if (umv_first_on_device(attr_set)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_tiled_kernel<WN, WM, TN, TM, KTS, NBUF>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        UMV_CHECK(e == hipSuccess, UMV_ERR_LAUNCH, "conv_tiled: cannot reserve %d bytes of LDS", (int)lds);
    }
    const int M = geo.B * geo.Hout * geo.Wout;
    const int mblocks = (M + BM - 1) / BM, nblocks = (geo.Cout + BN - 1) / BN;
    hipLaunchKernelGGL((conv_tiled_kernel<WN, WM, TN, TM, KTS, NBUF>), dim3(mblocks * nblocks), dim3(WN * WM * 64), lds, s, x, wp, bias,
                       residual, out, geo, KT, NTT, mblocks);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_conv2d_nhwc_bf16(const uint16_t* x, const uint16_t* wp, const uint16_t* bias, const uint16_t* residual,
                                    uint16_t* out, int B, int Cin, int Hin, int Win, int Cout, int ksize, int mode,
                                    umv_stream_t stream) {
    UMV_CHECK(x && wp && out, UMV_ERR_ARG, "conv2d: null pointer");
    UMV_CHECK(Cin > 0 && Cin % 8 == 0, UMV_ERR_ARG, "conv2d: Cin (%d) must be a positive multiple of 8 (pad the input channels)", Cin);
    UMV_CHECK(B >= 0 && Hin >= 0 && Win >= 0 && Cout > 0, UMV_ERR_ARG, "conv2d: B %d Hin %d Win %d Cout %d", B, Hin, Win, Cout);
    const int force = mode & ~3;       // tests / A-B: | 16 = the input-stationary 3x3 kernel whatever the grid, | 32 = the gather kernel
    mode &= 3;
    UMV_CHECK((ksize == 3 || ksize == 1) && mode >= 0 && mode <= 2 && (force == 0 || force == 16 || force == 32), UMV_ERR_ARG,
              "conv2d: ksize %d mode %d", ksize, mode | force);
    // the up- and downsample are 3x3 only (Upsample / Downsample of the reference): the gather's mode 1 / 2 arithmetic has the 3-wide window built in
    UMV_CHECK(ksize == 3 || mode == 0, UMV_ERR_UNSUPPORTED, "conv2d: mode %d needs ksize 3 (got %d)", mode, ksize);
    ConvGeom geo;
    geo.B = B; geo.Cin = Cin; geo.Hin = Hin; geo.Win = Win; geo.Cout = Cout; geo.ks = ksize; geo.mode = mode;
    if (mode == 0) { geo.Hout = Hin; geo.Wout = Win; }
    else if (mode == 1) { geo.Hout = 2 * Hin; geo.Wout = 2 * Win; }
    else { geo.Hout = Hin / 2; geo.Wout = Win / 2; }       // floor((Hin + 1 - 3) / 2) + 1 for Hin >= 0: one row or column gives none, not one
    const int M = B * geo.Hout * geo.Wout;
    if (M == 0) return UMV_OK;
    const int K = ksize * ksize * Cin;
    const int KT = (K + 31) / 32, NTT = (Cout + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    // 3x3, stride 1, input channels in whole 64-channel slices, 4-channel-aligned outputs, and enough 16 x 16 tiles to fill the
    // chip: the input-stationary kernel
    const bool patch_ok = ksize == 3 && (mode == 0 || mode == 1) && Cin % 64 == 0 && Cout % 4 == 0 &&
        ((reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(out)) & 7) == 0;
    UMV_CHECK(force != 16 || patch_ok, UMV_ERR_UNSUPPORTED, "conv2d: the input-stationary kernel needs 3x3 / stride 1 / Cin %% 64 == 0 / Cout %% 4 == 0");
    // (whatever the grid: even 16 workgroups of it beat the gather kernel on a 32 x 32 x 512 level, and a choice that depended
    // on the batch would break "a batch == its images one by one, bit for bit")
    if (patch_ok && force != 32)
        return mode == 1 ? launch_conv_patch<1>(x, wp, bias, residual, out, B, geo.Hout, geo.Wout, Cin, Cout, KT, NTT, s)
                         : launch_conv_patch<0>(x, wp, bias, residual, out, B, geo.Hout, geo.Wout, Cin, Cout, KT, NTT, s);
    if (Cout <= 16) return launch_conv<1, 4, 1, 4, 4, 2>(x, wp, bias, residual, out, geo, KT, NTT, s);     // conv_out: 16(n) x 256(m)
    const long wg128 = (long)((M + 127) / 128) * ((Cout + 127) / 128);
    if (wg128 >= 384) return launch_conv<2, 2, 4, 4, 2, 2>(x, wp, bias, residual, out, geo, KT, NTT, s);  // 128 x 128 x 64
    return launch_conv<2, 2, 4, 2, 2, 3>(x, wp, bias, residual, out, geo, KT, NTT, s);                    // 128(n) x 64(m) x 64
}
