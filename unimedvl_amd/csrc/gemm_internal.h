// The frame shared by the MFMA-tiled GEMM kernels of libunimedvl_hip (gemm_tiled.h, gemm_w4.hip, gemm_fp8mfma.hip, gemm_mxfp4t.hip):
// the workgroup -> tile order with its raster width and super-block size, the instruction slots of the interleaved schedules, the
// zero page, the ds_read_b128 wrapper, the bias-to-LDS staging, the argument checks of the weight-format entry points, the launcher
// of the 4-wave kernels, and the environment knobs of every GEMM launcher.  The weight-streaming decode GEMM is gemm_skinny.h, the
// weight formats' conversions quant.h.  Internal to csrc/.
#pragma once
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include <stdlib.h>

// A/B and tuning knobs are read from the environment ONCE per process: `static const int v = umv_env_int("NAME", default);` at the
// point of use (the initialisation of a function-local static is thread-safe)
static inline int umv_env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// K tails, n-rows past N and surplus staging slots are staged from here (one copy per translation unit)
static __device__ __attribute__((aligned(16))) const uint32_t umv_zero_page[4] = {0, 0, 0, 0};

typedef __attribute__((address_space(3))) void* umv_lds_ptr_t;

// one ds_read_b128 at a compile-time offset (a free function: clang rejects asm operands that name locals of the enclosing
// function from inside a generic lambda)
template <int OFF, class V>
__device__ __forceinline__ void umv_lds_read128(V& dst, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}

// The tile's BN bias values wait in LDS behind the staging buffers: read after the main loop, a global load there would expose its
// whole latency once per tile (the first barrier of the main loop orders this write before any read).  Zero past N.
template <int BN, int NTHREADS>
__device__ __forceinline__ void umv_bias_to_lds(const umv_gemm_args& a, bf16_t* bias_lds, int nt_blk, int tid) {
#pragma unroll
    for (int o = 0; o < BN; o += NTHREADS) {
        if ((a.epilogue & UMV_EPI_BIAS) && tid + o < BN) {
            const int n = nt_blk * 16 + tid + o;
            bias_lds[tid + o] = n < a.N ? a.bias[n] : (bf16_t)0;
        }
    }
}

// read r of NRD goes right after MFMA number (r * SPAN) / NRD, SPAN = 3/4 of the step's MFMAs: evenly spread over the first three
// quarters, first one after the first MFMA, so that the last quarter's MFMAs cover the latency of the last reads before the
// step's closing s_waitcnt lgkmcnt(0)
__host__ __device__ constexpr int umv_interleave_slot(int i, int nmma, int nrd) {
    const int span = (nmma * 3 / 4 >= nrd) ? nmma * 3 / 4 : nmma;
    for (int r = 0; r < nrd; ++r)
        if ((r * span) / nrd == i) return r;
    return -1;
}
// piece p of n_pieces goes behind MFMA floor((2p + 1) * n_mma / (2 * n_pieces)): evenly spread, never behind the last MFMA
__host__ __device__ constexpr int umv_dma_slot(int i, int n_mma, int n_pieces) {
    for (int p = 0; p < n_pieces; ++p)
        if (((2 * p + 1) * n_mma) / (2 * n_pieces) == i) return p;
    return -1;
}

// XCD-aware tile order (blockIdx round-robins over the 8 XCDs): every XCD gets a contiguous run of tiles; inside the run,
// strips of gn n-blocks, m-block next, n-block within the strip fastest, so that the ~32 tiles an XCD works on at a time share
// both operands' k-slices in its L2.  M super-blocks of ms m-blocks: all XCDs finish one before the next (x stays in the
// memory-side cache while the strips of W stream past - with 32 images (M = 32 832, x = 235 MB, act = 1.2 GB) every strip of n-blocks
// otherwise re-streams all of x from HBM).  gn = 1 is plain m-fastest: every CU of the XCD streams its own x panel and only W is
// shared; ms = mblocks is one super-block.
__device__ __forceinline__ void umv_tile_order(int mblocks, int nblocks, int gn, int ms, int block, int& mblk, int& nblk) {
    const int sb_tiles = ms * nblocks;
    const int sb = block / sb_tiles;
    const int mb0 = sb * ms, mb_n = min(ms, mblocks - mb0);
    const int nwg = mb_n * nblocks;
    int bid = block - sb * sb_tiles;
    {
        const int q = nwg / 8, rem = nwg % 8, xcd = bid % 8, idx = bid / 8;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
    }
    const int per = mb_n * gn, strip = bid / per, rem = bid - strip * per;
    const int w = min(gn, nblocks - strip * gn);
    mblk = mb0 + rem / w;
    nblk = strip * gn + rem % w;
}

constexpr int UMV_TILE_GN = 4;      // n-blocks per strip of the tile order

// m-blocks per super-block: ~64 MB of x rows above 16k rows, one super-block below (host side)
static inline int umv_tile_superblock(int mblocks, int BM, int K) {
    int ms = (int)(((int64_t)64 << 20) / ((int64_t)BM * K * 2));
    ms = ms < 8 ? 8 : ms;
    if ((int64_t)mblocks * BM < 16384) ms = mblocks;   // measured (us, on / off): M = 32 832 gate/up 7040 / 7480, down 3880 / 4070, qkv 1013 / 1056;
                                                       // M = 16 416 down 1975 / 2010, gate/up 3543 / 3528; M = 8208 down 1062 / 1047: off below 16k rows
    if (ms > mblocks || ms * 3 / 2 >= mblocks) ms = mblocks;        // a short second super-block is not worth a second pass over W
    else ms = (mblocks + (mblocks + ms - 1) / ms - 1) / ((mblocks + ms - 1) / ms);   // equal super-blocks: no stub at the end
    return ms;
}

// The argument checks every weight-format entry point makes (umv_gemm_bf16 / _fp8w / _mxfp4w / _mxfp4t); `who` is the entry's name in
// the messages, kmul the multiple K has to be (8: bf16 / e4m3 images, 32: MXFP4 blocks)
static inline int umv_gemm_check_args(const umv_gemm_args& a, const char* who, int kmul) {
    UMV_CHECK(a.M >= 0 && a.N > 0 && a.K > 0, UMV_ERR_ARG, "%s: bad shape M=%d N=%d K=%d", who, a.M, a.N, a.K);
    if (kmul == 8)
        UMV_CHECK((a.K % 8) == 0 && (a.ldx % 8) == 0, UMV_ERR_ARG, "%s: K (%d) and ldx (%lld) must be multiples of 8", who, a.K, (long long)a.ldx);
    else
        UMV_CHECK((a.K % 32) == 0 && (a.ldx % 8) == 0, UMV_ERR_ARG, "%s: K (%d) must be a multiple of 32 and ldx (%lld) of 8", who, a.K,
                  (long long)a.ldx);
    UMV_CHECK(!(a.epilogue & UMV_EPI_BIAS) || a.bias, UMV_ERR_ARG, "%s: BIAS without bias pointer", who);
    UMV_CHECK(!(a.epilogue & UMV_EPI_RESIDUAL) || a.residual, UMV_ERR_ARG, "%s: RESIDUAL without residual pointer", who);
    UMV_CHECK(!(a.epilogue & UMV_EPI_SWIGLU) || (a.N % 32) == 0, UMV_ERR_ARG, "%s: SWIGLU needs N %% 32 == 0", who);
    UMV_CHECK(!a.lse_partial || a.argmax_partial, UMV_ERR_ARG, "%s: lse_partial rides on the argmax_partial epilogue and needs it set", who);
    return UMV_OK;
}
// The *_rows entries (the lm_head call with a per-row sampling table), after the null checks of the entry without the table
static inline int umv_gemm_check_rows(const umv_gemm_args& a, const umv_row_sampling* rows, const char* who) {
    UMV_CHECK(rows && ((uintptr_t)rows % 16) == 0 && a.argmax_partial && a.M >= 0 && a.M <= 64 && a.sample_temperature == 0.f, UMV_ERR_ARG,
              "%s: the per-row sampling table (16-byte aligned) needs argmax_partial, M <= 64 (got %d) and sample_temperature == 0 (got %g)",
              who, a.M, (double)a.sample_temperature);
    return UMV_OK;
}

// The decode-layout checks of the weight-streaming entry points (umv_gemm_fp8w / _mxfp4w / _z13w), after umv_gemm_check_args.  `image` and
// `instead` word the M <= 64 message; amax: the entry has the argmax / sampling-key epilogue; temperature: it also checks the sampling
// temperature (as umv_gemm_bf16 does)
static inline int umv_gemm_check_decode(const umv_gemm_args& a, const char* who, const char* image, const char* instead, bool amax,
                                        bool temperature) {
    UMV_CHECK(a.M <= 64, UMV_ERR_UNSUPPORTED, "%s: the %s image is the decode (M <= 64) layout; use %s for M=%d", who, image, instead, a.M);
    UMV_CHECK(!a.norm_w && (a.tile_rows == 0 || a.tile_rows == 16), UMV_ERR_UNSUPPORTED, "%s: no fused norm / th-row tiles", who);
    UMV_CHECK(amax || !a.argmax_partial, UMV_ERR_UNSUPPORTED, "%s: no argmax_partial (lm_head stays e4m3: umv_gemm_fp8w)", who);
    UMV_CHECK(a.k_splits <= 1 || (!(a.epilogue & UMV_EPI_SWIGLU) && a.split_stride > 0 && a.k_splits <= 64), UMV_ERR_UNSUPPORTED,
              "%s: split-K (k_splits=%d) needs no SwiGLU, split_stride > 0, k_splits <= 64", who, a.k_splits);
    UMV_CHECK(!a.argmax_partial || (a.k_splits <= 1 && !a.row_idx && !(a.epilogue & (UMV_EPI_SWIGLU | UMV_EPI_OUT_F32))), UMV_ERR_UNSUPPORTED,
              "%s: argmax_partial needs bf16 out, no SwiGLU / split-K / row_idx", who);
    if (temperature)
        UMV_CHECK(a.sample_temperature >= 0.f && (a.sample_temperature == 0.f || a.argmax_partial), UMV_ERR_ARG,
                  "%s: sample_temperature (%g) is a mode of the argmax_partial epilogue and must be >= 0", who, (double)a.sample_temperature);
    return UMV_OK;
}

// gemm_w4.hip: 4-wave tiles with the accumulators in AGPRs (cfg 466 / 468 / 4384); bf16 output, no split-K, operands within
// 2 GiB of their base pointers (umv_gemm_w4_can_take)
int umv_gemm_lean_epilogue(const umv_gemm_args& a);      // gemm.hip: >= 0 = the lean epilogue kind of this call, -1 = general
bool umv_gemm_w4_can_take(const umv_gemm_args& a, int KT, int NTT);
int umv_gemm_w4_launch(const umv_gemm_args& a, int KT, int NTT, int cfg, hipStream_t s);
