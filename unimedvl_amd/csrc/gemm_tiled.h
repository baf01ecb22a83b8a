// The 8-wave MFMA-tiled bf16 GEMM of libunimedvl_hip (gfx950): gemm_tiled_kernel = tile frame -> one of three main loops -> epilogue.
// Entry points, tile policy and dispatch are in gemm.hip; the frame pieces shared with the other tiled kernels in gemm_internal.h,
// the epilogues in gemm_epilogue.h.
//
// Workgroup tile 128(n) x 128(m) x 64(k) and its relatives, LDS buffers filled by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave
// instruction) while the MFMAs of the previous k-step run:
//   * the packed weight image IS the MFMA A-fragment order, so a W tile is a straight 1 KiB copy;
//   * an x fragment (16 rows x 64 B) is gathered by giving every lane its own source address
//     (row index list, K tail -> a zero page), so it lands in B-fragment order too.
// Every ds_read_b128 is lane-linear (conflict free) and no fragment passes through VGPRs on its way in.
#pragma once
#include "common.h"
#include "../../include/unimedvl_hip.h"
#include "gemm_epilogue.h"
#include "gemm_internal.h"

// inline-asm building block of the interleaved schedules (a free function, like umv_lds_read128: clang rejects asm operands that name
// locals of the enclosing function from inside a generic lambda)
__device__ __forceinline__ void mfma16_asm(f32x4& c, const bf16x8& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}

// WN x WM waves, each owning TN x TM MFMA tiles: workgroup tile (WN*TN*16)(n) x (WM*TM*16)(m) x (KTS*32)(k).
// SCHED: 0 = plain loop, 1 = MFMAs and fragment reads interleaved by hand, 3 = the same with x staged in full 128-byte lines.
template <int WN, int WM, int TN_, int TM_, int KTS_, int NBUF_, int SCHED_>
struct TiledCfg {
    static constexpr int TN = TN_, TM = TM_, KTS = KTS_, NBUF = NBUF_, SCHED = SCHED_;
    static_assert(SCHED == 0 || SCHED == 1 || SCHED == 3, "SCHED: 0 plain, 1 interleaved, 3 full-line x staging");
    static constexpr int NW = WN * WM;
    static constexpr int BN = WN * TN * 16, BM = WM * TM * 16;
    static constexpr int WTILES = BN / 16 * KTS, XTILES = BM / 16 * KTS;      // 1 KiB fragment tiles per k-step
    static constexpr int NT_ALL = WTILES + XTILES;
    static constexpr int TPW = (NT_ALL + NW - 1) / NW;                        // tiles staged per wave per k-step (SCHED 0 / 1)
    // A tile whose 1 KiB pieces do not divide evenly over the waves (288 x 128: 26) rounds TPW up: the surplus slots copy the zero
    // page into a spare KiB each behind the buffers and the bias, so that every wave issues the same number of LDS-DMA pieces per
    // k-step and the counted s_waitcnt vmcnt(N) stay exact.
    static constexpr int NDUMMY = SCHED == 3 ? 0 : NW * TPW - NT_ALL;
    static constexpr int BUF = NT_ALL * 1024;
    // bytes of the staging area: NBUF whole-step buffers [W tiles [BN/16][KTS], then x tiles [BM/16][KTS]], or - SCHED = 3 - a
    // 3-slot ring of W k-steps + a 3-slot ring of x k-step pairs
    static constexpr int STAGE_BYTES = SCHED == 3 ? 3 * WTILES * 1024 + 3 * BM * 128 : NBUF * BUF;
    static constexpr int DUMPOFF = STAGE_BYTES + (BN * 2 + 15) / 16 * 16;     // behind the tile's bias
    static constexpr int LDS_BYTES = DUMPOFF + NDUMMY * 1024;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
    // bf16 outputs leave through LDS as whole rows (every wave's TN x TM x 512 bytes fit the staging area): the direct epilogue is
    // the one of fp32 outputs only
    static_assert(BN * BM * 2 <= STAGE_BYTES, "the tile fits the LDS epilogue");
};

// where a workgroup (and this wave of it) stands: set up by the kernel's frame, read by the main loops
struct TilePos {
    int lane, wave, wn, wm;
    int m0;              // first row of the workgroup tile
    int nt_blk;          // first 16-column tile of the workgroup tile
    int kt0, kt1;        // this block's k-tiles [kt0, kt1) (split-K: blockIdx.y's range)
    int KTL, nsteps;     // kt1 - kt0, and the k-steps of KTS k-tiles that cover them
};

// ----------------------------------------------------------------------------- half-line staging (SCHED 0 / 1)
// Tile f = wave*TPW + i of a k-step: f < WTILES copies a W tile, otherwise gathers an x tile of 16 rows x 64 bytes.
template <class Cf>
struct HalfLineStage {
    static constexpr int TPW = Cf::TPW, KTS = Cf::KTS, WTILES = Cf::WTILES, NT_ALL = Cf::NT_ALL;
    const bf16_t* src[TPW];      // piece i at k-step 0
    bool tvalid[TPW];            // false: n-rows past N or a surplus slot - the zero page with a zero bump
    // Fast path (every k-step but a ragged last one): one pointer bump per tile, no branches - this code sits between the barrier
    // and the first MFMA of every step.  Steps are staged in order, so the pointers advance incrementally.
    const bf16_t* cur[TPW];
    int bump[TPW];
    bool ragged;                 // the last k-step needs per-tile / per-lane zero fill

    __device__ __forceinline__ void init(const umv_gemm_args& a, const TilePos& p, int KT, int NTT) {
        const int r = p.lane & 15, g = p.lane >> 4;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int f = p.wave * TPW + i;
            if (f < WTILES) {
                const int nt = p.nt_blk + f / KTS;
                tvalid[i] = nt < NTT;
                src[i] = a.wp + ((int64_t)(tvalid[i] ? nt : 0) * KT + p.kt0 + f % KTS) * 512 + p.lane * 8;
            } else if (Cf::NDUMMY != 0 && f >= NT_ALL) {
                tvalid[i] = false;
                src[i] = zero();
            } else {
                const int fx = f - WTILES;
                const int m = p.m0 + fx / KTS * 16 + r;
                tvalid[i] = true;                       // rows past M are clamped (their outputs are masked)
                const int mm = m < a.M ? m : a.M - 1;
                const int64_t row = a.row_idx ? (int64_t)a.row_idx[mm] : (int64_t)mm;
                src[i] = a.x + row * a.ldx + (p.kt0 + fx % KTS) * 32 + g * 8;
            }
            cur[i] = tvalid[i] ? src[i] : zero();
            bump[i] = !tvalid[i] ? 0 : (f < WTILES ? KTS * 512 : KTS * 32);
        }
        ragged = (p.KTL % KTS) != 0 || ((a.K & 31) != 0 && p.kt1 == KT);
    }
    static __device__ __forceinline__ const bf16_t* zero() { return reinterpret_cast<const bf16_t*>(umv_zero_page); }
    // (char* and a cast at the call: a lambda RETURNING an address_space(3) pointer makes the host pass drop the kernel's stub
    // without a diagnostic - the library then fails to load with an undefined __device_stub__ symbol)
    static __device__ __forceinline__ char* dst_of(char* smem, const TilePos& p, int buf, int i) {
        const int f = p.wave * TPW + i;
        return (Cf::NDUMMY == 0 || f < NT_ALL) ? smem + buf * Cf::BUF + f * 1024 : smem + Cf::DUMPOFF + (f - NT_ALL) * 1024;
    }
    static __device__ __forceinline__ void issue(const bf16_t* s, char* dst) {
        __builtin_amdgcn_global_load_lds((const void*)s, (umv_lds_ptr_t)dst, 16, 0, 0);
    }
    // the source of piece i at the ragged last k-step `step`: zero page for k-tiles past the range and lanes past K
    __device__ __forceinline__ const bf16_t* tail_src(const umv_gemm_args& a, const TilePos& p, int i, int step) const {
        const int f = p.wave * TPW + i;
        if (f < WTILES) {
            const int kt = step * KTS + f % KTS;
            return (tvalid[i] && kt < p.KTL) ? src[i] + (int64_t)step * (KTS * 512) : zero();
        }
        if (Cf::NDUMMY != 0 && f >= NT_ALL) return zero();
        const int kt = step * KTS + (f - WTILES) % KTS;
        const int k = (p.kt0 + kt) * 32 + (p.lane >> 4) * 8;
        return (kt < p.KTL && k < a.K) ? src[i] + (int64_t)step * (KTS * 32) : zero();
    }
    // all pieces of k-step `step` (staged in order) into buffer `buf`
    __device__ __forceinline__ void stage(const umv_gemm_args& a, char* smem, const TilePos& p, int step, int buf) {
        if (ragged && step == p.nsteps - 1) {
#pragma unroll
            for (int i = 0; i < TPW; ++i) issue(tail_src(a, p, i, step), dst_of(smem, p, buf, i));
            return;
        }
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            issue(cur[i], dst_of(smem, p, buf, i));
            cur[i] += bump[i];
        }
    }
};

// ----------------------------------------------------------------------------- SCHED = 0: the plain loop
// NBUF LDS buffers.  Pipeline per k-step t (one raw s_barrier, never a full vmcnt drain in steady state):
//     s_waitcnt vmcnt((NBUF-2) tiles)   my part of tile t has landed, tiles t+1.. stay in flight
//     s_barrier                         everyone's part of tile t landed AND everyone finished reading tile t-1
//     issue LDS-DMA for tile t+NBUF-1   into the buffer tile t-1 just vacated
//     ds_read fragments of tile t, MFMAs
template <class Cf>
__device__ __forceinline__ void tiled_loop_plain(const umv_gemm_args& a, char* smem, const TilePos& p, int KT, int NTT,
                                                 f32x4 (&acc)[Cf::TN][Cf::TM]) {
    constexpr int TN = Cf::TN, TM = Cf::TM, KTS = Cf::KTS, NBUF = Cf::NBUF, TPW = Cf::TPW;
    HalfLineStage<Cf> st;
    st.init(a, p, KT, NTT);
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b)
        if (b < p.nsteps) st.stage(a, smem, p, b, b);
    for (int step = 0; step < p.nsteps; ++step) {
        // tiles still allowed in flight behind tile `step`
        const int ahead = min(NBUF - 2, p.nsteps - 1 - step);
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * TPW) : "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        UMV_BARRIER();
        if (step + NBUF - 1 < p.nsteps) st.stage(a, smem, p, step + NBUF - 1, (step + NBUF - 1) % NBUF);
        const char* wb = smem + (step % NBUF) * Cf::BUF;
        const char* xb = wb + Cf::WTILES * 1024;
#pragma unroll
        for (int kk = 0; kk < KTS; ++kk) {
            bf16x8 wf[TN], xf[TM];
#pragma unroll
            for (int t = 0; t < TN; ++t) wf[t] = *reinterpret_cast<const bf16x8*>(wb + ((p.wn * TN + t) * KTS + kk) * 1024 + p.lane * 16);
#pragma unroll
            for (int j = 0; j < TM; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(xb + ((p.wm * TM + j) * KTS + kk) * 1024 + p.lane * 16);
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
                for (int j = 0; j < TM; ++j) acc[t][j] = mfma16(wf[t], xf[j], acc[t][j]);
        }
    }
}

// what the two interleaved loops do between k-steps: all fragment reads issued so far have landed
template <int TN, int TM>
__device__ __forceinline__ void frags_landed(bf16x8 (&wf)[TN], bf16x8 (&xf)[TM]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < TN; ++t) asm volatile("" : "+v"(wf[t]));
#pragma unroll
    for (int j = 0; j < TM; ++j) asm volatile("" : "+v"(xf[j]));
}
// ... and behind their last k-step: the trailing zero-page pieces have landed (the epilogue reuses the buffers), and - the asm MFMAs
// are opaque to the compiler's hazard recogniser - the XDL-write -> VALU-read wait states are covered by hand
template <int TN, int TM>
__device__ __forceinline__ void interleaved_loop_end(f32x4 (&acc)[TN][TM]) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int j = 0; j < TM; ++j) asm volatile("" : "+v"(acc[t][j]));
}

// ----------------------------------------------------------------------------- SCHED = 1: the interleaved loop (KTS == 1)
// With the plain loop every wave leaves the barrier, issues its 12 ds_read_b128 at once and only then its 32 MFMAs: the 8 waves'
// 96 KiB of fragment reads keep the LDS pipe busy for ~768 cycles during which the matrix pipes mostly wait, then LDS idles for
// the ~1024 cycles of MFMAs - the two phases add up (MfmaUtil 44 % from the PMC counters).  Here the fragments of tile t+1 are
// requested one ds_read at a time, spread evenly between the MFMAs of tile t (every 2-3 MFMAs for the 256 x 256 tile), so each wave
// starts its MFMAs right after the barrier and the LDS traffic is spread over the whole step.  MFMAs and ds_reads are inline asm
// so that the order is exactly the one written.
template <class Cf>
__device__ __forceinline__ void tiled_loop_interleaved(const umv_gemm_args& a, char* smem, const TilePos& p, int KT, int NTT,
                                                       f32x4 (&acc)[Cf::TN][Cf::TM]) {
    constexpr int TN = Cf::TN, TM = Cf::TM, NBUF = Cf::NBUF, TPW = Cf::TPW, BUF = Cf::BUF;
    static_assert(Cf::KTS == 1 && NBUF >= 3, "interleaved schedule needs KTS == 1 and >= 3 LDS buffers");
    using St = HalfLineStage<Cf>;
    St st;
    st.init(a, p, KT, NTT);
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b) {
        if (b < p.nsteps) st.stage(a, smem, p, b, b);
        else {       // (K < 96) keep the number of pieces in flight uniform: see below
#pragma unroll
            for (int i = 0; i < TPW; ++i) St::issue(St::zero(), St::dst_of(smem, p, b, i));
        }
    }
    bf16x8 wfA[TN], xfA[TM], wfB[TN], xfB[TM];
    const uint32_t lds0 = (uint32_t)(uintptr_t)(umv_lds_ptr_t)smem;
    const uint32_t woff = p.wn * TN * 1024 + p.lane * 16, xoff = Cf::WTILES * 1024 + p.wm * TM * 1024 + p.lane * 16;
    auto wait_tiles = [&](int allowed) {   // tiles (of TPW DMA ops each) that may stay in flight
        if (allowed >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * TPW) : "memory");
        else if (allowed == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    wait_tiles(NBUF - 2);
    UMV_BARRIER();
    static_for<0, TN>([&](auto T) {
        constexpr int t = decltype(T)::value;
        umv_lds_read128<t * 1024>(wfA[t], lds0 + woff);
    });
    static_for<0, TM>([&](auto J) {
        constexpr int j = decltype(J)::value;
        umv_lds_read128<j * 1024>(xfA[j], lds0 + xoff);
    });
    frags_landed(wfA, xfA);
    constexpr int NRD = TN + TM, NMMA = TN * TM;
    static_assert(NRD <= NMMA, "at most one fragment read per MFMA");
    // The TPW LDS-DMA pieces of tile step + NBUF - 1 are issued BETWEEN the MFMAs as well, one every NMMA / TPW MFMAs.
    // Issued in a burst behind the barrier (as the fragment reads once were) they keep the wave off the matrix pipe for
    // TPW x 100-185 cycles per k-step (the guide's price of a piece inside a busy phase) while its twin on the SIMD, in
    // lockstep, does the same.  That tile's buffer has been free since the barrier of the step before, and the counted
    // waits only need the pieces to be issued before the next step's wait: placement inside the step is free.  One
    // sequence for every step: the ragged last tile swaps its source pointers in before the sequence, and the last
    // NBUF - 1 steps, which have nothing left to stage, copy the zero page into the (free) buffer so that the count of
    // pieces in flight stays the same at every wait.
    static_assert(TPW <= NMMA, "at most one DMA piece per MFMA");
    auto body = [&](int step, bf16x8(&wc)[TN], bf16x8(&xc)[TM], bf16x8(&wnx)[TN], bf16x8(&xnx)[TM]) {
        wait_tiles(NBUF - 3);                                        // tile step+1 landed (mine); tile step+2's pieces may fly
        UMV_BARRIER();                                               // ... everyone's; and tile step-1's buffer is free
        const int sn = step + NBUF - 1;                              // the tile staged during this step
        if (sn >= p.nsteps) {
#pragma unroll
            for (int i = 0; i < TPW; ++i) { st.cur[i] = St::zero(); st.bump[i] = 0; }
        } else if (st.ragged && sn == p.nsteps - 1) {
#pragma unroll
            for (int i = 0; i < TPW; ++i) { st.cur[i] = st.tail_src(a, p, i, sn); st.bump[i] = 0; }
        }
        const int dma_buf = sn % NBUF;
        // the reads of the last step fetch a tile nobody uses (the buffer exists): no branch inside the sequence
        const uint32_t nb = lds0 + ((step + 1) % NBUF) * BUF;
        const uint32_t wa = nb + woff, xa = nb + xoff;
        static_for<0, NMMA>([&](auto I) {
            constexpr int i = decltype(I)::value, t = i / TM, j = i % TM;
            mfma16_asm(acc[t][j], wc[t], xc[j]);
            constexpr int rd = umv_interleave_slot(i, NMMA, NRD);   // the read (if any) that follows MFMA i
            if constexpr (rd >= 0 && rd < TN) umv_lds_read128<(rd < TN ? rd : 0) * 1024>(wnx[rd < TN ? rd : 0], wa);
            else if constexpr (rd >= TN) umv_lds_read128<(rd >= TN ? rd - TN : 0) * 1024>(xnx[rd >= TN ? rd - TN : 0], xa);
            constexpr int pc = umv_dma_slot(i, NMMA, TPW);          // the DMA piece (if any) that follows MFMA i
            if constexpr (pc >= 0) {
                __builtin_amdgcn_sched_barrier(0);
                St::issue(st.cur[pc], St::dst_of(smem, p, dma_buf, pc));
                st.cur[pc] += st.bump[pc];
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        frags_landed(wnx, xnx);
    };
    for (int step = 0; step < p.nsteps; step += 2) {
        body(step, wfA, xfA, wfB, xfB);
        if (step + 1 < p.nsteps) body(step + 1, wfB, xfB, wfA, xfA);
    }
    interleaved_loop_end(acc);
}

// ----------------------------------------------------------------------------- SCHED = 3: the interleaved loop, x in full lines
// The interleaved schedule of SCHED = 1 with the x operand staged in FULL 128-byte lines.  The 1 KiB x piece of
// SCHED = 1 gathers 16 rows x 64 bytes - half a line per row; the other half is fetched by the next k-step's piece, ~0.8 us
// later, when the line has long left the 32 KiB L1 - so an x byte costs twice the L1 miss entries and L2 -> L1 traffic of a
// W byte.  Measured at 8192^3 (TIMING-ONLY ablations, profiles/r04_gemm_ablations.txt): x pieces read as contiguous KiB 827 -> 766 us, no
// x pieces 712, no W pieces 663, no pieces at all 535 (2.05 PFLOP/s), pieces and fragment reads without MFMAs 722 us AT
// 2.4 GHz: the staging path, not the matrix pipe, sets the pace of this kernel.  (Issuing the two half-line pieces back
// to back in one step was tried first: 846 -> 941 us - the second request does not merge with the miss in flight.)
// Here a piece is 8 rows x 128 bytes = one k-step PAIR of 8 rows: lane L brings the 16-byte chunk (L & 7) ^ ((L >> 3) & 7) of
// row L >> 3, so that the row-major image [row][8 chunks] in LDS is XOR-swizzled by the row and the B fragment read of k-tile
// 2q + h, lane (r, g) -> chunk (4h + g) ^ (r & 7) of row r, is conflict free (each quarter-wave group covers all 64 banks).
// Rings: W 3 slots of one k-step (W(t+3) takes the slot of tile t, free behind the head barrier of body t), x 3 slots of one
// k-step pair (pair q is issued half in body 2q-5, half in body 2q-4): every wave issues WPW + XPB pieces per body, x first,
// so the counted wait at the head of a body - W(t+1) landed, the pieces of the previous body may fly - is one constant.
// Same MFMAs on the same operands in the same order: bit-identical to SCHED = 1.
template <class Cf>
__device__ __forceinline__ void tiled_loop_full_line(const umv_gemm_args& a, char* smem, const TilePos& p, int KT, int NTT,
                                                     f32x4 (&acc)[Cf::TN][Cf::TM]) {
    constexpr int TN = Cf::TN, TM = Cf::TM, NW = Cf::NW, WTILES = Cf::WTILES, BM = Cf::BM;
    constexpr int WPW = WTILES / NW, XPP = (BM / 8) / NW, XPB = XPP / 2, NP = WPW + XPB;
    static_assert(Cf::KTS == 1 && WTILES % NW == 0 && (BM / 8) % NW == 0 && XPP % 2 == 0, "full-line x staging: even split of the pieces over the waves");
    constexpr int WSLOT = WTILES * 1024, XSLOT = BM * 128, XBASE = 3 * WSLOT;
    constexpr int NRD = TN + TM, NMMA = TN * TM;
    static_assert(NRD <= NMMA && NP <= NMMA, "at most one read / piece per MFMA");
    const int lane = p.lane, wave = p.wave, r = lane & 15, g = lane >> 4;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(umv_zero_page);
    const int kx_rel = min(a.K, p.kt1 * 32) - p.kt0 * 32;             // valid k (elements) of this block's range, relative to kt0
    const bf16_t* curW[WPW];
    int bumpW[WPW];
    const bf16_t* curX[XPP];
    const int xchunk = (lane & 7) ^ ((lane >> 3) & 7);
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
        const int nt = p.nt_blk + wave * WPW + i;
        const bool ok = nt < NTT;
        curW[i] = ok ? a.wp + ((int64_t)nt * KT + p.kt0) * 512 + lane * 8 : zero;
        bumpW[i] = ok ? 512 : 0;
    }
#pragma unroll
    for (int i = 0; i < XPP; ++i) {
        const int m = p.m0 + (wave * XPP + i) * 8 + (lane >> 3);
        const int mm = m < a.M ? m : a.M - 1;                // rows past M are clamped (their outputs are masked)
        const int64_t row = a.row_idx ? (int64_t)a.row_idx[mm] : (int64_t)mm;
        curX[i] = a.x + row * a.ldx + p.kt0 * 32 + xchunk * 8;
    }
    // (char* and a cast at the call: a lambda RETURNING an address_space(3) pointer makes the host pass drop the kernel's stub
    // without a diagnostic - the library then fails to load with an undefined __device_stub__ symbol)
    auto dstW = [&](int slot, int i) -> char* { return smem + slot * WSLOT + (wave * WPW + i) * 1024; };
    auto dstX = [&](int slot, int i) -> char* { return smem + XBASE + slot * XSLOT + (wave * XPP + i) * 1024; };
    const bf16_t* pw[WPW];
    const bf16_t* px[XPB];
    auto prep_w = [&](int kt) {                 // the W pieces of k-tile kt (relative to kt0): zero page past the K range
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            pw[i] = kt < p.KTL ? curW[i] : zero;
            curW[i] += bumpW[i];
        }
    };
    auto prep_x = [&](int q, auto HALF) {       // pieces [HALF * XPB, +XPB) of k-step pair q: per-lane zero fill at the K tail
        constexpr int hf = decltype(HALF)::value;
        const int k0 = q * 64;
        if (k0 + 64 <= kx_rel) {
#pragma unroll
            for (int i = 0; i < XPB; ++i) { px[i] = curX[hf * XPB + i]; curX[hf * XPB + i] += 64; }
        } else {
#pragma unroll
            for (int i = 0; i < XPB; ++i) { px[i] = (k0 + xchunk * 8 < kx_rel) ? curX[hf * XPB + i] : zero; curX[hf * XPB + i] += 64; }
        }
    };
    // prologue, in the order the loop would have issued it: x pair 0, W(0), x pair 1, W(1), first half of x pair 2, W(2)
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        prep_x(t, std::integral_constant<int, 0>{});
#pragma unroll
        for (int i = 0; i < XPB; ++i) __builtin_amdgcn_global_load_lds((const void*)px[i], (umv_lds_ptr_t)dstX(t, i), 16, 0, 0);
        if (t < 2) {
            prep_x(t, std::integral_constant<int, 1>{});
#pragma unroll
            for (int i = 0; i < XPB; ++i) __builtin_amdgcn_global_load_lds((const void*)px[i], (umv_lds_ptr_t)dstX(t, XPB + i), 16, 0, 0);
        }
        prep_w(t);
#pragma unroll
        for (int i = 0; i < WPW; ++i) __builtin_amdgcn_global_load_lds((const void*)pw[i], (umv_lds_ptr_t)dstW(t, i), 16, 0, 0);
    }
    bf16x8 wfA[TN], xfA[TM], wfB[TN], xfB[TM];
    const uint32_t lds0 = (uint32_t)(uintptr_t)(umv_lds_ptr_t)smem;
    const uint32_t woff = p.wn * TN * 1024 + lane * 16;
    // x fragment of k half h: row (wm * TM + j) * 16 + r, chunk (4h + g) ^ (r & 7)
    const uint32_t xoff0 = XBASE + (p.wm * TM * 16 + r) * 128 + ((g ^ (r & 7)) << 4), xoff1 = xoff0 ^ 64;
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XPP + XPB + 2 * WPW) : "memory");      // x pair 0 and W(0) landed; pair 1, W(1), half of pair 2 and W(2) may fly
    UMV_BARRIER();
    static_for<0, TN>([&](auto T) {
        constexpr int t = decltype(T)::value;
        umv_lds_read128<t * 1024>(wfA[t], lds0 + woff);
    });
    static_for<0, TM>([&](auto J) {
        constexpr int j = decltype(J)::value;
        umv_lds_read128<j * 2048>(xfA[j], lds0 + xoff0);
    });
    frags_landed(wfA, xfA);
    auto body = [&](auto EVEN, int step, bf16x8(&wc)[TN], bf16x8(&xc)[TM], bf16x8(&wnx)[TN], bf16x8(&xnx)[TM]) {
        constexpr bool even = decltype(EVEN)::value;
        // the fragments of tile `step` are in registers; tile step + 1 must have landed before its reads below
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");
        UMV_BARRIER();                                   // ... everyone's; and the slot of W tile `step` is free
        const int q = (step + 5) >> 1;                   // the x pair this body stages half of
        if constexpr (even) prep_x(q, std::integral_constant<int, 1>{});
        else prep_x(q, std::integral_constant<int, 0>{});
        prep_w(step + 3);
        const int sw = step % 3, sx = q % 3;
        const uint32_t wa = lds0 + ((step + 1) % 3) * WSLOT + woff;
        const uint32_t xa = lds0 + (((step + 1) >> 1) % 3) * XSLOT + (even ? xoff1 : xoff0);     // tile step + 1 is the odd half in an even body
        static_for<0, NMMA>([&](auto I) {
            constexpr int i = decltype(I)::value, t = i / TM, j = i % TM;
            mfma16_asm(acc[t][j], wc[t], xc[j]);
            constexpr int rd = umv_interleave_slot(i, NMMA, NRD);
            if constexpr (rd >= 0 && rd < TN) umv_lds_read128<(rd < TN ? rd : 0) * 1024>(wnx[rd < TN ? rd : 0], wa);
            else if constexpr (rd >= TN) umv_lds_read128<(rd >= TN ? rd - TN : 0) * 2048>(xnx[rd >= TN ? rd - TN : 0], xa);
            constexpr int pc = umv_dma_slot(i, NMMA, NP);
            if constexpr (pc >= 0) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (pc < XPB)
                    __builtin_amdgcn_global_load_lds((const void*)px[pc < XPB ? pc : 0], (umv_lds_ptr_t)dstX(sx, (even ? XPB : 0) + pc), 16, 0, 0);
                else
                    __builtin_amdgcn_global_load_lds((const void*)pw[pc >= XPB ? pc - XPB : 0], (umv_lds_ptr_t)dstW(sw, pc - XPB), 16, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        frags_landed(wnx, xnx);
    };
    for (int step = 0; step < p.nsteps; step += 2) {
        body(std::true_type{}, step, wfA, xfA, wfB, xfB);
        if (step + 1 < p.nsteps) body(std::false_type{}, step + 1, wfB, xfB, wfA, xfA);
    }
    interleaved_loop_end(acc);
}

// ----------------------------------------------------------------------------- the kernel: frame -> main loop -> epilogue
template <int WN, int WM, int TN, int TM, int KTS, int NBUF, int SCHED = 0>
__global__ __launch_bounds__(WN * WM * 64) void gemm_tiled_kernel(umv_gemm_args a, int KT, int NTT, int mblocks, int nblocks, int gn,
                                                                  int ksplit, int ms, int lean) {
    using Cf = TiledCfg<WN, WM, TN, TM, KTS, NBUF, SCHED>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    TilePos p;
    p.lane = tid & 63;
    p.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    p.wn = p.wave % WN, p.wm = p.wave / WN;
    int mblk, nblk;
    umv_tile_order(mblocks, nblocks, gn, ms, (int)blockIdx.x, mblk, nblk);
    p.m0 = mblk * Cf::BM;
    p.nt_blk = nblk * (Cf::BN / 16);
    const int nt_base = p.nt_blk + p.wn * TN;
    bf16_t* bias_lds = reinterpret_cast<bf16_t*>(smem + Cf::STAGE_BYTES);
    umv_bias_to_lds<Cf::BN, Cf::NW * 64>(a, bias_lds, p.nt_blk, tid);
    // split-K (ksplit = k-tiles per split, 0 = none): blockIdx.y owns k-tiles [kt0, kt1) and stores raw fp32 partial sums
    // (the decode GEMMs with N = 3584 / 4608 at 65..128 rows: 14-36 workgroups otherwise)
    p.kt0 = ksplit ? (int)blockIdx.y * ksplit : 0;
    p.kt1 = ksplit ? min(KT, p.kt0 + ksplit) : KT;
    p.KTL = max(0, p.kt1 - p.kt0);
    p.nsteps = (p.KTL + KTS - 1) / KTS;

    f32x4 acc[TN][TM];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (SCHED == 3) tiled_loop_full_line<Cf>(a, smem, p, KT, NTT, acc);
    else if constexpr (SCHED == 1) tiled_loop_interleaved<Cf>(a, smem, p, KT, NTT, acc);
    else tiled_loop_plain<Cf>(a, smem, p, KT, NTT, acc);

    // epilogue with compile-time accumulator indices (a runtime-indexed acc[][] would be demoted to scratch)
    EpiCtx e{a.bias, a.residual, a.ldr, a.out, a.ldo, a.N, a.epilogue};
    if (ksplit) {   // partial sums: fp32, no bias / activation / residual (umv_qkv_post / umv_residual_rmsnorm_bf16 finish the row)
        e.out = reinterpret_cast<float*>(a.out) + (int64_t)blockIdx.y * a.split_stride;
        e.flags = UMV_EPI_OUT_F32;
    }
    const int m_wave0 = p.m0 + p.wm * TM * 16;
    // bf16 outputs leave through LDS as whole rows (gemm_epilogue.h); fp32 outputs (split-K partials, OUT_F32) directly
    if (e.flags & UMV_EPI_OUT_F32) {
        epi_wave_tile_direct<TN, TM>(e, acc, p.lane, m_wave0, a.M, a.row_idx, nt_base, NTT);
        return;
    }
    UMV_BARRIER();      // every wave has read its last fragments: the staging buffers are free
    char* wreg = smem + p.wave * (TN * TM * 512);
    // lean >= 0: the branch-free form of gemm_epilogue.h for this call's flag combination (epi_lean_kind); bit-identical
    if (lean >= 0 && !ksplit && epi_wave_tile_lean_any<TN, TM>(lean, a, acc, wreg, p.lane, m_wave0, nt_base, bias_lds + p.wn * TN * 16)) return;
    epi_wave_tile_lds<TN, TM>(e, acc, wreg, p.lane, m_wave0, a.M, a.row_idx, nt_base, NTT, bias_lds + p.wn * TN * 16);
}
