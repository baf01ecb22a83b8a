// q/k norm + RoPE + KV append: the fused QKV row of a GEMM becomes q rows and K / V^T slab entries.
#include "common.h"
#include "../../include/unimedvl_hip.h"

// Where token t's K row / V^T column goes: the (segment, slot) pair of tok_seg / tok_slot, or - paged KV (umv_qkv_post_args.page_table) -
// (pool page, slot inside the page); every kernel below addresses  base + seg * seg_stride + ... + slot  with these two values
__device__ __forceinline__ int kv_seg(const umv_qkv_post_args& a, int t) {
    const int seg = a.tok_seg[t];
    return a.page_table ? a.page_table[(int64_t)seg * a.page_table_stride + (a.tok_slot[t] >> UMV_KV_PAGE_LOG2)] : seg;
}
__device__ __forceinline__ int kv_slot(const umv_qkv_post_args& a, int t) {
    const int slot = a.tok_slot[t];
    return a.page_table ? (slot & (UMV_KV_PAGE - 1)) : slot;
}

// ----------------------------------------------------------------------------- q/k norm + RoPE + KV append
// Qwen2RMSNorm + RoPE of one rotate_half pair (x1 = x[d], x2 = x[d + hd/2]; c / s: cos / sin at d and at d + hd/2), the ONE
// statement of both chains - every kernel that normalises a head calls it, so a decode step equals the prefill of the same token:
// und chain (bf16 tensors, qwen2_navit.py:544-545,576-583):
//    n = bf16(w * bf16(x*rstd));  out = bf16(bf16(n*cos) + bf16(rot(n)*sin))
// gen chain (fp32 tensors, qwen2_navit.py:568-583):
//    n = w * (x*rstd);  out = bf16(n*cos + rot(n)*sin)      (cos/sin are bf16 values; the caller's store rounds)
__device__ __forceinline__ void norm_rope_pair(bool gen, float x1, float x2, float w1, float w2, float c1, float s1, float c2, float s2,
                                               float rstd, float& o1, float& o2) {
    if (!gen) {
        const float n1 = rbf(w1 * rbf(x1 * rstd)), n2 = rbf(w2 * rbf(x2 * rstd));
        o1 = rbf(rbf(n1 * c1) + rbf(-n2 * s1));
        o2 = rbf(rbf(n2 * c2) + rbf(n1 * s2));
    } else {
        const float n1 = __fmul_rn(w1, __fmul_rn(x1, rstd)), n2 = __fmul_rn(w2, __fmul_rn(x2, rstd));
        o1 = __fadd_rn(__fmul_rn(n1, c1), __fmul_rn(-n2, s1));
        o2 = __fadd_rn(__fmul_rn(n2, c2), __fmul_rn(n1, s2));
    }
}

// x1 / x2 += sum_s p[s * split_stride (+ half)] + bias[col (+ half)] for up to W splits, added in order 0..S-1: every split (and the
// bias) is requested before the first add - one memory round trip instead of one per split
template <int W>
__device__ __forceinline__ void split_sum_wide(const float* p, int n_splits, int64_t split_stride, int half, const bf16_t* bias, int64_t col,
                                               float& x1, float& x2) {
    float t1[W], t2[W];
#pragma unroll
    for (int s = 0; s < W; ++s) {
        const int ss = s < n_splits ? s : 0;     // clamped address, masked below: no branch around the loads
        t1[s] = p[ss * split_stride];
        t2[s] = p[ss * split_stride + half];
    }
    const float b1 = bias ? bf2f(bias[col]) : 0.f, b2 = bias ? bf2f(bias[col + half]) : 0.f;
#pragma unroll
    for (int s = 0; s < W; ++s)
        if (s < n_splits) { x1 += t1[s]; x2 += t2[s]; }
    if (bias) { x1 += b1; x2 += b2; }
}

// One wavefront per (token, head) over the nq + 2*nkv heads of the fused QKV row.
// Lane i owns element i of the first half and the matching one of the second
// half (rotate_half pairs x[d] with x[d + hd/2], modeling_qwen2.py:188-192).
template <int HD>
__global__ __launch_bounds__(256) void qkv_post_kernel(umv_qkv_post_args a) {
    constexpr int HALF = HD / 2;
    const int lane = threadIdx.x & 63;
    const int nheads = a.nq + 2 * a.nkv;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)a.T * nheads) return;
    const int t = (int)(item / nheads);
    const int h = (int)(item % nheads);
    const bf16_t* src = a.qkv + (int64_t)t * nheads * HD + (int64_t)h * HD;
    const int seg = kv_seg(a, t), slot = kv_slot(a, t);
    const bool is_q = h < a.nq, is_k = !is_q && h < a.nq + a.nkv;
    const bool act = lane < HALF;  // HD=128: all 64 lanes; HD=72: 36 lanes
    // The kernel is one dependent chain of memory round trips at decode sizes, so everything that does not depend on the
    // row itself is requested first: position -> cos / sin, expert flag -> norm weight (this kernel always has the norms).
    const bool is_v = !is_q && !is_k;
    const int pos = a.tok_pos[t];
    const bf16_t* nw = is_q ? a.q_norm_w : a.k_norm_w;
    if (a.expert && a.expert[t]) nw = is_q ? a.q_norm_w_gen : a.k_norm_w_gen;
    float c1 = 0.f, s1 = 0.f, c2 = 0.f, s2 = 0.f, w1 = 0.f, w2 = 0.f;
    if (act && !is_v) {
        c1 = bf2f(a.cos_tab[(int64_t)pos * HD + lane]);
        s1 = bf2f(a.sin_tab[(int64_t)pos * HD + lane]);
        c2 = bf2f(a.cos_tab[(int64_t)pos * HD + lane + HALF]);
        s2 = bf2f(a.sin_tab[(int64_t)pos * HD + lane + HALF]);
        w1 = bf2f(nw[lane]);
        w2 = bf2f(nw[lane + HALF]);
    }
    float x1 = 0.f, x2 = 0.f;
    if (act) {
        if (a.qkv_partials) {   // split-K QKV GEMM: x = bf16(sum_s P[s] + bias), the rounding of the GEMM epilogue it replaces
            const int64_t col = (int64_t)h * HD + lane;
            const float* p = a.qkv_partials + (int64_t)t * nheads * HD + col;
            const int64_t sst = a.split_stride;
            if (a.n_splits <= 4) split_sum_wide<4>(p, a.n_splits, sst, HALF, a.qkv_bias, col, x1, x2);   // the usual case
            else if (a.n_splits <= 8) split_sum_wide<8>(p, a.n_splits, sst, HALF, a.qkv_bias, col, x1, x2);   // 65..128 samples (6 splits)
            else {
                for (int s = 0; s < a.n_splits; ++s) { x1 += p[s * sst]; x2 += p[s * sst + HALF]; }
                if (a.qkv_bias) { x1 += bf2f(a.qkv_bias[col]); x2 += bf2f(a.qkv_bias[col + HALF]); }
            }
            x1 = rbf(x1);
            x2 = rbf(x2);
        } else {
            x1 = bf2f(src[lane]);
            x2 = bf2f(src[lane + HALF]);
        }
    }
    if (is_v) {  // V head: transposed store V^T[seg][kvh][d][slot]
        const int kvh = h - a.nq - a.nkv;
        bf16_t* dst = a.vt_slab + seg * a.v_seg_stride + kvh * a.v_head_stride + slot;
        if (act) {
            dst[(int64_t)lane * a.v_d_stride] = f2bf(x1);
            dst[(int64_t)(lane + HALF) * a.v_d_stride] = f2bf(x2);
        }
        return;
    }
    const float rstd = rsqrt_ieee(wave_sum(x1 * x1 + x2 * x2) / (float)HD + a.eps);
    float o1, o2;
    norm_rope_pair(a.fp32_chain != 0, x1, x2, w1, w2, c1, s1, c2, s2, rstd, o1, o2);
    if (is_q) {
        bf16_t* dst = a.q_out + (int64_t)t * a.nq * HD + (int64_t)h * HD;
        if (act) { dst[lane] = f2bf(o1); dst[lane + HALF] = f2bf(o2); }
    } else {
        const int kvh = h - a.nq;
        bf16_t* dst = a.k_slab + seg * a.k_seg_stride + kvh * a.k_head_stride + (int64_t)slot * HD;
        if (act) { dst[lane] = f2bf(o1); dst[lane + HALF] = f2bf(o2); }
    }
}

// No norm / no RoPE (ViT, VAE mid-block attention): split the fused QKV row into q rows and
// K / V^T slab entries, any head_dim.
__global__ __launch_bounds__(256) void qkv_split_kernel(umv_qkv_post_args a) {
    const int lane = threadIdx.x & 63;
    const int HD = a.hd;
    const int nheads = a.nq + 2 * a.nkv;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)a.T * nheads) return;
    const int t = (int)(item / nheads);
    const int h = (int)(item % nheads);
    const bf16_t* src = a.qkv + (int64_t)t * nheads * HD + (int64_t)h * HD;
    const int seg = kv_seg(a, t), slot = kv_slot(a, t);
    if (h < a.nq) {
        bf16_t* dst = a.q_out + (int64_t)t * a.nq * HD + (int64_t)h * HD;
        for (int d = lane; d < HD; d += 64) dst[d] = src[d];
    } else if (h < a.nq + a.nkv) {
        bf16_t* dst = a.k_slab + seg * a.k_seg_stride + (h - a.nq) * a.k_head_stride + (int64_t)slot * HD;
        for (int d = lane; d < HD; d += 64) dst[d] = src[d];
    } else {
        bf16_t* dst = a.vt_slab + seg * a.v_seg_stride + (h - a.nq - a.nkv) * a.v_head_stride + slot;
        for (int d = lane; d < HD; d += 64) dst[(int64_t)d * a.v_d_stride] = src[d];
    }
}

// The same split for hd % 8 == 0, eight tokens per workgroup: q and K rows move as 16-byte pieces, and the eight V rows
// meet in LDS so that a thread writes 8 consecutive slots (16 bytes) of one V^T row instead of eight 2-byte stores a
// cache line apart (one wave per (token, head) with 2-byte accesses took 75 us per ViT layer for 112 MB of traffic).
// Groups whose tokens are not 8 consecutive, 8-aligned slots of one segment fall back to element stores.
__global__ __launch_bounds__(256) void qkv_split_tile_kernel(umv_qkv_post_args a) {
    extern __shared__ __attribute__((aligned(16))) bf16_t vs[];      // [8][nkv * hd]
    const int HD = a.hd, CH = HD / 8, nheads = a.nq + 2 * a.nkv;
    const int t0 = blockIdx.x * 8, nt = min(8, a.T - t0);
    const int q_ch = a.nq * CH, qk_ch = (a.nq + a.nkv) * CH, row_ch = nheads * CH, nv = a.nkv * HD;
    // q_out == null: V only - q and K stay where the GEMM wrote them (umv_attn_varlen's q_row_stride / k_key_stride form)
    const int c_lo = a.q_out ? 0 : qk_ch, span = row_ch - c_lo;
    for (int i = threadIdx.x; i < nt * span; i += 256) {
        const int tt = i / span, c = c_lo + (i - tt * span);
        const int t = t0 + tt;
        const bf16x8 v = ldg_frag(a.qkv + (int64_t)t * nheads * HD + (int64_t)c * 8);
        if (c < q_ch) {
            *reinterpret_cast<bf16x8*>(a.q_out + (int64_t)t * a.nq * HD + (int64_t)c * 8) = v;
        } else if (c < qk_ch) {
            const int h = (c - q_ch) / CH, cc = (c - q_ch) - h * CH;
            *reinterpret_cast<bf16x8*>(a.k_slab + kv_seg(a, t) * a.k_seg_stride + h * a.k_head_stride + (int64_t)kv_slot(a, t) * HD + cc * 8) = v;
        } else {
            *reinterpret_cast<bf16x8*>(vs + tt * nv + (c - qk_ch) * 8) = v;
        }
    }
    __syncthreads();
    const int seg0 = kv_seg(a, t0), slot0 = kv_slot(a, t0);
    bool run8 = nt == 8 && (slot0 & 7) == 0;
    for (int tt = 1; tt < nt && run8; ++tt) run8 = kv_seg(a, t0 + tt) == seg0 && kv_slot(a, t0 + tt) == slot0 + tt;
    if (run8) {
        for (int e = threadIdx.x; e < nv; e += 256) {
            const int h = e / HD, d = e - h * HD;
            bf16x8 o;
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) o[tt] = (short)vs[tt * nv + e];
            *reinterpret_cast<bf16x8*>(a.vt_slab + seg0 * a.v_seg_stride + h * a.v_head_stride + (int64_t)d * a.v_d_stride + slot0) = o;
        }
    } else {
        for (int i = threadIdx.x; i < nt * nv; i += 256) {
            const int tt = i / nv, e = i - tt * nv;
            const int h = e / HD, d = e - h * HD;
            const int t = t0 + tt;
            a.vt_slab[kv_seg(a, t) * a.v_seg_stride + h * a.v_head_stride + (int64_t)d * a.v_d_stride + kv_slot(a, t)] = vs[tt * nv + e];
        }
    }
}

// V-only split (the cache-less SigLIP tower: q and K are read by the attention kernel where the QKV GEMM wrote them) as an
// in-register transpose: a thread owns 8 tokens x 8 dims - eight 16-byte loads (one per token), an 8 x 8 transpose of bf16
// pairs with v_perm_b32, eight 16-byte stores (one per dim: 8 consecutive slots of a V^T row).  A wave is 8 dim-octets x 8
// token-octets, so a load instruction covers 8 x 128 contiguous bytes of 8 token rows and a store instruction 8 x 128
// contiguous bytes of 8 V^T rows: whole cache lines both ways (the LDS version above writes 16 bytes per V^T row and
// workgroup: 19.6 us per ViT layer for 2 x 18.9 MB).  Token octets that are not 8 consecutive, 8-aligned slots of one
// segment fall back to element stores.
__global__ __launch_bounds__(256) void v_transpose_kernel(umv_qkv_post_args a) {
    const int HD = a.hd, nheads = a.nq + 2 * a.nkv, nv = a.nkv * HD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane & 7, jl = lane >> 3;
    const int e0 = (blockIdx.y * 8 + cl) * 8;                       // first of this thread's 8 V dims (over all kv heads)
    const int t0 = ((int)blockIdx.x * 4 + wave) * 64 + jl * 8;      // first of its 8 tokens
    if (e0 >= nv || t0 >= a.T) return;
    const int nt = min(8, a.T - t0);
    const bf16_t* src = a.qkv + (int64_t)t0 * nheads * HD + (int64_t)(a.nq + a.nkv) * HD + e0;
    u32x4 r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = i < nt ? *reinterpret_cast<const u32x4*>(src + (int64_t)i * nheads * HD) : (u32x4){0u, 0u, 0u, 0u};
    const int seg0 = kv_seg(a, t0), slot0 = kv_slot(a, t0);
    bool run8 = nt == 8 && (slot0 & 7) == 0;
#pragma unroll
    for (int i = 1; i < 8; ++i)
        if (i < nt) run8 = run8 && kv_seg(a, t0 + i) == seg0 && kv_slot(a, t0 + i) == slot0 + i;
    const int h = e0 / HD, d0 = e0 - h * HD;                        // HD % 8 == 0: the 8 dims lie in one head
    if (run8) {
        bf16_t* dst = a.vt_slab + seg0 * a.v_seg_stride + h * a.v_head_stride + (int64_t)d0 * a.v_d_stride + slot0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            // bytes of {hi = r[2k+1], lo = r[2k]}.dword[d >> 1]: low halves 0x05040100, high halves 0x07060302
            const uint32_t sel = (d & 1) ? 0x07060302u : 0x05040100u;
            u32x4 o;
            o.x = __builtin_amdgcn_perm(r[1][d >> 1], r[0][d >> 1], sel);
            o.y = __builtin_amdgcn_perm(r[3][d >> 1], r[2][d >> 1], sel);
            o.z = __builtin_amdgcn_perm(r[5][d >> 1], r[4][d >> 1], sel);
            o.w = __builtin_amdgcn_perm(r[7][d >> 1], r[6][d >> 1], sel);
            *reinterpret_cast<u32x4*>(dst + (int64_t)d * a.v_d_stride) = o;
        }
    } else {
        for (int i = 0; i < nt; ++i) {
            bf16_t* dst = a.vt_slab + kv_seg(a, t0 + i) * a.v_seg_stride + h * a.v_head_stride + (int64_t)d0 * a.v_d_stride + kv_slot(a, t0 + i);
#pragma unroll
            for (int d = 0; d < 8; ++d) dst[(int64_t)d * a.v_d_stride] = (bf16_t)(r[i][d >> 1] >> ((d & 1) * 16));
        }
    }
}

// q / k heads of a LONG forward (prefill, flow passes: T >= 64 rows of bf16 qkv, head_dim 128): qkv_post_kernel's arithmetic with
// 8-byte accesses - 16 lanes per (token, head), lane `sub` owns elements 4 sub .. 4 sub + 3 of the first half and the matching
// ones of the second half (rotate_half pairs x[d] with x[d + 64]), four items per wave.  The per-(token, head) wave with 2-byte
// accesses took 25-27 us per layer of a guided flow pass (2064 rows) and 100 us per layer of an 8-image prefill.  The row sum of
// squares follows qkv_post_kernel's butterfly exactly (lane bits 5, 4, 3, 2 there are sub bits 3, 2, 1, 0 here, lane bits 1, 0
// the element index), so the results are bit-identical and a decode step still equals the prefill of the same token.
// V heads go through v_transpose_kernel.
__global__ __launch_bounds__(256) void qk_post_vec128_kernel(umv_qkv_post_args a) {
    constexpr int HD = 128, HALF = 64;
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int nqk = a.nq + a.nkv, nheads = a.nq + 2 * a.nkv;
    const int64_t item = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const bool live = item < (int64_t)a.T * nqk;
    const int t = live ? (int)(item / nqk) : 0;
    const int h = live ? (int)(item % nqk) : 0;
    const bool is_q = h < a.nq;
    const int pos = a.tok_pos[t];
    const bf16_t* nw = is_q ? a.q_norm_w : a.k_norm_w;
    if (a.expert && a.expert[t]) nw = is_q ? a.q_norm_w_gen : a.k_norm_w_gen;
    auto ld4 = [](const bf16_t* p, float* o) {
        const u32x2 v = *reinterpret_cast<const u32x2*>(p);
        o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xFFFF0000u);
        o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xFFFF0000u);
    };
    const bf16_t* src = a.qkv + (int64_t)t * nheads * HD + (int64_t)h * HD + 4 * sub;
    float x1[4], x2[4], c1[4], s1[4], c2[4], s2[4], w1[4], w2[4];
    ld4(src, x1); ld4(src + HALF, x2);
    ld4(a.cos_tab + (int64_t)pos * HD + 4 * sub, c1); ld4(a.sin_tab + (int64_t)pos * HD + 4 * sub, s1);
    ld4(a.cos_tab + (int64_t)pos * HD + HALF + 4 * sub, c2); ld4(a.sin_tab + (int64_t)pos * HD + HALF + 4 * sub, s2);
    ld4(nw + 4 * sub, w1); ld4(nw + HALF + 4 * sub, w2);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float q = x1[e] * x1[e] + x2[e] * x2[e];
        q += row_xor<8>(q);      // lane bit 5 of the per-head wave
        q += row_xor<4>(q);      // bit 4
        q += row_xor<2>(q);      // bit 3
        q += row_xor<1>(q);      // bit 2
        v[e] = q;
    }
    const float ss = (v[0] + v[2]) + (v[1] + v[3]);       // bits 1, 0
    const float rstd = rsqrt_ieee(ss / (float)HD + a.eps);
    const bool gen = a.fp32_chain != 0;
    float o1[4], o2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) norm_rope_pair(gen, x1[e], x2[e], w1[e], w2[e], c1[e], s1[e], c2[e], s2[e], rstd, o1[e], o2[e]);
    if (!live) return;
    bf16_t* dst = is_q ? a.q_out + (int64_t)t * a.nq * HD + (int64_t)h * HD
                       : a.k_slab + kv_seg(a, t) * a.k_seg_stride + (h - a.nq) * a.k_head_stride + (int64_t)kv_slot(a, t) * HD;
    u32x2 p1, p2;
    p1.x = pack2bf(o1[0], o1[1]); p1.y = pack2bf(o1[2], o1[3]);
    p2.x = pack2bf(o2[0], o2[1]); p2.y = pack2bf(o2[2], o2[3]);
    *reinterpret_cast<u32x2*>(dst + 4 * sub) = p1;
    *reinterpret_cast<u32x2*>(dst + HALF + 4 * sub) = p2;
}

extern "C" int umv_qkv_post(const umv_qkv_post_args* ap, umv_stream_t stream) {
    UMV_CHECK(ap, UMV_ERR_ARG, "qkv_post: null args");
    const umv_qkv_post_args& a = *ap;
    const bool v_only = !a.q_out && !a.k_slab;      // plain split of V only (no norm / RoPE, head_dim % 8 == 0): q and K are read in place
    UMV_CHECK((a.qkv || a.qkv_partials) && (v_only || (a.q_out && a.k_slab)) && a.vt_slab && a.tok_seg && a.tok_slot, UMV_ERR_ARG, "qkv_post: null pointer");
    UMV_CHECK(!v_only || (a.qkv && !a.q_norm_w && (a.hd % 8) == 0 && (size_t)8 * a.nkv * a.hd * sizeof(bf16_t) <= 64 * 1024), UMV_ERR_UNSUPPORTED,
              "qkv_post: the V-only split needs bf16 qkv rows, no norm / RoPE and head_dim %% 8 == 0");
    // v_transpose_kernel stores 8 slots of one V^T row with one 16-byte store: every V^T stride must keep those stores aligned
    UMV_CHECK(!v_only || ((a.v_d_stride % 8) == 0 && (a.v_head_stride % 8) == 0 && (a.v_seg_stride % 8) == 0), UMV_ERR_UNSUPPORTED,
              "qkv_post: the V-only split needs V^T strides that are multiples of 8 elements (d %lld, head %lld, segment %lld)",
              (long long)a.v_d_stride, (long long)a.v_head_stride, (long long)a.v_seg_stride);
    UMV_CHECK(!a.qkv_partials || (a.q_norm_w && a.n_splits >= 1 && a.n_splits <= 64), UMV_ERR_ARG,
              "qkv_post: fp32 partial input needs the norm + RoPE path and 1 <= n_splits <= 64");
    UMV_CHECK(!a.q_norm_w || (a.k_norm_w && a.cos_tab && a.sin_tab && a.tok_pos), UMV_ERR_ARG, "qkv_post: norm without rope tables");
    UMV_CHECK(!a.expert || (a.q_norm_w_gen && a.k_norm_w_gen), UMV_ERR_ARG, "qkv_post: expert routing without gen norms");
    UMV_CHECK(!a.page_table || (a.page_table_stride > 0 && a.v_d_stride == UMV_KV_PAGE), UMV_ERR_ARG,
              "qkv_post: paged KV needs page_table_stride > 0 and V^T rows of UMV_KV_PAGE = %d keys (v_d_stride %lld)", UMV_KV_PAGE, (long long)a.v_d_stride);
    if (a.T == 0) return UMV_OK;
    int64_t items = (int64_t)a.T * (a.nq + 2 * a.nkv);
    dim3 grid((unsigned)((items + 3) / 4)), block(256);
    const size_t tile_lds = (size_t)8 * a.nkv * a.hd * sizeof(bf16_t);
    const bool tile_ok = (a.hd % 8) == 0 && tile_lds <= 64 * 1024;
    if (v_only) {       // (hd % 8 == 0 checked above)
        const int nv8 = a.nkv * a.hd / 8;
        hipLaunchKernelGGL(v_transpose_kernel, dim3((unsigned)((a.T + 255) / 256), (unsigned)((nv8 + 7) / 8)), block, 0, (hipStream_t)stream, a);
    } else if (!a.q_norm_w && tile_ok) {
        hipLaunchKernelGGL(qkv_split_tile_kernel, dim3((unsigned)((a.T + 7) / 8)), block, tile_lds, (hipStream_t)stream, a);
    } else if (!a.q_norm_w) {
        hipLaunchKernelGGL(qkv_split_kernel, grid, block, 0, (hipStream_t)stream, a);
    } else {
        UMV_CHECK(a.hd == 128 || a.hd == 72, UMV_ERR_UNSUPPORTED, "qkv_post: head_dim %d unsupported (128, 72)", a.hd);
        static const int vec = [] { const char* e = getenv("UMV_QKV_POST_VEC"); return e ? atoi(e) : 1; }();      // UMV_QKV_POST_VEC=0: the per-(token, head) wave for every size (A/B only; read once, thread-safe)
        if (vec && a.hd == 128 && !a.qkv_partials && a.T >= 64 && (a.v_d_stride % 8) == 0) {
            const int64_t qk_items = (int64_t)a.T * (a.nq + a.nkv);
            hipLaunchKernelGGL(qk_post_vec128_kernel, dim3((unsigned)((qk_items + 15) / 16)), block, 0, (hipStream_t)stream, a);
            const int nv8 = a.nkv * a.hd / 8;
            hipLaunchKernelGGL(v_transpose_kernel, dim3((unsigned)((a.T + 255) / 256), (unsigned)((nv8 + 7) / 8)), block, 0, (hipStream_t)stream, a);
            UMV_LAUNCH_CHECK();
            return UMV_OK;
        }
        // (sending the V heads of a long prefill through the tile kernel and only q / k through this one was measured on the
        // flow passes, T = 2064: 20.4 + 11.4 us against 24.8 us in one kernel - the per-(token, head) wave with 2-byte
        // accesses is the cost here, not the V scatter)
        if (a.hd == 128) hipLaunchKernelGGL((qkv_post_kernel<128>), grid, block, 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((qkv_post_kernel<72>), grid, block, 0, (hipStream_t)stream, a);
    }
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
