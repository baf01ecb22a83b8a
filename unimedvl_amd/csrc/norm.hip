// The norms: RMSNorm (prefill and decode forms), the split-K consumer residual + RMSNorm, LayerNorm.
// One wavefront or one workgroup per row; 16-byte bf16x8 accesses; IEEE 1/sqrt to match torch's bits.
#include "block_reduce.h"
#include "../../include/unimedvl_hip.h"

// ----------------------------------------------------------------------------- RMSNorm
// modeling_qwen2.py:89-94: h = x.float(); h = h * rsqrt(mean(h^2) + eps); out = w * h.to(bf16)
// 4 waves per block, one row per wave; row held in registers when H <= 64*8*MAXV.
template <int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                      const bf16_t* __restrict__ wg, const int32_t* __restrict__ expert,
                                                      bf16_t* __restrict__ out, int T, int H, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const bf16_t* xr = x + (int64_t)row * H;
    const bf16_t* wr = (expert && expert[row]) ? wg : w;
    bf16x8 v[MAXV];
    float ss = 0.f;
    const int nv = H / 8;  // H % 8 == 0
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = i * 64 + lane;
        if (c < nv) {
            v[i] = ldg_frag(xr + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float f = bf2f((bf16_t)v[i][j]);
                ss += f * f;
            }
        }
    }
    ss = wave_sum(ss);
    const float rstd = rsqrt_ieee(ss / (float)H + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = i * 64 + lane;
        if (c < nv) {
            bf16x8 ww = ldg_frag(wr + c * 8);
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float h = rbf(bf2f((bf16_t)v[i][j]) * rstd);
                o[j] = (short)f2bf(bf2f((bf16_t)ww[j]) * h);
            }
            *reinterpret_cast<bf16x8*>(out + (int64_t)row * H + c * 8) = o;
        }
    }
}

// The tail the two decode norms below share (test_residual_rmsnorm holds them bit-equal): a 256-thread workgroup owns the row,
// thread t holds chunks i * 256 + t of x (v) and of the weight (ww), ss is its sum of squares.  rstd from the four-wave sum,
// then out = w * bf16(v * rstd).
template <int MAXV>
__device__ __forceinline__ void rowblock_norm_store(float ss, const bf16x8 (&v)[MAXV], const bf16x8 (&ww)[MAXV], bf16_t* __restrict__ out_row,
                                                    int H, float eps) {
    __shared__ float part[4];
    const float rstd = rsqrt_ieee(four_wave_sum(ss, part) / (float)H + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = i * 256 + threadIdx.x;
        if (c < H / 8) {
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(bf2f((bf16_t)ww[i][j]) * rbf(bf2f((bf16_t)v[i][j]) * rstd));
            *reinterpret_cast<bf16x8*>(out_row + c * 8) = o;
        }
    }
}

// Few rows (decode): latency bound, so one 256-thread workgroup per row with the x AND weight
// loads issued together up front (one memory round trip) and a single LDS exchange.
template <int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_rowblock_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                               const bf16_t* __restrict__ wg, const int32_t* __restrict__ expert,
                                                               bf16_t* __restrict__ out, int H, float eps) {
    const int row = blockIdx.x;
    const bf16_t* xr = x + (int64_t)row * H;
    const bf16_t* wr = (expert && expert[row]) ? wg : w;
    const int nv = H / 8;
    bf16x8 v[MAXV], ww[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = i * 256 + threadIdx.x;
        v[i] = c < nv ? ldg_frag(xr + c * 8) : zero_frag();
        ww[i] = c < nv ? ldg_frag(wr + c * 8) : zero_frag();
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = bf2f((bf16_t)v[i][j]);
            ss += f * f;
        }
    rowblock_norm_store<MAXV>(ss, v, ww, out + (int64_t)row * H, H, eps);
}

extern "C" int umv_rmsnorm_bf16(const uint16_t* x, const uint16_t* w, const uint16_t* w_gen, const int32_t* expert,
                                uint16_t* out, int T, int H, float eps, umv_stream_t stream) {
    UMV_CHECK(x && w && out, UMV_ERR_ARG, "rmsnorm: null pointer");
    UMV_CHECK(H % 8 == 0 && H <= 64 * 8 * 16, UMV_ERR_ARG, "rmsnorm: H=%d unsupported", H);
    UMV_CHECK(!expert || w_gen, UMV_ERR_ARG, "rmsnorm: expert routing without w_gen");
    if (T == 0) return UMV_OK;
    hipStream_t s = (hipStream_t)stream;
    if (T <= 64 && H >= 1024) {
        if (H <= 256 * 8 * 2)
            hipLaunchKernelGGL((rmsnorm_rowblock_kernel<2>), dim3(T), dim3(256), 0, s, x, w, w_gen, expert, out, H, eps);
        else
            hipLaunchKernelGGL((rmsnorm_rowblock_kernel<4>), dim3(T), dim3(256), 0, s, x, w, w_gen, expert, out, H, eps);
        UMV_LAUNCH_CHECK();
        return UMV_OK;
    }
    dim3 grid((T + 3) / 4), block(256);
    if (H <= 512 * 2)
        hipLaunchKernelGGL((rmsnorm_kernel<2>), grid, block, 0, s, x, w, w_gen, expert, out, T, H, eps);
    else if (H <= 512 * 8)
        hipLaunchKernelGGL((rmsnorm_kernel<8>), grid, block, 0, s, x, w, w_gen, expert, out, T, H, eps);
    else
        hipLaunchKernelGGL((rmsnorm_kernel<16>), grid, block, 0, s, x, w, w_gen, expert, out, T, H, eps);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// Consumer of a split-K decode GEMM (umv_gemm_args.k_splits): finishes o_proj / down_proj and runs the next RMSNorm in
// one launch.   seq[t,:] = bf16( bf16(sum_s P[s][t,:]) + seq[t,:] )   (the GEMM output rounding, then the residual add:
// qwen2_navit.py:873-874,897-898), splits added in order 0..S-1;   out[t,:] = w * bf16(seq * rstd)   (modeling_qwen2.py:89-94)
// NS > 0: that many splits, known at compile time so that all their loads are requested before the first add (a run-time
// loop costs one L2 round trip per split on this latency-bound kernel); NS = 0: S of them at run time.
template <int MAXV, int NS>
__global__ __launch_bounds__(256) void residual_rmsnorm_kernel(const float* __restrict__ P, int S, int64_t sstride, int64_t ldp,
                                                               bf16_t* __restrict__ seq, const bf16_t* __restrict__ w,
                                                               bf16_t* __restrict__ out, int H, float eps) {
    const int row = blockIdx.x;
    const int nv = H / 8;
    bf16x8 v[MAXV], ww[MAXV];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = i * 256 + threadIdx.x;
        v[i] = zero_frag();
        ww[i] = zero_frag();
        if (c < nv) {
            const bf16x8 res = ldg_frag(seq + (int64_t)row * H + c * 8);
            ww[i] = ldg_frag(w + c * 8);
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const float* p = P + (int64_t)row * ldp + c * 8;
            if constexpr (NS > 0) {
                f32x4 a0[NS], a1[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    a0[s] = *reinterpret_cast<const f32x4*>(p + s * sstride);
                    a1[s] = *reinterpret_cast<const f32x4*>(p + s * sstride + 4);
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    acc[0] += a0[s].x; acc[1] += a0[s].y; acc[2] += a0[s].z; acc[3] += a0[s].w;
                    acc[4] += a1[s].x; acc[5] += a1[s].y; acc[6] += a1[s].z; acc[7] += a1[s].w;
                }
            } else
            for (int s = 0; s < S; ++s) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(p + s * sstride);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(p + s * sstride + 4);
                acc[0] += a0.x; acc[1] += a0.y; acc[2] += a0.z; acc[3] += a0.w;
                acc[4] += a1.x; acc[5] += a1.y; acc[6] += a1.z; acc[7] += a1.w;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float f = rbf(rbf(acc[j]) + bf2f((bf16_t)res[j]));
                v[i][j] = (short)f2bf(f);
                ss += f * f;
            }
            *reinterpret_cast<bf16x8*>(seq + (int64_t)row * H + c * 8) = v[i];
        }
    }
    rowblock_norm_store<MAXV>(ss, v, ww, out + (int64_t)row * H, H, eps);
}

extern "C" int umv_residual_rmsnorm_bf16(const float* partials, int n_splits, int64_t split_stride, int64_t ldp, uint16_t* seq,
                                         const uint16_t* w, uint16_t* out, int T, int H, float eps, umv_stream_t stream) {
    UMV_CHECK(partials && seq && w && out, UMV_ERR_ARG, "residual_rmsnorm: null pointer");
    UMV_CHECK(n_splits >= 1 && n_splits <= 64 && split_stride >= 0 && ldp >= H, UMV_ERR_ARG, "residual_rmsnorm: bad split layout");
    UMV_CHECK(H % 8 == 0 && H <= 256 * 8 * 4 && (ldp % 4) == 0 && (split_stride % 4) == 0, UMV_ERR_ARG,
              "residual_rmsnorm: H=%d (multiple of 8, <= 8192) / ldp / split_stride (multiples of 4) unsupported", H);
    if (T == 0) return UMV_OK;
    hipStream_t s = (hipStream_t)stream;
#define UMV_RRN_LAUNCH(MAXV, NS) \
    hipLaunchKernelGGL((residual_rmsnorm_kernel<MAXV, NS>), dim3(T), dim3(256), 0, s, partials, n_splits, split_stride, ldp, seq, w, out, H, eps)
    if (H <= 256 * 8 * 2) {
        switch (n_splits) {
            case 2: UMV_RRN_LAUNCH(2, 2); break;
            case 3: UMV_RRN_LAUNCH(2, 3); break;
            case 4: UMV_RRN_LAUNCH(2, 4); break;
            case 6: UMV_RRN_LAUNCH(2, 6); break;      // (65..128 samples: 6 / 8 / 8 splits)
            case 8: UMV_RRN_LAUNCH(2, 8); break;
            default: UMV_RRN_LAUNCH(2, 0); break;
        }
    } else {
        UMV_RRN_LAUNCH(4, 0);
    }
#undef UMV_RRN_LAUNCH
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- LayerNorm
// F.layer_norm on bf16 (siglip_navit.py:283,296,370): fp32 statistics, one rounding to bf16.
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                        const bf16_t* __restrict__ b, bf16_t* __restrict__ out, int T, int H,
                                                        float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const bf16_t* xr = x + (int64_t)row * H;
    bf16x8 v[MAXV];
    float s = 0.f;
    const int nv = H / 8;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = i * 64 + lane;
        if (c < nv) {
            v[i] = ldg_frag(xr + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += bf2f((bf16_t)v[i][j]);
        }
    }
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = i * 64 + lane;
        if (c < nv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = bf2f((bf16_t)v[i][j]) - mean;
                q += d * d;
            }
        }
    }
    const float rstd = rsqrt_ieee(wave_sum(q) / (float)H + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = i * 64 + lane;
        if (c < nv) {
            bf16x8 ww = ldg_frag(w + c * 8), bb = ldg_frag(b + c * 8), o;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                o[j] = (short)f2bf((bf2f((bf16_t)v[i][j]) - mean) * rstd * bf2f((bf16_t)ww[j]) + bf2f((bf16_t)bb[j]));
            *reinterpret_cast<bf16x8*>(out + (int64_t)row * H + c * 8) = o;
        }
    }
}

extern "C" int umv_layernorm_bf16(const uint16_t* x, const uint16_t* w, const uint16_t* b, uint16_t* out, int T, int H,
                                  float eps, umv_stream_t stream) {
    UMV_CHECK(x && w && b && out, UMV_ERR_ARG, "layernorm: null pointer");
    UMV_CHECK(H % 8 == 0 && H <= 64 * 8 * 8, UMV_ERR_ARG, "layernorm: H=%d unsupported", H);
    if (T == 0) return UMV_OK;
    dim3 grid((T + 3) / 4), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (H <= 512 * 3)
        hipLaunchKernelGGL((layernorm_kernel<3>), grid, block, 0, s, x, w, b, out, T, H, eps);
    else
        hipLaunchKernelGGL((layernorm_kernel<8>), grid, block, 0, s, x, w, b, out, T, H, eps);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
