// Image-head kernels: CFG combine + renorm + Euler step, and the timestep sinusoid.
#include "block_reduce.h"
#include "../../include/unimedvl_hip.h"

// ----------------------------------------------------------------------------- CFG + renorm + Euler
// bagel.py:1173-1207 and :983, with every intermediate rounded to bf16 where the reference
// holds a bf16 tensor (v_t and friends are bf16; x_t is fp32):
//   v_text_ = v_c + s_t*(v_t - v_c) ; v_ = v_i + s_i*(v_text_ - v_i)
//   scale = clamp(norm(v_t)/(norm(v_)+1e-8), min, 1) ; v = v_*scale ; x_t -= v*dt
// One workgroup per sample ("global" norms are per sample; the reference is batch-1 here).
__device__ __forceinline__ float cfg_mix(float v, float vc, float s) {
    // vc + s*(v - vc) with bf16 rounding after each op
    return rbf(vc + rbf(s * rbf(v - vc)));
}
// the guided velocity at offset `off` of the velocity buffers: text guidance of v, then (img) image guidance of that
__device__ __forceinline__ float guided(float v, int64_t off, const bf16_t* __restrict__ v_text, const bf16_t* __restrict__ v_img,
                                        float s_text, float s_img, bool img) {
    const float vm = cfg_mix(v, bf2f(v_text[off]), s_text);
    return img ? cfg_mix(vm, bf2f(v_img[off]), s_img) : vm;
}
// clamp(norm(v_t) / (norm(v_) + 1e-8), min, 1) from the two sums of squares
__device__ __forceinline__ float renorm_scale(float a0, float a1, float rmin) {
    const float nv = rbf(sqrtf(a0)), nm = rbf(sqrtf(a1));
    return fminf(fmaxf(rbf(nv / rbf(nm + 1e-8f)), rmin), 1.0f);
}

__global__ __launch_bounds__(1024) void cfg_renorm_euler_kernel(float* __restrict__ x_t, const bf16_t* __restrict__ v_t,
                                                                const bf16_t* __restrict__ v_text, const bf16_t* __restrict__ v_img,
                                                                int64_t ldv, const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ seg_off, float s_text, float s_img,
                                                                float renorm_min, int rtype, float dt, int D) {
    __shared__ float sm[16];
    const int s = blockIdx.x;
    const int n0 = seg_off[s], n1 = seg_off[s + 1];
    const int total = (n1 - n0) * D;
    const bool use_text = s_text > 1.0f, use_img = s_img > 1.0f;
    const float rmin = rbf(renorm_min);
    if (!use_text) {  // no guidance: v = v_t
        for (int i = threadIdx.x; i < total; i += blockDim.x) {
            int n = n0 + i / D, d = i % D;
            float v = bf2f(v_t[(int64_t)rows[n] * ldv + d]);
            x_t[(int64_t)n * D + d] -= rbf(v * dt);
        }
        return;
    }
    if (rtype == 0) {  // global: one scale per sample
        float a0 = 0.f, a1 = 0.f;
        for (int i = threadIdx.x; i < total; i += blockDim.x) {
            int n = n0 + i / D, d = i % D;
            int64_t off = (int64_t)rows[n] * ldv + d;
            float v = bf2f(v_t[off]);
            float vm = guided(v, off, v_text, v_img, s_text, s_img, use_img);
            a0 += v * v;
            a1 += vm * vm;
        }
        a0 = block_reduce_sum(a0, sm);
        a1 = block_reduce_sum(a1, sm);
        const float scale = renorm_scale(a0, a1, rmin);
        for (int i = threadIdx.x; i < total; i += blockDim.x) {
            int n = n0 + i / D, d = i % D;
            int64_t off = (int64_t)rows[n] * ldv + d;
            float vm = guided(bf2f(v_t[off]), off, v_text, v_img, s_text, s_img, use_img);
            x_t[(int64_t)n * D + d] -= rbf(rbf(vm * scale) * dt);
        }
        return;
    }
    // per-token norms: one wave per token (D <= 64*? handled by looping).  channel (1): the scale is the guided velocity's;
    // text_channel (2): renorm the text-guided velocity, then image guidance
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const bool img_first = rtype == 1 && use_img, img_last = rtype == 2 && use_img;
    for (int n = n0 + wave; n < n1; n += nwaves) {
        const int64_t base = (int64_t)rows[n] * ldv;
        float a0 = 0.f, a1 = 0.f;
        for (int d = lane; d < D; d += 64) {
            float v = bf2f(v_t[base + d]);
            float vm = guided(v, base + d, v_text, v_img, s_text, s_img, img_first);
            a0 += v * v;
            a1 += vm * vm;
        }
        const float scale = renorm_scale(wave_sum(a0), wave_sum(a1), rmin);
        for (int d = lane; d < D; d += 64) {
            float vm = guided(bf2f(v_t[base + d]), base + d, v_text, v_img, s_text, s_img, img_first);
            float out = rbf(vm * scale);
            if (img_last) out = cfg_mix(out, bf2f(v_img[base + d]), s_img);
            x_t[(int64_t)n * D + d] -= rbf(out * dt);
        }
    }
}

// ----------------------------------------------------------------------------- timestep sinusoid
// TimestepEmbedder.timestep_embedding (modeling_utils.py:87-109): args = t[:, None] * freqs[None] in fp32,
// emb = cat(cos(args), sin(args)) cast to bf16 by autocast in front of mlp[0].  `freqs` = exp(-ln(10000) * i / half) comes from
// the caller (computed once with torch, so t * freqs has the reference's bits); cos / sin are the full-range libm versions.
__global__ void timestep_embed_kernel(const float* __restrict__ t, const float* __restrict__ freqs, bf16_t* __restrict__ out, int n, int half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * half) return;
    const int row = i / half, j = i - row * half;
    const float a = t[row] * freqs[j];
    float sn, cs;
    sincosf(a, &sn, &cs);
    out[(int64_t)row * 2 * half + j] = f2bf(cs);
    out[(int64_t)row * 2 * half + half + j] = f2bf(sn);
}
extern "C" int umv_timestep_embed(const float* t, const float* freqs, uint16_t* out, int n, int half, umv_stream_t stream) {
    UMV_CHECK(t && freqs && out && n >= 0 && half > 0, UMV_ERR_ARG, "timestep_embed: bad args");
    if (n == 0) return UMV_OK;
    hipLaunchKernelGGL(timestep_embed_kernel, dim3((n * half + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, freqs, out, n, half);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

extern "C" int umv_cfg_renorm_euler(float* x_t, const uint16_t* v_t, const uint16_t* v_text, const uint16_t* v_img, int64_t ldv,
                                    const int32_t* rows, const int32_t* seg_off, int nseg, float cfg_text_scale,
                                    float cfg_img_scale, float renorm_min, int renorm_type, float dt, int D,
                                    umv_stream_t stream) {
    UMV_CHECK(x_t && v_t && rows && seg_off, UMV_ERR_ARG, "cfg_renorm_euler: null pointer");
    UMV_CHECK(renorm_type >= 0 && renorm_type <= 2, UMV_ERR_ARG, "cfg_renorm_euler: renorm_type %d", renorm_type);
    UMV_CHECK(!(cfg_text_scale > 1.0f) || v_text, UMV_ERR_ARG, "cfg_renorm_euler: cfg_text_scale>1 without v_text");
    UMV_CHECK(!(cfg_text_scale > 1.0f && cfg_img_scale > 1.0f) || v_img, UMV_ERR_ARG, "cfg_renorm_euler: cfg_img_scale>1 without v_img");
    if (nseg == 0) return UMV_OK;
    hipLaunchKernelGGL(cfg_renorm_euler_kernel, dim3(nseg), dim3(1024), 0, (hipStream_t)stream, x_t, v_t, v_text, v_img, ldv,
                       rows, seg_off, cfg_text_scale, cfg_img_scale, renorm_min, renorm_type, dt, D);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
