// VAE (FLUX autoencoder) kernels other than the convolutions (vae_conv.hip): GroupNorm(+swish), latent (un)patchify, sampling and
// pixel conversion, and the softmax / row scale between the two GEMMs of the mid-block attention.
#include "common.h"
#include "../../include/unimedvl_hip.h"

// ----------------------------------------------------------------------------- VAE: GroupNorm(32) (+ swish), NHWC
// F.group_norm on bf16 (autoencoder.py:75,77,166,237,43) then swish x*sigmoid(x) (:34-35): fp32
// statistics over (H*W, C/32) per (sample, group), one bf16 rounding of the normalised value,
// sigmoid rounded to bf16, product rounded to bf16.  Deterministic two-level reduction:
// pass 1 writes per-chunk partial sums, pass 2 folds them in a fixed order and applies.
#define GN_CHUNK 256   // pixels per partial-sum workgroup
// one pixel's channel octet into the running sums and sums of squares
__device__ __forceinline__ void gn_acc8(const bf16_t* p, float (&s)[8], float (&q)[8]) {
    const bf16x8 v = ldg_frag(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = bf2f((bf16_t)v[j]); s[j] += f; q[j] += f * f; }
}
__global__ __launch_bounds__(256) void gn_partial_kernel(const bf16_t* __restrict__ x, float* __restrict__ part, int HW, int C,
                                                         int nchunks) {
    // grid (nchunks, B); thread t owns channel octets t, t+256, ... ; cpg = C/32 channels per group
    extern __shared__ float sm[];   // [2][C]
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int p0 = chunk * GN_CHUNK, p1 = min(HW, p0 + GN_CHUNK);
    const int nv = C / 8;
    for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) sm[c] = 0.f;
    __syncthreads();
    // each thread walks (pixel, octet) pairs with a fixed assignment -> deterministic
    const int per_row = nv;
    const int lanes = blockDim.x;
    // thread handles octet (tid % per_row) when per_row <= lanes, striding pixels by lanes/per_row
    if (per_row <= lanes) {
        const int oct = threadIdx.x % per_row, prow = threadIdx.x / per_row, pstride = lanes / per_row;
        float s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (prow < pstride) {
            for (int p = p0 + prow; p < p1; p += pstride) gn_acc8(x + ((int64_t)b * HW + p) * C + oct * 8, s, q);
        }
        // fold pixel-rows in a fixed order through LDS
        for (int pr = 0; pr < pstride; ++pr) {
            if (prow == pr) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { sm[oct * 8 + j] += s[j]; sm[C + oct * 8 + j] += q[j]; }
            }
            __syncthreads();
        }
    } else {
        for (int oct = threadIdx.x; oct < per_row; oct += lanes) {
            float s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int p = p0; p < p1; ++p) gn_acc8(x + ((int64_t)b * HW + p) * C + oct * 8, s, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) { sm[oct * 8 + j] = s[j]; sm[C + oct * 8 + j] = q[j]; }
        }
        __syncthreads();
    }
    // per-group sums for this chunk
    const int cpg = C / 32;
    if (threadIdx.x < 32) {
        float s = 0.f, q = 0.f;
        for (int c = 0; c < cpg; ++c) { s += sm[threadIdx.x * cpg + c]; q += sm[C + threadIdx.x * cpg + c]; }
        float* dst = part + (((int64_t)b * nchunks + chunk) * 32 + threadIdx.x) * 2;
        dst[0] = s; dst[1] = q;
    }
}

// Fold the per-chunk partial sums into (mean, rstd) per (sample, group), ONCE per call: 8 lanes per group take contiguous chunk
// ranges (all loads of a lane independent, summed in chunk order), the 8 range sums are added in lane order - a fixed order, so
// the statistics do not depend on the launch geometry.  (Every workgroup of gn_apply used to repeat a serial walk over all
// chunks - 256 dependent L2 round trips at 256 x 256 - before touching a pixel: 193 us for a 134 MB pass.)
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* __restrict__ part, float* __restrict__ stats, int nchunks,
                                                          float n_per_group, float eps) {
    __shared__ float ps[32][8], pq[32][8];
    const int b = blockIdx.x;
    const int grp = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int per = (nchunks + 7) / 8;
    const int c0 = sub * per, c1 = min(nchunks, c0 + per);
    float s = 0.f, q = 0.f;
    int ch = c0;
    for (; ch + 4 <= c1; ch += 4) {
        const float* p = part + (((int64_t)b * nchunks + ch) * 32 + grp) * 2;
        const float a0 = p[0], b0 = p[1], a1 = p[64], b1 = p[65], a2 = p[128], b2 = p[129], a3 = p[192], b3 = p[193];
        s += a0; q += b0; s += a1; q += b1; s += a2; q += b2; s += a3; q += b3;
    }
    for (; ch < c1; ++ch) {
        const float* p = part + (((int64_t)b * nchunks + ch) * 32 + grp) * 2;
        s += p[0]; q += p[1];
    }
    ps[grp][sub] = s; pq[grp][sub] = q;
    __syncthreads();
    if (sub == 0) {
        float S = 0.f, Q = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { S += ps[grp][i]; Q += pq[grp][i]; }
        const float mean = S / n_per_group;
        const float var = fmaxf(Q / n_per_group - mean * mean, 0.f);
        stats[((int64_t)b * 32 + grp) * 2] = mean;
        stats[((int64_t)b * 32 + grp) * 2 + 1] = rsqrt_ieee(var + eps);
    }
}

// y = bf16((x - mean) * rstd * gamma + beta), then swish with the reference's roundings (sigmoid -> bf16, product -> bf16).  A thread
// keeps ONE channel octet for its whole grid-stride walk (the stride is a multiple of C / 8), so its gamma / beta / statistics
// live in registers; sigmoid on v_exp_f32 / v_rcp_f32.
__global__ __launch_bounds__(256) void gn_apply_kernel(const bf16_t* __restrict__ x, const float* __restrict__ stats,
                                                       const bf16_t* __restrict__ gamma, const bf16_t* __restrict__ beta,
                                                       bf16_t* __restrict__ out, int HW, int C, int swish) {
    const int b = blockIdx.y;
    const int cpg = C / 32;
    const int nv = C / 8;
    const int64_t total = (int64_t)HW * nv;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;        // a multiple of nv (host side)
    const int oct = (int)(i0 % nv);
    const bf16x8 gm = ldg_frag(gamma + oct * 8), bt = ldg_frag(beta + oct * 8);
    float mean[8], rstd[8], gw[8], bw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int grp = (oct * 8 + j) / cpg;
        mean[j] = stats[((int64_t)b * 32 + grp) * 2];
        rstd[j] = stats[((int64_t)b * 32 + grp) * 2 + 1];
        gw[j] = bf2f((bf16_t)gm[j]);
        bw[j] = bf2f((bf16_t)bt[j]);
    }
    const bf16_t* xb = x + (int64_t)b * HW * C;
    bf16_t* ob = out + (int64_t)b * HW * C;
    for (int64_t i = i0; i < total; i += stride) {
        const int64_t off = i * 8;                                   // (pixel * nv + oct) * 8
        const bf16x8 v = ldg_frag(xb + off);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float y = rbf((bf2f((bf16_t)v[j]) - mean[j]) * rstd[j] * gw[j] + bw[j]);
            if (swish) {
                // torch.sigmoid on the bf16 tensor, then the bf16 product.  v_exp_f32 / v_rcp_f32 give the same bf16 sigmoid as torch for
                // EVERY bf16 y > -87.5 (tests/test_vae_gpu.py::test_groupnorm_swish_every_bf16_value walks all 65280 finite values);
                // below that e^-y leaves the range the hardware units keep (denormal results flush), so those few values take IEEE
                // division and libm's expf - y -> -0 once the sigmoid underflows, as in the reference.
                float sg = rbf(__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fminf(-y * 1.4426950408889634f, 126.0f))));
                if (y < -87.0f) sg = rbf(__fdiv_rn(1.0f, 1.0f + expf(-y)));
                y = rbf(y * sg);
            }
            o[j] = (short)f2bf(y);
        }
        *reinterpret_cast<bf16x8*>(ob + off) = o;
    }
}

extern "C" size_t umv_groupnorm_workspace_bytes(int B, int HW) {
    return (size_t)B * ((HW + GN_CHUNK - 1) / GN_CHUNK) * 32 * 2 * sizeof(float) + (size_t)B * 32 * 2 * sizeof(float);   // partials + (mean, rstd)
}

extern "C" int umv_groupnorm_nhwc_bf16(const uint16_t* x, const uint16_t* gamma, const uint16_t* beta, uint16_t* out, void* workspace,
                                       int B, int HW, int C, float eps, int swish, umv_stream_t stream) {
    UMV_CHECK(x && gamma && beta && out && workspace, UMV_ERR_ARG, "groupnorm: null pointer");
    UMV_CHECK(C % 32 == 0, UMV_ERR_ARG, "groupnorm: C=%d must be a multiple of 32", C);
    if (B == 0 || HW == 0) return UMV_OK;
    const int nchunks = (HW + GN_CHUNK - 1) / GN_CHUNK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_partial_kernel, dim3(nchunks, B), dim3(256), 2 * C * sizeof(float), s, x, (float*)workspace, HW, C, nchunks);
    UMV_LAUNCH_CHECK();
    float* stats = (float*)workspace + (size_t)B * nchunks * 32 * 2;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(256), 0, s, (const float*)workspace, stats, nchunks, (float)HW * (float)(C / 32), eps);
    UMV_LAUNCH_CHECK();
    const int nv = C / 8;                                            // 256 * blocks is a multiple of nv for every C = 32 * 2^k <= 2048;
    int blocks = (int)min((int64_t)2048, ((int64_t)HW * nv + 255) / 256);   // other widths: round the grid up to a multiple of nv
    if ((256 * blocks) % nv != 0) blocks = ((blocks + nv - 1) / nv) * nv;
    hipLaunchKernelGGL(gn_apply_kernel, dim3(blocks, B), dim3(256), 0, s, x, (const float*)stats, gamma, beta, out, HW, C, swish);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- VAE: layout / boundary kernels
// image [B,3,H,W] fp32 NCHW -> NHWC bf16 with channels zero padded to Cp (autocast's cast before conv_in)
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int B, int C, int H, int W, int Cp) {
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = (int64_t)B * H * W * Cp;
    if (gid >= total) return;
    int c = (int)(gid % Cp);
    int64_t p = gid / Cp;
    int xw = (int)(p % W);
    int y = (int)((p / W) % H);
    int b = (int)(p / ((int64_t)W * H));
    out[gid] = c < C ? f2bf(x[(((int64_t)b * C + c) * H + y) * W + xw]) : (bf16_t)0;
}
extern "C" int umv_nchw_f32_to_nhwc_bf16(const float* x, uint16_t* out, int B, int C, int H, int W, int Cp, umv_stream_t stream) {
    UMV_CHECK(x && out && Cp >= C, UMV_ERR_ARG, "nchw_to_nhwc: bad args");
    int64_t total = (int64_t)B * H * W * Cp;
    if (total == 0) return UMV_OK;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, B, C, H, W, Cp);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// latent tokens [h*w, p*p*c] fp32 (the flow's x_t) -> NHWC bf16 [1, h*p, w*p, c] with z/scale + shift
// (inferencer.py:239-241 "nhwpqc->nchpwq" and autoencoder.py:306), bf16 rounding per op: bf16(bf16(bf16(tok) / scale) + shift).
// scale and shift are fp32 constants, as torch hands a Python scalar to a device kernel.  torch on the CPU rounds the scalar of
// `bf16_tensor + scalar` to bf16 first (0.1159 -> 0.11572265625), so the CPU oracle and its goldens differ from this kernel by at
// most one bf16 ulp at the addition (DESIGN.md "The VAE's shift constant"; tests/test_vae_ref_cpu.py, tests/test_vae_boundary_gpu.py).
__global__ void unpatchify_latent_kernel(const float* __restrict__ tok, bf16_t* __restrict__ out, int h, int w, int p, int c,
                                         float scale, float shift) {
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = (int64_t)h * p * w * p * c;
    if (gid >= total) return;
    int ch = (int)(gid % c);
    int64_t pix = gid / c;
    int X = (int)(pix % (w * p)), Y = (int)(pix / (w * p));
    int hy = Y / p, py = Y % p, wx = X / p, px = X % p;
    float v = rbf(tok[((int64_t)hy * w + wx) * (p * p * c) + (py * p + px) * c + ch]);   // latent.to(bf16)
    v = rbf(rbf(v / scale) + shift);
    out[gid] = f2bf(v);
}
extern "C" int umv_unpatchify_latent(const float* tokens, uint16_t* out, int h, int w, int p, int c, float scale, float shift,
                                     umv_stream_t stream) {
    UMV_CHECK(tokens && out, UMV_ERR_ARG, "unpatchify_latent: null pointer");
    int64_t total = (int64_t)h * p * w * p * c;
    if (total == 0) return UMV_OK;
    hipLaunchKernelGGL(unpatchify_latent_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tokens, out,
                       h, w, p, c, scale, shift);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// decoder output NHWC bf16 [H,W,Cs] (first 3 channels) -> uint8 [H,W,3]:
// ((x*0.5+0.5).clamp(0,1))*255 in bf16, truncating cast (inferencer.py:253-254)
__global__ void pixels_u8_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ out, int64_t npix, int Cs) {
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= npix * 3) return;
    int c = (int)(gid % 3);
    int64_t p = gid / 3;
    float v = bf2f(x[p * Cs + c]);
    v = rbf(rbf(v * 0.5f) + 0.5f);
    v = fminf(fmaxf(v, 0.f), 1.f);
    v = rbf(v * 255.0f);
    out[gid] = (uint8_t)v;
}
extern "C" int umv_pixels_to_u8(const uint16_t* x, uint8_t* out, int64_t npix, int Cs, umv_stream_t stream) {
    UMV_CHECK(x && out && Cs >= 3, UMV_ERR_ARG, "pixels_to_u8: bad args");
    if (npix == 0) return UMV_OK;
    hipLaunchKernelGGL(pixels_u8_kernel, dim3((unsigned)((npix * 3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, npix, Cs);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// encoder tail: moments NHWC bf16 [B,Hm,Wm,2z] -> z = mean + exp(0.5*logvar)*noise ; scale*(z - shift)
// (autoencoder.py:266-272,300-303) then 2x2 patchify "chpwq->hwpqc" of the top-left h*p x w*p window
// (bagel.py:771-775) -> tokens bf16 [h*w, p*p*z].  noise is NCHW bf16 [B,z,Hm,Wm] as torch.randn_like draws it.
// bf16(scale * bf16(bf16(mean + bf16(bf16(exp(bf16(0.5 * logvar))) * noise)) - shift)) with fp32 scale and shift, as torch computes
// them on a device; the CPU oracle subtracts the shift rounded to bf16 and differs by at most one bf16 ulp of that step (see
// unpatchify_latent_kernel).
__global__ void latent_sample_patchify_kernel(const bf16_t* __restrict__ mom, const bf16_t* __restrict__ noise, bf16_t* __restrict__ tok,
                                              int b, int Hm, int Wm, int z, int h, int w, int p, float scale, float shift) {
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = (int64_t)h * w * p * p * z;
    if (gid >= total) return;
    int ch = (int)(gid % z);
    int64_t r = gid / z;
    int px = (int)(r % p); r /= p;
    int py = (int)(r % p); r /= p;
    int wx = (int)(r % w);
    int hy = (int)(r / w);
    int Y = hy * p + py, X = wx * p + px;
    const bf16_t* m = mom + (((int64_t)b * Hm + Y) * Wm + X) * (2 * z);
    float mean = bf2f(m[ch]), logvar = bf2f(m[z + ch]);
    float stdv = rbf(expf(rbf(0.5f * logvar)));
    float nz = bf2f(noise[(((int64_t)b * z + ch) * Hm + Y) * Wm + X]);
    float zz = rbf(mean + rbf(stdv * nz));
    zz = rbf(scale * rbf(zz - shift));
    tok[gid] = f2bf(zz);
}
extern "C" int umv_latent_sample_patchify(const uint16_t* moments, const uint16_t* noise, uint16_t* tokens, int b, int Hm, int Wm,
                                          int z, int h, int w, int p, float scale, float shift, umv_stream_t stream) {
    UMV_CHECK(moments && noise && tokens, UMV_ERR_ARG, "latent_sample_patchify: null pointer");
    UMV_CHECK(h * p <= Hm && w * p <= Wm, UMV_ERR_ARG, "latent_sample_patchify: window exceeds the latent");
    int64_t total = (int64_t)h * w * p * p * z;
    if (total == 0) return UMV_OK;
    hipLaunchKernelGGL(latent_sample_patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, moments,
                       noise, tokens, b, Hm, Wm, z, h, w, p, scale, shift);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- single-head attention of the VAE mid block as two GEMMs
// AttnBlock.attention (autoencoder.py:50-62) is ONE head of C = 512 channels over H*W positions: as S = Q K^T and O = P V those are
// ordinary GEMMs at the tiled kernel's rate (3136 x 3136 x 512 at 448 x 448), where the streaming attention kernel at hd 512 keeps
// 128 accumulator registers per lane and runs at 27 TFLOP/s (750 us of a 4.1 ms encode).  Between the GEMMs:
//   umv_softmax_rows_f32:   P[r][c] = bf16(exp((S[r][c] - max_c S[r][c]) * scale)), l[r] = sum_c of the unrounded weights
//   umv_rowscale_f32_bf16:  out[r][c] = bf16(O[r][c] / l[r])
// i.e. the flash-attention arithmetic (fp32 scores and sums, bf16 weights, one division at the end) with the row's true maximum.
template <int MAXI>             // 2 columns per thread and pass: n <= 2 * 256 * MAXI (16: 8192, 32: 16384 = a 1024 x 1024 image's latent)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* S, int64_t lds_, bf16_t* P, int64_t ldp, float* l, int n,
                                                           float scale_log2e) {
    __shared__ float red[8];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* s = S + (int64_t)r * lds_;
    float2 v[MAXI];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
        const int c = 2 * (tid + 256 * i);
        v[i] = c < n ? *reinterpret_cast<const float2*>(s + c) : make_float2(-INFINITY, -INFINITY);
        mx = fmaxf(mx, fmaxf(v[i].x, v[i].y));
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float mref = (mx == -INFINITY) ? 0.f : mx;
    float sum = 0.f;
    bf16_t* p = P + (int64_t)r * ldp;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
        const int c = 2 * (tid + 256 * i);
        if (c < n) {
            const float p0 = umv_exp2((v[i].x - mref) * scale_log2e), p1 = umv_exp2((v[i].y - mref) * scale_log2e);
            sum += p0;
            sum += p1;
            *reinterpret_cast<uint32_t*>(p + c) = pack2bf(p0, p1);
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    if (tid == 0) l[r] = (red[4] + red[5]) + (red[6] + red[7]);
}
extern "C" int umv_softmax_rows_f32(const float* S, int64_t ld_s, uint16_t* P, int64_t ld_p, float* l, int rows, int n, float scale,
                                    umv_stream_t stream) {
    UMV_CHECK(S && P && l, UMV_ERR_ARG, "softmax_rows: null pointer");
    UMV_CHECK(n > 0 && n <= 16384 && (n % 2) == 0 && (ld_s % 2) == 0 && (ld_p % 2) == 0 && ld_s >= n && ld_p >= n, UMV_ERR_UNSUPPORTED,
              "softmax_rows: n (%d) must be even and <= 16384, row strides even and >= n", n);
    if (rows <= 0) return UMV_OK;
    if (n <= 8192)
        hipLaunchKernelGGL(softmax_rows_kernel<16>, dim3(rows), dim3(256), 0, (hipStream_t)stream, S, ld_s, P, ld_p, l, n, scale * 1.4426950408889634f);
    else
        hipLaunchKernelGGL(softmax_rows_kernel<32>, dim3(rows), dim3(256), 0, (hipStream_t)stream, S, ld_s, P, ld_p, l, n, scale * 1.4426950408889634f);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

__global__ __launch_bounds__(256) void rowscale_kernel(const float* O, int64_t ldo_in, const float* l, bf16_t* out, int64_t ldo, int rows, int C) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cpr = C / 2;
    const int64_t r = gid / cpr;
    if (r >= rows) return;
    const int c = (int)(gid - r * cpr) * 2;
    const float lv = l[r];
    const float inv = lv > 0.f ? 1.0f / lv : 0.f;
    const float2 v = *reinterpret_cast<const float2*>(O + r * ldo_in + c);
    *reinterpret_cast<uint32_t*>(out + r * ldo + c) = pack2bf(v.x * inv, v.y * inv);
}
extern "C" int umv_rowscale_f32_bf16(const float* O, int64_t ld_in, const float* l, uint16_t* out, int64_t ld_out, int rows, int C,
                                     umv_stream_t stream) {
    UMV_CHECK(O && l && out, UMV_ERR_ARG, "rowscale: null pointer");
    UMV_CHECK(C > 0 && (C % 2) == 0 && (ld_in % 2) == 0 && (ld_out % 2) == 0, UMV_ERR_ARG, "rowscale: C and the row strides must be even");
    if (rows <= 0) return UMV_OK;
    const int64_t total = (int64_t)rows * (C / 2);
    hipLaunchKernelGGL(rowscale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, O, ld_in, l, out, ld_out, rows, C);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
