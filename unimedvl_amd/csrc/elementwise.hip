// HBM-bound row kernels: embedding gather, row adds, the fp32 -> bf16 cast and patchify in front of the patch embedding.
// One wavefront per row; 16-byte bf16x8 accesses.
#include "common.h"
#include "../../include/unimedvl_hip.h"

// ----------------------------------------------------------------------------- embedding gather / add rows
__global__ __launch_bounds__(256) void embed_gather_kernel(const bf16_t* __restrict__ table, const int64_t* __restrict__ ids,
                                                           const int32_t* __restrict__ out_rows, bf16_t* __restrict__ out, int T,
                                                           int H) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const bf16_t* src = table + ids[t] * (int64_t)H;
    bf16_t* dst = out + (int64_t)(out_rows ? out_rows[t] : t) * H;
    for (int c = lane; c < H / 8; c += 64) *reinterpret_cast<bf16x8*>(dst + c * 8) = ldg_frag(src + c * 8);
}

extern "C" int umv_embed_gather_bf16(const uint16_t* table, const int64_t* ids, const int32_t* out_rows, uint16_t* out, int T,
                                     int H, umv_stream_t stream) {
    UMV_CHECK(table && ids && out && H % 8 == 0, UMV_ERR_ARG, "embed_gather: bad args");
    if (T == 0) return UMV_OK;
    hipLaunchKernelGGL(embed_gather_kernel, dim3((T + 3) / 4), dim3(256), 0, (hipStream_t)stream, table, ids, out_rows, out, T, H);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

__global__ __launch_bounds__(256) void add_rows_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ bcast,
                                                       const bf16_t* __restrict__ table, const int64_t* __restrict__ idx,
                                                       const int32_t* __restrict__ out_rows, bf16_t* __restrict__ out, int T, int H) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const bf16_t* ar = a + (int64_t)t * H;
    const bf16_t* tr = table ? table + idx[t] * (int64_t)H : nullptr;
    bf16_t* dst = out + (int64_t)(out_rows ? out_rows[t] : t) * H;
    for (int c = lane; c < H / 8; c += 64) {
        bf16x8 va = ldg_frag(ar + c * 8), o;
        bf16x8 vb = bcast ? ldg_frag(bcast + c * 8) : zero_frag();
        bf16x8 vt = tr ? ldg_frag(tr + c * 8) : zero_frag();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float f = bf2f((bf16_t)va[j]);
            if (bcast) f = rbf(f + bf2f((bf16_t)vb[j]));
            if (tr) f = rbf(f + bf2f((bf16_t)vt[j]));
            o[j] = (short)f2bf(f);
        }
        *reinterpret_cast<bf16x8*>(dst + c * 8) = o;
    }
}

extern "C" int umv_add_rows_bf16(const uint16_t* a, const uint16_t* bcast, const uint16_t* table, const int64_t* idx,
                                 const int32_t* out_rows, uint16_t* out, int T, int H, umv_stream_t stream) {
    UMV_CHECK(a && out && H % 8 == 0, UMV_ERR_ARG, "add_rows: bad args");
    UMV_CHECK(!table || idx, UMV_ERR_ARG, "add_rows: table without idx");
    if (T == 0) return UMV_OK;
    hipLaunchKernelGGL(add_rows_kernel, dim3((T + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, bcast, table, idx, out_rows, out, T, H);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- fp32 -> bf16 with zero padding
__global__ void cast_pad_kernel(const float* __restrict__ x, int64_t ldx, bf16_t* __restrict__ out, int64_t ldo, int T, int K, int Kp) {
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)T * Kp) return;
    int t = (int)(gid / Kp), k = (int)(gid % Kp);
    out[(int64_t)t * ldo + k] = k < K ? f2bf(x[(int64_t)t * ldx + k]) : (bf16_t)0;
}
extern "C" int umv_cast_pad_f32_bf16(const float* x, int64_t ldx, uint16_t* out, int64_t ldo, int T, int K, int Kp,
                                     umv_stream_t stream) {
    UMV_CHECK(x && out && Kp >= K, UMV_ERR_ARG, "cast_pad: bad args");
    if (T == 0) return UMV_OK;
    int64_t total = (int64_t)T * Kp;
    hipLaunchKernelGGL(cast_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, out, ldo, T, K, Kp);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}

// ----------------------------------------------------------------------------- patchify on the device
// patchify() of data_utils.py:43-50 + the fp32 -> bf16 cast autocast applies in front of the patch-embed linear (siglip_navit.py:190),
// from the transformed [C, H, W] fp32 image: token (ph, pw), column (pp * p + qq) * C + c  =  image[c][ph * p + pp][pw * p + qq], columns
// K = p * p * C .. Kp - 1 zero.  One workgroup per token; the host-side permute of the reference costs 4 ms per 448 x 448 image.
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, int C, int H, int W, int p, bf16_t* __restrict__ out, int64_t ldo,
                                                       int Kp) {
    const int nw = W / p;
    const int tok = blockIdx.x, ph = tok / nw, pw = tok % nw;
    const int K = p * p * C;
    bf16_t* o = out + (int64_t)tok * ldo;
    for (int col = threadIdx.x; col < Kp; col += blockDim.x) {
        bf16_t v = 0;
        if (col < K) {
            const int c = col % C, t = col / C, qq = t % p, pp = t / p;
            v = f2bf(img[((int64_t)c * H + ph * p + pp) * W + pw * p + qq]);
        }
        o[col] = v;
    }
}
extern "C" int umv_patchify_f32_bf16(const float* img, int C, int H, int W, int p, uint16_t* out, int64_t ldo, int Kp, umv_stream_t stream) {
    UMV_CHECK(img && out, UMV_ERR_ARG, "patchify: null pointer");
    UMV_CHECK(C > 0 && p > 0 && H > 0 && W > 0 && H % p == 0 && W % p == 0, UMV_ERR_ARG, "patchify: image %d x %d x %d is not a whole number of %d-pixel patches", C, H, W, p);
    UMV_CHECK(Kp >= p * p * C && ldo >= Kp, UMV_ERR_ARG, "patchify: Kp %d / ldo %lld too small for %d values per patch", Kp, (long long)ldo, p * p * C);
    hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)((H / p) * (W / p))), dim3(256), 0, (hipStream_t)stream, img, C, H, W, p, out, ldo, Kp);
    UMV_LAUNCH_CHECK();
    return UMV_OK;
}
