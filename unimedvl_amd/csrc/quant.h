// Format conversions of the quantised weight images (gfx950), shared by the packers (pack.hip) and the decode GEMMs that stream the
// images (gemm_skinny.h).  Internal to csrc/.
#pragma once
#include "common.h"

// 16 e4m3 values x one power-of-two scale -> 16 bf16 (exact: an e4m3 value times 2^e is a bf16 value)
__device__ __forceinline__ void cvt_fp8x16(u32x4 q, float scale, bf16x8& lo, bf16x8& hi) {
    union { umv_bf16x2_hw h[4]; bf16x8 v; } a, b;
    a.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.x, scale, false);
    a.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.x, scale, true);
    a.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.y, scale, false);
    a.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.y, scale, true);
    b.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.z, scale, false);
    b.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.z, scale, true);
    b.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.w, scale, false);
    b.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q.w, scale, true);
    lo = a.v;
    hi = b.v;
}

// E8M0 byte -> the f32 scale operand of v_cvt_scalef32_*: 2^(b - 127); b = 0 is the subnormal 2^-127
__device__ __forceinline__ float e8m0_scale(uint32_t b) { return __uint_as_float(b ? b << 23 : 0x00400000u); }

// 8 e2m1 codes (low nibble first) x one scale -> 8 bf16 (exact)
__device__ __forceinline__ bf16x8 cvt_fp4x8(uint32_t q, float scale) {
    union { umv_bf16x2_hw h[4]; bf16x8 v; } a;
    a.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0);
    a.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1);
    a.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2);
    a.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3);
    return a.v;
}

// E8M0 byte of a block from the bf16 bits of its largest magnitude (bits & 0x7FFF; the order of the bit patterns is the order of
// the values).  amax = 1.m * 2^(E-127): 6 * 2^e >= amax  <=>  e >= E - 129 when 1.m <= 1.5 (m <= 0x40), else e >= E - 128.
__device__ __forceinline__ uint32_t mxfp4_scale_byte(uint32_t amax_bits) {
    if (amax_bits == 0) return 127u;
    const int E = (int)(amax_bits >> 7), m = (int)(amax_bits & 0x7F);
    int e = E == 0 ? -127 : ((m <= 0x40) ? E - 129 : E - 128);      // bf16 subnormals: e <= -129, clamped
    e = e < -127 ? -127 : (e > 127 ? 127 : e);
    return (uint32_t)(e + 127);
}

// |v| / 2^e (exact where it matters: at and above the first threshold 0.25) -> e2m1 code by round to nearest even, sign kept
__device__ __forceinline__ uint32_t e2m1_code(uint16_t h, int e) {
    const float a = ldexpf(fabsf(bf2f(h)), -e);
    uint32_t c;
    if (a <= 0.25f) c = 0;            // ties go to the even code: 0.25 -> 0, 0.75 -> 1 (code 2), 1.25 -> 1, 1.75 -> 2, 2.5 -> 2,
    else if (a < 0.75f) c = 1;        // 3.5 -> 4, 5 -> 4
    else if (a <= 1.25f) c = 2;
    else if (a < 1.75f) c = 3;
    else if (a <= 2.5f) c = 4;
    else if (a < 3.5f) c = 5;
    else if (a <= 5.0f) c = 6;
    else c = 7;
    return c | ((uint32_t)(h >> 15) << 3);
}
