// OCP Microscaling MXFP4 (MX v1.0) -> bf16, the one conversion of the weight-only 4-bit linears (lm_kernels.h, WQ = 4).
//   code   E2M1, 4 bits: bit 3 sign, bits 2..0 magnitude {0, 0.5, 1, 1.5, 2, 3, 4, 6}; two codes per byte, element 2i in the
//          low nibble
//   scale  E8M0, one byte per block of 32 consecutive input features: 2^(s - 127).  The engine admits s in 2..252 (checked at
//          load): every product magnitude * scale is then a NORMAL bf16 value (>= 0.5 * 2^-125, <= 6 * 2^125) with at most one
//          mantissa bit, so the conversion is exact - no rounding, no overflow, no subnormal
// Device code takes the gfx950 instruction v_cvt_scalef32_pk_bf16_fp4 (two codes of one byte -> one packed bf16 pair, times
// a fp32 scale); host code and the simulator take the plain restatement below.  The two must agree bit for bit: the one-hot
// cases of tests/mxfp4_cases.py hold them to each other through the GEMM.
#pragma once
#include <mmi_device.h>  // u32x4; resolved through -I like mmi_common.h does
#include <stdint.h>

// 2^(s - 127) as fp32 (s in 1..254: a normal float whose exponent field is s)
__host__ __device__ __forceinline__ float mmi_e8m0_to_f32(uint32_t s) { return __builtin_bit_cast(float, (s & 0xffu) << 23); }

// the restatement: decode the nibble, multiply by the scale, take the bf16 bits (the product has <= 1 mantissa bit: the upper
// half of the fp32 IS the bf16)
__host__ __device__ __forceinline__ uint32_t mmi_fp4_to_bf16_bits(uint32_t code, float scale) {
    const uint32_t m = code & 7u;
    const float mag = m < 2u ? 0.5f * (float)m : (float)(2u + (m & 1u)) * (float)(1u << ((m >> 1) - 1u)) * 0.5f;
    const uint32_t bits = __builtin_bit_cast(uint32_t, mag * scale) >> 16;
    return bits | ((code & 8u) << 12);
}

// byte `SEL` of `w` (codes 2 SEL, 2 SEL + 1 of the word's eight) -> packed bf16 pair, low half = the low nibble's value
template <int SEL>
__host__ __device__ __forceinline__ uint32_t mmi_fp4x2_to_bf16x2(uint32_t w, float scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL));
#else
    const uint32_t b = (w >> (8 * SEL)) & 0xffu;
    return mmi_fp4_to_bf16_bits(b & 15u, scale) | (mmi_fp4_to_bf16_bits(b >> 4, scale) << 16);
#endif
}

// eight codes (one word = one k-step's share of a lane's weight entry) -> one bf16 MFMA fragment, scaled by 2^(s - 127)
__host__ __device__ __forceinline__ u32x4 mmi_fp4x8_to_bf16(uint32_t w, uint32_t s) {
    const float scale = mmi_e8m0_to_f32(s);
    u32x4 r;
    r[0] = mmi_fp4x2_to_bf16x2<0>(w, scale);
    r[1] = mmi_fp4x2_to_bf16x2<1>(w, scale);
    r[2] = mmi_fp4x2_to_bf16x2<2>(w, scale);
    r[3] = mmi_fp4x2_to_bf16x2<3>(w, scale);
    return r;
}

// ---- the 4-bit KV ring: E2M1 codes under one E8M0 scale byte per block of 16 consecutive head-dim elements ----
// Quantising a block of bf16 values x[0..15] (held as fp32):
//   E = biased exponent of the block's absmax (the largest |bits|, so a NaN counts as the largest magnitude there is);
//   E < 3 (a zero block, or an absmax below 2^-124): scale byte 0 and sixteen zero codes;
//   else s = min(E - 2, 253), every magnitude clamped to 6 * 2^(s - 127) first - Inf and NaN become +-6 under their sign, the
//   conversion itself never sees an overflow - then |x| / 2^(s - 127) rounded to the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6},
//   ties to the even code.  This is weights.quantize_lm_state_dict_mxfp4's rule on blocks of 16.
// Device code converts with v_cvt_scalef32_pk_fp4_f32 and widens with v_cvt_scalef32_pk_f32_fp4; host code and the simulator
// take the restatements.  tests/kv4_cases.py holds both to a numpy statement of the rule over all 65536 bf16 patterns.
// Widening: code * 2^(s - 127); scale byte 0 gives the factor 0.0f, so a zeroed ring (and a flushed block) reads as zeros.
__host__ __device__ __forceinline__ uint32_t mmi_kv4_scale_byte(uint32_t absmax_bits) {
    const uint32_t E = (absmax_bits >> 23) & 0xffu;
    return E < 3u ? 0u : (E - 2u > 253u ? 253u : E - 2u);
}
// one E2M1 code of a finite value already clamped to +-6 * 2^(s - 127); inv = 2^(127 - s)
__host__ __device__ __forceinline__ uint32_t mmi_kv4_code_ref(float x, float inv) {
    const uint32_t sign = (__builtin_bit_cast(uint32_t, x) >> 28) & 8u;
    const float q = __builtin_fabsf(x) * inv;
    uint32_t c;
    if (q < 2.f) c = (uint32_t)__builtin_rintf(q * 2.f);                      // 0, .5, 1, 1.5, 2 -> codes 0..4
    else if (q < 4.f) c = 2u + (uint32_t)__builtin_rintf(q);                  // 2, 3, 4 -> codes 4..6
    else c = 4u + (uint32_t)__builtin_rintf(q * 0.5f);                        // 4, 6 -> codes 6, 7
    return sign | c;
}
// eight values -> eight codes in one word (value 2i in the low nibble of byte i), under scale byte s >= 1
__host__ __device__ __forceinline__ uint32_t mmi_kv4_quant8(const float* x, uint32_t s) {
    // 6 * 2^(s - 127) = 1.5 * 2^(s + 2 - 127); under s = 253 (an Inf or NaN in the block) that is no fp32 value: the finite ones
    // (below 4 * 2^126) need no clamp there, and Inf / NaN take the largest finite value and then the code 7 by hand
    const uint32_t lim = s >= 253u ? 0x7f7fffffu : ((s + 2u) << 23 | 0x400000u);
    float c[8];
    uint32_t r = 0u, top = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t b = __builtin_bit_cast(uint32_t, x[e]), m = b & 0x7fffffffu;
        c[e] = __builtin_bit_cast(float, (b & 0x80000000u) | (m < lim ? m : lim));
        if (m >= 0x7f800000u) top |= 7u << (4 * e);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    const float scale = mmi_e8m0_to_f32(s);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, c[0], c[1], scale, 0);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, c[2], c[3], scale, 1);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, c[4], c[5], scale, 2);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(r, c[6], c[7], scale, 3);
#else
    const float inv = mmi_e8m0_to_f32(254u - s);
#pragma unroll
    for (int e = 0; e < 8; ++e) r |= mmi_kv4_code_ref(c[e], inv) << (4 * e);
#endif
    return r | top;
}
// |bits| maximum of eight values (the absmax of a half block, as bits: monotonic in the magnitude)
__host__ __device__ __forceinline__ uint32_t mmi_kv4_absmax8(const float* x) {
    uint32_t m = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t b = __builtin_bit_cast(uint32_t, x[e]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    return m;
}
// eight codes of one word -> eight fp32 values, times 2^(s - 127) (s = 0: all zero)
__host__ __device__ __forceinline__ void mmi_kv4_widen8(uint32_t w, uint32_t s, float* f) {
    const float scale = mmi_e8m0_to_f32(s);
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 1);
    const f32x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 3);
    f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1]; f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
#else
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t code = (w >> (4 * e)) & 15u, m = code & 7u;
        const float mag = m < 2u ? 0.5f * (float)m : (float)(2u + (m & 1u)) * (float)(1u << ((m >> 1) - 1u)) * 0.5f;
        f[e] = (code & 8u) ? -(mag * scale) : mag * scale;
    }
#endif
}
