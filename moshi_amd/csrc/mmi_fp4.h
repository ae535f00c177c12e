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
