// The MXFP4 weight format (OCP microscaling FP4, gfx950), ONE definition per rule for the quantiser and its inverse
// (weight_mxfp4.hip) and the MXFP4 arms of the weight-streaming GEMMs (gemm_smallm.hip, gemm_midm.hip).
//
//   codes   uint8 [N, K / 2]    byte i of a row holds element 2 i in bits 3:0 and element 2 i + 1 in bits 7:4.  An element is
//                               e2m1: 1 sign, 2 exponent, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 (codes 0 .. 7),
//                               both zeros legal
//   scales  uint8 [N, K / 32]   e8m0: byte b means 2^(b - 127), shared by elements 32 j .. 32 j + 31 of the row.  Bytes 1 .. 254
//                               are in contract; 0 (2^-127, not a normal fp32) and 255 (e8m0's NaN) are not
//
// The quantiser's rule per block of 32: e is the smallest integer >= kMinExp with amax <= 6 * 2^e, taken from the exponent and
// mantissa bits of amax = m * 2^x, m in [1, 2): 6 = 1.5 * 2^2, so e = x - 2 if m <= 1.5, else x - 1 (kv_fp8.h's rule with 6
// in 448's place).  code = e2m1(w * 2^-e), round to nearest, ties to the even mantissa bit, the sign bit the input's;
// |w * 2^-e| <= 6, so nothing saturates.  amax == 0 lands on e = kMinExp with zero codes.
//
// Expansion is exact: a code has 2 significant bits and the scale is a power of two, so for every scale the quantiser writes
// (b >= 27) code * scale is a bf16 number, and v_cvt_scalef32_pk_bf16_fp4 — byte `sel` of a dword of codes, low nibble
// first, times the scale operand's power of two — has nothing to round.  The consumers therefore hand the bf16 kernels'
// arithmetic the very values dequantize(codes, scales) holds.
#pragma once
#include "common.h"

namespace tn {
namespace mx4 {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
constexpr int kBlock = 32;                 // elements under one scale
constexpr int kMinExp = -100;              // lowest scale exponent the quantiser writes
constexpr uint32_t kInfBits = 0x7f800000u;

// scale byte b in 1 .. 254 -> 2^(b - 127) as fp32
__device__ __forceinline__ float scale_f32(uint32_t b) { return __uint_as_float(b << 23); }

// a dword of 8 codes under one scale -> their 8 bf16 values as 4 packed pairs, element 2 i in the low half of dword i
__device__ __forceinline__ u32x4_t expand8(uint32_t c, float scale) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 0));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 1));
  r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 2));
  r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 3));
  return r;
}

// amax of a block (finite, as the bits of |w|) -> e
__device__ __forceinline__ int scale_exp(uint32_t amax_bits) {
  const int x = (int)(amax_bits >> 23) - 127;
  const int e = x - ((amax_bits & 0x7fffffu) <= 0x400000u ? 2 : 1);
  return e < kMinExp ? kMinExp : e;
}

// 8 values times inv = 2^-e (|f * inv| <= 6) -> a dword of 8 codes.  The magnitude code counts the rounding thresholds at
// or below a: the midpoints of neighbouring magnitudes, each belonging to the neighbour whose mantissa bit is 0.
__device__ __forceinline__ uint32_t encode8(const float (&f)[8], float inv) {
  uint32_t c = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float a = fabsf(f[i]) * inv;
    const uint32_t mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    c |= (((__float_as_uint(f[i]) >> 28) & 8u) | mag) << (4 * i);
  }
  return c;
}

}  // namespace mx4
}  // namespace tn
