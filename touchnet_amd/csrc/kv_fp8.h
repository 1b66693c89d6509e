// The FP8 KV-cache format (gfx950), ONE definition per rule for the quantiser (kv_quantize.hip), the decode kernels
// (attn_decode.hip) and the extend kernel (attn_extend.hip).
//
//   codes  uint8 [.., Nkv, D]   OCP e4m3 (torch.float8_e4m3fn's bits): 1 sign, 4 exponent (bias 7), 3 mantissa bits, largest
//                               finite value 448, subnormal step 2^-9
//   scale  fp32  [.., Nkv]      one per key (row, position, kv head), a power of two 2^e shared by the key's D elements;
//                               V has its own
//
// e is the smallest integer with amax <= 448 * 2^e, taken from the exponent and mantissa bits of amax = m * 2^x, m in
// [1, 2): 448 = 1.75 * 2^8, so e = x - 8 if m <= 1.75, else x - 7; never below kMinExp, so that code * scale is zero or a
// normal number (amax == 0 lands there too, with codes 0).  code = e4m3(x * 2^-e), round to nearest even
// (v_cvt_pk_fp8_f32): the product is exact and |x * 2^-e| <= 448, so nothing saturates.  A key that holds a NaN or an
// infinity gets scale NaN and codes 0: whatever attends to it is NaN, as with a bf16 cache.
//
// Dequantisation is exact: a code has at most 4 significant bits and the scale is a power of two, so code * scale is a
// bf16 (and fp32) number.  The consumers therefore hand the bf16 kernels' arithmetic the very values a bf16 cache holding
// dequantize(codes, scale) would.
//
// A key is held by LPK = D / 8 neighbouring lanes, 8 consecutive elements each (the decode kernels' layout); amax crosses
// the lanes of the group with xor shuffles, on the integer bit patterns: |x| as an unsigned integer orders finite values
// as fp32 does and puts infinity and every NaN above them, so one integer max finds the amax and the non-finite keys.
#pragma once
#include "common.h"

namespace tn {
namespace kvq {

typedef uint8_t fp8_t;                     // raw e4m3 bits
constexpr int kMinExp = -100;              // lowest scale exponent
constexpr uint32_t kInfBits = 0x7f800000u;

// 2^e for e in [-126, 127]
__device__ __forceinline__ float exp2i(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }

// max over the 8 values of |f| as bit patterns, then over the LPK lanes of the key
template <int LPK>
__device__ __forceinline__ uint32_t key_amax_bits(const float (&f)[8]) {
  uint32_t a = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t b = __float_as_uint(f[i]) & 0x7fffffffu;
    a = b > a ? b : a;
  }
#pragma unroll
  for (int off = LPK / 2; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)a, off, 64);
    a = o > a ? o : a;
  }
  return a;
}

// amax (finite, as bits) -> e
__device__ __forceinline__ int scale_exp(uint32_t amax_bits) {
  const int x = (int)(amax_bits >> 23) - 127;
  const int e = x - ((amax_bits & 0x7fffffu) <= 0x600000u ? 8 : 7);
  return e < kMinExp ? kMinExp : e;
}

// 8 values times inv = 2^-e -> 8 codes (element i in byte i)
__device__ __forceinline__ uint2 encode8(const float (&f)[8], float inv) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

// 8 codes and their key's scale -> the 8 fp32 values (exact)
__device__ __forceinline__ void decode8(const uint2 c, float scale, float (&f)[8]) {
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
  const f32x2 g = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), h = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
  f[0] = a.x * scale; f[1] = a.y * scale; f[2] = b.x * scale; f[3] = b.y * scale;
  f[4] = g.x * scale; f[5] = g.y * scale; f[6] = h.x * scale; f[7] = h.y * scale;
}

// ... -> the same values as 4 packed bf16 pairs (exact: the rounding of pack2bf has nothing to round)
__device__ __forceinline__ uint4 decode8_bf16(const uint2 c, float scale) {
  float f[8];
  decode8(c, scale, f);
  return make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
}

// One key held by LPK lanes (f: this lane's 8 elements) -> this lane's 8 codes and the key's scale (every lane of the
// group gets the same scale).  All lanes of the group must be active.
template <int LPK>
__device__ __forceinline__ void quantize_key(const float (&f)[8], uint2& codes, float& scale) {
  const uint32_t a = key_amax_bits<LPK>(f);
  if (a >= kInfBits) {
    codes = make_uint2(0u, 0u);
    scale = __builtin_nanf("");
    return;
  }
  const int e = scale_exp(a);
  codes = encode8(f, exp2i(-e));
  scale = exp2i(e);
}

}  // namespace kvq
}  // namespace tn
