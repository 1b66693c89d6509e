// MXFP4 weight-only storage for the decode step's linear layers (gfx950): tn_weight_quantize_mxfp4 turns a bf16 weight
// [N, K] into e2m1 codes uint8 [N, K / 2] and ONE e8m0 scale byte per 32 elements along K, uint8 [N, K / 32], by the rules of
// mxfp4.h; tn_weight_dequantize_mxfp4 is the exact way back, for the products the weight-streaming kernels do not take
// (prefill).  What reads the codes are the MXFP4 arms of csrc/gemm_smallm.hip and csrc/gemm_midm.hip.
//
// Work split: a lane owns whole blocks.  The quantiser's lane reads its block's 64 bytes as four 16-byte loads, keeps the max
// of |w| on the integer bit patterns (infinities and NaNs order above every finite value), encodes the 32 elements and
// stores them as ONE 16-byte store plus the scale byte: no cross-lane step, no second pass.  A block that holds a NaN or an
// infinity gets scale byte 255 (e8m0's NaN, out of the kernels' contract) and zero codes; functional.quantize_weight_mxfp4
// refuses such weights, and any |w| >= 2^120, before it comes to that.  The inverse's lane expands one dword of 8 codes
// (mxfp4.h's expand8, the GEMMs' own rule) into one 16-byte store.  Both run once per weight: correct, not tuned.
#include "mxfp4.h"

namespace tn {
namespace wq4 {

using namespace mx4;

__global__ void __launch_bounds__(256) quantize_kernel(const bf16_t* __restrict__ w, uint8_t* __restrict__ codes,
                                                       uint8_t* __restrict__ scales, int N, int K, long long ldw,
                                                       long long ldc, long long lds) {
  const int per_row = K / kBlock;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * per_row) return;
  const long long row = i / per_row;
  const int j = (int)(i % per_row);
  const bf16_t* src = w + row * ldw + kBlock * j;
  float f[4][8];
  uint32_t a = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    Vec16<bf16_t> v;
    v.load(src + 8 * q);
    v.unpack(f[q]);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const uint32_t b = __float_as_uint(f[q][t]) & 0x7fffffffu;
      a = b > a ? b : a;
    }
  }
  const bool finite = a < kInfBits;
  const int e = finite ? scale_exp(a) : 128;
  const float inv = __uint_as_float((uint32_t)(127 - (finite ? e : 0)) << 23);      // 2^-e
  u32x4_t c;
#pragma unroll
  for (int q = 0; q < 4; ++q) c[q] = finite ? encode8(f[q], inv) : 0u;
  *reinterpret_cast<u32x4_t*>(codes + row * ldc + (kBlock / 2) * j) = c;
  scales[row * lds + j] = (uint8_t)(e + 127);
}

__global__ void __launch_bounds__(256) dequantize_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                         bf16_t* __restrict__ w, int N, int K, long long ldc, long long lds,
                                                         long long ldw) {
  const int per_row = K >> 3;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * per_row) return;
  const long long row = i / per_row;
  const int q = (int)(i % per_row);
  const uint32_t c = *reinterpret_cast<const uint32_t*>(codes + row * ldc + 4 * q);
  *reinterpret_cast<u32x4_t*>(w + row * ldw + 8 * q) = expand8(c, scale_f32(scales[row * lds + (q >> 2)]));
}

static bool ok(const void* w, const void* codes, const void* scales, int N, int K, long long ldw, long long ldc, long long lds) {
  return w != nullptr && codes != nullptr && scales != nullptr && ((uintptr_t)w & 15) == 0 && ((uintptr_t)codes & 15) == 0 &&
         N > 0 && K > 0 && K % kBlock == 0 && ldw >= K && ldw % 8 == 0 && ldc >= K / 2 && ldc % 16 == 0 && lds >= K / kBlock;
}

}  // namespace wq4
}  // namespace tn

extern "C" int tn_weight_quantize_mxfp4(const void* w, void* codes, void* scales, int N, int K, long long ldw, long long ldc,
                                        long long lds, void* stream) {
  using namespace tn::wq4;
  if (!ok(w, codes, scales, N, K, ldw, ldc, lds)) return TN_EINVAL;
  const long long blocks = ((long long)N * (K / kBlock) + 255) / 256;
  if (blocks > 0x7fffffffll) return TN_EINVAL;
  hipLaunchKernelGGL(quantize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const tn::bf16_t*)w,
                     (uint8_t*)codes, (uint8_t*)scales, N, K, ldw, ldc, lds);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

extern "C" int tn_weight_dequantize_mxfp4(const void* codes, const void* scales, void* w, int N, int K, long long ldc,
                                          long long lds, long long ldw, void* stream) {
  using namespace tn::wq4;
  if (!ok(w, codes, scales, N, K, ldw, ldc, lds)) return TN_EINVAL;
  const long long blocks = ((long long)N * (K >> 3) + 255) / 256;
  if (blocks > 0x7fffffffll) return TN_EINVAL;
  hipLaunchKernelGGL(dequantize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes,
                     (const uint8_t*)scales, (tn::bf16_t*)w, N, K, ldc, lds, ldw);
  TN_LAUNCH_CHECK();
  return TN_OK;
}
