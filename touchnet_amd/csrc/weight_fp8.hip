// FP8 (e4m3) weight-only storage for the decode step's linear layers (gfx950): tn_weight_quantize_fp8 turns a bf16 weight
// [N, K] into e4m3 codes uint8 [N, K] and ONE fp32 power-of-two scale per output row [N], by the rules of kv_fp8.h (a row
// here is what a key is there: scale = 2^e, e the smallest integer with amax <= 448 * 2^e, never below kMinExp; code =
// e4m3(w * 2^-e), round to nearest even; code * scale is exact in bf16).  tn_weight_dequantize_fp8 is the way back, for
// the products the small-M kernel does not take (prefill).  What reads the codes is csrc/gemm_smallm.hip's FP8 variant.
//
// Work split: one wave per weight row, four rows per workgroup.  Pass 1: each lane walks the row in 16-byte loads (8
// elements, 512 per wave and step) and keeps the max of |w| on the integer bit patterns (key_amax_bits's rule: infinities and
// NaNs order above every finite value), then six xor shuffles cross the wave.  Pass 2 reads the row again (it is in L2),
// encodes 8 elements with four v_cvt_pk_fp8_f32 and stores them as one 8-byte store.  K is any multiple of 8.  A row
// with a NaN or an infinity gets scale NaN and codes 0 as a key does; functional.quantize_weight_fp8 refuses such weights
// before it comes to that.  Both kernels run once per weight at load time (or once per prefill): correct, not tuned.
#include "kv_fp8.h"

namespace tn {
namespace wq {

using namespace kvq;
constexpr int kWaves = 4;

__global__ void __launch_bounds__(kWaves * 64) quantize_kernel(const bf16_t* __restrict__ w, fp8_t* __restrict__ codes,
                                                               float* __restrict__ scale, int N, int K, long long ldw,
                                                               long long ldc) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= N) return;                       // (a whole wave: the shuffles below see 64 live lanes)
  const bf16_t* src = w + row * ldw;
  uint32_t a = 0u;
  for (int k = 8 * lane; k < K; k += 512) {
    Vec16<bf16_t> v;
    v.load(src + k);
    float f[8];
    v.unpack(f);
    const uint32_t b = key_amax_bits<1>(f);
    a = b > a ? b : a;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)a, off, 64);
    a = o > a ? o : a;
  }
  const bool finite = a < kInfBits;
  const int e = finite ? scale_exp(a) : 0;
  const float inv = exp2i(-e);
  for (int k = 8 * lane; k < K; k += 512) {
    Vec16<bf16_t> v;
    v.load(src + k);
    float f[8];
    v.unpack(f);
    *reinterpret_cast<uint2*>(codes + row * ldc + k) = finite ? encode8(f, inv) : make_uint2(0u, 0u);
  }
  if (lane == 0) scale[row] = finite ? exp2i(e) : __builtin_nanf("");
}

__global__ void __launch_bounds__(256) dequantize_kernel(const fp8_t* __restrict__ codes, const float* __restrict__ scale,
                                                         bf16_t* __restrict__ w, int N, int K, long long ldc, long long ldw) {
  const int per_row = K >> 3;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * per_row) return;
  const long long row = i / per_row;
  const int k = 8 * (int)(i % per_row);
  const uint2 c = *reinterpret_cast<const uint2*>(codes + row * ldc + k);
  *reinterpret_cast<uint4*>(w + row * ldw + k) = decode8_bf16(c, scale[row]);
}

static bool ok(const void* w, const void* codes, const void* scale, int N, int K, long long ldw, long long ldc) {
  return w != nullptr && codes != nullptr && scale != nullptr && ((uintptr_t)w & 15) == 0 && ((uintptr_t)codes & 7) == 0 &&
         ((uintptr_t)scale & 3) == 0 && N > 0 && K > 0 && K % 8 == 0 && ldw >= K && ldw % 8 == 0 && ldc >= K && ldc % 8 == 0;
}

}  // namespace wq
}  // namespace tn

extern "C" int tn_weight_quantize_fp8(const void* w, void* codes, float* scale, int N, int K, long long ldw, long long ldc,
                                      void* stream) {
  using namespace tn::wq;
  if (!ok(w, codes, scale, N, K, ldw, ldc)) return TN_EINVAL;
  hipLaunchKernelGGL(quantize_kernel, dim3((N + kWaves - 1) / kWaves), dim3(kWaves * 64), 0, (hipStream_t)stream,
                     (const tn::bf16_t*)w, (fp8_t*)codes, scale, N, K, ldw, ldc);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

extern "C" int tn_weight_dequantize_fp8(const void* codes, const float* scale, void* w, int N, int K, long long ldc,
                                        long long ldw, void* stream) {
  using namespace tn::wq;
  if (!ok(w, codes, scale, N, K, ldw, ldc)) return TN_EINVAL;
  const long long blocks = ((long long)N * (K >> 3) + 255) / 256;
  if (blocks > 0x7fffffffll) return TN_EINVAL;
  hipLaunchKernelGGL(dequantize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const fp8_t*)codes, scale,
                     (tn::bf16_t*)w, N, K, ldc, ldw);
  TN_LAUNCH_CHECK();
  return TN_OK;
}
