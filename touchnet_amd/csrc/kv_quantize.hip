// tn_kv_quantize (gfx950): bf16 keys or values [T, Nkv, D] -> FP8 codes uint8 [T, Nkv, D] and fp32 scales [T, Nkv] in the
// format of kv_fp8.h — what the prefill, extend(append=True) and the new rows handed to tn_attn_extend_fp8 go through
// before they meet an FP8 KV cache (the decode kernels quantise their one new key themselves).
//
// Work split: a key (one (row, kv head) pair, D contiguous elements) is held by D / 8 neighbouring lanes, 8 elements
// each: one 16-byte load per lane, 64 / (D / 8) keys per wave, 4 waves per workgroup.  amax crosses the key's lanes with
// log2(D / 8) xor shuffles; each lane converts its 8 elements (four v_cvt_pk_fp8_f32) and stores them with one 8-byte
// store — the lanes of a wave write 512 contiguous bytes —, the group's first lane stores the scale.  No LDS, no atomics;
// a key's codes depend on its own D elements alone, not on T or on where the key sits.
#include "kv_fp8.h"

namespace tn {
namespace kvq {

constexpr int kThreads = 256;

template <int D>
__global__ void __launch_bounds__(kThreads) kv_quantize_kernel(const bf16_t* __restrict__ x, fp8_t* __restrict__ codes,
                                                               float* __restrict__ scales, long long keys) {
  constexpr int LPK = D / 8;
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long key = t / LPK;
  const int part = (int)(t % LPK);
  const bool live = key < keys;            // (a key's lanes are all live or all idle: LPK divides the wave)
  Vec16<bf16_t> v;
  v.raw = make_uint4(0u, 0u, 0u, 0u);
  if (live) v.load(x + key * D + part * 8);
  float f[8];
  v.unpack(f);
  uint2 c;
  float s;
  quantize_key<LPK>(f, c, s);
  if (!live) return;
  *reinterpret_cast<uint2*>(codes + key * D + part * 8) = c;
  if (part == 0) scales[key] = s;
}

}  // namespace kvq
}  // namespace tn

extern "C" int tn_kv_quantize(const void* x, void* codes, float* scales, long long T, int Nkv, int D, void* stream) {
  using namespace tn::kvq;
  if (T < 0 || Nkv <= 0 || (D != 64 && D != 128)) return TN_EINVAL;
  const long long keys = T * Nkv;
  const long long blocks = (keys * (D / 8) + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffll) return TN_EINVAL;
  if (T == 0) return TN_OK;
  if (x == nullptr || ((uintptr_t)x & 15) || codes == nullptr || ((uintptr_t)codes & 7) || scales == nullptr ||
      ((uintptr_t)scales & 3))
    return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (D == 64)
    hipLaunchKernelGGL((kv_quantize_kernel<64>), dim3((unsigned)blocks), dim3(kThreads), 0, st, (const tn::bf16_t*)x,
                       (fp8_t*)codes, scales, keys);
  else
    hipLaunchKernelGGL((kv_quantize_kernel<128>), dim3((unsigned)blocks), dim3(kThreads), 0, st, (const tn::bf16_t*)x,
                       (fp8_t*)codes, scales, keys);
  TN_LAUNCH_CHECK();
  return TN_OK;
}
