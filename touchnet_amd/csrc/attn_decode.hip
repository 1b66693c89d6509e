// Single-token attention over a KV cache (greedy ASR decoding, touchnet/models/touch_audio/inference_touch_audio.py:177-192:
// HF generate() with use_cache=True) — flash-decoding for the decoder geometries of the project (D 64 / 128, GQA groups up
// to 16 query heads per key/value head).
//
//   q      bf16 [B, Nh, D]        rotated query of the new token
//   k_new  bf16 [B, Nkv, D]       rotated key of the new token;  v_new bf16 [B, Nkv, D]
//   k_cache, v_cache bf16 [B, S_max, Nkv, D]   (the projection GEMM's output layout: one key row = D * 2 contiguous bytes)
//   cache_len int32 [B]           entries valid before this call
//   o      bf16 [B, Nh, D]
//
// The new key / value go to slot cache_len[b]; the attention covers cache_len[b] + 1 keys; cache_len is NOT advanced here
// (every layer of a step shares it; tn_greedy_step advances it).  cache_len[b] outside [0, S_max) poisons row b's output
// with NaN and leaves its cache untouched.
//
// One workgroup per (key split, kv head, batch row); its 4 waves stream disjoint keys of the split straight into VGPRs with
// 16-byte loads (no LDS staging: every byte is read once, by one lane).  D / 8 lanes hold one key row; each lane keeps the
// matching 8 elements of all G query heads of the group, so ONE pass over K and V serves the whole group.  Online softmax
// per lane group in the log2 domain (scores * scale * log2(e), the forward kernels' convention), fp32 state; the lane
// groups, then the waves, are merged at the end.  With more than one split the partials (O / l and m + log2 l) go to an fp32
// workspace and a second launch combines them.  Split boundaries depend only on (B, Nkv, S_max) and cache_len: results are
// bit-reproducible.  The slot cache_len[b] is read by nobody: the key at index cache_len[b] is taken from k_new / v_new,
// and only the workgroup whose split contains that index writes the slot.
#include <type_traits>

#include "common.h"

namespace tn {
namespace decode {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMinKeysPerSplit = 64;
constexpr int kMaxSplits = 64;
constexpr int kTargetWorkgroups = 512;    // 2 per CU on the 256 CUs

__host__ __device__ inline int num_splits(int B, int Nkv, int S_max) {
  const int units = B * Nkv;
  int s = (kTargetWorkgroups + units - 1) / units;
  const int by_len = (S_max + kMinKeysPerSplit - 1) / kMinKeysPerSplit;
  if (s > by_len) s = by_len;
  if (s > kMaxSplits) s = kMaxSplits;
  return s < 1 ? 1 : s;
}

// keys per split of a row with `total` keys: a multiple of 64, at least 64
__device__ inline int split_keys(int total, int nsplit) {
  int c = (total + nsplit - 1) / nsplit;
  c = (c + kMinKeysPerSplit - 1) / kMinKeysPerSplit * kMinKeysPerSplit;
  return c < kMinKeysPerSplit ? kMinKeysPerSplit : c;
}

__device__ __forceinline__ void unpack8(const uint4 r, float (&f)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

template <int LPK>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = LPK / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Partial results: ws_o [B, Nkv, nsplit, G, D] fp32 (normalised by l), ws_lse [B, Nkv, nsplit, G] fp32 (m + log2 l, -inf =
// empty split).  With nsplit == 1 the normalised output goes straight to o.
//
// BEAM (tn_attn_decode_beam): key / value s < cache_len[b] of row b is read at cache[src[b, s], s] — beams of one utterance
// share the rows of their common ancestors, nothing is copied when beams are reordered.  The new key / value still go to
// cache[b, cache_len[b]].  A table entry outside [0, B) is replaced by b (nothing is read out of bounds) and poisons the
// row's output with NaN.  Everything else, the order of every floating-point operation included, is the dense kernel's.
// Precondition: no consulted entry names the slot another row stores in this launch (src[b, s] == r' with s ==
// cache_len[r'], s < cache_len[b]): that read would race with the store.  Rows that share a cache_len cannot do it.
struct NoTable {};                        // the dense kernel's `src`: an empty argument, so its code is what it was
struct Table {
  const int* __restrict__ p;
};

template <int D, int G, bool BEAM = false>
__global__ void __launch_bounds__(kThreads) attn_decode_split_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k_new, const bf16_t* __restrict__ v_new,
    bf16_t* __restrict__ k_cache, bf16_t* __restrict__ v_cache, const int* __restrict__ cache_len, bf16_t* __restrict__ o,
    float* __restrict__ ws_o, float* __restrict__ ws_lse, int Nkv, int S_max, int nsplit, float scale_log2,
    std::conditional_t<BEAM, Table, NoTable> src) {
  constexpr int LPK = D / 8;              // lanes per key row
  constexpr int KPW = 64 / LPK;           // keys per wave per iteration
  constexpr int KPI = KPW * kWaves;       // keys per workgroup per iteration
  constexpr int U = 2;                    // iterations in flight per lane
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = lane % LPK, kg = lane / LPK;
  const int Nh = Nkv * G;
  const int len = cache_len[b];
  const bool overflow = len < 0 || len >= S_max;

  const size_t row_stride = (size_t)Nkv * D;                           // one cache position
  const bf16_t* kc = k_cache + (size_t)b * S_max * row_stride + (size_t)kvh * D + part * 8;
  const bf16_t* vc = v_cache + (size_t)b * S_max * row_stride + (size_t)kvh * D + part * 8;
  const bf16_t* kn = k_new + ((size_t)b * Nkv + kvh) * D + part * 8;
  const bf16_t* vn = v_new + ((size_t)b * Nkv + kvh) * D + part * 8;

  const size_t ws_row = (((size_t)b * Nkv + kvh) * nsplit + split) * G;
  if (overflow) {
    // poisoned row: nothing read or written in the cache
    if (nsplit == 1) {
      for (int i = tid; i < G * D; i += kThreads)
        o[((size_t)b * Nh + kvh * G + i / D) * D + i % D] = 0x7fc0;    // bf16 quiet NaN
    } else if (tid < G) {
      ws_lse[ws_row + tid] = __builtin_nanf("");
    }
    return;
  }
  const int total = len + 1;
  const int chunk = split_keys(total, nsplit);
  const int k0 = split * chunk;
  const int k1 = min(k0 + chunk, total);

  // the owner of the new key's index stores it into the slot (nobody else touches that slot in this launch)
  if (len >= k0 && len < k1 && wave == 0 && kg == 0) {
    *reinterpret_cast<uint4*>(k_cache + ((size_t)b * S_max + len) * row_stride + (size_t)kvh * D + part * 8) =
        *reinterpret_cast<const uint4*>(kn);
    *reinterpret_cast<uint4*>(v_cache + ((size_t)b * S_max + len) * row_stride + (size_t)kvh * D + part * 8) =
        *reinterpret_cast<const uint4*>(vn);
  }

  float qf[G][8];
#pragma unroll
  for (int h = 0; h < G; ++h) {
    const uint4 r = *reinterpret_cast<const uint4*>(q + ((size_t)b * Nh + kvh * G + h) * D + part * 8);
    unpack8(r, qf[h]);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[h][e] *= scale_log2;
  }
  [[maybe_unused]] int R = 0;
  [[maybe_unused]] const int* srow = nullptr;
  [[maybe_unused]] bool bad = false;
  if constexpr (BEAM) {
    R = gridDim.z;
    srow = src.p + (size_t)b * S_max;
  }
  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int h = 0; h < G; ++h) {
    m[h] = -INFINITY;
    l[h] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[h][e] = 0.f;
  }

  for (int base = k0; base < k1; base += U * KPI) {
    uint4 kr[U], vr[U];
    int jj[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = base + u * KPI + wave * KPW + kg;
      jj[u] = j;
      const int js = j < k1 ? j : k0;                                       // (in-bounds filler, never used)
      const bf16_t *kp, *vp;
      if constexpr (BEAM) {
        int r = b;
        if (js != len) {
          r = srow[js];
          if (r < 0 || r >= R) {
            bad = true;
            r = b;
          }
        }
        const size_t off = ((size_t)r * S_max + js) * row_stride + (size_t)kvh * D + part * 8;
        kp = js == len ? kn : k_cache + off;
        vp = js == len ? vn : v_cache + off;
      } else {
        kp = js == len ? kn : kc + (size_t)js * row_stride;
        vp = js == len ? vn : vc + (size_t)js * row_stride;
      }
      kr[u] = *reinterpret_cast<const uint4*>(kp);
      vr[u] = *reinterpret_cast<const uint4*>(vp);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8], vf[8];
      unpack8(kr[u], kf);
      unpack8(vr[u], vf);
      const bool valid = jj[u] < k1;
#pragma unroll
      for (int h = 0; h < G; ++h) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s = __builtin_fmaf(qf[h][e], kf[e], s);
        s = group_sum<LPK>(s);
        if (valid) {
          const float mn = fmaxf(m[h], s);
          const float alpha = fast_exp2(m[h] - mn);          // m = -inf on the first key: 2^-inf = 0
          const float p = fast_exp2(s - mn);
          l[h] = __builtin_fmaf(l[h], alpha, p);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[h][e] = __builtin_fmaf(acc[h][e], alpha, p * vf[e]);
          m[h] = mn;
        }
      }
    }
  }

  // merge the key groups of the wave (lanes part, part + LPK, ...)
#pragma unroll
  for (int off = LPK; off < 64; off <<= 1) {
#pragma unroll
    for (int h = 0; h < G; ++h) {
      const float mo = __shfl_xor(m[h], off, 64);
      const float lo = __shfl_xor(l[h], off, 64);
      const float mn = fmaxf(m[h], mo);
      const float a = mn == -INFINITY ? 0.f : fast_exp2(m[h] - mn);
      const float c = mn == -INFINITY ? 0.f : fast_exp2(mo - mn);
      l[h] = l[h] * a + lo * c;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ao = __shfl_xor(acc[h][e], off, 64);
        acc[h][e] = acc[h][e] * a + ao * c;
      }
      m[h] = mn;
    }
  }
  // ... then the waves, through LDS
  __shared__ float s_acc[kWaves][G][D];
  __shared__ float s_m[kWaves][G], s_l[kWaves][G];
  if (kg == 0) {
#pragma unroll
    for (int h = 0; h < G; ++h) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s_acc[wave][h][part * 8 + e] = acc[h][e];
      if (part == 0) {
        s_m[wave][h] = m[h];
        s_l[wave][h] = l[h];
      }
    }
  }
  if constexpr (BEAM) {
    bad = __syncthreads_or(bad) != 0;
    if (bad) {
      if (nsplit == 1) {
        for (int i = tid; i < G * D; i += kThreads)
          o[((size_t)b * Nh + kvh * G + i / D) * D + i % D] = 0x7fc0;    // bf16 quiet NaN
      } else if (tid < G) {
        ws_lse[ws_row + tid] = __builtin_nanf("");
      }
      return;
    }
  } else {
    __syncthreads();
  }
  for (int i = tid; i < G * D; i += kThreads) {
    const int h = i / D, d = i % D;
    float mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) mx = fmaxf(mx, s_m[w][h]);
    float lt = 0.f, ot = 0.f;
    if (mx != -INFINITY) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const float c = fast_exp2(s_m[w][h] - mx);
        lt = __builtin_fmaf(s_l[w][h], c, lt);
        ot = __builtin_fmaf(s_acc[w][h][d], c, ot);
      }
    }
    const float on = lt > 0.f ? ot / lt : 0.f;
    if (nsplit == 1) {
      o[((size_t)b * Nh + kvh * G + h) * D + d] = f2bf(on);
    } else {
      ws_o[(ws_row + h) * D + d] = on;
      if (d == 0) ws_lse[ws_row + h] = lt > 0.f ? mx + __log2f(lt) : -INFINITY;
    }
  }
}

// o[b, h, :] = sum_s 2^(lse_s - max) O_s / sum_s 2^(lse_s - max); one workgroup per (kv head, batch row)
template <int D, int G>
__global__ void __launch_bounds__(kThreads) attn_decode_combine_kernel(const float* __restrict__ ws_o,
                                                                      const float* __restrict__ ws_lse, bf16_t* __restrict__ o,
                                                                      int Nkv, int nsplit) {
  const int kvh = blockIdx.x, b = blockIdx.y;
  const int Nh = Nkv * G;
  const size_t base = ((size_t)b * Nkv + kvh) * nsplit;
  for (int i = threadIdx.x; i < G * D; i += kThreads) {
    const int h = i / D, d = i % D;
    float mx = -INFINITY;
    bool nan = false;
    for (int s = 0; s < nsplit; ++s) {
      const float v = ws_lse[(base + s) * G + h];
      nan |= v != v;
      mx = fmaxf(mx, v);
    }
    float wsum = 0.f, acc = 0.f;
    for (int s = 0; s < nsplit; ++s) {
      const float v = ws_lse[(base + s) * G + h];
      if (v == -INFINITY) continue;                                   // empty split
      const float w = fast_exp2(v - mx);
      wsum += w;
      acc = __builtin_fmaf(w, ws_o[((base + s) * G + h) * D + d], acc);
    }
    o[((size_t)b * Nh + kvh * G + h) * D + d] = nan ? (bf16_t)0x7fc0 : f2bf(acc / wsum);
  }
}

template <int D, int G>
static int launch(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_len,
                  const int* src, void* o, void* workspace, int B, int Nkv, int S_max, float scale, hipStream_t st) {
  const int nsplit = num_splits(B, Nkv, S_max);
  float* ws_o = (float*)workspace;
  float* ws_lse = ws_o ? ws_o + (size_t)B * Nkv * nsplit * G * D : nullptr;
  const float sl2 = scale * kLog2e;
  if (src)
    hipLaunchKernelGGL((attn_decode_split_kernel<D, G, true>), dim3(nsplit, Nkv, B), dim3(kThreads), 0, st,
                       (const bf16_t*)q, (const bf16_t*)k_new, (const bf16_t*)v_new, (bf16_t*)k_cache, (bf16_t*)v_cache,
                       cache_len, (bf16_t*)o, ws_o, ws_lse, Nkv, S_max, nsplit, sl2, Table{src});
  else
    hipLaunchKernelGGL((attn_decode_split_kernel<D, G, false>), dim3(nsplit, Nkv, B), dim3(kThreads), 0, st,
                       (const bf16_t*)q, (const bf16_t*)k_new, (const bf16_t*)v_new, (bf16_t*)k_cache, (bf16_t*)v_cache,
                       cache_len, (bf16_t*)o, ws_o, ws_lse, Nkv, S_max, nsplit, sl2, NoTable{});
  TN_LAUNCH_CHECK();
  if (nsplit > 1) {
    hipLaunchKernelGGL((attn_decode_combine_kernel<D, G>), dim3(Nkv, B), dim3(kThreads), 0, st, (const float*)ws_o,
                       (const float*)ws_lse, (bf16_t*)o, Nkv, nsplit);
    TN_LAUNCH_CHECK();
  }
  return TN_OK;
}

template <int D>
static int dispatch_g(int G, const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                      const int* cache_len, const int* src, void* o, void* ws, int B, int Nkv, int S_max, float scale,
                      hipStream_t st) {
#define TN_DECODE_G(g) \
  case g: return launch<D, g>(q, k_new, v_new, k_cache, v_cache, cache_len, src, o, ws, B, Nkv, S_max, scale, st);
  switch (G) {
    TN_DECODE_G(1) TN_DECODE_G(2) TN_DECODE_G(3) TN_DECODE_G(4) TN_DECODE_G(5) TN_DECODE_G(6) TN_DECODE_G(7)
    TN_DECODE_G(8) TN_DECODE_G(9) TN_DECODE_G(10) TN_DECODE_G(11) TN_DECODE_G(12) TN_DECODE_G(13) TN_DECODE_G(14)
    TN_DECODE_G(15) TN_DECODE_G(16)
    default: return TN_EINVAL;
  }
#undef TN_DECODE_G
}

static inline bool al16(const void* p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }

}  // namespace decode
}  // namespace tn

extern "C" {

long long tn_attn_decode_workspace_bytes(int B, int Nh, int Nkv, int D, int S_max) {
  if (B <= 0 || Nh <= 0 || Nkv <= 0 || D <= 0 || S_max <= 0 || Nh % Nkv) return 0;
  const int ns = tn::decode::num_splits(B, Nkv, S_max);
  if (ns == 1) return 0;
  return (long long)B * Nh * ns * (D + 1) * 4;
}

static int decode_entry(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                        const int* cache_len, const int* src, bool beam, void* o, void* workspace, int B, int Nh, int Nkv,
                        int D, int S_max, float scale, void* stream) {
  using namespace tn::decode;
  if (B <= 0 || Nh <= 0 || Nkv <= 0 || S_max <= 0 || (D != 64 && D != 128) || Nh % Nkv || Nh / Nkv > 16) return TN_EINVAL;
  if (!al16(q) || !al16(k_new) || !al16(v_new) || !al16(k_cache) || !al16(v_cache) || !al16(o) || cache_len == nullptr ||
      ((uintptr_t)cache_len & 3))
    return TN_EINVAL;
  if (beam && (src == nullptr || ((uintptr_t)src & 3))) return TN_EINVAL;
  if (num_splits(B, Nkv, S_max) > 1 && !al16(workspace)) return TN_EINVAL;
  const int G = Nh / Nkv;
  hipStream_t st = (hipStream_t)stream;
  return D == 64
             ? dispatch_g<64>(G, q, k_new, v_new, k_cache, v_cache, cache_len, src, o, workspace, B, Nkv, S_max, scale, st)
             : dispatch_g<128>(G, q, k_new, v_new, k_cache, v_cache, cache_len, src, o, workspace, B, Nkv, S_max, scale, st);
}

int tn_attn_decode(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_len,
                   void* o, void* workspace, int B, int Nh, int Nkv, int D, int S_max, float scale, void* stream) {
  return decode_entry(q, k_new, v_new, k_cache, v_cache, cache_len, nullptr, false, o, workspace, B, Nh, Nkv, D, S_max,
                      scale, stream);
}

// as tn_attn_decode on R = B_utt * K rows, reading the cached keys / values through src int32 [R, S_max]
int tn_attn_decode_beam(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                        const int* cache_len, const int* src, void* o, void* workspace, int R, int Nh, int Nkv, int D,
                        int S_max, float scale, void* stream) {
  return decode_entry(q, k_new, v_new, k_cache, v_cache, cache_len, src, true, o, workspace, R, Nh, Nkv, D, S_max, scale,
                      stream);
}

}  // extern "C"
