// One sampling (or greedy) decoding step on the device — the logits pipeline of HF generate() in its own order, as
// Qwen2-Audio's generation_config.json asks for it (touchnet/models/qwen2_audio/inference_qwen2_audio.py calls
// model.generate(**inputs, max_length=..., use_cache=True) and leaves every knob to that file):
//
//   l = fp32(logits[b])                                                  (generation/utils.py: .to(torch.float32))
//   RepetitionPenaltyLogitsProcessor: every id in hist[b, :hist_len[b]] once:  l < 0 ? l * p : l / p
//   do_sample:
//     TemperatureLogitsWarper   l / T
//     TopKLogitsWarper          drop l < the k-th largest l (ties at the threshold stay)
//     TopPLogitsWarper          keep a token iff the softmax mass of the tokens strictly above it is < top_p (the
//                               ascending-cumsum rule restated as a threshold); the maximum always stays
//     draw                      u in [0, 1) from Philox4x32-10 keyed by (seed, row_key[b], hist_len[b]); the first kept
//                               token, in id order, whose running sum of exp(l - max) exceeds u * Z_kept
//   else argmax (lowest id on ties, torch.argmax)
//   a finished row emits `pad`;  hist[b, hist_len[b]] = token;  hist_len[b]++;  cache_len[b]++;
//   finished[b] |= token in eos_ids  (then n_unfinished--)          — the bookkeeping of tn_greedy_step
//
// One workgroup (1024 threads) per batch row; the row is re-read from L2 by every pass, nothing is written to HBM but
// the bookkeeping.  Thresholds are found on d = max - l >= 0 (monotone in l):
//   * a selection level histograms the tokens of the current set into 1024 LDS bins — counts (top-k) or masses (top-p);
//     level 0 covers d in [0, 64) in steps of 1/16 (the last bin also takes everything farther below the maximum), every
//     deeper level splits the chosen bin of the level above into 1024.  Binning on d relative to the maximum spreads the
//     tokens of a wave over many bins; the top bits of the raw float keys are the same for most logits of a row (sign and
//     exponent), which would serialise the LDS atomics.
//   * once the chosen bin holds <= 2048 tokens they are gathered into LDS and the threshold is exact there; a bin whose
//     tokens all have one value (bf16 ties) is resolved without gathering.
//   * masses are fixed point, w = exp(-d) * 2^40 in uint64, so every sum is exact and independent of the order of the
//     atomics: the same (seed, row_key, step) draws the same token whatever the batch.  Tokens more than ~28 below the
//     maximum (w = 0) can be kept but are never drawn.
//   * 0 < top_k <= 1024: after top-k the candidates (d <= d_k) are compacted into LDS; top-p and the draw then work on
//     them alone (all-pairs sums over <= 2048 entries).  Otherwise the draw scans the row in id order, one contiguous
//     chunk per thread, with a workgroup prefix sum of the chunk masses.
#include "decode_step.h"

namespace tn {
namespace sample {

using namespace step;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 1024;
constexpr int kCap = 2048;                 // tokens gathered into LDS
constexpr int kMaxEos = 8;
constexpr int kMaxLevels = 8;
constexpr float kStep0 = 16.f;             // level-0 bins per unit of d: [0, 64) over 1024 bins
constexpr float kFix = 1099511627776.f;    // 2^40

struct Params {
  int V, S_hist, do_sample, top_k, n_eos, pad;
  float penalty, temperature, top_p;
  uint32_t seed_lo, seed_hi;
  int eos[kMaxEos];
};

__device__ __forceinline__ u64 weight(float d) { return (u64)(__expf(-d) * kFix); }

struct Smem {
  uint32_t seen[kWords];
  float cd[kCap];                          // gathered tokens: d and id
  int ci[kCap];
  u64 hm[kBins];                           // mass histogram; also the scan scratch of the draw
  uint32_t hc[kBins];                      // count histogram
  float red_f[kWaves];
  int red_i[kWaves];
  u64 red_u[kWaves];
  u64 sh_u[4];
  uint32_t dmin, dmax;                     // float bits of d >= 0 (order-preserving as uint)
  int n_cand, sh_i[4];
};

// --------------------------------------------------------------------------------------------- workgroup reductions
__device__ __forceinline__ u64 block_sum_u64(u64 v, Smem& s) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s.red_u[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 t = 0;
  for (int w = 0; w < kWaves; ++w) t += s.red_u[w];
  return t;
}

// inclusive prefix sum of one value per thread, in thread order; *total = the sum of all
__device__ __forceinline__ u64 block_scan_u64(u64 v, Smem& s, u64* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const u64 o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  __syncthreads();
  if (lane == 63) s.red_u[w] = v;
  __syncthreads();
  u64 before = 0, t = 0;
  for (int j = 0; j < kWaves; ++j) {
    const u64 x = s.red_u[j];
    if (j < w) before += x;
    t += x;
  }
  *total = t;
  return v + before;
}

// ------------------------------------------------------------------------------------------------ the row's values
template <typename T>
struct Row {
  const T* row;
  const uint32_t* seen;
  float penalty, temperature, M;
  bool use_pen, do_sample;
  __device__ __forceinline__ float value(int i) const {
    float v = Elem<T>::ld(row + i);
    if (use_pen && (seen[i >> 5] & (1u << (i & 31)))) v = penalise(v, penalty);
    if (do_sample) v = v / temperature;
    return v;
  }
  __device__ __forceinline__ float dist(int i) const {          // d = M - l >= 0; NaN / -inf logits: +inf
    const float d = M - value(i);
    return d >= 0.f ? d : (d == d ? 0.f : INFINITY);
  }
};

struct Chain {
  int n;
  int bin[kMaxLevels];
  float lo[kMaxLevels], scale[kMaxLevels];
};

__device__ __forceinline__ int bin_of(float d, float lo, float scale) {
  const float x = fminf(fmaxf((d - lo) * scale, 0.f), (float)(kBins - 1));
  return (int)x;
}

__device__ __forceinline__ bool member(float d, const Chain& c) {
  for (int j = 0; j < c.n; ++j)
    if (bin_of(d, c.lo[j], c.scale[j]) != c.bin[j]) return false;
  return true;
}

// Selection over the tokens with d <= dcap.  mass == false (top-k): the largest d among the `rank` smallest d (the k-th
// largest logit; ties stay).  mass == true (top-p): the largest d whose "mass strictly above" is < top_p * Z, Z = the mass
// of all tokens with d <= dcap.  Returns the threshold: keep d <= result.  Every thread gets the result.
template <typename T>
__device__ float select(const Row<T>& r, int V, float dcap, bool mass, int rank, float top_p, Smem& s) {
  const int tid = threadIdx.x;
  Chain c;
  c.n = 0;
  float lo = 0.f, scale = kStep0;
  u64 above = 0;                     // mass of the tokens above the current set (top-p)
  double P = 0.0;
  for (int level = 0;; ++level) {
    s.hc[tid] = 0u;
    s.hm[tid] = 0ull;
    if (tid == 0) {
      s.dmin = 0x7f800000u;
      s.dmax = 0u;
    }
    __syncthreads();
    uint32_t mn = 0x7f800000u, mx = 0u;
    for (int i = tid; i < V; i += kThreads) {
      const float d = r.dist(i);
      if (!(d <= dcap) || !member(d, c)) continue;
      const int b = bin_of(d, lo, scale);
      atomicAdd(&s.hc[b], 1u);
      if (mass) {
        const u64 w = weight(d);
        if (w) atomicAdd(&s.hm[b], w);
      }
      mn = min(mn, __float_as_uint(d));
      mx = max(mx, __float_as_uint(d));
    }
    for (int off = 32; off > 0; off >>= 1) {
      mn = min(mn, (uint32_t)__shfl_xor((int)mn, off, 64));
      mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    }
    if ((tid & 63) == 0) {
      atomicMin(&s.dmin, mn);
      atomicMax(&s.dmax, mx);
    }
    __syncthreads();
    const uint32_t set_min = s.dmin, set_max = s.dmax;
    __syncthreads();
    if (set_min == set_max) return __uint_as_float(set_min);    // one value left (or the whole row tied): it is the threshold
    // the bin holding the threshold
    const u64 cnt = s.hc[tid];
    const u64 own = mass ? s.hm[tid] : cnt;
    u64 total;
    const u64 incl = block_scan_u64(own, s, &total);
    const u64 excl = incl - own;
    if (mass && level == 0) P = (double)top_p * (double)total;
    if (tid == 0) s.sh_i[0] = -1;
    __syncthreads();
    if (mass) {
      if (cnt && (double)(above + excl) < P) atomicMax(&s.sh_i[0], tid);
    } else if (excl < (u64)rank && (u64)rank <= incl) {
      s.sh_i[0] = tid;
    }
    __syncthreads();
    int b = s.sh_i[0];
    if (b < 0) b = 0;                                            // (unreachable: the maximum is in bin 0 with nothing above)
    if (tid == b) {
      s.sh_u[0] = excl;
      s.sh_i[1] = (int)cnt;
    }
    __syncthreads();
    const u64 b_excl = s.sh_u[0];
    const int b_cnt = s.sh_i[1];
    if (mass) above += b_excl;
    else rank -= (int)b_excl;
    if (level == 0 && b == kBins - 1) return INFINITY;          // the far tail (w = 0 there): keep all of it
    c.bin[c.n] = b;
    c.lo[c.n] = lo;
    c.scale[c.n] = scale;
    c.n++;
    if (b_cnt <= kCap || c.n == kMaxLevels) {
      // gather the bin and resolve it exactly
      if (tid == 0) s.n_cand = 0;
      __syncthreads();
      for (int i = tid; i < V; i += kThreads) {
        const float d = r.dist(i);
        if (!(d <= dcap) || !member(d, c)) continue;
        const int slot = atomicAdd(&s.n_cand, 1);
        if (slot < kCap) {
          s.cd[slot] = d;
          s.ci[slot] = i;
        }
      }
      __syncthreads();
      const int n = min(s.n_cand, kCap);
      if (tid == 0) s.dmax = 0u;
      __syncthreads();
      if (s.n_cand > kCap) {                                     // (level cap reached with a wide bin: keep the bin)
        for (int j = tid; j < n; j += kThreads) atomicMax(&s.dmax, __float_as_uint(s.cd[j]));
      } else {
        for (int j = tid; j < n; j += kThreads) {
          const float dj = s.cd[j];
          bool keep;
          if (mass) {
            u64 a = above;
            for (int m = 0; m < n; ++m)
              if (s.cd[m] < dj) a += weight(s.cd[m]);
            keep = (double)a < P;
          } else {
            int lt = 0;
            for (int m = 0; m < n; ++m) lt += s.cd[m] < dj;
            keep = lt < rank;                                    // the k-th smallest d and every d below it
          }
          if (keep) atomicMax(&s.dmax, __float_as_uint(dj));
        }
      }
      __syncthreads();
      const float thr = __uint_as_float(s.dmax);
      __syncthreads();
      return thr;
    }
    lo = lo + (float)b / scale;
    scale = scale * (float)kBins;
    __syncthreads();
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) sample_step_kernel(const T* __restrict__ logits, int* __restrict__ hist,
                                                                int* __restrict__ hist_len, int* __restrict__ cache_len,
                                                                int* __restrict__ finished, int* __restrict__ n_unfinished,
                                                                const long long* __restrict__ row_key,
                                                                const float* __restrict__ uniforms, int* __restrict__ n_kept,
                                                                Params p) {
  __shared__ Smem s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V;
  const int len = min(max(hist_len[b], 0), p.S_hist);
  const bool done = finished[b] != 0;
  int tok = p.pad;
  if (!done) {
    const int* h = hist + (size_t)b * p.S_hist;
    const bool use_pen = p.penalty != 1.f;
    const int words = (V + 31) / 32;
    if (use_pen) {
      for (int w = tid; w < words; w += kThreads) s.seen[w] = 0u;
      __syncthreads();
      mark_seen(s.seen, h, 0, len, V, tid, kThreads);
      __syncthreads();
    }
    Row<T> r{logits + (size_t)b * V, s.seen, p.penalty, p.temperature, 0.f, use_pen, p.do_sample != 0};
    // pass 1: the maximum (argmax with torch.argmax's rules)
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += kThreads) take(r.value(i), i, bv, bi);
    block_argmax(bv, bi, s.red_f, s.red_i);
    tok = bi < V ? bi : 0;
    const bool finite_max = bv == bv && bv > -INFINITY && bv < INFINITY;
    if (p.do_sample && finite_max) {
      r.M = bv;
      const double u = row_uniform(uniforms, row_key, b, len, p.seed_lo, p.seed_hi);
      const int k = (p.top_k > 0 && p.top_k < V) ? p.top_k : 0;
      const bool use_p = p.top_p < 1.f;
      float dk = INFINITY;
      if (k) dk = select(r, V, INFINITY, false, k, 0.f, s);
      bool compact = false;
      if (k && k <= 1024) {                      // compact the top-k candidates into LDS
        if (tid == 0) s.n_cand = 0;
        __syncthreads();
        for (int i = tid; i < V; i += kThreads) {
          const float d = r.dist(i);
          if (!(d <= dk)) continue;
          const int slot = atomicAdd(&s.n_cand, 1);
          if (slot < kCap) {
            s.cd[slot] = d;
            s.ci[slot] = i;
          }
        }
        __syncthreads();
        compact = s.n_cand <= kCap;
      }
      int kept = 0;
      if (compact) {
        const int n = s.n_cand;
        // top-p on the candidates: mass strictly above each one
        u64 zsum = 0;
        for (int j = tid; j < n; j += kThreads) zsum += weight(s.cd[j]);
        const u64 Z = block_sum_u64(zsum, s);
        float dp = INFINITY;
        if (use_p) {
          const double P = (double)p.top_p * (double)Z;
          if (tid == 0) s.dmax = 0u;
          __syncthreads();
          for (int j = tid; j < n; j += kThreads) {
            const float dj = s.cd[j];
            u64 a = 0;
            for (int m = 0; m < n; ++m)
              if (s.cd[m] < dj) a += weight(s.cd[m]);
            if ((double)a < P) atomicMax(&s.dmax, __float_as_uint(dj));
          }
          __syncthreads();
          dp = __uint_as_float(s.dmax);
        }
        // the draw over the kept candidates in id order
        u64 zk = 0;
        int kc = 0;
        for (int j = tid; j < n; j += kThreads)
          if (s.cd[j] <= dp) {
            zk += weight(s.cd[j]);
            ++kc;
          }
        const u64 Zk = block_sum_u64(zk, s);
        kept = (int)block_sum_u64((u64)kc, s);
        u64 target = (u64)(u * (double)Zk);
        if (target >= Zk) target = Zk - 1;
        if (tid == 0) s.sh_i[2] = 0x7fffffff;
        __syncthreads();
        for (int j = tid; j < n; j += kThreads) {
          const float dj = s.cd[j];
          if (!(dj <= dp)) continue;
          const int ij = s.ci[j];
          const u64 wj = weight(dj);
          u64 pre = 0;
          for (int m = 0; m < n; ++m)
            if (s.ci[m] < ij && s.cd[m] <= dp) pre += weight(s.cd[m]);
          if (pre <= target && target < pre + wj) atomicMin(&s.sh_i[2], ij);
        }
        __syncthreads();
        if (s.sh_i[2] != 0x7fffffff) tok = s.sh_i[2];
      } else {
        const float dp = use_p ? select(r, V, dk, true, 0, p.top_p, s) : INFINITY;
        const float dthr = fminf(dk, dp);
        // the draw: one contiguous chunk of ids per thread, prefix sums of the chunk masses in thread order
        const int C = (V + kThreads - 1) / kThreads;
        const int i0 = min(tid * C, V), i1 = min(i0 + C, V);
        u64 own = 0;
        int kc = 0;
        for (int i = i0; i < i1; ++i) {
          const float d = r.dist(i);
          if (d <= dthr) {
            own += weight(d);
            ++kc;
          }
        }
        u64 Zk;
        const u64 incl = block_scan_u64(own, s, &Zk);
        kept = (int)block_sum_u64((u64)kc, s);
        u64 target = (u64)(u * (double)Zk);
        if (Zk && target >= Zk) target = Zk - 1;
        if (tid == 0) s.sh_i[2] = 0x7fffffff;
        __syncthreads();
        u64 run = incl - own;
        if (run <= target && target < incl) {
          for (int i = i0; i < i1; ++i) {
            const float d = r.dist(i);
            if (!(d <= dthr)) continue;
            run += weight(d);
            if (target < run) {
              s.sh_i[2] = i;
              break;
            }
          }
        }
        __syncthreads();
        if (s.sh_i[2] != 0x7fffffff) tok = s.sh_i[2];
      }
      if (n_kept && tid == 0) n_kept[b] = kept;
    } else if (n_kept && tid == 0) {
      n_kept[b] = 1;
    }
  } else if (n_kept && tid == 0) {
    n_kept[b] = 0;
  }
  if (tid == 0) {
    bool is_eos = false;
    for (int e = 0; e < p.n_eos; ++e) is_eos |= tok == p.eos[e];
    append_token(hist, hist_len, cache_len, finished, n_unfinished, b, p.S_hist, len, tok, done, is_eos);
  }
}

}  // namespace sample
}  // namespace tn

extern "C" {

int tn_sample_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* finished, int* n_unfinished,
                   const long long* row_key, const float* uniforms, int* n_kept, int B, int V, int S_hist, float penalty,
                   int do_sample, float temperature, int top_k, float top_p, unsigned long long seed, const int* eos_ids,
                   int n_eos, int pad, int dtype, void* stream) {
  using namespace tn::sample;
  if (!logits_ok(logits, dtype) || !hist || !hist_len || !cache_len || !finished || !n_unfinished) return TN_EINVAL;
  if (!aligned(3, {hist, hist_len, cache_len, finished, n_unfinished, uniforms, n_kept}) || !aligned(7, {row_key}))
    return TN_EINVAL;
  if (B <= 0 || V <= 0 || V > kMaxVocab || S_hist <= 0 || !(penalty > 0.f)) return TN_EINVAL;
  if (n_eos < 0 || n_eos > kMaxEos || (n_eos > 0 && !eos_ids)) return TN_EINVAL;
  if (do_sample && (!(temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f))) return TN_EINVAL;
  Params p;
  p.V = V;
  p.S_hist = S_hist;
  p.do_sample = do_sample ? 1 : 0;
  p.top_k = top_k;
  p.n_eos = n_eos;
  p.pad = pad;
  p.penalty = penalty;
  p.temperature = temperature;
  p.top_p = top_p;
  p.seed_lo = (uint32_t)seed;
  p.seed_hi = (uint32_t)(seed >> 32);
  for (int e = 0; e < kMaxEos; ++e) p.eos[e] = e < n_eos ? eos_ids[e] : -1;
  hipStream_t st = (hipStream_t)stream;
#define TN_SAMPLE_LAUNCH(T)                                                                                             \
  hipLaunchKernelGGL(sample_step_kernel<T>, dim3(B), dim3(kThreads), 0, st, (const T*)logits, hist, hist_len, cache_len, \
                     finished, n_unfinished, row_key, uniforms, n_kept, p)
  TN_STEP_DISPATCH(dtype, TN_SAMPLE_LAUNCH);
#undef TN_SAMPLE_LAUNCH
  TN_LAUNCH_CHECK();
  return TN_OK;
}

// Philox4x32-10 on the host (tests compare the device draws against it)
void tn_philox4x32_10(unsigned int* ctr4, unsigned long long key) {
  tn::step::philox4x32_10(ctr4, (uint32_t)key, (uint32_t)(key >> 32));
}

}  // extern "C"
