// Per-token confidences of a decoder: what transformers' compute_transition_scores(normalize_logits=True) gives for the
// chosen token of a [R, V] logits matrix, plus the row's entropy and its k most likely tokens — one pass family over the
// logits the step kernels (generate.hip, sample.hip, kimi_step.hip) already consume, or over thousands of rows of a
// teacher-forced rescoring forward.
//
//   m = max_v l_v                      d_v = l_v - m                     e_v = exp(d_v)   (a -inf logit: 0, skipped)
//   s = sum_v e_v                      w = sum_v e_v d_v
//   logp(t) = d_t - log s              entropy = log s - w / s           (= lse - sum_v p_v l_v; m cancels)
//   alternatives: the k largest (l_v, lower id first on ties), each with its logp
//
// One workgroup per row.  Which thread sums which element depends on the element's INDEX alone: thread t owns the chunks
// c = t, t + 1024, ... of N consecutive ids (N = 16 bytes of T), sums them in ascending order, then a fixed xor tree in
// the wave and the 16 wave partials in order.  A row therefore gives the same bits in any batch and at any address.  A
// chunk is one 16-byte load when the row's address allows it (every row when V * sizeof(T) is a multiple of 16: the real
// vocabularies) and N scalar loads otherwise (odd V: a bf16 row may sit on any 2-byte boundary); the last, partial chunk
// is always scalar.  Two passes over the row (the maximum, then the sums); the second one hits the L2.
// The alternatives ride on the second pass.  After the first, every wave knows the largest logit of its own chunks; the
// k-th largest of those 16 values (tau) is a lower bound of the row's k-th largest logit (k distinct logits reach it), so
// only logits >= tau can be among the k best: a few dozen per row unless the row is flat.  A thread keeps its own best 8 of them (sorted; the
// insertion sits behind one wave-uniform test per chunk, "does any lane's chunk reach tau", so the common path pays one
// max per logit), and k rounds of "best head of all lists" merge them.  A flat row (everything >= tau) takes the
// insertion path everywhere: slower, the same result.
// No atomics; nothing is written but the outputs.
#include "decode_step.h"

namespace tn {
namespace tokscore {

using namespace step;

constexpr int kThreads = 1024;
constexpr int kMaxAlt = 8;
constexpr int kNone = 0x7fffffff;        // id of an empty candidate slot

// the best (value, id) pair of the workgroup, handed to every thread — by `better` alone, a total order on pairs with
// distinct ids and no NaN (a row with a NaN is flagged `sick` before this runs), not step::block_argmax's torch.argmax
__device__ __forceinline__ void block_best_finite(float& bv, int& bi, float* red_v, int* red_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red_v[threadIdx.x >> 6] = bv;
    red_i[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = red_v[0];
  bi = red_i[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) {
    const float ov = red_v[w];
    const int oi = red_i[w];
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
}

// ids [base, base + N) of the row as fp32; ids >= V read as -inf (they add nothing and are never candidates)
template <typename T>
__device__ __forceinline__ void load_chunk(const T* __restrict__ row, int base, int V, bool vec, float (&f)[Vec16<T>::N]) {
  constexpr int N = Vec16<T>::N;
  if (vec && base + N <= V) {
    Vec16<T> x;
    x.load(row + base);
    x.unpack(f);
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e) f[e] = base + e < V ? Elem<T>::ld(row + base + e) : -INFINITY;
  }
}

template <typename T, bool ALT>
__global__ void __launch_bounds__(kThreads) token_scores_kernel(const T* __restrict__ logits, const int* __restrict__ tok,
                                                                 const int* __restrict__ hist,
                                                                 const int* __restrict__ hist_len, float* __restrict__ logp,
                                                                 float* __restrict__ entropy, int* __restrict__ alt_id,
                                                                 float* __restrict__ alt_logp, int V, int S_hist, int k) {
  constexpr int N = Vec16<T>::N;
  __shared__ float red[kThreads / 64];
  __shared__ float red_v[kThreads / 64];
  __shared__ int red_i[kThreads / 64];
  const int r = blockIdx.x, tid = threadIdx.x;

  int t;
  size_t out;                                  // the row's slot in logp / entropy (alternatives: out * k)
  if (tok != nullptr) {
    t = tok[r];
    out = (size_t)r;
  } else {
    const int n = hist_len[r];
    if (n < 1 || n > S_hist) return;           // (the whole workgroup: nothing is written)
    t = hist[(size_t)r * S_hist + n - 1];
    out = (size_t)r * S_hist + (n - 1);
  }

  const T* row = logits + (size_t)r * V;
  const bool vec = ((uintptr_t)row & 15) == 0;
  const int chunks = (V + N - 1) / N;

  // ---- pass 1: the maximum (every thread's own, then the row's) and the unhealthy values
  float own = -INFINITY;
  int sick = 0;
  for (int c = tid; c < chunks; c += kThreads) {
    float f[N];
    load_chunk<T>(row, c * N, V, vec, f);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      sick |= (f[e] != f[e]) || (f[e] == INFINITY);
      own = fmaxf(own, f[e]);
    }
  }
  const float m = block_max(own, red);                                 // (leaves the 16 waves' maxima in red[])

  // tau: the k-th largest of the waves' maxima (k <= 8 of 16; -inf when fewer than k waves own anything) — every thread
  // selects it from red[] by itself: no round trip
  float tau = -INFINITY;
  if (ALT) {
    float wm[kThreads / 64];
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) wm[i] = red[i];
    for (int j = 0; j < k; ++j) {
      float b = wm[0];
      int at = 0;
#pragma unroll
      for (int i = 1; i < kThreads / 64; ++i) {
        if (wm[i] > b) {
          b = wm[i];
          at = i;
        }
      }
      tau = b;
#pragma unroll
      for (int i = 0; i < kThreads / 64; ++i) wm[i] = i == at ? -INFINITY : wm[i];
    }
  }
  const bool bad = __syncthreads_or(sick) != 0 || m == -INFINITY;      // NaN, +inf, or nothing but -inf

  // every thread's own best kMaxAlt candidates (sorted, best first)
  float tv[kMaxAlt];
  int ti[kMaxAlt];
#pragma unroll
  for (int j = 0; j < kMaxAlt; ++j) {
    tv[j] = -INFINITY;
    ti[j] = kNone;
  }

  // ---- pass 2: s and w, every thread its chunks in ascending order; the candidates on the way
  float log_s = NAN, ent = NAN;
  if (!bad) {
    float s = 0.f, w = 0.f;
    for (int c = tid; c < chunks; c += kThreads) {
      float f[N];
      load_chunk<T>(row, c * N, V, vec, f);
      float top = f[0];
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float v = f[e];
        top = fmaxf(top, v);
        if (v > -INFINITY) {
          const float d = v - m;
          const float ex = expf(d);
          s += ex;
          w = fmaf(ex, d, w);
        }
      }
      // a wave-uniform branch (so that it stays a branch): some lane's chunk holds a logit that may be among the k best
      if (ALT && __ballot(top >= tau) != 0) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const float v = f[e];
          const int i = c * N + e;
          if (v >= tau && i < V && better(v, i, tv[kMaxAlt - 1], ti[kMaxAlt - 1])) {
            tv[kMaxAlt - 1] = v;
            ti[kMaxAlt - 1] = i;
#pragma unroll
            for (int j = kMaxAlt - 1; j > 0; --j) {
              if (better(tv[j], ti[j], tv[j - 1], ti[j - 1])) {
                const float sv = tv[j];
                const int si = ti[j];
                tv[j] = tv[j - 1];
                ti[j] = ti[j - 1];
                tv[j - 1] = sv;
                ti[j - 1] = si;
              }
            }
          }
        }
      }
    }
    s = block_sum(s, red);
    w = block_sum(w, red);
    log_s = logf(s);
    ent = log_s - w / s;
  }

  if (tid == 0) {
    float lp = NAN;
    if (!bad && t >= 0 && t < V) lp = (Elem<T>::ld(row + t) - m) - log_s;
    logp[out] = lp;
    entropy[out] = ent;
  }

  // ---- the k best of the row: k rounds of "the best head of all lists", the winner's owner pops it
  if (ALT) {
    float my_v = -INFINITY;
    int my_i = kNone;
    for (int j = 0; j < k; ++j) {
      float bv = tv[0];
      int bi = ti[0];
      block_best_finite(bv, bi, red_v, red_i);
      if (tid == j) {
        my_v = bv;
        my_i = bi;
      }
      if (bi != kNone && ti[0] == bi) {          // (ids are unique: exactly one owner)
#pragma unroll
        for (int q = 0; q < kMaxAlt - 1; ++q) {
          tv[q] = tv[q + 1];
          ti[q] = ti[q + 1];
        }
        tv[kMaxAlt - 1] = -INFINITY;
        ti[kMaxAlt - 1] = kNone;
      }
    }
    if (tid < k) {
      int id = -1;
      float lp = -INFINITY;                      // (k > V: the tail)
      if (bad) {
        lp = NAN;
      } else if (my_i != kNone) {
        id = my_i;
        lp = (my_v - m) - log_s;
      }
      alt_id[out * k + tid] = id;
      alt_logp[out * k + tid] = lp;
    }
  }
}

template <typename T>
int launch(const void* logits, const int* tok, const int* hist, const int* hist_len, float* logp, float* entropy,
           int* alt_id, float* alt_logp, int R, int V, int S_hist, int k, hipStream_t st) {
  if (k > 0)
    hipLaunchKernelGGL((token_scores_kernel<T, true>), dim3(R), dim3(kThreads), 0, st, (const T*)logits, tok, hist,
                       hist_len, logp, entropy, alt_id, alt_logp, V, S_hist, k);
  else
    hipLaunchKernelGGL((token_scores_kernel<T, false>), dim3(R), dim3(kThreads), 0, st, (const T*)logits, tok, hist,
                       hist_len, logp, entropy, alt_id, alt_logp, V, S_hist, k);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // namespace tokscore
}  // namespace tn

extern "C" {

int tn_token_scores(const void* logits, const int* tok, const int* hist, const int* hist_len, float* logp, float* entropy,
                    int* alt_id, float* alt_logp, int R, int V, int S_hist, int k, int dtype, void* stream) {
  using namespace tn::tokscore;
  if (!logits_ok(logits, dtype) || !logp || !entropy) return TN_EINVAL;
  if (R < 0 || V < 1 || V > kMaxVocab || k < 0 || k > kMaxAlt) return TN_EINVAL;
  const bool by_tok = tok != nullptr, by_hist = hist != nullptr || hist_len != nullptr;
  if (by_tok == by_hist) return TN_EINVAL;                         // both ways of naming the token, or neither
  if (by_hist && (!hist || !hist_len || S_hist < 1)) return TN_EINVAL;
  if (k > 0 && (!alt_id || !alt_logp)) return TN_EINVAL;
  if (!aligned(3, {tok, hist, hist_len, logp, entropy, alt_id, alt_logp})) return TN_EINVAL;
  if (R == 0) return TN_OK;
  hipStream_t st = (hipStream_t)stream;
  int rc = TN_OK;
#define TN_TOKSCORE_LAUNCH(T) rc = launch<T>(logits, tok, hist, hist_len, logp, entropy, alt_id, alt_logp, R, V, S_hist, k, st)
  TN_STEP_DISPATCH(dtype, TN_TOKSCORE_LAUNCH);
#undef TN_TOKSCORE_LAUNCH
  return rc;
}

}  // extern "C"
