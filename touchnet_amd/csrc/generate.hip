// One greedy decoding step on the device — the logits processing of HF generate() as the reference calls it
// (touchnet/models/touch_audio/inference_touch_audio.py:177-192: do_sample=False, num_beams=1, repetition_penalty,
// no_repeat_ngram_size, eos / pad), without a host synchronisation:
//
//   l = fp32(logits[b])                                                  (generation/utils.py: .to(torch.float32))
//   RepetitionPenaltyLogitsProcessor: every id in hist[b, :hist_len[b]] once:  l < 0 ? l * p : l / p
//   NoRepeatNGramLogitsProcessor(n): -inf for every id that would complete an n-gram already in the history
//   token = argmax (lowest id on ties, torch.argmax);  a finished row emits `pad`
//   hist[b, hist_len[b]] = token;  hist_len[b]++;  cache_len[b]++;  finished[b] |= token == eos  (then n_unfinished--)
//
// One workgroup per batch row.  The seen-token set is a bitmap of V bits in LDS (16 KB at V = 128256), the banned set a
// second one, filled by a scan of the history against its last n - 1 ids.  The row of logits is read once.
#include "history_sets.h"

namespace tn {
namespace greedy {

constexpr int kThreads = 1024;
using histsets::kMaxVocab;
using histsets::kWords;

template <typename T>
__device__ __forceinline__ float ld(const T* p);
template <>
__device__ __forceinline__ float ld<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ld<bf16_t>(const bf16_t* p) { return bf2f(*p); }

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) greedy_step_kernel(const T* __restrict__ logits, int* __restrict__ hist,
                                                                int* __restrict__ hist_len, int* __restrict__ cache_len,
                                                                int* __restrict__ finished, int* __restrict__ n_unfinished,
                                                                int V, int S_hist, float penalty, int ngram, int eos, int pad) {
  __shared__ uint32_t seen[kWords];
  __shared__ uint32_t banned[kWords];
  __shared__ float red_v[kThreads / 64];
  __shared__ int red_i[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(hist_len[b], 0), S_hist);      // (a length past the row is never read past it)
  const int* h = hist + (size_t)b * S_hist;
  histsets::fill(seen, banned, h, len, V, penalty != 1.f, ngram, tid, kThreads);

  const T* row = logits + (size_t)b * V;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < V; i += kThreads) {
    float v = ld<T>(row + i);
    const uint32_t bit = 1u << (i & 31);
    if (seen[i >> 5] & bit) v = v < 0.f ? v * penalty : v / penalty;
    if (banned[i >> 5] & bit) v = -INFINITY;
    if (better(v, i, bv, bi) || (v != v && bv == bv)) {           // (NaN wins, as in torch.argmax)
      bv = v;
      bi = i;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (better(ov, oi, bv, bi) || (ov != ov && (bv == bv || oi < bi))) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    red_v[tid >> 6] = bv;
    red_i[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    bv = red_v[0];
    bi = red_i[0];
    for (int w = 1; w < kThreads / 64; ++w) {
      const float ov = red_v[w];
      const int oi = red_i[w];
      if (better(ov, oi, bv, bi) || (ov != ov && (bv == bv || oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    const bool done = finished[b] != 0;
    const int tok = done ? pad : (bi < V ? bi : 0);
    if (len < S_hist) {
      hist[(size_t)b * S_hist + len] = tok;
      hist_len[b] = len + 1;
      cache_len[b] += 1;
    }
    if (!done && tok == eos) {
      finished[b] = 1;
      atomicSub(n_unfinished, 1);
    }
  }
}

}  // namespace greedy
}  // namespace tn

extern "C" {

int tn_greedy_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* finished, int* n_unfinished, int B,
                   int V, int S_hist, float penalty, int ngram, int eos, int pad, int dtype, void* stream) {
  using namespace tn::greedy;
  if (!logits || !hist || !hist_len || !cache_len || !finished || !n_unfinished) return TN_EINVAL;
  if (((uintptr_t)hist | (uintptr_t)hist_len | (uintptr_t)cache_len | (uintptr_t)finished | (uintptr_t)n_unfinished) & 3)
    return TN_EINVAL;
  if (B <= 0 || V <= 0 || V > kMaxVocab || S_hist <= 0 || ngram < 0 || !(penalty > 0.f) || (dtype != 0 && dtype != 1))
    return TN_EINVAL;
  if ((uintptr_t)logits & (dtype == 0 ? 3 : 1)) return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(greedy_step_kernel<float>, dim3(B), dim3(kThreads), 0, st, (const float*)logits, hist, hist_len,
                       cache_len, finished, n_unfinished, V, S_hist, penalty, ngram, eos, pad);
  else
    hipLaunchKernelGGL(greedy_step_kernel<tn::bf16_t>, dim3(B), dim3(kThreads), 0, st, (const tn::bf16_t*)logits, hist,
                       hist_len, cache_len, finished, n_unfinished, V, S_hist, penalty, ngram, eos, pad);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
