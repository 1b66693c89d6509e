// The two token sets HF's logits processors derive from a row's history, as bitmaps of V bits in LDS — shared by
// tn_greedy_step (generate.hip) and tn_beam_step (beam.hip):
//   seen    RepetitionPenaltyLogitsProcessor: every id of hist[0 .. len)
//   banned  NoRepeatNGramLogitsProcessor(n): every id that would complete an n-gram already in the history
#pragma once
#include "common.h"

namespace tn {
namespace histsets {

constexpr int kMaxVocab = 262144;
constexpr int kWords = kMaxVocab / 32;

// Called by every thread of the workgroup (it synchronises).  `seen` is filled only when use_pen, `banned` only when
// ngram > 0; both are cleared first.
__device__ __forceinline__ void fill(uint32_t* seen, uint32_t* banned, const int* __restrict__ h, int len, int V,
                                     bool use_pen, int ngram, int tid, int nthreads) {
  const int words = (V + 31) / 32;
  for (int w = tid; w < words; w += nthreads) {
    seen[w] = 0u;
    banned[w] = 0u;
  }
  __syncthreads();
  if (use_pen) {
    for (int i = tid; i < len; i += nthreads) {
      const int t = h[i];
      if (t >= 0 && t < V) atomicOr(&seen[t >> 5], 1u << (t & 31));
    }
  }
  if (ngram > 0 && len + 1 >= ngram) {
    // n-grams h[i .. i+n-1] (i + n - 1 < len) whose first n - 1 ids equal the last n - 1 ids of the history
    const int pre = len - (ngram - 1);
    for (int i = tid; i + ngram - 1 < len; i += nthreads) {
      bool match = true;
      for (int j = 0; j < ngram - 1 && match; ++j) match = h[i + j] == h[pre + j];
      if (match) {
        const int t = h[i + ngram - 1];
        if (t >= 0 && t < V) atomicOr(&banned[t >> 5], 1u << (t & 31));
      }
    }
  }
  __syncthreads();
}

}  // namespace histsets
}  // namespace tn
