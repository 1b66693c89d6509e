// The rules the decode step kernels share, each written once — tn_greedy_step (generate.hip), tn_sample_step (sample.hip),
// tn_kimi_text_step (kimi_step.hip), tn_beam_step (beam.hip), tn_token_scores (token_scores.hip) and tn_logits_constrain
// (constrain.hip): the vocabulary bound, the order of (value, id) pairs, torch.argmax and its workgroup reduction, the
// repetition penalty, the history's bitmaps, the Philox draw of a row and step, the append of a token, and the argument
// checks of the C entries.  Nothing here knows which kernel calls it.
#pragma once
#include <initializer_list>
#include "common.h"

namespace tn {
namespace step {

constexpr int kMaxVocab = 262144;
constexpr int kWords = kMaxVocab / 32;         // a bitmap of kMaxVocab bits in LDS: 32 KB

typedef unsigned long long u64;

// larger value first, the lower id on ties (a total order on pairs of distinct ids, NaN aside).  Here and in `take` the
// comparisons are joined with | and &, not || and &&: nothing is skipped, so the per-element loops that call them are
// straight-line code (five compares, two selects) instead of a nest of exec-mask regions.
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return (v > bv) | ((v == bv) & (i < bi)); }

// torch.argmax's merge of (v, i) into the running best: NaN wins, the lowest id among NaNs — whatever order the pairs
// arrive in (a thread's ascending stride, a wave's xor tree, the waves' slots)
__device__ __forceinline__ void take(float v, int i, float& bv, int& bi) {
  const bool win = better(v, i, bv, bi) | ((v != v) & ((bv == bv) | (i < bi)));
  bv = win ? v : bv;
  bi = win ? i : bi;
}

// Workgroup argmax (`take`) of one pair per thread of a 1024-thread workgroup: xor tree in the wave, one slot per wave in
// red_v / red_i (16 each, LDS), every thread scans the 16 and gets the result.  The barrier in front lets a loop call it
// again on the same slots.
__device__ __forceinline__ void block_argmax(float& bv, int& bi, float* red_v, int* red_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    take(ov, oi, bv, bi);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red_v[threadIdx.x >> 6] = bv;
    red_i[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = red_v[0];
  bi = red_i[0];
  for (int w = 1; w < 16; ++w) take(red_v[w], red_i[w], bv, bi);
}

// RepetitionPenaltyLogitsProcessor on one score of a seen id
__device__ __forceinline__ float penalise(float v, float p) { return v < 0.f ? v * p : v / p; }

// seen |= the ids of h[first .. last) that lie in [0, V), thread tid of nthreads taking every nthreads-th.  Clearing the
// bitmap before and the barrier after are the caller's.  (h carries no __restrict__ of its own: a second no-alias scope
// inside `fill`, whose h has one, made the compiler lay out fill's callers differently.)
__device__ __forceinline__ void mark_seen(uint32_t* seen, const int* h, int first, int last, int V, int tid, int nthreads) {
  for (int i = first + tid; i < last; i += nthreads) {
    const int t = h[i];
    if (t >= 0 && t < V) atomicOr(&seen[t >> 5], 1u << (t & 31));
  }
}

// The two token sets HF's logits processors derive from a row's history, as bitmaps of V bits in LDS:
//   seen    RepetitionPenaltyLogitsProcessor: every id of h[0 .. len)
//   banned  NoRepeatNGramLogitsProcessor(n): every id that would complete an n-gram already in the history
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
  if (use_pen) mark_seen(seen, h, 0, len, V, tid, nthreads);
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

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * c[0];
    const u64 p1 = (u64)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// The uniform of row b at history length len, in [0, 1]: uniforms[b] when the caller supplies them, else 53 bits of
// Philox keyed by the seed with counter (len, row_key[b]) — the row's own index without row_key — so that an utterance
// draws the same numbers in any batch.
__device__ __forceinline__ double row_uniform(const float* __restrict__ uniforms, const long long* __restrict__ row_key,
                                              int b, int len, uint32_t seed_lo, uint32_t seed_hi) {
  double u;
  if (uniforms) {
    u = (double)uniforms[b];
  } else {
    const u64 key = row_key ? (u64)row_key[b] : (u64)b;
    uint32_t ctr[4] = {(uint32_t)len, (uint32_t)key, (uint32_t)(key >> 32), 0u};
    philox4x32_10(ctr, seed_lo, seed_hi);
    u = (double)(((u64)ctr[0] << 21) ^ (u64)(ctr[1] >> 11)) * 0x1p-53;
  }
  return fmin(fmax(u, 0.0), 1.0);
}

// The bookkeeping of one emitted token, by one thread of row b's workgroup: a row with room (len < S_hist) appends and
// advances both lengths; a live row (!done) that emitted an eos is marked finished.
__device__ __forceinline__ void append_token(int* __restrict__ hist, int* __restrict__ hist_len, int* __restrict__ cache_len,
                                             int* __restrict__ finished, int* __restrict__ n_unfinished, int b, int S_hist,
                                             int len, int tok, bool done, bool is_eos) {
  if (len < S_hist) {
    hist[(size_t)b * S_hist + len] = tok;
    hist_len[b] = len + 1;
    cache_len[b] += 1;
  }
  if (!done && is_eos) {
    finished[b] = 1;
    atomicSub(n_unfinished, 1);
  }
}

// ------------------------------------------------------------------------------------------------ host: the C entries
// every pointer of the list is a multiple of mask + 1 (a null pointer is: whether it may be null is the entry's rule)
inline bool aligned(uintptr_t mask, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & mask) == 0;
}

// dtype names fp32 (0) or bf16 (1), and logits is a non-null pointer to elements of it
inline bool logits_ok(const void* logits, int dtype) {
  return (dtype == 0 || dtype == 1) && logits != nullptr && aligned(dtype == 0 ? 3 : 1, {logits});
}

// LAUNCH(T) once, with T the element type dtype names (logits_ok has passed)
#define TN_STEP_DISPATCH(dtype, LAUNCH) \
  do {                                  \
    if ((dtype) == 0) {                 \
      LAUNCH(float);                    \
    } else {                            \
      LAUNCH(tn::bf16_t);               \
    }                                   \
  } while (0)

}  // namespace step
}  // namespace tn
