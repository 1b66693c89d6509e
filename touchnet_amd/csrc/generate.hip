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
#include "decode_step.h"

namespace tn {
namespace greedy {

constexpr int kThreads = 1024;
using namespace step;

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
  fill(seen, banned, h, len, V, penalty != 1.f, ngram, tid, kThreads);

  const T* row = logits + (size_t)b * V;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < V; i += kThreads) {
    float v = Elem<T>::ld(row + i);
    const uint32_t bit = 1u << (i & 31);
    if (seen[i >> 5] & bit) v = penalise(v, penalty);
    if (banned[i >> 5] & bit) v = -INFINITY;
    take(v, i, bv, bi);
  }
  block_argmax(bv, bi, red_v, red_i);
  if (tid == 0) {
    const bool done = finished[b] != 0;
    const int tok = done ? pad : (bi < V ? bi : 0);
    append_token(hist, hist_len, cache_len, finished, n_unfinished, b, S_hist, len, tok, done, tok == eos);
  }
}

}  // namespace greedy
}  // namespace tn

extern "C" {

int tn_greedy_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* finished, int* n_unfinished, int B,
                   int V, int S_hist, float penalty, int ngram, int eos, int pad, int dtype, void* stream) {
  using namespace tn::greedy;
  if (!logits_ok(logits, dtype) || !hist || !hist_len || !cache_len || !finished || !n_unfinished) return TN_EINVAL;
  if (!aligned(3, {hist, hist_len, cache_len, finished, n_unfinished})) return TN_EINVAL;
  if (B <= 0 || V <= 0 || V > kMaxVocab || S_hist <= 0 || ngram < 0 || !(penalty > 0.f)) return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define TN_GREEDY_LAUNCH(T)                                                                                             \
  hipLaunchKernelGGL(greedy_step_kernel<T>, dim3(B), dim3(kThreads), 0, st, (const T*)logits, hist, hist_len, cache_len, \
                     finished, n_unfinished, V, S_hist, penalty, ngram, eos, pad)
  TN_STEP_DISPATCH(dtype, TN_GREEDY_LAUNCH);
#undef TN_GREEDY_LAUNCH
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
