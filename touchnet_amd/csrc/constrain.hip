// Hotword biasing and forbidden sequences on the device — transformers' SequenceBiasLogitsProcessor and
// MinNewTokensLengthLogitsProcessor (generation/logits_process.py), the knobs `sequence_bias` and `min_new_tokens` that a
// checkpoint's generation_config.json may carry (touchnet/models/qwen2_audio/inference_qwen2_audio.py hands the file to
// model.generate()).  HF loops over the biased sequences on the host, a handful of torch ops per sequence per step; here
// the matching is one launch over state the decoder already keeps on the device (hist, hist_len).  No host synchronisation.
//
// The table (built once per generate() call on the host, generation.ConstraintPlan):
//   seq_off int [n_seq + 1], seq_ids int [n_ids]   the sequences' ids, packed
//   seq_bias float [n_seq]                         their biases (finite or -inf)
//   grp_off int [n_grp + 1], grp_tok int [n_grp]   groups of sequences that share their LAST id, grp_tok ascending; within a
//                                                  group the length-1 sequence first, then the longer ones in dict order:
//                                                  HF's order of summation
//   grp_eos int [n_grp]                            1: grp_tok is an eos id (a group may hold no sequence at all)
//
// One workgroup per logits row.  Phase 1, one thread per sequence, strided: the sequence of length L matches history row r
// of n ids when L == 1, or L <= n and hist[r, n-L+1 .. n-1] equals its first L - 1 ids (compared from the newest id
// backwards: a mismatch leaves at the first id).  One byte per sequence in LDS.  Phase 2, one thread per group, strided: the
// owner adds the biases of the group's matching sequences in listed order (plain fp32 additions: nothing to contract or
// reassociate), and replaces the total by -inf for an eos id while fewer than min_new ids were generated.  Every target id
// has exactly one writer: no atomics, and the result depends on the inputs alone.
//   apply  logits[row, t] = T(fp32(logits[row, t]) + total), only where a sequence matched or the eos rule holds
//   emit   edit_ids[row, g] = t where that is so, else -1 - t;  edit_val[row, g] = total;  edit_cnt[row] = active groups
// Finished rows (greedy, sampling) and rows of done utterances (beam) are edited like any other: the step kernels ignore them.
#include "decode_step.h"

namespace tn {
namespace constrain {

using step::aligned;
using step::kMaxVocab;
using step::logits_ok;

constexpr int kThreads = 256;
constexpr int kMaxSeqs = 16384;
constexpr int kMaxLen = 64;

template <typename T, bool kApply>
__global__ void __launch_bounds__(kThreads) constrain_kernel(
    T* __restrict__ logits, const int* __restrict__ hist, const int* __restrict__ hist_len,
    const int* __restrict__ prompt_len, const int* __restrict__ seq_off, const int* __restrict__ seq_ids,
    const float* __restrict__ seq_bias, const int* __restrict__ grp_off, const int* __restrict__ grp_tok,
    const int* __restrict__ grp_eos, int* __restrict__ edit_ids, float* __restrict__ edit_val, int* __restrict__ edit_cnt,
    int K, int K_in, int V, int S_hist, int n_seq, int n_ids, int n_grp, int min_new) {
  __shared__ unsigned char hit[kMaxSeqs];
  __shared__ float red[kThreads / 64];
  const int row_in = blockIdx.x, tid = threadIdx.x;
  const int r = (row_in / K_in) * K + row_in % K_in;
  const int n = min(max(hist_len[r], 0), S_hist);
  const int* __restrict__ h = hist + (size_t)r * S_hist;

  for (int s = tid; s < n_seq; s += kThreads) {
    const int o = seq_off[s], L = seq_off[s + 1] - o;
    bool m = L >= 1 && L <= kMaxLen && o >= 0 && o + L <= n_ids && (L == 1 || L <= n);
    for (int j = L - 2; j >= 0 && m; --j) m = h[n - L + 1 + j] == seq_ids[o + j];
    hit[s] = m;
  }
  __syncthreads();

  const bool hold_eos = min_new > 0 && n - prompt_len[r] < min_new;
  int active_groups = 0;
  for (int g = tid; g < n_grp; g += kThreads) {
    const int s0 = max(grp_off[g], 0), s1 = min(grp_off[g + 1], n_seq);
    float total = 0.f;
    bool active = false;
    for (int s = s0; s < s1; ++s)
      if (hit[s]) {
        total += seq_bias[s];
        active = true;
      }
    if (hold_eos && grp_eos[g] != 0) {
      total = -INFINITY;
      active = true;
    }
    const int t = grp_tok[g];
    if (t < 0 || t >= V) active = false;
    if (kApply) {
      if (active) {
        T* p = logits + (size_t)row_in * V + t;
        Elem<T>::st(p, Elem<T>::ld(p) + total);
      }
    } else {
      edit_ids[(size_t)row_in * n_grp + g] = active ? t : -1 - t;
      edit_val[(size_t)row_in * n_grp + g] = total;
      active_groups += active;
    }
  }
  if (!kApply) {
    const float c = block_sum((float)active_groups, red);      // (<= 16392: exact)
    if (tid == 0) edit_cnt[row_in] = (int)c;
  }
}

}  // namespace constrain
}  // namespace tn

extern "C" {

int tn_logits_constrain(void* logits, const int* hist, const int* hist_len, const int* prompt_len, const int* seq_off,
                        const int* seq_ids, const float* seq_bias, const int* grp_off, const int* grp_tok,
                        const int* grp_eos, int* edit_ids, float* edit_val, int* edit_cnt, int R_in, int K, int K_in, int V,
                        int S_hist, int n_seq, int n_ids, int n_grp, int min_new, int mode, int dtype, void* stream) {
  using namespace tn::constrain;
  if (R_in <= 0 || K < 1 || (K_in != 1 && K_in != K) || R_in % K_in != 0 || V < 1 || V > kMaxVocab || S_hist <= 0 ||
      n_seq < 0 || n_seq > kMaxSeqs || n_ids < n_seq || (long long)n_ids > (long long)kMaxSeqs * kMaxLen || n_grp < 1 ||
      n_grp > n_seq + 8 || min_new < 0 || (mode != 0 && mode != 1) || (dtype != 0 && dtype != 1))
    return TN_EINVAL;
  if (!hist || !hist_len || !seq_off || !grp_off || !grp_tok || !grp_eos) return TN_EINVAL;
  if (n_seq > 0 && (seq_ids == nullptr || seq_bias == nullptr)) return TN_EINVAL;
  if (min_new > 0 && prompt_len == nullptr) return TN_EINVAL;
  if (!aligned(3, {hist, hist_len, seq_off, grp_off, grp_tok, grp_eos, seq_ids, seq_bias, prompt_len})) return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define TN_CONSTRAIN_ARGS                                                                                              \
  hist, hist_len, prompt_len, seq_off, seq_ids, seq_bias, grp_off, grp_tok, grp_eos, edit_ids, edit_val, edit_cnt, K, K_in, \
      V, S_hist, n_seq, n_ids, n_grp, min_new
  if (mode == 0) {
    if (!logits_ok(logits, dtype)) return TN_EINVAL;
#define TN_CONSTRAIN_APPLY(T) \
  hipLaunchKernelGGL((constrain_kernel<T, true>), dim3(R_in), dim3(kThreads), 0, st, (T*)logits, TN_CONSTRAIN_ARGS)
    TN_STEP_DISPATCH(dtype, TN_CONSTRAIN_APPLY);
#undef TN_CONSTRAIN_APPLY
  } else {
    if (!edit_ids || !edit_val || !edit_cnt || !aligned(3, {edit_ids, edit_val, edit_cnt})) return TN_EINVAL;
    hipLaunchKernelGGL((constrain_kernel<float, false>), dim3(R_in), dim3(kThreads), 0, st, (float*)nullptr,
                       TN_CONSTRAIN_ARGS);
  }
#undef TN_CONSTRAIN_ARGS
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
