// One step of HF's beam search on the device — the vectorised `_beam_search` of transformers (generation/utils.py:
// _get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic), the
// search mode the reference's ASR call switches off by hand (touchnet/models/touch_audio/inference_touch_audio.py:177-192,
// num_beams=1) and Qwen2-Audio's script takes from the checkpoint's generation_config.json.  No host synchronisation.
//
// R = B * K rows; utterance b owns rows b K .. b K + K - 1, of which K_in are live (1 right after the prefill, K afterwards).
// Per utterance, keep = max(2, 1 + n_eos) K:
//
//   lp  = log_softmax(fp32(logits row))                     HF applies its processors to the LOG-PROBABILITIES:
//         repetition penalty over the row's history (lp < 0 ? lp * p : lp / p, each id once), -inf on ids that complete an
//         n-gram of the history;  acc = lp + running_score[row]
//   the top `keep` of the K_in V candidates, descending, ties to the lower flat index row V + id;  parent = row, id
//   hit = id in eos_ids or generated + 1 >= n_new
//   running beams: the first K candidates that did not hit (then, if fewer exist, candidates that hit, at acc - 1e9: HF's
//         rule; it happens only when every candidate hit, which ends the utterance)
//   finished set (K slots: ids, length, score, flag; an empty slot scores -1e9): the candidates among the first K that
//         hit, scored acc / (generated + 1) ^ length_penalty, merged with the held ones; the best K kept, descending
//   unsat &= running_score[0] / L ^ length_penalty > worst slot score   (L = n_new for "never" with a positive penalty,
//         else generated + 1);  done = !unsat, or the set is full under early_stopping = True, or every candidate hit
//   history and table rows are permuted by parent; the id is appended; src[row, cache_len] = parent row; lengths advance
//
// A done utterance is frozen: both kernels leave at once, no byte of its state changes (HF keeps stepping it while other
// utterances run, but masks every candidate out of its finished set: the outputs are equal).  HF's two masks of
// _update_finished_beams (set full under early_stopping, heuristic satisfied) are exactly the conditions that froze the
// utterance one step earlier, so a live utterance never needs them.
//
// Two launches.  beam_topk_kernel, one 1024-thread workgroup per live row: the history's bitmaps (decode_step.h), one pass
// for the row maximum, one for the sum of exponentials, one in which every thread finds the best of its strided
// candidates as a 64-bit key (order-preserving bits of acc, then the inverted index: all keys differ, ties cost nothing);
// then `keep` rounds of a workgroup argmax, after each of which only the winner's owner rescans its candidates.  The
// sorted (acc, id) pairs go to a workspace of 32 pairs per row: no [R, V] intermediate.  beam_book_kernel, one workgroup per
// utterance: thread 0 merges the K_in sorted lists and does the bookkeeping in LDS, then every thread owns columns of the
// history, the table and the finished set, reads the K entries of its column and writes them permuted (no second buffer).
//
// tn_beam_step_edits: the same two kernels with the per-row edit list of tn_logits_constrain (constrain.hip: sequence_bias
// and min_new_tokens).  HF's SequenceBiasLogitsProcessor is the first of the processors, so lp = log_softmax(..) + total,
// then the penalty, then the ban.  beam_topk_kernel is a template on kEdits: without a list the instantiation that runs is
// the one tn_beam_step always ran.
#include "decode_step.h"

namespace tn {
namespace beam {

constexpr int kThreads = 1024;
constexpr int kBookThreads = 256;
constexpr int kMaxK = 8;
constexpr int kMaxEos = 3;
constexpr int kMaxKeep = 32;
constexpr float kMasked = -1.0e9f;        // HF's "cannot be chosen" score

struct Eos {
  int n;
  int id[kMaxEos];
};

__device__ __forceinline__ uint32_t ordered_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float from_ordered(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ unsigned long long make_key(float v, int idx) {
  return ((unsigned long long)ordered_bits(v) << 32) | (uint32_t)(0x7fffffff - idx);
}
__device__ __forceinline__ unsigned long long max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// The optional per-row edit list of tn_logits_constrain's emit mode (constrain.hip): n slots in ascending order of their
// distinct ids; ids[s] >= 0: val[s] is added to the log-probability of that id; ids[s] = -1 - id: the slot is idle this
// step; cnt: the active slots of the row (0: the index below stays empty).
struct Edits {
  const int* ids;
  const float* val;
  const int* cnt;
  int n;
};

// The slots' ids as a bitmap of V bits (`edited`, active or idle alike) and, per word, the number of slots with a lower id
// (`rank`): the slot of id i is rank[i >> 5] + popc(the word's bits below i) — no search, no dependent loads.  Called by
// every thread of the workgroup (it synchronises).
__device__ __forceinline__ void fill_edit_index(uint32_t* edited, uint16_t* rank, uint32_t* wave_total,
                                                const int* __restrict__ ids, int n, int V, int tid) {
  const int words = (V + 31) / 32;
  for (int w = tid; w < words; w += kThreads) edited[w] = 0u;
  __syncthreads();
  for (int s = tid; s < n; s += kThreads) {
    const int e = ids[s], t = e >= 0 ? e : -1 - e;
    if (t >= 0 && t < V) atomicOr(&edited[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
  const int per = (words + kThreads - 1) / kThreads, w0 = tid * per, w1 = min(w0 + per, words);
  int own = 0;
  for (int w = w0; w < w1; ++w) own += __popc(edited[w]);
  int incl = own;
  const int lane = tid & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wave_total[tid >> 6] = (uint32_t)incl;
  __syncthreads();
  int before = incl - own;
  for (int i = 0; i < (tid >> 6); ++i) before += (int)wave_total[i];
  for (int w = w0; w < w1; ++w) {
    rank[w] = (uint16_t)before;
    before += __popc(edited[w]);
  }
  __syncthreads();
}

// acc of candidate i: HF's arithmetic, every operation rounded on its own.  kEdits: SequenceBiasLogitsProcessor comes
// first in HF's processor list, so the total is added to the log-probability before the penalty divides or multiplies.
template <typename T, bool kEdits>
__device__ __forceinline__ float candidate(const T* __restrict__ row, int i, float mx, float lse, const uint32_t* seen,
                                           const uint32_t* banned, float penalty, float base, const uint32_t* edited,
                                           const uint16_t* rank, const int* __restrict__ e_ids,
                                           const float* __restrict__ e_val) {
#pragma clang fp contract(off)
  float lp = (Elem<T>::ld(row + i) - mx) - lse;
  const uint32_t bit = 1u << (i & 31);
  if (kEdits) {
    const uint32_t word = edited[i >> 5];
    if (word & bit) {
      const int slot = rank[i >> 5] + __popc(word & (bit - 1u));
      if (e_ids[slot] >= 0) lp = lp + e_val[slot];
    }
  }
  if (seen[i >> 5] & bit) lp = step::penalise(lp, penalty);
  if (banned[i >> 5] & bit) lp = -INFINITY;
  return (lp + base) + 0.f;                                  // (+ 0: no -0 among the keys)
}

template <typename T, bool kEdits>
__global__ void __launch_bounds__(kThreads) beam_topk_kernel(const T* __restrict__ logits, const int* __restrict__ hist,
                                                              const int* __restrict__ hist_len,
                                                              const float* __restrict__ run_score,
                                                              const int* __restrict__ done, float* __restrict__ ws_val,
                                                              int* __restrict__ ws_idx, int K, int K_in, int V, int S_hist,
                                                              float penalty, int ngram, int keep, Edits edits) {
  __shared__ uint32_t seen[step::kWords];
  __shared__ uint32_t banned[step::kWords];
  __shared__ uint32_t edited[kEdits ? step::kWords : 1];   // (with the two above and `rank`: 112 KB of the CU's 160,
  __shared__ uint16_t rank[kEdits ? step::kWords : 1];     // so one workgroup per CU; a step launches at most B K)
  __shared__ uint32_t wave_total[kThreads / 64];
  __shared__ float red[kThreads / 64];
  __shared__ unsigned long long red_key[kThreads / 64];
  const int row_in = blockIdx.x, tid = threadIdx.x;
  const int b = row_in / K_in, r = b * K + row_in % K_in;
  if (done[b] != 0) return;
  const int len = min(max(hist_len[r], 0), S_hist);
  step::fill(seen, banned, hist + (size_t)r * S_hist, len, V, penalty != 1.f, ngram, tid, kThreads);
  const int* __restrict__ e_ids = kEdits ? edits.ids + (size_t)row_in * edits.n : nullptr;
  const float* __restrict__ e_val = kEdits ? edits.val + (size_t)row_in * edits.n : nullptr;
  if (kEdits) fill_edit_index(edited, rank, wave_total, e_ids, edits.cnt[row_in] > 0 ? edits.n : 0, V, tid);

  const T* row = logits + (size_t)row_in * V;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += kThreads) mx = fmaxf(mx, Elem<T>::ld(row + i));
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int i = tid; i < V; i += kThreads) sum += expf(Elem<T>::ld(row + i) - mx);
  sum = block_sum(sum, red);
  const float lse = logf(sum);
  const float base = run_score[r];

  unsigned long long best = 0ull;                            // (no candidate: every real key is larger)
  for (int i = tid; i < V; i += kThreads)
    best = max_u64(best, make_key(candidate<T, kEdits>(row, i, mx, lse, seen, banned, penalty, base, edited, rank, e_ids, e_val), i));

  for (int round = 0; round < keep; ++round) {
    unsigned long long w = best;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)w, off, 64);
      const uint32_t hi = __shfl_xor((uint32_t)(w >> 32), off, 64);
      w = max_u64(w, ((unsigned long long)hi << 32) | lo);
    }
    if ((tid & 63) == 0) red_key[tid >> 6] = w;
    __syncthreads();
    unsigned long long top = red_key[0];
#pragma unroll
    for (int i = 1; i < kThreads / 64; ++i) top = max_u64(top, red_key[i]);
    __syncthreads();
    const int idx = 0x7fffffff - (int)(uint32_t)(top & 0xffffffffu);
    if (tid == 0) {
      ws_val[(size_t)row_in * kMaxKeep + round] = from_ordered((uint32_t)(top >> 32));
      ws_idx[(size_t)row_in * kMaxKeep + round] = idx;
    }
    if (best == top) {                                       // the owner: its next best below the one just taken
      unsigned long long nb = 0ull;
      for (int i = tid; i < V; i += kThreads) {
        const unsigned long long k = make_key(candidate<T, kEdits>(row, i, mx, lse, seen, banned, penalty, base, edited, rank, e_ids, e_val), i);
        if (k < top) nb = max_u64(nb, k);
      }
      best = nb;
    }
  }
}

__global__ void __launch_bounds__(kBookThreads) beam_book_kernel(
    const float* __restrict__ ws_val, const int* __restrict__ ws_idx, int* __restrict__ hist, int* __restrict__ hist_len,
    int* __restrict__ cache_len, int* __restrict__ src, float* __restrict__ run_score, int* __restrict__ fin_ids,
    int* __restrict__ fin_len, float* __restrict__ fin_score, int* __restrict__ fin_flag, int* __restrict__ gen,
    int* __restrict__ unsat, int* __restrict__ done, int* __restrict__ n_unfinished, int* __restrict__ out_ids,
    int* __restrict__ out_parent, int K, int K_in, int V, int S_hist, int keep, Eos eos, int n_new, float length_penalty,
    int early) {
  __shared__ float c_val[kMaxKeep];
  __shared__ int c_parent[kMaxKeep], c_id[kMaxKeep], c_hit[kMaxKeep];
  __shared__ int pos[kMaxK], s_parent[kMaxK], s_id[kMaxK], s_fsrc[kMaxK];
  __shared__ float h_score[kMaxK];
  __shared__ int h_flag[kMaxK], h_len[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, r0 = b * K;
  if (done[b] != 0) return;
  const int len = hist_len[r0], cl = cache_len[r0];
  if (len < 1 || len >= S_hist || cl < 0 || cl >= S_hist) return;      // no room to append: the caller grows the state first
  __syncthreads();                          // every thread has read done / the lengths before thread 0 rewrites them

  if (tid == 0) {
    // merge the K_in sorted lists: the larger acc first, the lower row on ties (the lower flat index)
    for (int k = 0; k < K_in; ++k) pos[k] = 0;
    for (int n = 0; n < keep; ++n) {
      int bk = -1;
      float bv = 0.f;
      for (int k = 0; k < K_in; ++k) {
        if (pos[k] >= keep) continue;
        const float v = ws_val[(size_t)(b * K_in + k) * kMaxKeep + pos[k]];
        if (bk < 0 || v > bv) {
          bk = k;
          bv = v;
        }
      }
      c_val[n] = bv;
      c_parent[n] = bk;
      c_id[n] = ws_idx[(size_t)(b * K_in + bk) * kMaxKeep + pos[bk]];
      pos[bk] += 1;
    }
    const int g1 = gen[b] + 1;
    const bool budget = g1 >= n_new;
    int n_open = 0;
    for (int n = 0; n < keep; ++n) {
      bool hit = budget;
#pragma unroll
      for (int e = 0; e < kMaxEos; ++e) hit |= e < eos.n && c_id[n] == eos.id[e];
      c_hit[n] = hit;
      n_open += !hit;
    }
    // finished set: held slots (sorted) merged with the hits among the first K candidates (sorted); held first on ties
    for (int k = 0; k < K; ++k) {
      h_score[k] = fin_score[r0 + k];
      h_flag[k] = fin_flag[r0 + k];
      h_len[k] = fin_len[r0 + k];
    }
    const float div = (float)pow((double)g1, (double)length_penalty);
    int hi = 0, ci = 0;
    bool full = true;
    float worst = 0.f;
    for (int j = 0; j < K; ++j) {
      while (ci < K && !c_hit[ci]) ++ci;
      const bool take_new = ci < K && (c_val[ci] / div) > h_score[hi];
      if (take_new) {
        s_fsrc[j] = K + ci;
        fin_score[r0 + j] = worst = c_val[ci] / div;
        fin_flag[r0 + j] = 1;
        fin_len[r0 + j] = len + 1;
        ++ci;
      } else {
        s_fsrc[j] = hi;
        fin_score[r0 + j] = worst = h_score[hi];
        fin_flag[r0 + j] = h_flag[hi];
        fin_len[r0 + j] = h_len[hi];
        full &= h_flag[hi] != 0;
        ++hi;
      }
    }
    // running beams
    int cnt = 0;
    float best_run = 0.f;
    for (int pass = 0; pass < 2 && cnt < K; ++pass)
      for (int n = 0; n < keep && cnt < K; ++n)
        if ((c_hit[n] != 0) == (pass == 1)) {
          s_parent[cnt] = c_parent[n];
          s_id[cnt] = c_id[n];
          const float sc = pass == 1 ? c_val[n] + kMasked : c_val[n];
          run_score[r0 + cnt] = sc;
          if (cnt == 0) best_run = sc;
          out_ids[r0 + cnt] = c_id[n];
          out_parent[r0 + cnt] = r0 + c_parent[n];
          hist_len[r0 + cnt] = len + 1;
          cache_len[r0 + cnt] = cl + 1;
          ++cnt;
        }
    const int L = (early == 2 && length_penalty > 0.f) ? n_new : g1;
    const float best = best_run / (float)pow((double)L, (double)length_penalty);
    const bool u = unsat[b] != 0 && best > worst;
    gen[b] = g1;
    unsat[b] = u;
    if (!u || (full && early == 1) || n_open == 0) {
      done[b] = 1;
      atomicSub(n_unfinished, 1);
    }
  }
  __syncthreads();

  // column owners: read the K sources of a column, then write its K rows (loads of a thread precede its stores)
  for (int c = tid; c <= len; c += kBookThreads) {
    int nh[kMaxK], ns[kMaxK], nf[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      if (j < K) {
        const size_t from = (size_t)(r0 + s_parent[j]) * S_hist + c;
        nh[j] = c < len ? hist[from] : s_id[j];
        ns[j] = c < cl ? src[from] : r0 + s_parent[j];
        const int f = s_fsrc[j];
        if (f < K) nf[j] = fin_ids[(size_t)(r0 + f) * S_hist + c];
        else nf[j] = c < len ? hist[(size_t)(r0 + c_parent[f - K]) * S_hist + c] : c_id[f - K];
      }
    }
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      if (j < K) {
        const size_t at = (size_t)(r0 + j) * S_hist + c;
        hist[at] = nh[j];
        if (c <= cl) src[at] = ns[j];
        fin_ids[at] = nf[j];
      }
    }
  }
}

}  // namespace beam
}  // namespace tn

extern "C" {

long long tn_beam_step_workspace_bytes(int B, int K) {
  if (B <= 0 || K <= 0) return 0;
  return (long long)B * K * tn::beam::kMaxKeep * 8;
}

static int beam_step_launch(const void* logits, int* hist, int* hist_len, int* cache_len, int* src, float* run_score,
                            int* fin_ids, int* fin_len, float* fin_score, int* fin_flag, int* gen, int* unsat, int* done,
                            int* n_unfinished, int* out_ids, int* out_parent, void* workspace, int B, int K, int K_in, int V,
                            int S_hist, float penalty, int ngram, const int* eos_ids, int n_eos, int n_new,
                            float length_penalty, int early_stopping, int dtype, tn::beam::Edits edits, void* stream) {
  using namespace tn::beam;
  if (!tn::step::logits_ok(logits, dtype)) return TN_EINVAL;
  const void* state[] = {hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen, unsat, done,
                         n_unfinished, out_ids, out_parent, workspace};
  for (const void* p : state)
    if (p == nullptr || ((uintptr_t)p & 3)) return TN_EINVAL;
  if (B <= 0 || K < 2 || K > kMaxK || (K_in != 1 && K_in != K) || V < 64 || V > tn::step::kMaxVocab || S_hist <= 0 ||
      ngram < 0 || !(penalty > 0.f) || n_eos < 0 || n_eos > kMaxEos || (n_eos > 0 && eos_ids == nullptr) || n_new <= 0 ||
      early_stopping < 0 || early_stopping > 2 || !(length_penalty == length_penalty))
    return TN_EINVAL;
  Eos eos;
  eos.n = n_eos;
  for (int e = 0; e < kMaxEos; ++e) eos.id[e] = e < n_eos ? eos_ids[e] : -1;
  const int keep = (n_eos + 1 > 2 ? n_eos + 1 : 2) * K;
  float* ws_val = (float*)workspace;
  int* ws_idx = (int*)workspace + (size_t)B * K * kMaxKeep;
  hipStream_t st = (hipStream_t)stream;
  const bool with_edits = edits.ids != nullptr;
#define TN_BEAM_TOPK(T, E)                                                                                              \
  hipLaunchKernelGGL((beam_topk_kernel<T, E>), dim3(B * K_in), dim3(kThreads), 0, st, (const T*)logits, hist, hist_len,  \
                     run_score, done, ws_val, ws_idx, K, K_in, V, S_hist, penalty, ngram, keep, edits)
#define TN_BEAM_LAUNCH(T)                    \
  if (with_edits) TN_BEAM_TOPK(T, true);     \
  else TN_BEAM_TOPK(T, false)
  TN_STEP_DISPATCH(dtype, TN_BEAM_LAUNCH);
#undef TN_BEAM_LAUNCH
#undef TN_BEAM_TOPK
  TN_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_book_kernel, dim3(B), dim3(kBookThreads), 0, st, (const float*)ws_val, (const int*)ws_idx, hist,
                     hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen, unsat, done,
                     n_unfinished, out_ids, out_parent, K, K_in, V, S_hist, keep, eos, n_new, length_penalty,
                     early_stopping);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

int tn_beam_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* src, float* run_score, int* fin_ids,
                 int* fin_len, float* fin_score, int* fin_flag, int* gen, int* unsat, int* done, int* n_unfinished,
                 int* out_ids, int* out_parent, void* workspace, int B, int K, int K_in, int V, int S_hist, float penalty,
                 int ngram, const int* eos_ids, int n_eos, int n_new, float length_penalty, int early_stopping, int dtype,
                 void* stream) {
  return beam_step_launch(logits, hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen,
                          unsat, done, n_unfinished, out_ids, out_parent, workspace, B, K, K_in, V, S_hist, penalty, ngram,
                          eos_ids, n_eos, n_new, length_penalty, early_stopping, dtype,
                          tn::beam::Edits{nullptr, nullptr, nullptr, 0}, stream);
}

int tn_beam_step_edits(const void* logits, int* hist, int* hist_len, int* cache_len, int* src, float* run_score,
                       int* fin_ids, int* fin_len, float* fin_score, int* fin_flag, int* gen, int* unsat, int* done,
                       int* n_unfinished, int* out_ids, int* out_parent, void* workspace, int B, int K, int K_in, int V,
                       int S_hist, float penalty, int ngram, const int* eos_ids, int n_eos, int n_new, float length_penalty,
                       int early_stopping, int dtype, const int* edit_ids, const float* edit_val, const int* edit_cnt,
                       int n_edit, void* stream) {
  tn::beam::Edits edits{nullptr, nullptr, nullptr, 0};
  if (edit_ids != nullptr || edit_val != nullptr || edit_cnt != nullptr) {
    if (edit_ids == nullptr || edit_val == nullptr || edit_cnt == nullptr || n_edit < 1 ||
        !tn::step::aligned(3, {edit_ids, edit_val, edit_cnt}))
      return TN_EINVAL;
    edits = tn::beam::Edits{edit_ids, edit_val, edit_cnt, n_edit};
  }
  return beam_step_launch(logits, hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen,
                          unsat, done, n_unfinished, out_ids, out_parent, workspace, B, K, K_in, V, S_hist, penalty, ngram,
                          eos_ids, n_eos, n_new, length_penalty, early_stopping, dtype, edits, stream);
}

}  // extern "C"
