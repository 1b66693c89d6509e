// One text-stream decoding step of Kimi-Audio on the device — KimiASampler.sample_text_logits and the per-row
// bookkeeping of MoonshotKimiaForCausalLM._generate_loop (touchnet/models/kimi_audio/modeling_kimi_audio.py:797-844 and
// :1153-1214), one launch per step, without the loop's `.item()` host synchronisations:
//
//   gen = hist_len[b] - prompt_len[b]                       tokens this row has emitted so far (the loop's step index i)
//   penalty > 1 and gen > W:  every id of hist[b, hist_len - W : hist_len], once:  l = l < 0 ? l * p : l / p, rounded to
//                             the logits' dtype (the reference gathers, scales and scatters inside the logits tensor)
//   temperature <= 1e-6:      token = argmax, lowest id on ties.  The reference takes argmax(log_softmax(float(l))); the
//                             log-softmax subtracts one constant per row, so wherever two log-probabilities do not round to
//                             the same float this is the argmax of the penalised logits themselves, which is compared here.
//   else (1 <= top_k <= 64):  the top_k largest, ties to the lower id, in descending order; w_j = exp((l_j - max) / T) in
//                             fp32 — the reference's exp((l_j - lse) / T) up to the factor exp((max - lse) / T) that all
//                             candidates share and that cancels against the total (kept out so that a small T cannot
//                             underflow every weight); the first candidate whose running weight exceeds u * total, u from
//                             uniforms[b] or from Philox4x32-10 keyed by `seed` with counter (hist_len[b], row_key[b]), as
//                             tn_sample_step keys it
//   a finished row emits `blank` (it keeps stepping, as in the reference)
//   hist[b, hist_len[b]] = token;  hist_len[b]++;  cache_len[b]++;  token == eos: finished[b] = 1, n_unfinished--
//   x_next[b, :] = bf16(float(embed[token]) + float(embed[audio_token]))     the next step's input row: the reference's
//                             embed(audio token) + embed(text token), one bf16 add
//
// A row with no room in hist (hist_len[b] >= S_hist) does not advance — the rule of tn_greedy_step / tn_sample_step: the
// caller grows the history with the caches.  Its token, finished flag and x_next are still computed.
// temperature > 1e-6 with top_k == 0 (multinomial over the whole vocabulary) is out of scope and refused.
//
// One workgroup (1024 threads) per row.  Pass 1 reads the row once: every thread keeps the best of its strided elements,
// the workgroup reduces them to the argmax.  Sampling: the top_k-th best of the 1024 thread maxima bounds the top_k-th best
// of the row from below, so a second pass gathers the few elements at or above it into LDS, where they are ranked exactly.
// If they do not fit (rows of ties), top_k reduction passes pick the candidates one by one instead.
#include "decode_step.h"

namespace tn {
namespace kimi {

using namespace step;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kCap = 2048;                 // candidates gathered into LDS
constexpr int kMaxK = 64;
constexpr int kMaxWindow = 64;
constexpr int kNone = 0x7fffffff;

struct Params {
  int V, S_hist, H, window, top_k, eos, blank, audio_token;
  float penalty, temperature;
  uint32_t seed_lo, seed_hi;
};

// a penalised value as the reference leaves it in the logits tensor
template <typename T>
__device__ __forceinline__ float round_to(float v);
template <>
__device__ __forceinline__ float round_to<float>(float v) { return v; }
template <>
__device__ __forceinline__ float round_to<bf16_t>(float v) { return bf2f(f2bf(v)); }

struct Smem {
  uint32_t seen[kWords];
  float tv[kThreads];                      // every thread's best element
  int ti[kThreads];
  float cv[kCap];                          // gathered candidates
  int ci[kCap];
  float sv[kMaxK];                         // the top_k, descending
  int si[kMaxK];
  float red_v[kWaves];
  int red_i[kWaves];
  float thr_v;
  int thr_i, n_cand, tok;
};

template <typename T>
struct Row {
  const T* row;
  const uint32_t* seen;
  float penalty;
  bool use_pen;
  __device__ __forceinline__ float value(int i) const {
    float v = Elem<T>::ld(row + i);
    if (use_pen && (seen[i >> 5] & (1u << (i & 31)))) v = round_to<T>(penalise(v, penalty));
    return v;
  }
};

template <typename T>
__global__ void __launch_bounds__(kThreads) kimi_text_step_kernel(
    const T* __restrict__ logits, int* __restrict__ hist, int* __restrict__ hist_len, int* __restrict__ cache_len,
    int* __restrict__ finished, int* __restrict__ n_unfinished, const int* __restrict__ prompt_len,
    const bf16_t* __restrict__ embed, bf16_t* __restrict__ x_next, const long long* __restrict__ row_key,
    const float* __restrict__ uniforms, Params p) {
  __shared__ Smem s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.V;
  const int len = min(max(hist_len[b], 0), p.S_hist);        // (a length past the row is never read past it)
  const bool done = finished[b] != 0;
  int tok = p.blank;
  if (!done) {
    const int* h = hist + (size_t)b * p.S_hist;
    const int W = p.window;
    const bool use_pen = p.penalty > 1.f && len - prompt_len[b] > W && len >= W;
    if (use_pen) {
      const int words = (V + 31) / 32;
      for (int w = tid; w < words; w += kThreads) s.seen[w] = 0u;
      __syncthreads();
      mark_seen(s.seen, h, len - W, len, V, tid, kThreads);
      __syncthreads();
    }
    const Row<T> r{logits + (size_t)b * V, s.seen, p.penalty, use_pen};
    // pass 1: every thread's best element, then the row's
    float bv = -INFINITY;
    int bi = kNone;
    for (int i = tid; i < V; i += kThreads) take(r.value(i), i, bv, bi);
    const float my_v = bv;
    const int my_i = bi;
    block_argmax(bv, bi, s.red_v, s.red_i);
    tok = bi < V ? bi : 0;
    const float M = bv;
    const bool finite_max = M == M && M > -INFINITY && M < INFINITY;
    if (p.temperature > 1e-6f && finite_max) {               // (a row without a finite maximum keeps its argmax)
      const int k = min(p.top_k, V);
      s.tv[tid] = my_v;
      s.ti[tid] = my_i;
      if (tid == 0) s.n_cand = 0;
      __syncthreads();
      // the k-th best thread maximum: at least k elements of the row are at or above it
      if (my_i != kNone) {
        int rank = 0;
        for (int j = 0; j < kThreads; ++j) rank += better(s.tv[j], s.ti[j], my_v, my_i);
        if (rank == k - 1) {
          s.thr_v = my_v;
          s.thr_i = my_i;
        }
      }
      __syncthreads();
      const float thr_v = s.thr_v;
      const int thr_i = s.thr_i;
      for (int i = tid; i < V; i += kThreads) {
        const float v = r.value(i);
        if (better(thr_v, thr_i, v, i)) continue;
        const int slot = atomicAdd(&s.n_cand, 1);
        if (slot < kCap) {
          s.cv[slot] = v;
          s.ci[slot] = i;
        }
      }
      __syncthreads();
      const int n = s.n_cand;
      if (n <= kCap) {
        for (int j = tid; j < n; j += kThreads) {
          const float vj = s.cv[j];
          const int ij = s.ci[j];
          int rank = 0;
          for (int m = 0; m < n; ++m) rank += better(s.cv[m], s.ci[m], vj, ij);
          if (rank < k) {
            s.sv[rank] = vj;
            s.si[rank] = ij;
          }
        }
      } else {
        // more ties than LDS holds: pick the candidates one by one, each the best element behind the previous pick
        float pv = INFINITY;
        int pi = -1;
        for (int c = 0; c < k; ++c) {
          float cvb = -INFINITY;
          int cib = kNone;
          for (int i = tid; i < V; i += kThreads) {
            const float v = r.value(i);
            if (better(pv, pi, v, i) && better(v, i, cvb, cib)) {
              cvb = v;
              cib = i;
            }
          }
          block_argmax(cvb, cib, s.red_v, s.red_i);
          if (tid == 0) {
            s.sv[c] = cvb;
            s.si[c] = cib;
          }
          pv = cvb;
          pi = cib;
        }
      }
      __syncthreads();
      if (tid == 0) {
        const double u = row_uniform(uniforms, row_key, b, len, p.seed_lo, p.seed_hi);
        float total = 0.f;
        for (int c = 0; c < k; ++c) total += expf((s.sv[c] - M) / p.temperature);
        const double target = u * (double)total;
        int pick = s.si[k - 1];
        float run = 0.f;
        for (int c = 0; c < k; ++c) {
          run += expf((s.sv[c] - M) / p.temperature);
          if ((double)run > target) {
            pick = s.si[c];
            break;
          }
        }
        s.tok = pick;
      }
      __syncthreads();
      tok = s.tok;
    }
  }
  if (tid == 0)
    append_token(hist, hist_len, cache_len, finished, n_unfinished, b, p.S_hist, len, tok, done, tok == p.eos);
  // the next input row: embed[token] + embed[audio_token], one bf16 rounding (torch's bf16 add)
  const bf16_t* et = embed + (size_t)tok * p.H;
  const bf16_t* ea = embed + (size_t)p.audio_token * p.H;
  bf16_t* xo = x_next + (size_t)b * p.H;
  for (int c = tid * 8; c < p.H; c += kThreads * 8) {
    Vec16<bf16_t> a, t, o;
    float fa[8], ft[8];
    a.load(ea + c);
    t.load(et + c);
    a.unpack(fa);
    t.unpack(ft);
#pragma unroll
    for (int j = 0; j < 8; ++j) ft[j] = fa[j] + ft[j];
    o.pack(ft);
    o.store(xo + c);
  }
}

}  // namespace kimi
}  // namespace tn

extern "C" {

int tn_kimi_text_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* finished, int* n_unfinished,
                      const int* prompt_len, const void* embed, void* x_next, const long long* row_key,
                      const float* uniforms, int B, int V, int S_hist, int H, float penalty, int window, float temperature,
                      int top_k, unsigned long long seed, int eos, int blank, int audio_token, int dtype, void* stream) {
  using namespace tn::kimi;
  if (!logits_ok(logits, dtype) || !hist || !hist_len || !cache_len || !finished || !n_unfinished || !prompt_len || !embed ||
      !x_next)
    return TN_EINVAL;
  if (!aligned(3, {hist, hist_len, cache_len, finished, n_unfinished, prompt_len, uniforms}) || !aligned(7, {row_key}) ||
      !aligned(15, {embed, x_next}))
    return TN_EINVAL;
  if (B <= 0 || V <= 0 || V > kMaxVocab || S_hist <= 0 || H <= 0 || H % 8) return TN_EINVAL;
  if (!(penalty > 0.f) || window < 1 || window > kMaxWindow || top_k < 0 || top_k > kMaxK) return TN_EINVAL;
  if (temperature > 1e-6f && top_k == 0) return TN_EINVAL;       // full-vocabulary multinomial: out of scope
  if (blank < 0 || blank >= V || audio_token < 0 || audio_token >= V) return TN_EINVAL;    // rows of `embed`
  Params p;
  p.V = V;
  p.S_hist = S_hist;
  p.H = H;
  p.window = window;
  p.top_k = top_k;
  p.eos = eos;
  p.blank = blank;
  p.audio_token = audio_token;
  p.penalty = penalty;
  p.temperature = temperature;
  p.seed_lo = (uint32_t)seed;
  p.seed_hi = (uint32_t)(seed >> 32);
  hipStream_t st = (hipStream_t)stream;
#define TN_KIMI_LAUNCH(T)                                                                                              \
  hipLaunchKernelGGL(kimi_text_step_kernel<T>, dim3(B), dim3(kThreads), 0, st, (const T*)logits, hist, hist_len,        \
                     cache_len, finished, n_unfinished, prompt_len, (const tn::bf16_t*)embed, (tn::bf16_t*)x_next, row_key, \
                     uniforms, p)
  TN_STEP_DISPATCH(dtype, TN_KIMI_LAUNCH);
#undef TN_KIMI_LAUNCH
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
