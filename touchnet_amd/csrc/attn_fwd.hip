// Packed (document-masked, causal) flash attention FORWARD for gfx950 — LDS-tiled, MFMA 32x32x16 bf16.
//
// Replaces the flex_attention / SDPA call the reference makes per decoder layer
// (SURVEY.md §2.3 K6/K6'; transformers/integrations/flex_attention.py:264-340 driven by the document-id
// `attention_mask` of touchnet/models/llama/processing_llama.py:38-40 and
// touchnet/models/touch_audio/processing_touch_audio.py:205-206; plain causal for the Qwen2-Audio path,
// touchnet/models/qwen2_audio/__init__.py:190-193,231-236 = all ids 1).
//
// Layout (chosen for the producing GEMMs, no transposes anywhere):
//   Q [B, T, Nh, D]   K, V [B, T, Nkv, D]   O [B, T, Nh, D]   bf16, D in {64, 128}
//   LSE2 [B, Nh, T] fp32 = log2-domain log-sum-exp of scale*log2(e)*S (+inf on fully masked rows)
//   doc [B, T] int32 document ids (0 = pad)
//
// This file: the mask metadata the attention kernels share (built once per batch), the merge of two partial results,
// and the forward entry points, which pick one of two kernels by shape (fwd_pingpong below):
//   attn_fwd_stream.hip  precomputed tile lists, K / V / Q by LDS-DMA, whole-row stores: every shape but the longest;
//   attn_fwd_pp.hip      ping-pong 256-row workgroups: causal, D = 128, 32768 <= T <= 65536.
// Both consume KV in 64-row tiles; tiles whose document-id range cannot meet the query tile's range are never loaded
// (block-sparse over the packed batch), tiles fully inside one document strictly below the diagonal skip the
// per-element mask.  Per KV tile and wave S^T = K Q^T (A = K from LDS, B = Q in registers), so that every lane owns
// ONE query column: softmax statistics are lane-local, and P never leaves registers on its way into O^T += V^T P^T.
#include "attn_common.h"

namespace tn {

// ------------------------------------------------------------------------------------------------
// Metadata pre-pass: one thread per 64-position tile.
// ------------------------------------------------------------------------------------------------
__global__ void attn_meta_stats_kernel(const int* __restrict__ doc, int* tmin, int* tmax, int* tminpos, int B, int T,
                                       int nt) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * nt) return;
  const int b = idx / nt, t = idx % nt;
  int mn = 0x7fffffff, mx = 0, mnp = 0x7fffffff;
  for (int i = 0; i < kTile; ++i) {
    const int p = t * kTile + i;
    const int d = p < T ? doc[(size_t)b * T + p] : 0;
    mn = min(mn, d);
    mx = max(mx, d);
    if (d > 0) mnp = min(mnp, d);
  }
  tmin[idx] = mn;
  tmax[idx] = mx;
  tminpos[idx] = mnp;
}

__global__ void attn_meta_range_kernel(const int* __restrict__ tmax, const int* __restrict__ tminpos, int* q_lo,
                                       int* kv_hi, int B, int nt) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * nt) return;
  const int b = idx / nt, t = idx % nt;
  const int* mx = tmax + (size_t)b * nt;
  const int* mp = tminpos + (size_t)b * nt;
  int lo = t + 1;
  for (int j = 0; j <= t; ++j)
    if (tile_may_interact(mp[t], mx[t], mp[j], mx[j])) {
      lo = j;
      break;
    }
  int hi = t - 1;
  for (int i = nt - 1; i >= t; --i)
    if (tile_may_interact(mp[i], mx[i], mp[t], mx[t])) {
      hi = i;
      break;
    }
  q_lo[idx] = lo;
  kv_hi[idx] = hi;
}

// Per 32 positions: the id statistics of one wave's query rows (attn_common.h qstat).
__global__ void attn_meta_qstat_kernel(const int* __restrict__ doc, int* __restrict__ qstat, int B, int T, int nq32) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * nq32) return;
  const int b = idx / nq32, g = idx % nq32;
  int mnp = 0x7fffffff, mx = 0, zero = 0;
  for (int i = 0; i < 32; ++i) {
    const int p = g * 32 + i;
    const int d = p < T ? doc[(size_t)b * T + p] : 0;
    mx = max(mx, d);
    if (d > 0) mnp = min(mnp, d);
    zero |= d == 0;
  }
  reinterpret_cast<int4*>(qstat)[idx] = make_int4(mnp, mx, zero, 0);
}

// Per 128-position causal query tile: the KV tiles it meets (attn_common.h klist) — one wave per tile, ballot compaction
// in tile order, i.e. exactly the list the forward / dQ workgroups build for themselves.
__global__ void attn_meta_klist_kernel(const int* __restrict__ tmin, const int* __restrict__ tmax,
                                       const int* __restrict__ tminpos, const int* __restrict__ q_lo,
                                       int* __restrict__ klist, int B, int nt, int nq128) {
  const int qt = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int* mn = tmin + (size_t)b * nt;
  const int* mx = tmax + (size_t)b * nt;
  const int* mp = tminpos + (size_t)b * nt;
  const int t0 = 2 * qt, t1 = min(2 * qt + 1, nt - 1);
  int bminpos = 0x7fffffff, bmax = 0, j_lo = nt;
  for (int t = t0; t <= t1; ++t) {
    bminpos = min(bminpos, mp[t]);
    bmax = max(bmax, mx[t]);
    j_lo = min(j_lo, q_lo[(size_t)b * nt + t]);
  }
  int4* out = reinterpret_cast<int4*>(klist + ((size_t)b * nq128 + qt) * (4 + 4 * kListPre));
  int count = 0;
  for (int base = j_lo; base <= t1; base += 64) {
    const int j = base + lane;
    const bool ok = j <= t1 && tile_may_interact(bminpos, bmax, mp[j <= t1 ? j : t1], mx[j <= t1 ? j : t1]);
    const unsigned long long bal = __ballot(ok);
    const int pos = count + __popcll(bal & ((1ull << lane) - 1ull));
    if (ok && pos < kListPre) out[1 + pos] = make_int4(j, mn[j], mx[j], mp[j]);
    count += __popcll(bal);
  }
  if (lane == 0) out[0] = make_int4(count, qt, 0, 0);
}

// Per 128-position KV tile: the 64-position query tiles it meets under the causal mask (attn_common.h qlist) — what the
// dK / dV workgroups derive for themselves in attn_bwd.hip (first tile = the diagonal, last = kv_hi of its two halves).
__global__ void attn_meta_qlist_kernel(const int* __restrict__ tmin, const int* __restrict__ tmax,
                                       const int* __restrict__ tminpos, const int* __restrict__ kv_hi,
                                       int* __restrict__ qlist, int B, int nt, int nq128) {
  const int kt = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int* mn = tmin + (size_t)b * nt;
  const int* mx = tmax + (size_t)b * nt;
  const int* mp = tminpos + (size_t)b * nt;
  const int t0 = 2 * kt, t1 = min(2 * kt + 1, nt - 1);
  const int bminpos = min(mp[t0], mp[t1]), bmax = max(mx[t0], mx[t1]);
  const int qt_end = min(max(kv_hi[(size_t)b * nt + t0], kv_hi[(size_t)b * nt + t1]) + 1, nt);      // exclusive
  int4* out = reinterpret_cast<int4*>(qlist + ((size_t)b * nq128 + kt) * (4 + 4 * kListPre));
  int count = 0;
  for (int base = t0; base < qt_end; base += 64) {
    const int t = base + lane;
    const int tc = t < qt_end ? t : t0;
    const bool ok = t < qt_end && tile_may_interact(mp[tc], mx[tc], bminpos, bmax);
    const unsigned long long bal = __ballot(ok);
    const int pos = count + __popcll(bal & ((1ull << lane) - 1ull));
    if (ok && pos < kListPre) out[1 + pos] = make_int4(t, mn[t], mx[t], mp[t]);
    count += __popcll(bal);
  }
  if (lane == 0) out[0] = make_int4(count, kt, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// Merge of two partial attention results over DISJOINT key sets (context parallel: own chunks / received chunks):
//   lse = log2(2^lse_a + 2^lse_b),  O = (2^lse_a O_a + 2^lse_b O_b) / 2^lse      (LSE2 convention of the forward kernels:
// log2 domain, +inf = the row saw no key in that part).  HBM-bound: 3 x rows x Nh x D x 2 B + the statistics.
// The reference's ring attention merges its per-step (out, lse) the same way
// (torch/distributed/tensor/experimental/_context_parallel/_attention.py:182-183 via touchnet/utils/distributed.py:292-315).
// ------------------------------------------------------------------------------------------------
__global__ void attn_merge_kernel(const bf16_t* __restrict__ oa, const float* __restrict__ la,
                                  const bf16_t* __restrict__ ob, const float* __restrict__ lb, bf16_t* __restrict__ o,
                                  float* __restrict__ l, int B, int R, int Nh, int D) {
  const int dv = D / 8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)B * R * Nh * dv;
  if (idx >= total) return;
  const int d8 = (int)(idx % dv);
  const int h = (int)((idx / dv) % Nh);
  const size_t br = idx / ((size_t)dv * Nh);                 // b * R + r
  const int b = (int)(br / R), r = (int)(br % R);
  const size_t li = ((size_t)b * Nh + h) * R + r;
  const float a = la[li], c = lb[li];
  const bool ea = a == INFINITY, ec = c == INFINITY;          // empty parts
  const float m = ea ? c : (ec ? a : fmaxf(a, c));
  const float wa = ea ? 0.f : fast_exp2(a - m), wc = ec ? 0.f : fast_exp2(c - m);
  const float tot = wa + wc;
  const float inv = tot > 0.f ? 1.f / tot : 0.f;
  Vec16<bf16_t> va, vc, vo;
  va.load(oa + idx * 8);
  vc.load(ob + idx * 8);
  float fa[8], fc[8], fo[8];
  va.unpack(fa);
  vc.unpack(fc);
#pragma unroll
  for (int e = 0; e < 8; ++e) fo[e] = (wa * fa[e] + wc * fc[e]) * inv;
  vo.pack(fo);
  vo.store(o + idx * 8);
  if (d8 == 0) l[li] = tot > 0.f ? m + log2f(tot) : INFINITY;
}

}  // namespace tn

using namespace tn;

int tn_attn_fwd_pp_launch(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                          AttnMeta m, QView qv, int B, int T, int Nh, int Nkv, int D, float sl2, hipStream_t st);
// attn_fwd_stream.hip: precomputed tile lists, K / V / Q by LDS-DMA, whole-row stores
int tn_attn_fwd_stream_launch(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                              AttnMeta m, QView qv, int B, int T, int Nh, int Nkv, int D, float sl2, hipStream_t st);

// Schedule by shape: the ping-pong kernel (attn_fwd_pp.hip: 256-row workgroups, causal only, its tile list in LDS)
// is the fastest on the long-sequence recipes — T >= 32768, D = 128: config D's 20-minute recordings, 8.81 vs 9.00 ms at
// T = 32768 plain causal; every other shape goes to the stream kernel (attn_fwd_stream.hip).
static bool fwd_pingpong(int T, int D, int nt, const QView& qv) {
  return T >= 32768 && D == 128 && !qv.bidir && nt <= 1024;
}

extern "C" {

// meta buffers: 5 int32 arrays of B*nt each, nt = ceil(T/64):  [tmin | tmax | tminpos | q_lo | kv_hi], then
// [qstat | klist] (attn_common.h AttnMeta)
int tn_attn_meta_ints(int B, int T) { return attn_meta_ints(B, T); }

int tn_attn_build_meta(const int* doc, int* meta, int B, int T, void* stream) {
  if (B <= 0 || T <= 0) return TN_EINVAL;
  const int nt = (T + kTile - 1) / kTile, n = B * nt;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_meta_stats_kernel, dim3((n + 127) / 128), dim3(128), 0, st, doc, meta, meta + n,
                     meta + 2 * n, B, T, nt);
  TN_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_meta_range_kernel, dim3((n + 127) / 128), dim3(128), 0, st, meta + n, meta + 2 * n,
                     meta + 3 * n, meta + 4 * n, B, nt);
  TN_LAUNCH_CHECK();
  const AttnMeta m = make_attn_meta(meta, B, T);
  hipLaunchKernelGGL(attn_meta_qstat_kernel, dim3((B * m.nq32 + 127) / 128), dim3(128), 0, st, doc,
                     const_cast<int*>(m.qstat), B, T, m.nq32);
  TN_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_meta_klist_kernel, dim3(m.nq128, B), dim3(64), 0, st, m.tmin, m.tmax, m.tminpos, m.q_lo,
                     const_cast<int*>(m.klist), B, nt, m.nq128);
  TN_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_meta_qlist_kernel, dim3(m.nq128, B), dim3(64), 0, st, m.tmin, m.tmax, m.tminpos, m.kv_hi,
                     const_cast<int*>(m.qlist), B, nt, m.nq128);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

static int attn_fwd_launch(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                           const int* meta, int B, int T, int Nh, int Nkv, int D, float scale, QView qv,
                           void* stream) {
  if (!attn_shape_ok(B, T, Nh, Nkv, D)) return TN_EINVAL;
  const int nt = (T + kTile - 1) / kTile;
  const AttnMeta m = make_attn_meta(meta, B, T);
  const float sl2 = scale * kLog2e;
  hipStream_t st = (hipStream_t)stream;
  if (fwd_pingpong(T, D, nt, qv)) return tn_attn_fwd_pp_launch(q, k, v, o, lse2, doc, m, qv, B, T, Nh, Nkv, D, sl2, st);
  return tn_attn_fwd_stream_launch(q, k, v, o, lse2, doc, m, qv, B, T, Nh, Nkv, D, sl2, st);
}

int tn_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc, const int* meta,
                int B, int T, int Nh, int Nkv, int D, float scale, void* stream) {
  const QView qv = QView::whole(T);
  return attn_fwd_launch(q, k, v, o, lse2, doc, meta, B, T, Nh, Nkv, D, scale, qv, stream);
}

// Bidirectional inside a document (no causal term): the Whisper speech encoder of Kimi-Audio.
int tn_attn_fwd_bidir(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                      const int* meta, int B, int T, int Nh, int Nkv, int D, float scale, void* stream) {
  QView qv = QView::whole(T);
  qv.bidir = 1;
  return attn_fwd_launch(q, k, v, o, lse2, doc, meta, B, T, Nh, Nkv, D, scale, qv, stream);
}

// Sequence-sharded query side (context parallel): q / o are [B, rows_per_batch, Nh, D], lse2 [B, Nh, rows_per_batch];
// segs = host int[3 * nseg] {row0_a, rows_a, off_a, row0_b, rows_b, off_b}; k / v / doc / meta stay global ([B, T, ...]).
// What a segment list may hold: attn_common.h seg_view (refused with TN_EINVAL before any launch otherwise).
int tn_attn_fwd_seg(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                    const int* meta, int B, int T, int Nh, int Nkv, int D, float scale, int nseg, const int* segs,
                    int rows_per_batch, void* stream) {
  QView qv;
  if (seg_view(nseg, segs, rows_per_batch, T, &qv) != TN_OK) return TN_EINVAL;
  return attn_fwd_launch(q, k, v, o, lse2, doc, meta, B, T, Nh, Nkv, D, scale, qv, stream);
}

// The same, restricted on the KEY side to the sequence chunks whose bit is set in `chunk_mask` (chunk c = positions
// [c * chunk_len, (c + 1) * chunk_len); chunk_len a multiple of 64, at most 64 chunks).  Rows that see no key in those
// chunks get O = 0 and LSE2 = +inf, which tn_attn_merge treats as "no contribution".
int tn_attn_fwd_seg_chunks(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                           const int* meta, int B, int T, int Nh, int Nkv, int D, float scale, int nseg, const int* segs,
                           int rows_per_batch, int chunk_len, unsigned long long chunk_mask, void* stream) {
  QView qv;
  if (seg_view(nseg, segs, rows_per_batch, T, &qv) != TN_OK) return TN_EINVAL;
  if (chunk_len <= 0 || chunk_len % kTile || (T + chunk_len - 1) / chunk_len > 64) return TN_EINVAL;
  qv.kv_tpc = chunk_len / kTile;
  qv.kv_mask = chunk_mask;
  return attn_fwd_launch(q, k, v, o, lse2, doc, meta, B, T, Nh, Nkv, D, scale, qv, stream);
}

// O / LSE2 of two partial attentions over disjoint key sets -> merged (o may alias o_a, lse2 may alias lse2_a).
// o_* [B, rows, Nh, D] bf16, lse2_* [B, Nh, rows] fp32 (log2 domain, +inf = no key seen).
int tn_attn_merge(const void* o_a, const float* lse2_a, const void* o_b, const float* lse2_b, void* o, float* lse2,
                  int B, int rows, int Nh, int D, void* stream) {
  if (B <= 0 || rows <= 0 || Nh <= 0 || D <= 0 || D % 8) return TN_EINVAL;
  const size_t total = (size_t)B * rows * Nh * (D / 8);
  hipLaunchKernelGGL(attn_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)o_a, lse2_a, (const bf16_t*)o_b, lse2_b, (bf16_t*)o, lse2, B, rows, Nh, D);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
