// Edit-distance alignment of token sequences: the scorer's `EditDistance` and `CountEdits`,
// touchnet/bin/error_rate_zh:44-149,192-205, for a batch of (reference, hypothesis) pairs.
//
// The reference scores a match 0 and a substitution, an insertion and a deletion -1 each, and updates each cell's
// backpointer in the order diagonal, deletion, insertion, each with `>=`.  In integer COSTS (cost = -score) that is
//     ins = D[r][h-1] + 1,  del = D[r-1][h] + 1,  dia = D[r-1][h-1] + (ref[r-1] != hyp[h-1])
//     insertion  if ins <= del and ins <= dia;  else deletion  if del <= dia;  else diagonal
// with D[r][0] = r (deletions only) and D[0][h] = h (insertions only); the backtrace starts at (R, H).  The rule decides
// which of several minimal alignments is printed, and with it the C / S / I / D breakdown, so it is reproduced exactly.
//
// Forward (edit_forward_kernel): ONE WAVE PER PAIR, kEditWaves pairs per workgroup.  The hypothesis is cut into strips of
// 64 columns; lane j owns column 64 s + j + 1 of strip s and the rows run in skew: at step t lane j fills row t - j + 1.
// So the left neighbour's value of the same row, and the reference token of that row, are what lane j - 1 held one step
// earlier: both arrive by a DPP wavefront shift (no LDS), and the diagonal is the left value of the step before.  Lane 0
// takes its left value from the last column of the previous strip (the carry column; D[r][0] = r in strip 0) and its
// token from the reference;
// both are fetched 64 rows at a time, one coalesced load per 64 steps, and handed to lane 0 by v_readlane.  Lane 63's
// results are collected the same way and stored 64 rows at a time, in place: row rho of the carry column is read at step
// 64 floor((rho - 1) / 64) and written at step rho + 62, always later.  The carry column lives in LDS (16-bit: a cost is
// at most 16383) when R <= kEditLdsRows, in the pair's workspace otherwise.
//
// Each cell leaves its arc in two bits, already as the output's code (0 = C, 1 = S, 2 = I, 3 = D); a lane packs 16
// consecutive rows of its column into one 32-bit word and stores whole words:
//     word(r, h) = ws[ws_base + ((r - 1) / 16) * Hpad + (h - 1)],   bits 2 ((r - 1) % 16) ..,   Hpad = 64 ceil(H / 64)
//     words per pair = ceil(R / 16) * Hpad  (+ R for the carry column when R > kEditLdsRows)      -> edit_ws_words()
//
// Backtrace (edit_backtrace_kernel), a second launch: ONE LANE PER PAIR walks back from (R, H), at most R + H dependent
// steps, writes the arcs right-aligned into the pair's R + H bytes of `ops` and the pair's row of `counts`.
// No atomics, no host synchronisation, plain vector stores; the results do not depend on the schedule.
//
// The descriptor table arrives on the host, so tn_edit_align checks every pair before it uploads the table or launches
// anything; the kernels trust it.
#include "common.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace tn {

constexpr int kEditWaves = 4, kEditLdsRows = 2048, kEditMaxLen = 16383, kEditBackThreads = 256;
enum : int { kEditC = 0, kEditS = 1, kEditI = 2, kEditD = 3 };

static inline long long edit_ws_words(int R, int H) {
  const long long hpad = (long long)((H + 63) / 64) * 64;
  return (long long)((R + 15) / 16) * hpad + (R > kEditLdsRows ? R : 0);
}

// lane j <- lane j - 1, lane 0 keeps its own: the DPP wavefront shift right by one (no LDS crossbar trip, unlike ds_bpermute)
__device__ __forceinline__ int from_lane_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

// desc[p] = {ref_start, R, hyp_start, H, ws_base, ops_base}
__global__ __launch_bounds__(kEditWaves * 64) void edit_forward_kernel(const int* __restrict__ ref_tok,
                                                                        const int* __restrict__ hyp_tok,
                                                                        const int* __restrict__ desc, uint32_t* ws, int P) {
  __shared__ uint16_t carry_lds[kEditWaves][kEditLdsRows];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // in an SGPR: the pair's lengths, and with them every
  const int p = blockIdx.x * kEditWaves + wave;                        // loop bound and row test below, are wave-uniform
  if (p >= P) return;                                     // (the kernel has no workgroup barrier)
  const int* d = desc + 6 * (long long)p;
  const int R = d[1], H = d[3];
  const int* ref = ref_tok + d[0];
  const int* hyp = hyp_tok + d[2];
  const int strips = (H + 63) / 64, hpad = strips * 64;
  uint32_t* dirs = ws + d[4];
  uint32_t* carry_ws = dirs + (long long)((R + 15) / 16) * hpad;
  uint16_t* carry_sm = carry_lds[wave];
  const bool in_lds = R <= kEditLdsRows;

  for (int s = 0; s < strips; ++s) {
    const int col = s * 64 + lane + 1;                    // 1-based column of the grid
    const bool live = col <= H;
    const int hv = live ? hyp[col - 1] : 0;
    const bool more = s + 1 < strips;                     // another strip will read this one's last column
    int cur = col, diag = col - 1;                        // D[0][col], D[0][col - 1]
    int rv = 0, ref_chunk = 0, left_chunk = 0, out_chunk = 0;
    uint32_t word = 0;
    for (int t0 = 0; t0 < R + 63; t0 += 64) {             // rows t0 + 1 .. t0 + 64 for lane 0, one per lane; the only
      const int row0 = t0 + lane + 1;                     // loads of the strip, so the 64 steps below wait for no memory
      if (row0 <= R) {
        ref_chunk = ref[row0 - 1];
        left_chunk = s == 0 ? row0 : (in_lds ? (int)carry_sm[row0 - 1] : (int)carry_ws[row0 - 1]);
      }
      const int t1 = min(t0 + 64, R + 63);
      for (int t = t0; t < t1; ++t) {
      int left = from_lane_below(cur), tok = from_lane_below(rv);
      const int left0 = __builtin_amdgcn_readlane(left_chunk, t & 63), tok0 = __builtin_amdgcn_readlane(ref_chunk, t & 63);
      if (lane == 0) { left = left0; tok = tok0; }
      rv = tok;
      const int r = t - lane + 1;
      if (r >= 1 && r <= R) {
        const int ne = rv != hv;
        const int ins = left + 1, del = cur + 1, dia = diag + ne;
        int best, code;
        if (ins <= del && ins <= dia) { best = ins; code = kEditI; }
        else if (del <= dia) { best = del; code = kEditD; }
        else { best = dia; code = ne; }
        diag = left;
        cur = best;
        word |= (uint32_t)code << (((r - 1) & 15) * 2);
        if ((r & 15) == 0 || r == R) {
          if (live) dirs[(long long)((r - 1) >> 4) * hpad + (col - 1)] = word;
          word = 0;
        }
      }
      if (more) {                                         // lane 63 has just filled row t - 62
        const int r63 = t - 62;
        if (r63 >= 1 && r63 <= R) {
          const int v = __builtin_amdgcn_readlane(cur, 63);
          if (lane == ((r63 - 1) & 63)) out_chunk = v;
          if ((r63 & 63) == 0 || r63 == R) {
            const int row = ((r63 - 1) & ~63) + lane + 1;
            if (row <= r63) {
              if (in_lds) carry_sm[row - 1] = (uint16_t)out_chunk;
              else carry_ws[row - 1] = (uint32_t)out_chunk;
            }
          }
        }
      }
      }
    }
    __threadfence_block();                                // the next strip reads the carry column other lanes wrote
  }
}

__global__ __launch_bounds__(kEditBackThreads) void edit_backtrace_kernel(const int* __restrict__ desc,
                                                                           const uint32_t* __restrict__ ws,
                                                                           uint8_t* __restrict__ ops, int* __restrict__ counts,
                                                                           int P) {
  const int p = blockIdx.x * kEditBackThreads + threadIdx.x;
  if (p >= P) return;
  const int* d = desc + 6 * (long long)p;
  const int R = d[1], H = d[3];
  const int hpad = (H + 63) / 64 * 64;
  const uint32_t* dirs = ws + d[4];
  uint8_t* out = ops + d[5];
  int r = R, h = H, pos = R + H, n[4] = {0, 0, 0, 0};
  while (r > 0 || h > 0) {
    int code;
    if (r == 0) code = kEditI;
    else if (h == 0) code = kEditD;
    else code = (dirs[(long long)((r - 1) >> 4) * hpad + (h - 1)] >> (((r - 1) & 15) * 2)) & 3;
    out[--pos] = (uint8_t)code;
    n[0] += code == kEditC;
    n[1] += code == kEditS;
    n[2] += code == kEditI;
    n[3] += code == kEditD;
    r -= code != kEditI;
    h -= code != kEditD;
  }
  int* c = counts + 5 * (long long)p;
  c[0] = n[0]; c[1] = n[1]; c[2] = n[2]; c[3] = n[3];
  c[4] = R + H - pos;
}

}  // namespace tn

using namespace tn;

extern "C" {

long long tn_edit_align_ws_words(int R, int H) {
  if (R < 1 || R > kEditMaxLen || H < 0 || H > kEditMaxLen) return -1;
  return edit_ws_words(R, H);
}

int tn_edit_align(const int* ref_tok, long long n_ref, const int* hyp_tok, long long n_hyp, const int* host_desc,
                  int* desc_dev, int P, unsigned int* ws, long long ws_words, unsigned char* ops, long long n_ops,
                  int* counts, void* stream) {
  if (P < 0 || n_ref < 0 || n_hyp < 0 || ws_words < 0 || n_ops < 0) return TN_EINVAL;
  if (P == 0) return TN_OK;
  if (host_desc == nullptr) return TN_EINVAL;
  long long ws_end = 0;                                   // the workspace ranges ascend in table order
  std::vector<std::pair<long long, long long>> spans;    // (ops_base, R + H)
  spans.reserve((size_t)P);
  bool any_ws = false, any_hyp = false;
  for (int p = 0; p < P; ++p) {
    const int* d = host_desc + 6 * (long long)p;
    const long long ref_start = d[0], R = d[1], hyp_start = d[2], H = d[3], ws_base = d[4], ops_base = d[5];
    if (R < 1 || R > kEditMaxLen || H < 0 || H > kEditMaxLen) return TN_EINVAL;
    if (ref_start < 0 || ref_start + R > n_ref || hyp_start < 0 || hyp_start + H > n_hyp) return TN_EINVAL;
    if (ws_base < ws_end) return TN_EINVAL;
    ws_end = ws_base + edit_ws_words((int)R, (int)H);
    if (ws_end > ws_words) return TN_EINVAL;
    if (ops_base < 0 || ops_base + R + H > n_ops) return TN_EINVAL;
    spans.emplace_back(ops_base, R + H);
    any_ws = any_ws || edit_ws_words((int)R, (int)H) > 0;
    any_hyp = any_hyp || H > 0;
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].first + spans[i - 1].second) return TN_EINVAL;
  if (ref_tok == nullptr || desc_dev == nullptr || ops == nullptr || counts == nullptr || (any_hyp && hyp_tok == nullptr) ||
      (any_ws && ws == nullptr))
    return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(desc_dev, host_desc, sizeof(int) * 6 * (size_t)P, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  if (any_hyp) {
    hipLaunchKernelGGL(edit_forward_kernel, dim3((unsigned)((P + kEditWaves - 1) / kEditWaves)), dim3(kEditWaves * 64), 0, st,
                       ref_tok, hyp_tok, (const int*)desc_dev, ws, P);
    TN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(edit_backtrace_kernel, dim3((unsigned)((P + kEditBackThreads - 1) / kEditBackThreads)),
                     dim3(kEditBackThreads), 0, st, (const int*)desc_dev, (const uint32_t*)ws, ops, counts, P);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
