// Small-M weight-streaming GEMM for the decode step (gfx950): Y[m, n] = sum_k X[m, k] W[n, k] (+ bias[n]) for 1 <= M <= 128
// rows — the seven linear products per layer of generation.decode_logits and lm_head on the decode rows, which the 256 x 256
// tiles of csrc/gemm.hip cannot fill.  The bound here is the HBM bytes of W, read exactly once; the
// design follows from that and shares nothing with the training kernel:
//
//  * A STRIP is 16 weight rows.  v_mfma_f32_16x16x32_bf16 takes W as its 16-row operand and 16 rows of X as the other, so
//    a lane ends up with FOUR output features of ONE row of X: lane l, element e = feature row 4 (l >> 4) + e of the strip,
//    X row l & 15.
//  * W goes from global memory straight into the MFMA operand registers (no LDS): of a 64-deep chunk of the contraction —
//    one 128-byte line per weight row — lane l reads bytes 32 (l >> 4) .. + 31 of row l & 15 as two 16-byte loads, so the
//    four lanes of a row cover the whole line.  The first 16 bytes feed the chunk's first MFMA, the second 16 its second:
//    MFMA j of a chunk contracts k = 64 c + 16 g + 8 j + s over lane group g and slot s.  X is read from L2 with the SAME
//    lane pattern, so the permutation of the contraction index cancels.  Rows >= M of X are zero registers, never loads.
//  * The four waves of a workgroup split the contraction: wave w takes the chunks c = w, w + 4, ..; their partial tiles
//    are summed through LDS as ((w0 + w1) + w2) + w3.  No atomics, nothing crosses workgroups, and the order of the K
//    terms of an output element depends on K alone — not on M, the row or the other rows.
//  * A workgroup owns S consecutive strips (template parameter, chosen by the host from M and the strip count): a fragment
//    of X in registers is used S times, so the L2 traffic of X stays at M / (16 S) of the HBM traffic of W.
//  * Epilogues apply the row kernels' rules (common.h: rope_rotate, sigmoid_fast) to the bf16-ROUNDED accumulator + bias,
//    so they are bit-identical to the product followed by tn_rope_apply / tn_swiglu_fwd.  For both, a strip's 16 weight
//    rows are two runs of 8: rows r .. r + 7 and r + head_dim / 2 .. of one head (RoPE), or 8 gate rows and the 8 up rows of
//    the same features (SwiGLU).  The second run sits in lane groups 2, 3, so the partner of every output is in lane
//    l ^ 32, same element: one cross-lane exchange, no second pass, no LDS round trip.
//
// FP8 weights (F8 = true; tn_gemm_smallm_fp8, tn_gemm_smallm_swiglu_fp8): W is e4m3 codes uint8 [N, K] with
// one fp32 power-of-two scale per row (weight_fp8.hip, the rules of kv_fp8.h).  A 128-byte line of a weight row now holds
// 128 contraction steps, so the chunk is 128 deep: lane l still reads bytes 32 (l >> 4) .. + 31 of row l & 15 as two
// 16-byte loads — 32 codes, expanded exactly to bf16 in registers (v_cvt_pk_f32_fp8 + v_perm_b32 of the high halves), the
// operands of FOUR MFMAs: MFMA j of a chunk contracts k = 128 c + 32 g + 8 j + s.  X is read with the matching pattern, four
// 16-byte loads per lane and chunk.  The accumulators hold x . code; the row's scale multiplies them ONCE in the epilogue,
// own = rbf(acc * scale[f] + bias[f]) (a power of two: the product is exact, so this is the bf16 kernel's arithmetic on
// the dequantised weights), and everything behind it is unchanged.  F = kBf16 compiles to the bf16 kernel as before.
//
// MXFP4 weights (F = kMxfp4; tn_gemm_smallm_mxfp4, tn_gemm_smallm_swiglu_mxfp4): W is e2m1 codes, two per
// byte, with one e8m0 scale byte per 32 elements of K (weight_mxfp4.hip, the rules of mxfp4.h).  The chunk stays 128 deep,
// which is now a 64-byte HALF line per weight row: lane l reads bytes 16 (l >> 4) .. + 15 of row l & 15 as ONE 16-byte load
// — 32 codes, exactly one scale block, so the lane also loads ONE scale byte, block 4 c + (l >> 4) of its row, issued with
// the codes and independent of them.  Dword j of the 16 bytes expands to the operand of MFMA j in four
// v_cvt_scalef32_pk_bf16_fp4 that take the scale as an operand: MFMA j contracts k = 128 c + 32 g + 8 j + s, the FP8 arm's
// map, so X is read exactly as there (Frag4) and the permutation cancels.  The two halves of a line are chunks 2 i and
// 2 i + 1; the split of chunks over waves hands a wave whole lines (its i-th chunk is 8 (i >> 1) + 2 w + (i & 1)), so it asks
// for both halves in consecutive loads (handing them to two waves cost a second fetch of most lines).  A fragment of W is 5 registers instead of 8 and the fragment of X is unchanged, so U is
// chosen from the registers of X (U MT <= 4) and the loads of W in flight (U S <= 8).  No scale in the epilogue.
#include <type_traits>

#include "gemm_stream.h"

namespace tn {
namespace smallm {
using namespace wstream;      // Seg / Params, the strip map, load_w, expand16 and the tile epilogue: shared with gemm_midm.hip

constexpr int kWaves = 4;          // waves per workgroup = parts the contraction is cut into (fixed: the summation order)
constexpr int kMaxM = 128;

struct Frag4 {           // F8: a lane's 64 bytes of X of one 128-deep chunk, the second operands of the chunk's four MFMAs
  u32x4_t v[4];
};

__device__ __forceinline__ Frag load_x(const bf16_t* p, bool row_ok) {
  Frag f = {u32x4_t{0, 0, 0, 0}, u32x4_t{0, 0, 0, 0}};
  if (row_ok) {
    f.lo = *reinterpret_cast<const u32x4_t*>(p);
    f.hi = *(reinterpret_cast<const u32x4_t*>(p) + 1);
  }
  return f;
}

__device__ __forceinline__ Frag4 load_x4(const bf16_t* p, bool row_ok) {
  Frag4 f;
#pragma unroll
  for (int j = 0; j < 4; ++j) f.v[j] = row_ok ? *(reinterpret_cast<const u32x4_t*>(p) + j) : u32x4_t{0, 0, 0, 0};
  return f;
}

struct FragM {           // kMxfp4: a lane's 16 bytes of one 64-byte chunk of a weight row, and the scale byte of those 32 codes
  u32x4_t c;
  uint32_t sb;
};

// chunks a wave keeps in flight per register set
template <int MT, int S, Format F>
constexpr int unroll_of() {
  if (F == kMxfp4) return S == 4 ? (MT <= 2 ? 2 : 1) : MT == 1 ? 4 : MT == 2 ? 2 : 1;
  return S + MT <= 2 ? 4 : S + MT <= 4 ? 2 : 1;
}

template <int MT, int S, Format F>
__global__ __launch_bounds__(kWaves * 64) void kernel(const Params p) {
  constexpr bool F8 = F == kFp8, F4 = F == kMxfp4;
  using w_t = std::conditional_t<F == kBf16, bf16_t, uint8_t>;   // one stored element of W (kMxfp4: a byte of two codes)
  using XFrag = std::conditional_t<F == kBf16, Frag, Frag4>;
  using WFrag = std::conditional_t<F4, FragM, Frag>;
  constexpr int kDepth = kDepthOf<F>, kLane = kLaneBytesOf<F>;    // a chunk: its contraction steps; a lane's bytes of a row's
  __shared__ f32x4_t red[kWaves][MT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int strip0 = blockIdx.x * S;

  // a workgroup past the last whole group of S re-reads the last strip and stores nothing for it
  const w_t* wp[S];
  const uint8_t* sp[F4 ? S : 1];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    int j;
    const Seg& sg = p.seg[locate(p, min(strip0 + s, p.nstrip - 1), j)];
    wp[s] = strip_row<w_t, kLane>(sg, p.head_dim, j, lane);
    if constexpr (F4) sp[s] = strip_scale_row(sg, p.head_dim, j, lane);
  }
  const bf16_t* xp[MT];
  bool xok[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + l15;
    xok[t] = m < p.M;
    xp[t] = p.X + (long long)(xok[t] ? m : 0) * p.ldx + (kDepth / 4) * g;
  }

  f32x4_t acc[S][MT];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[s][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // A wave moves through its chunks U at a time (chunks c, c + 4, .., still in ascending order): with few strips and
  // tiles one chunk is only 2 KiB per wave, too little in flight to cover the HBM latency.  (F8: a chunk of a strip is the
  // same 16 lines of 128 bytes, so the same U keeps the same bytes of W in flight per wave.)
  constexpr int U = unroll_of<MT, S, F>(), kStep = U * kWaves;
  const int nch = p.K / kDepth;
  // kMxfp4: a wave's i-th chunk is 8 (i >> 1) + 2 wave + (i & 1): it owns both 64-byte halves of a 128-byte line and asks for
  // them in consecutive loads.  `c` below then counts slots (wave + 4 i) up to nch rounded up to whole groups of eight.
  const int nslot = F4 ? (nch + 7) & ~7 : nch;
  auto chunk_of = [&](int t) { return F4 ? 8 * (t >> 3) + 2 * (t & 3) + ((t >> 2) & 1) : t; };
  WFrag wa[U][S], wb[U][S];
  XFrag xa[U][MT], xb[U][MT];
  auto load = [&](WFrag (&w)[U][S], XFrag (&x)[U][MT], int c) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cu = chunk_of(c + u * kWaves);
      if (cu < nch) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if constexpr (F4) {
            w[u][s].c = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wp[s] + 64 * (long long)cu));
            w[u][s].sb = sp[s][4 * (long long)cu];
          } else {
            w[u][s] = load_w(wp[s] + (128 / (int)sizeof(w_t)) * (long long)cu);
          }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          if constexpr (F != kBf16)
            x[u][t] = load_x4(xp[t] + kDepth * (long long)cu, xok[t]);
          else
            x[u][t] = load_x(xp[t] + kDepth * (long long)cu, xok[t]);
        }
      }
    }
  };
  auto mac = [&](const WFrag (&w)[U][S], const XFrag (&x)[U][MT], int c) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (chunk_of(c + u * kWaves) < nch) {
#pragma unroll
        for (int s = 0; s < S; ++s)
          if constexpr (F != kBf16) {
            u32x4_t e[4];
            if constexpr (F4) {
              expand32(w[u][s].c, w[u][s].sb, e);
            } else {
              expand16(w[u][s].lo, e[0], e[1]);
              expand16(w[u][s].hi, e[2], e[3]);
            }
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
              for (int j = 0; j < 4; ++j)
                acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, e[j]),
                                                                    __builtin_bit_cast(bf16x8_t, x[u][t].v[j]), acc[s][t], 0, 0, 0);
          } else {
#pragma unroll
            for (int t = 0; t < MT; ++t) {
              acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[u][s].lo),
                                                                  __builtin_bit_cast(bf16x8_t, x[u][t].lo), acc[s][t], 0, 0, 0);
              acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[u][s].hi),
                                                                  __builtin_bit_cast(bf16x8_t, x[u][t].hi), acc[s][t], 0, 0, 0);
            }
          }
      }
  };
  // two register sets in turn: the loads of a wave's next chunks are in flight under the MFMAs of these
  int c = wave;
  load(wa, xa, c);
  while (c < nslot) {
    load(wb, xb, c + kStep);
    mac(wa, xa, c);
    c += kStep;
    if (c >= nslot) break;
    load(wa, xa, c + kStep);
    mac(wb, xb, c);
    c += kStep;
  }

  // strip by strip: the four partial tiles through LDS, summed in wave order, then the strip's epilogue on tile t by wave t & 3
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int t = 0; t < MT; ++t) red[wave][t][lane] = acc[s][t];
    __syncthreads();
    const int st = strip0 + s;
    if (st < p.nstrip) {
      int j;
      const Seg& sg = p.seg[locate(p, st, j)];
      for (int t = wave; t < MT; t += kWaves) {
        if (16 * t >= p.M) break;
        f32x4_t v = red[0][t][lane];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += red[w][t][lane];
        tile_epilogue<F>(p, sg, j, t, lane, v);
      }
    }
    __syncthreads();
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// Strips per workgroup.  More strips re-use a fragment of X more often (the L2 bytes of X per HBM byte of W are
// M / (16 S)), fewer give more workgroups: S = 4 while that still leaves two workgroups per CU, never below one strip per
// four 16-row tiles of X, and two above six tiles (four strips x seven tiles of accumulators and operands no longer fit
// the register file).  Depends on M and the strip count; the summation order does not depend on S.
// FP8: a chunk's fragment of X is 16 registers instead of 8 (two register sets: 32 per tile), so four strips stop at
// four tiles: four strips x five and six tiles compile without scratch, but to 442 and 508 of the 512 registers, over a
// hundred of them operands parked in AGPRs and copied back for every use (DESIGN.md §9.13's table).  Otherwise the same rule.
// MXFP4: the fragment of X is the FP8 arm's, so the same table holds; a fragment of W is 5 registers instead of 8, which
// buys nothing at five tiles and more, where X fills the file (DESIGN.md §9.15's table).
template <Format F> constexpr int kMaxTilesAt4 = F == kBf16 ? 6 : 4;      // (only the selectable (tiles, S) pairs are instantiated)
template <Format F> constexpr int kMaxTilesAt1 = 4;
template <Format F>
static inline int strips_per_group(int mt, int nstrip) {
  const int least = mt > kMaxTilesAt1<F> ? 2 : 1;
  int s = mt > kMaxTilesAt4<F> ? 2 : 4;
  while (s > least && (nstrip + s - 1) / s < 2 * 256) s >>= 1;
  return s;
}

template <int MT, Format F>
static int launch_s(const Params& p, int S, hipStream_t st) {
  const dim3 block(kWaves * 64);
  if constexpr (MT <= kMaxTilesAt4<F>) {
    if (S == 4) {
      hipLaunchKernelGGL((kernel<MT, 4, F>), dim3((p.nstrip + 3) / 4), block, 0, st, p);
      TN_LAUNCH_CHECK();
      return TN_OK;
    }
  }
  if constexpr (MT <= kMaxTilesAt1<F>) {
    if (S == 1) {
      hipLaunchKernelGGL((kernel<MT, 1, F>), dim3(p.nstrip), block, 0, st, p);
      TN_LAUNCH_CHECK();
      return TN_OK;
    }
  }
  hipLaunchKernelGGL((kernel<MT, 2, F>), dim3((p.nstrip + 1) / 2), block, 0, st, p);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

template <Format F>
static int launch(const Params& p, hipStream_t st) {
  const int mt = (p.M + 15) / 16, S = strips_per_group<F>(mt, p.nstrip);
  switch (mt) {
    case 1: return launch_s<1, F>(p, S, st);
    case 2: return launch_s<2, F>(p, S, st);
    case 3: return launch_s<3, F>(p, S, st);
    case 4: return launch_s<4, F>(p, S, st);
    case 5: return launch_s<5, F>(p, S, st);
    case 6: return launch_s<6, F>(p, S, st);
    case 7: return launch_s<7, F>(p, S, st);
    default: return launch_s<8, F>(p, S, st);
  }
}

}  // namespace smallm
}  // namespace tn

using namespace tn;
using namespace tn::smallm;

static int run(int rc, const Params& p, Format f, void* stream) {
  if (rc != TN_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  return f == kMxfp4 ? launch<kMxfp4>(p, st) : f == kFp8 ? launch<kFp8>(p, st) : launch<kBf16>(p, st);
}

extern "C" int tn_gemm_smallm(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                              const long long* ldw, const void* const* bias, void* const* y, const long long* ldy,
                              const int* N, const void* cos_t, const void* sin_t, int head_dim, int rope_mask,
                              void* stream) {
  Params p;
  return run(linear_params(p, kMaxM, kBf16, x, ldx, M, K, nseg, w, ldw, nullptr, nullptr, bias, y, ldy, N, cos_t, sin_t,
                           head_dim, rope_mask),
             p, kBf16, stream);
}

extern "C" int tn_gemm_smallm_swiglu(const void* x, const void* w_gate, const void* w_up, void* act, int M, int I, int K,
                                     long long ldx, long long ldw, long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, kBf16, x, w_gate, w_up, nullptr, nullptr, 0, act, M, I, K, ldx, ldw, ldact), p, kBf16,
             stream);
}

extern "C" int tn_gemm_smallm_fp8(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                  const long long* ldw, const float* const* scale, const void* const* bias, void* const* y,
                                  const long long* ldy, const int* N, const void* cos_t, const void* sin_t, int head_dim,
                                  int rope_mask, void* stream) {
  Params p;
  return run(linear_params(p, kMaxM, kFp8, x, ldx, M, K, nseg, w, ldw, reinterpret_cast<const void* const*>(scale), nullptr,
                           bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask),
             p, kFp8, stream);
}

extern "C" int tn_gemm_smallm_swiglu_fp8(const void* x, const void* w_gate, const void* w_up, const float* scale_gate,
                                         const float* scale_up, void* act, int M, int I, int K, long long ldx, long long ldw,
                                         long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, kFp8, x, w_gate, w_up, scale_gate, scale_up, 0, act, M, I, K, ldx, ldw, ldact), p, kFp8,
             stream);
}

extern "C" int tn_gemm_smallm_mxfp4(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                    const long long* ldw, const unsigned char* const* scales, const long long* lds,
                                    const void* const* bias, void* const* y, const long long* ldy, const int* N,
                                    const void* cos_t, const void* sin_t, int head_dim, int rope_mask, void* stream) {
  Params p;
  return run(linear_params(p, kMaxM, kMxfp4, x, ldx, M, K, nseg, w, ldw, reinterpret_cast<const void* const*>(scales), lds,
                           bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask),
             p, kMxfp4, stream);
}

extern "C" int tn_gemm_smallm_swiglu_mxfp4(const void* x, const void* w_gate, const void* w_up,
                                           const unsigned char* scales_gate, const unsigned char* scales_up, void* act, int M,
                                           int I, int K, long long ldx, long long ldw, long long lds, long long ldact,
                                           void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, kMxfp4, x, w_gate, w_up, scales_gate, scales_up, lds, act, M, I, K, ldx, ldw, ldact), p,
             kMxfp4, stream);
}
