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
// the dequantised weights), and everything behind it is unchanged.  F8 = false compiles to the bf16 kernel as before.
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

template <int MT, int S, bool F8>
__global__ __launch_bounds__(kWaves * 64) void kernel(const Params p) {
  using w_t = std::conditional_t<F8, kvq::fp8_t, bf16_t>;      // one stored element of W
  using XFrag = std::conditional_t<F8, Frag4, Frag>;
  constexpr int kDepth = F8 ? 128 : 64;                          // contraction steps of a chunk: one 128-byte line of W
  __shared__ f32x4_t red[kWaves][MT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int strip0 = blockIdx.x * S;

  // a workgroup past the last whole group of S re-reads the last strip and stores nothing for it
  const w_t* wp[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    int j;
    const Seg& sg = p.seg[locate(p, min(strip0 + s, p.nstrip - 1), j)];
    wp[s] = strip_row<w_t>(sg, p.head_dim, j, lane);
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
  constexpr int U = S + MT <= 2 ? 4 : S + MT <= 4 ? 2 : 1, kStep = U * kWaves;
  const int nch = p.K / kDepth;
  Frag wa[U][S], wb[U][S];
  XFrag xa[U][MT], xb[U][MT];
  auto load = [&](Frag (&w)[U][S], XFrag (&x)[U][MT], int c) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cu = c + u * kWaves;
      if (cu < nch) {
#pragma unroll
        for (int s = 0; s < S; ++s) w[u][s] = load_w(wp[s] + (128 / (int)sizeof(w_t)) * (long long)cu);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          if constexpr (F8)
            x[u][t] = load_x4(xp[t] + kDepth * (long long)cu, xok[t]);
          else
            x[u][t] = load_x(xp[t] + kDepth * (long long)cu, xok[t]);
        }
      }
    }
  };
  auto mac = [&](const Frag (&w)[U][S], const XFrag (&x)[U][MT], int c) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c + u * kWaves < nch) {
#pragma unroll
        for (int s = 0; s < S; ++s)
          if constexpr (F8) {
            u32x4_t e[4];
            expand16(w[u][s].lo, e[0], e[1]);
            expand16(w[u][s].hi, e[2], e[3]);
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
  while (c < nch) {
    load(wb, xb, c + kStep);
    mac(wa, xa, c);
    c += kStep;
    if (c >= nch) break;
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
        tile_epilogue<F8>(p, sg, j, t, lane, v);
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
constexpr int kMaxTilesAt4 = 6, kMaxTilesAt1 = 4;      // (only the selectable (tiles, S) pairs are instantiated)
constexpr int kMaxTilesAt4F8 = 4, kMaxTilesAt1F8 = 4;
template <bool F8>
static inline int strips_per_group(int mt, int nstrip) {
  const int least = mt > (F8 ? kMaxTilesAt1F8 : kMaxTilesAt1) ? 2 : 1;
  int s = mt > (F8 ? kMaxTilesAt4F8 : kMaxTilesAt4) ? 2 : 4;
  while (s > least && (nstrip + s - 1) / s < 2 * 256) s >>= 1;
  return s;
}

template <int MT, bool F8>
static int launch_s(const Params& p, int S, hipStream_t st) {
  const dim3 block(kWaves * 64);
  if constexpr (MT <= (F8 ? kMaxTilesAt4F8 : kMaxTilesAt4)) {
    if (S == 4) {
      hipLaunchKernelGGL((kernel<MT, 4, F8>), dim3((p.nstrip + 3) / 4), block, 0, st, p);
      TN_LAUNCH_CHECK();
      return TN_OK;
    }
  }
  if constexpr (MT <= (F8 ? kMaxTilesAt1F8 : kMaxTilesAt1)) {
    if (S == 1) {
      hipLaunchKernelGGL((kernel<MT, 1, F8>), dim3(p.nstrip), block, 0, st, p);
      TN_LAUNCH_CHECK();
      return TN_OK;
    }
  }
  hipLaunchKernelGGL((kernel<MT, 2, F8>), dim3((p.nstrip + 1) / 2), block, 0, st, p);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

template <bool F8>
static int launch(const Params& p, hipStream_t st) {
  const int mt = (p.M + 15) / 16, S = strips_per_group<F8>(mt, p.nstrip);
  switch (mt) {
    case 1: return launch_s<1, F8>(p, S, st);
    case 2: return launch_s<2, F8>(p, S, st);
    case 3: return launch_s<3, F8>(p, S, st);
    case 4: return launch_s<4, F8>(p, S, st);
    case 5: return launch_s<5, F8>(p, S, st);
    case 6: return launch_s<6, F8>(p, S, st);
    case 7: return launch_s<7, F8>(p, S, st);
    default: return launch_s<8, F8>(p, S, st);
  }
}

}  // namespace smallm
}  // namespace tn

using namespace tn;
using namespace tn::smallm;


static int run(int rc, const Params& p, bool f8, void* stream) {
  if (rc != TN_OK) return rc;
  return f8 ? launch<true>(p, static_cast<hipStream_t>(stream)) : launch<false>(p, static_cast<hipStream_t>(stream));
}

extern "C" int tn_gemm_smallm(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                              const long long* ldw, const void* const* bias, void* const* y, const long long* ldy,
                              const int* N, const void* cos_t, const void* sin_t, int head_dim, int rope_mask,
                              void* stream) {
  Params p;
  return run(linear_params(p, kMaxM, x, ldx, M, K, nseg, w, ldw, nullptr, bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask),
             p, false, stream);
}

extern "C" int tn_gemm_smallm_swiglu(const void* x, const void* w_gate, const void* w_up, void* act, int M, int I, int K,
                                     long long ldx, long long ldw, long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, x, w_gate, w_up, nullptr, nullptr, false, act, M, I, K, ldx, ldw, ldact), p, false, stream);
}

extern "C" int tn_gemm_smallm_fp8(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                  const long long* ldw, const float* const* scale, const void* const* bias, void* const* y,
                                  const long long* ldy, const int* N, const void* cos_t, const void* sin_t, int head_dim,
                                  int rope_mask, void* stream) {
  if (scale == nullptr) return TN_EINVAL;
  Params p;
  return run(linear_params(p, kMaxM, x, ldx, M, K, nseg, w, ldw, scale, bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask),
             p, true, stream);
}

extern "C" int tn_gemm_smallm_swiglu_fp8(const void* x, const void* w_gate, const void* w_up, const float* scale_gate,
                                         const float* scale_up, void* act, int M, int I, int K, long long ldx, long long ldw,
                                         long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, x, w_gate, w_up, scale_gate, scale_up, true, act, M, I, K, ldx, ldw, ldact), p, true,
             stream);
}
