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

#include "kv_fp8.h"

namespace tn {
namespace smallm {

constexpr int kWaves = 4;          // waves per workgroup = parts the contraction is cut into (fixed: the summation order)
constexpr int kMaxSeg = 3;
constexpr int kMaxM = 128;
enum Mode { kPlain = 0, kRope = 1, kSwiglu = 2 };

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

struct Seg {
  const void* W;         // [N, K] bf16 (F8: e4m3 codes), pitch ldw elements (kSwiglu: gate_proj)
  const void* W2;        // kSwiglu: up_proj, same pitch
  const float* scale;    // F8: [N] row scales of W (else unused)
  const float* scale2;   // F8, kSwiglu: those of W2
  const bf16_t* bias;    // [N] or null
  bf16_t* Y;             // [M, N], pitch ldy (kSwiglu: act [M, I])
  long long ldw, ldy;
  int strip_end;         // strips of segments 0 .. this one
  int mode;
};

struct Params {
  const bf16_t* X;
  const bf16_t* cos_t;   // [M, head_dim / 2]
  const bf16_t* sin_t;
  long long ldx;
  int M, K, nstrip, head_dim;
  Seg seg[kMaxSeg];
};

struct Frag {            // a lane's 32 bytes of one 64-deep chunk of one row: the operands of the chunk's two MFMAs
  u32x4_t lo, hi;
};

struct Frag4 {           // F8: a lane's 64 bytes of X of one 128-deep chunk, the second operands of the chunk's four MFMAs
  u32x4_t v[4];
};

__device__ __forceinline__ Frag load_w(const void* p) {        // streamed: every byte of W is wanted exactly once
  Frag f;
  f.lo = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  f.hi = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p) + 1);
  return f;
}

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

// 16 codes -> their 16 bf16 values as the operands of two MFMAs (exact: a code has 4 significant bits).  kv_fp8.h's decode8
// with scale 1 (the multiplication folds away), then the high halves of each pair of fp32 in one v_perm_b32.
__device__ __forceinline__ void expand16(const u32x4_t c, u32x4_t& a, u32x4_t& b) {
  float f[8], h[8];
  kvq::decode8(make_uint2(c[0], c[1]), 1.0f, f);
  kvq::decode8(make_uint2(c[2], c[3]), 1.0f, h);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = __builtin_amdgcn_perm(__float_as_uint(f[2 * i + 1]), __float_as_uint(f[2 * i]), 0x07060302u);
    b[i] = __builtin_amdgcn_perm(__float_as_uint(h[2 * i + 1]), __float_as_uint(h[2 * i]), 0x07060302u);
  }
}

__device__ __forceinline__ float rbf(float v) { return bf2f(f2bf(v)); }

// where strip `st` of the launch lives: its segment and its index inside it
__device__ __forceinline__ int locate(const Params& p, int st, int& j) {
  int s = 0, first = 0;
#pragma unroll
  for (int i = 0; i + 1 < kMaxSeg; ++i)
    if (st >= p.seg[i].strip_end) {
      s = i + 1;
      first = p.seg[i].strip_end;
    }
  j = st - first;
  return s;
}

// first feature of the run of 8 that holds row `i` (0 .. 15) of strip j, by mode; `second` = the run is the partner run
__device__ __forceinline__ int run_base(int mode, int head_dim, int j, bool second) {
  if (mode == kPlain) return 16 * j + (second ? 8 : 0);
  if (mode == kSwiglu) return 8 * j;                              // (second: the same features of W2)
  const int per = head_dim >> 4;                                  // strips per head
  return (j / per) * head_dim + 8 * (j % per) + (second ? head_dim >> 1 : 0);
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
    const bool second = l15 >= 8;
    const w_t* base = static_cast<const w_t*>((sg.mode == kSwiglu && second) ? sg.W2 : sg.W);
    wp[s] = base + (long long)(run_base(sg.mode, p.head_dim, j, second) + (l15 & 7)) * sg.ldw + (kDepth / 4) * g;
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
      const int mode = sg.mode;
      const bool second = g >= 2;
      const int f0 = run_base(mode, p.head_dim, j, second) + 4 * (g & 1);      // the lane's four features f0 .. f0 + 3
      for (int t = wave; t < MT; t += kWaves) {
        if (16 * t >= p.M) break;
        f32x4_t v = red[0][t][lane];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += red[w][t][lane];
        const int m = 16 * t + l15;
        const bool row_ok = m < p.M;
        float own[4], other[4], y[4];
        u32x2_t bv = {0, 0};
        if (sg.bias != nullptr) bv = *reinterpret_cast<const u32x2_t*>(sg.bias + f0);
        if constexpr (F8)      // the row scales of the lane's four features: the up rows (second run of a SwiGLU strip) have their own
          v *= *reinterpret_cast<const f32x4_t*>((mode == kSwiglu && second ? sg.scale2 : sg.scale) + f0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float b = __uint_as_float(e & 1 ? bv[e >> 1] & 0xffff0000u : bv[e >> 1] << 16);
          own[e] = rbf(v[e] + b);
          y[e] = own[e];
        }
        if (mode != kPlain) {
#pragma unroll
          for (int e = 0; e < 4; ++e) other[e] = __shfl_xor(own[e], 32, 64);
        }
        if (mode == kRope) {
          u32x2_t cv = {0, 0}, sv = {0, 0};
          if (row_ok) {
            const long long at = (long long)m * (p.head_dim >> 1) + (f0 & ((p.head_dim >> 1) - 1));
            cv = *reinterpret_cast<const u32x2_t*>(p.cos_t + at);
            sv = *reinterpret_cast<const u32x2_t*>(p.sin_t + at);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float cf = __uint_as_float(e & 1 ? cv[e >> 1] & 0xffff0000u : cv[e >> 1] << 16);
            const float sf = __uint_as_float(e & 1 ? sv[e >> 1] & 0xffff0000u : sv[e >> 1] << 16);
            float ya, yb;
            rope_rotate(second ? other[e] : own[e], second ? own[e] : other[e], cf, sf, ya, yb);
            y[e] = second ? yb : ya;
          }
        } else if (mode == kSwiglu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = rbf(own[e] * sigmoid_fast(own[e])) * other[e];      // (lanes of the gate run)
        }
        if (row_ok && !(mode == kSwiglu && second))
          *reinterpret_cast<u32x2_t*>(sg.Y + (long long)m * sg.ldy + f0) = u32x2_t{pack2bf(y[0], y[1]), pack2bf(y[2], y[3])};
      }
    }
    __syncthreads();
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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

// (F8: whole 128-deep chunks; weight pitches are bytes of codes and keep the rows 16-byte aligned)
static bool x_ok(const void* x, int M, int K, long long ldx, bool f8 = false) {
  return x != nullptr && aligned16(x) && M >= 1 && M <= kMaxM && K > 0 && K % (f8 ? 128 : 64) == 0 && ldx >= K && ldx % 8 == 0;
}

// tn_gemm_smallm (scale == nullptr) and tn_gemm_smallm_fp8 (scale[i]: the row scales of w[i])
static int linear_entry(const void* x, long long ldx, int M, int K, int nseg, const void* const* w, const long long* ldw,
                        const float* const* scale, const void* const* bias, void* const* y, const long long* ldy,
                        const int* N, const void* cos_t, const void* sin_t, int head_dim, int rope_mask, void* stream) {
  const bool f8 = scale != nullptr;
  if (!x_ok(x, M, K, ldx, f8) || nseg < 1 || nseg > kMaxSeg || w == nullptr || ldw == nullptr || y == nullptr ||
      ldy == nullptr || N == nullptr || rope_mask < 0 || rope_mask >= (1 << nseg))
    return TN_EINVAL;
  if (rope_mask != 0 && (cos_t == nullptr || sin_t == nullptr || !aligned16(cos_t) || !aligned16(sin_t) ||
                         (head_dim != 64 && head_dim != 128)))
    return TN_EINVAL;
  Params p = {};
  p.X = static_cast<const bf16_t*>(x);
  p.cos_t = static_cast<const bf16_t*>(cos_t);
  p.sin_t = static_cast<const bf16_t*>(sin_t);
  p.ldx = ldx;
  p.M = M;
  p.K = K;
  p.head_dim = rope_mask != 0 ? head_dim : 64;
  int strips = 0;
  for (int i = 0; i < nseg; ++i) {
    const bool rope = (rope_mask >> i) & 1;
    const void* b = bias != nullptr ? bias[i] : nullptr;
    if (w[i] == nullptr || y[i] == nullptr || !aligned16(w[i]) || !aligned16(y[i]) || (b != nullptr && !aligned16(b)) ||
        N[i] <= 0 || N[i] % 16 != 0 || ldw[i] < K || ldw[i] % (f8 ? 16 : 8) != 0 || ldy[i] < N[i] || ldy[i] % 8 != 0 ||
        (rope && N[i] % head_dim != 0) || (f8 && (scale[i] == nullptr || !aligned16(scale[i]))))
      return TN_EINVAL;
    strips += N[i] / 16;
    p.seg[i] = Seg{w[i], nullptr, f8 ? scale[i] : nullptr, nullptr, static_cast<const bf16_t*>(b), static_cast<bf16_t*>(y[i]),
                   ldw[i], ldy[i], strips, rope ? kRope : kPlain};
  }
  for (int i = nseg; i < kMaxSeg; ++i) {
    p.seg[i] = p.seg[nseg - 1];
    p.seg[i].strip_end = 0x7fffffff;
  }
  p.nstrip = strips;
  return f8 ? launch<true>(p, static_cast<hipStream_t>(stream)) : launch<false>(p, static_cast<hipStream_t>(stream));
}

// tn_gemm_smallm_swiglu (no scales) and tn_gemm_smallm_swiglu_fp8
static int swiglu_entry(const void* x, const void* w_gate, const void* w_up, const float* s_gate, const float* s_up, bool f8,
                        void* act, int M, int I, int K, long long ldx, long long ldw, long long ldact, void* stream) {
  if (!x_ok(x, M, K, ldx, f8) || w_gate == nullptr || w_up == nullptr || act == nullptr || !aligned16(w_gate) ||
      !aligned16(w_up) || !aligned16(act) || I <= 0 || I % 16 != 0 || ldw < K || ldw % (f8 ? 16 : 8) != 0 || ldact < I ||
      ldact % 8 != 0 || (f8 && (s_gate == nullptr || s_up == nullptr || !aligned16(s_gate) || !aligned16(s_up))))
    return TN_EINVAL;
  Params p = {};
  p.X = static_cast<const bf16_t*>(x);
  p.ldx = ldx;
  p.M = M;
  p.K = K;
  p.head_dim = 64;
  p.nstrip = I / 8;                  // a strip = 8 rows of gate_proj + the same 8 of up_proj -> 8 features of act
  for (int i = 0; i < kMaxSeg; ++i)
    p.seg[i] = Seg{w_gate, w_up, s_gate, s_up, nullptr, static_cast<bf16_t*>(act), ldw, ldact, i == 0 ? p.nstrip : 0x7fffffff,
                   kSwiglu};
  return f8 ? launch<true>(p, static_cast<hipStream_t>(stream)) : launch<false>(p, static_cast<hipStream_t>(stream));
}

}  // namespace smallm
}  // namespace tn

using namespace tn;
using namespace tn::smallm;


extern "C" int tn_gemm_smallm(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                              const long long* ldw, const void* const* bias, void* const* y, const long long* ldy,
                              const int* N, const void* cos_t, const void* sin_t, int head_dim, int rope_mask,
                              void* stream) {
  return linear_entry(x, ldx, M, K, nseg, w, ldw, nullptr, bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask, stream);
}

extern "C" int tn_gemm_smallm_swiglu(const void* x, const void* w_gate, const void* w_up, void* act, int M, int I, int K,
                                     long long ldx, long long ldw, long long ldact, void* stream) {
  return swiglu_entry(x, w_gate, w_up, nullptr, nullptr, false, act, M, I, K, ldx, ldw, ldact, stream);
}

extern "C" int tn_gemm_smallm_fp8(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                  const long long* ldw, const float* const* scale, const void* const* bias, void* const* y,
                                  const long long* ldy, const int* N, const void* cos_t, const void* sin_t, int head_dim,
                                  int rope_mask, void* stream) {
  if (scale == nullptr) return TN_EINVAL;
  return linear_entry(x, ldx, M, K, nseg, w, ldw, scale, bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask, stream);
}

extern "C" int tn_gemm_smallm_swiglu_fp8(const void* x, const void* w_gate, const void* w_up, const float* scale_gate,
                                         const float* scale_up, void* act, int M, int I, int K, long long ldx, long long ldw,
                                         long long ldact, void* stream) {
  return swiglu_entry(x, w_gate, w_up, scale_gate, scale_up, true, act, M, I, K, ldx, ldw, ldact, stream);
}
