// What the two weight-streaming decode GEMMs share (gemm_smallm.hip: up to 128 rows, the waves split K; gemm_midm.hip: up to
// 256 rows, the waves split N and X is staged through LDS): how a launch's strips map to weights and outputs, the lane
// pattern of a weight fragment, the exact FP8 and MXFP4 expansions, the epilogue of one 16 x 16 tile, and the host's entry
// checks.
// Both kernels take W as the 16-row MFMA operand, so a lane holds FOUR output features of ONE row of X (lane l, element e =
// feature row 4 (l >> 4) + e of the strip, X row l & 15) and everything below holds for both.
#pragma once
#include "kv_fp8.h"
#include "mxfp4.h"

namespace tn {
namespace wstream {

constexpr int kMaxSeg = 3;
enum Mode { kPlain = 0, kRope = 1, kSwiglu = 2 };
// How W is stored.  kBf16: bf16 [N, K].  kFp8: e4m3 codes [N, K] with one fp32 scale per row (kv_fp8.h), applied in the
// epilogue.  kMxfp4: e2m1 codes [N, K / 2] with one e8m0 scale byte per 32 elements of K (mxfp4.h), applied in the expansion.
enum Format { kBf16 = 0, kFp8 = 1, kMxfp4 = 2 };
// contraction steps of a chunk, and the bytes of a weight row's chunk a lane reads (the four lanes of a row cover it)
template <Format F> constexpr int kDepthOf = F == kBf16 ? 64 : 128;
template <Format F> constexpr int kLaneBytesOf = F == kMxfp4 ? 16 : 32;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

struct Seg {
  const void* W;         // [N, K] bf16 (kFp8: e4m3 codes; kMxfp4: [N, K / 2] bytes of two codes), pitch ldw elements | bytes
  const void* W2;        // kSwiglu: up_proj, same pitch
  const void* scale;     // kFp8: fp32 [N] row scales of W; kMxfp4: uint8 [N, K / 32] block scales, pitch lds (else unused)
  const void* scale2;    // kFp8 / kMxfp4, kSwiglu: those of W2
  const bf16_t* bias;    // [N] or null
  bf16_t* Y;             // [M, N], pitch ldy (kSwiglu: act [M, I])
  long long ldw, ldy, lds;
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

struct Frag {            // a lane's 32 bytes of one 128-byte line of a weight row: bf16, the operands of two MFMAs; F8, of four
  u32x4_t lo, hi;
};

__device__ __forceinline__ Frag load_w(const void* p) {        // streamed: every byte of W is wanted exactly once
  Frag f;
  f.lo = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  f.hi = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p) + 1);
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

// kMxfp4: a lane's 16 bytes of a weight row's 64-byte chunk are 32 codes under ONE scale byte `sb`, the operands of four
// MFMAs: dword j -> MFMA j, its 8 codes element for element where an FP8 lane's 8 codes sit (mxfp4.h's expand8)
__device__ __forceinline__ void expand32(const u32x4_t c, uint32_t sb, u32x4_t (&e)[4]) {
  const float sc = mx4::scale_f32(sb);
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = mx4::expand8(c[j], sc);
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

// the lane's address in strip j of `sg` for a chunk's fragment: row l & 15 of the strip, bytes LB (l >> 4) .. of its chunk
// (LB = 32: a 128-byte line; kMxfp4's 16: half a line)
template <typename w_t, int LB = 32>
__device__ __forceinline__ const w_t* strip_row(const Seg& sg, int head_dim, int j, int lane) {
  const int l15 = lane & 15;
  const bool second = l15 >= 8;
  const w_t* base = static_cast<const w_t*>((sg.mode == kSwiglu && second) ? sg.W2 : sg.W);
  return base + (long long)(run_base(sg.mode, head_dim, j, second) + (l15 & 7)) * sg.ldw + (LB / (int)sizeof(w_t)) * (lane >> 4);
}

// kMxfp4: ... and of its scale byte: block (l >> 4) of the row's first chunk (a chunk is four blocks, one per lane group)
__device__ __forceinline__ const uint8_t* strip_scale_row(const Seg& sg, int head_dim, int j, int lane) {
  const int l15 = lane & 15;
  const bool second = l15 >= 8;
  const uint8_t* base = static_cast<const uint8_t*>((sg.mode == kSwiglu && second) ? sg.scale2 : sg.scale);
  return base + (long long)(run_base(sg.mode, head_dim, j, second) + (l15 & 7)) * sg.lds + (lane >> 4);
}

// The epilogue of tile t (rows 16 t .. + 15 of X) of strip j of `sg`, run by one whole wave with the finished sums `v` in the
// MFMA's layout: (kFp8: x row scale,) + bias, rounded to bf16, then the row kernels' RoPE / SwiGLU rule with the partner of
// every output in lane l ^ 32, and the store of the rows below M.
template <Format F>
__device__ __forceinline__ void tile_epilogue(const Params& p, const Seg& sg, int j, int t, int lane, f32x4_t v) {
  const int l15 = lane & 15, g = lane >> 4, mode = sg.mode;
  const bool second = g >= 2;
  const int f0 = run_base(mode, p.head_dim, j, second) + 4 * (g & 1);      // the lane's four features f0 .. f0 + 3
  const int m = 16 * t + l15;
  const bool row_ok = m < p.M;
  float own[4], other[4], y[4];
  u32x2_t bv = {0, 0};
  if (sg.bias != nullptr) bv = *reinterpret_cast<const u32x2_t*>(sg.bias + f0);
  if constexpr (F == kFp8)      // the row scales of the lane's four features: the up rows (second run of a SwiGLU strip) have their own
    v *= *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(mode == kSwiglu && second ? sg.scale2 : sg.scale) + f0);
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

// ---- host: the entries' checks, one set for both kernels (max_m: 128 or 256) -------------------------------------------------
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// (codes: whole 128-deep chunks; their weight pitches are bytes and keep the rows 16-byte aligned)
static inline bool x_ok(const void* x, int M, int max_m, int K, long long ldx, Format f) {
  return x != nullptr && aligned16(x) && M >= 1 && M <= max_m && K > 0 && K % (f == kBf16 ? 64 : 128) == 0 && ldx >= K && ldx % 8 == 0;
}

// a weight's row pitch, and its scales: kFp8 fp32 [N], 16-byte aligned; kMxfp4 bytes [N, K / 32], 4-byte aligned rows
static inline bool w_ok(Format f, int K, long long ldw, const void* scale, long long lds) {
  if (f == kBf16) return ldw >= K && ldw % 8 == 0;
  if (f == kFp8) return ldw >= K && ldw % 16 == 0 && scale != nullptr && aligned16(scale);
  return ldw >= K / 2 && ldw % 16 == 0 && scale != nullptr && aligned4(scale) && lds >= K / 32 && lds % 4 == 0;
}

// the linear entries (scale[i]: the scales of codes w[i], lds[i] their pitch, by `f`; kBf16: both unused) -> TN_OK and `p`, or -22
static inline int linear_params(Params& p, int max_m, Format f, const void* x, long long ldx, int M, int K, int nseg,
                                const void* const* w, const long long* ldw, const void* const* scale, const long long* lds,
                                const void* const* bias, void* const* y, const long long* ldy, const int* N,
                                const void* cos_t, const void* sin_t, int head_dim, int rope_mask) {
  if (!x_ok(x, M, max_m, K, ldx, f) || nseg < 1 || nseg > kMaxSeg || w == nullptr || ldw == nullptr || y == nullptr ||
      ldy == nullptr || N == nullptr || rope_mask < 0 || rope_mask >= (1 << nseg) || (f != kBf16 && scale == nullptr) ||
      (f == kMxfp4 && lds == nullptr))
    return TN_EINVAL;
  if (rope_mask != 0 && (cos_t == nullptr || sin_t == nullptr || !aligned16(cos_t) || !aligned16(sin_t) ||
                         (head_dim != 64 && head_dim != 128)))
    return TN_EINVAL;
  p = Params{};
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
    const void* sc = f != kBf16 ? scale[i] : nullptr;
    const long long sp = f == kMxfp4 ? lds[i] : 0;
    if (w[i] == nullptr || y[i] == nullptr || !aligned16(w[i]) || !aligned16(y[i]) || (b != nullptr && !aligned16(b)) ||
        N[i] <= 0 || N[i] % 16 != 0 || !w_ok(f, K, ldw[i], sc, sp) || ldy[i] < N[i] || ldy[i] % 8 != 0 ||
        (rope && N[i] % head_dim != 0))
      return TN_EINVAL;
    strips += N[i] / 16;
    p.seg[i] = Seg{w[i], nullptr, sc, nullptr, static_cast<const bf16_t*>(b), static_cast<bf16_t*>(y[i]), ldw[i], ldy[i], sp,
                   strips, rope ? kRope : kPlain};
  }
  for (int i = nseg; i < kMaxSeg; ++i) {
    p.seg[i] = p.seg[nseg - 1];
    p.seg[i].strip_end = 0x7fffffff;
  }
  p.nstrip = strips;
  return TN_OK;
}

// the SwiGLU entries (codes: s_gate / s_up their scales, of one pitch lds)
static inline int swiglu_params(Params& p, int max_m, Format f, const void* x, const void* w_gate, const void* w_up,
                                const void* s_gate, const void* s_up, long long lds, void* act, int M, int I, int K,
                                long long ldx, long long ldw, long long ldact) {
  if (!x_ok(x, M, max_m, K, ldx, f) || w_gate == nullptr || w_up == nullptr || act == nullptr || !aligned16(w_gate) ||
      !aligned16(w_up) || !aligned16(act) || I <= 0 || I % 16 != 0 || !w_ok(f, K, ldw, s_gate, lds) ||
      !w_ok(f, K, ldw, s_up, lds) || ldact < I || ldact % 8 != 0)
    return TN_EINVAL;
  p = Params{};
  p.X = static_cast<const bf16_t*>(x);
  p.ldx = ldx;
  p.M = M;
  p.K = K;
  p.head_dim = 64;
  p.nstrip = I / 8;                  // a strip = 8 rows of gate_proj + the same 8 of up_proj -> 8 features of act
  for (int i = 0; i < kMaxSeg; ++i)
    p.seg[i] = Seg{w_gate, w_up, s_gate, s_up, nullptr, static_cast<bf16_t*>(act), ldw, ldact, lds, i == 0 ? p.nstrip : 0x7fffffff,
                   kSwiglu};
  return TN_OK;
}

}  // namespace wstream
}  // namespace tn
