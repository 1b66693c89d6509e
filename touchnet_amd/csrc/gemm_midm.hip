// Mid-M weight-streaming GEMM (gfx950): Y[m, n] = sum_k X[m, k] W[n, k] (+ bias[n]) for 1 <= M <= 256 rows — the decode-side
// linear products at the row counts of beam search over a batch, large decode batches and chunked extends, where
// gemm_smallm.hip stops scaling: there every wave loads every tile of X from L2 into registers.  The bound
// is still the HBM bytes of W, read exactly once; what changes is how X reaches the MFMAs:
//
//  * The four waves of a workgroup split N, not K.  A wave owns S consecutive 16-row strips (gemm_stream.h) and walks the
//    whole contraction itself, chunk by chunk in ascending order (a chunk = one 128-byte line of every weight row: 64 deep
//    for bf16, 128 for FP8 codes), the MFMAs of a chunk in ascending order too.  Nothing is summed across waves or
//    workgroups: the order of an output's K terms depends on K alone, not on M, the row, S or the tile count.  (It is NOT
//    the small-M kernel's ((w0 + w1) + w2) + w3: the two kernels agree to the last bits only on integer data.)
//  * W goes from global memory straight into the MFMA operand registers with non-temporal loads, the small-M kernel's lane
//    pattern: lane l reads bytes 32 (l >> 4) .. + 31 of row l & 15 of its strip.  Three fragment sets per strip rotate: the
//    loads of chunk c + 2 are issued before the MFMAs of chunk c.
//  * X is staged through LDS once per workgroup and shared by the four waves.  A stage holds one chunk of all 16 MT rows,
//    [16 MT][128 B] (bf16) or [16 MT][256 B] (FP8: 128 deep), two stages.  While the MFMAs of chunk c read stage c & 1, every
//    thread has its share of chunk c + 1 in flight from L2 (MT / 2 or MT 16-byte slots) and writes it to the other stage
//    behind them; ONE barrier per chunk, at its start, orders both the fill and the re-use of a stage.  Rows >= M are
//    zeros, written once before the loop and never loaded.  The L2 traffic of X is M K 2 bytes per workgroup whatever MT.
//  * A lane reads its fragment of tile t as 16-byte LDS reads of row 16 t + (l & 15), slots (2 | 4) (l >> 4) + j — the
//    pattern of W, so the permutation of the contraction index cancels as in the small-M kernel.  Slot s of row r is stored
//    at slot s ^ swz(r) of the row: swz(r) = (r >> 1) & 7 for 128-byte rows, r & 15 for 256-byte rows.  The sixteen lanes of
//    a group read one slot of sixteen consecutive rows; with the swizzle they land in sixteen different 16-byte columns of
//    the 256 bytes the banks span (DESIGN.md §9.14 has the argument), so reads — and the fills — are free of bank conflicts.
//  * One fragment of X read from LDS feeds the MFMAs of S strips; accumulators are MT x S x 4 fp32 per lane.
//  * Epilogues are gemm_stream.h's, per wave on its own strips straight from the accumulators.
//
// MXFP4 weights (F = kMxfp4): the chunk stays 128 deep, a 64-byte half line per weight row, so the stage of
// X, its swizzle and the four LDS reads per tile are the FP8 arm's.  A lane's fragment of W is ONE 16-byte load (32 codes,
// one scale block) and ONE scale byte, block 4 c + (l >> 4) of its row, issued together; gemm_stream.h's expand32 applies the
// scale in the conversion.  A fragment is 5 registers, so the ring holds FIVE sets: chunks c + 1 .. c + 4 are in flight under
// the MFMAs of chunk c, the FP8 ring's bytes, and both halves of a line are asked for by one wave one chunk apart.
//
// Every barrier is reached by all four waves: the chunk loop's trip count depends on K alone, a wave whose strips lie past
// the last one re-reads the last strip and stores nothing, and there is no barrier behind the loop.
#include <type_traits>

#include "gemm_stream.h"

namespace tn {
namespace midm {
using namespace wstream;

constexpr int kWaves = 4, kThreads = kWaves * 64;
constexpr int kMaxM = 256;
// fragment sets of W per strip: chunk c + kRing - 1 is loaded under the MFMAs of chunk c
template <Format F> constexpr int kRingOf = F == kMxfp4 ? 5 : 3;

struct FragM {           // kMxfp4: a lane's 16 bytes of one 64-byte chunk of a weight row, and the scale byte of those 32 codes
  u32x4_t c;
  uint32_t sb;
};

template <int MT, int S, Format F>
__global__ __launch_bounds__(kThreads) void kernel(const Params p) {
  constexpr bool F8 = F != kBf16, F4 = F == kMxfp4;              // (F8: codes, 128-deep chunks and 256-byte rows of X)
  using w_t = std::conditional_t<F == kBf16, bf16_t, uint8_t>;   // one stored element of W (kMxfp4: a byte of two codes)
  using WFrag = std::conditional_t<F4, FragM, Frag>;
  constexpr int kDepth = kDepthOf<F>, kLane = kLaneBytesOf<F>, kRing = kRingOf<F>;
  constexpr int kRowBytes = 2 * kDepth, kSlots = kRowBytes / 16; // a row of X of one chunk, in 16-byte slots
  constexpr int kStage = 16 * MT * kRowBytes;
  constexpr int kRowStep = kThreads / kSlots;                    // rows between a thread's slots of a stage: 32 | 16
  constexpr int kPer = 16 * MT / kRowStep;                       // its slots per stage: MT / 2 | MT
  constexpr int kFrag = kSlots / 4;                              // 16-byte reads of a lane per tile and chunk = MFMAs: 2 | 4
  static_assert(MT % 2 == 0 && 2 * kStage <= 160 * 1024, "a stage is whole rounds of the 256 threads; two stages fit the LDS");
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * kStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int strip0 = (blockIdx.x * kWaves + wave) * S;

  // a wave past the last strip re-reads the last strip and stores nothing for it
  const w_t* wp[S];
  const uint8_t* sp[F4 ? S : 1];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    int j;
    const Seg& sg = p.seg[locate(p, min(strip0 + s, p.nstrip - 1), j)];
    wp[s] = strip_row<w_t, kLane>(sg, p.head_dim, j, lane);
    if constexpr (F4) sp[s] = strip_scale_row(sg, p.head_dim, j, lane);
  }

  // the fill: slot `fslot` of rows frow + kRowStep r.  (swz(row) does not change with r: kRowStep / 2 % 8 == 0 | kRowStep % 16 == 0.)
  const int fslot = tid % kSlots, frow = tid / kSlots;
  const int fdst = frow * kRowBytes + ((fslot ^ (F8 ? frow & 15 : (frow >> 1) & 7)) << 4);
  const bf16_t* xsrc = p.X + (long long)frow * p.ldx + 8 * fslot;
  u32x4_t xr[kPer];
  auto fetch = [&](int c) {
#pragma unroll
    for (int r = 0; r < kPer; ++r)
      if (frow + kRowStep * r < p.M)
        xr[r] = *reinterpret_cast<const u32x4_t*>(xsrc + (long long)(kRowStep * r) * p.ldx + (long long)kDepth * c);
  };
  auto put = [&](int stage) {
#pragma unroll
    for (int r = 0; r < kPer; ++r)
      if (frow + kRowStep * r < p.M)
        *reinterpret_cast<u32x4_t*>(xs + stage * kStage + fdst + kRowStep * r * kRowBytes) = xr[r];
  };
  // the reads: slot kFrag g + j of row 16 t + l15 (swz(16 t + l15) = swz(l15))
  int rd[kFrag];
#pragma unroll
  for (int j = 0; j < kFrag; ++j) rd[j] = l15 * kRowBytes + (((kFrag * g + j) ^ (F8 ? l15 : l15 >> 1)) << 4);

  f32x4_t acc[S][MT];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[s][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nch = p.K / kDepth;
  WFrag w[kRing][S];
  auto load = [&](WFrag (&f)[S], int c) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if constexpr (F4) {
        f[s].c = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wp[s] + 64 * (long long)c));
        f[s].sb = sp[s][4 * (long long)c];
      } else {
        f[s] = load_w(wp[s] + (128 / (int)sizeof(w_t)) * (long long)c);
      }
    }
  };
  auto mac = [&](const WFrag (&f)[S], const unsigned char* stage) {
    u32x4_t e[S][kFrag];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if constexpr (F4) {
        expand32(f[s].c, f[s].sb, e[s]);
      } else if constexpr (F8) {
        expand16(f[s].lo, e[s][0], e[s][1]);
        expand16(f[s].hi, e[s][2], e[s][3]);
      } else {
        e[s][0] = f[s].lo;
        e[s][1] = f[s].hi;
      }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      u32x4_t x[kFrag];
#pragma unroll
      for (int j = 0; j < kFrag; ++j) x[j] = *reinterpret_cast<const u32x4_t*>(stage + 16 * t * kRowBytes + rd[j]);
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int j = 0; j < kFrag; ++j)
          acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, e[s][j]),
                                                              __builtin_bit_cast(bf16x8_t, x[j]), acc[s][t], 0, 0, 0);
    }
  };

#pragma unroll
  for (int u = 0; u + 1 < kRing; ++u)
    if (u < nch) load(w[u], u);
  fetch(0);
#pragma unroll
  for (int r = 0; r < kPer; ++r)          // the rows behind M of both stages: zeros, once
    if (frow + kRowStep * r >= p.M) {
      *reinterpret_cast<u32x4_t*>(xs + fdst + kRowStep * r * kRowBytes) = u32x4_t{0, 0, 0, 0};
      *reinterpret_cast<u32x4_t*>(xs + kStage + fdst + kRowStep * r * kRowBytes) = u32x4_t{0, 0, 0, 0};
    }
  put(0);
  // (every condition in this loop depends on K alone: all four waves reach every barrier)
  for (int c = 0; c < nch; c += kRing) {
#pragma unroll
    for (int u = 0; u < kRing; ++u) {
      const int cu = c + u;
      if (cu >= nch) break;
      __syncthreads();          // stage cu & 1 is filled; nobody reads the other stage any more
      if (cu + 1 < nch) fetch(cu + 1);
      if (cu + kRing - 1 < nch) load(w[(u + kRing - 1) % kRing], cu + kRing - 1);
      mac(w[u], xs + (cu & 1) * kStage);
      if (cu + 1 < nch) put((cu + 1) & 1);
    }
  }

#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int st = strip0 + s;
    if (st < p.nstrip) {
      int j;
      const Seg& sg = p.seg[locate(p, st, j)];
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (16 * t < p.M) tile_epilogue<F>(p, sg, j, t, lane, acc[s][t]);
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// Strips per wave.  Two strips halve the LDS bytes read per MFMA (a fragment of X feeds both), but a workgroup then owns
// eight strips: S = 2 only while that leaves a workgroup for every one of the 256 CUs.  Depends on the strip count alone;
// the summation order does not depend on S.
static inline int strips_per_wave(int nstrip) { return (nstrip + 2 * kWaves - 1) / (2 * kWaves) >= 256 ? 2 : 1; }

template <int MT, Format F>
static int launch_mt(const Params& p, hipStream_t st) {
  const int S = strips_per_wave(p.nstrip);
  const dim3 grid((p.nstrip + kWaves * S - 1) / (kWaves * S)), block(kThreads);
  if (S == 2)
    hipLaunchKernelGGL((kernel<MT, 2, F>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((kernel<MT, 1, F>), grid, block, 0, st, p);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

// tile counts 4, 6, 8, 12, 16: M rounds up to the next one (the rows behind M are zeros in LDS and cost MFMAs, not traffic)
template <Format F>
static int launch(const Params& p, hipStream_t st) {
  const int mt = (p.M + 15) / 16;
  if (mt <= 4) return launch_mt<4, F>(p, st);
  if (mt <= 6) return launch_mt<6, F>(p, st);
  if (mt <= 8) return launch_mt<8, F>(p, st);
  if (mt <= 12) return launch_mt<12, F>(p, st);
  return launch_mt<16, F>(p, st);
}

static int run(int rc, const Params& p, Format f, void* stream) {
  if (rc != TN_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  return f == kMxfp4 ? launch<kMxfp4>(p, st) : f == kFp8 ? launch<kFp8>(p, st) : launch<kBf16>(p, st);
}

}  // namespace midm
}  // namespace tn

using namespace tn;
using namespace tn::midm;

extern "C" int tn_gemm_midm(const void* x, long long ldx, int M, int K, int nseg, const void* const* w, const long long* ldw,
                            const void* const* bias, void* const* y, const long long* ldy, const int* N, const void* cos_t,
                            const void* sin_t, int head_dim, int rope_mask, void* stream) {
  Params p;
  return run(linear_params(p, kMaxM, kBf16, x, ldx, M, K, nseg, w, ldw, nullptr, nullptr, bias, y, ldy, N, cos_t, sin_t,
                           head_dim, rope_mask),
             p, kBf16, stream);
}

extern "C" int tn_gemm_midm_swiglu(const void* x, const void* w_gate, const void* w_up, void* act, int M, int I, int K,
                                   long long ldx, long long ldw, long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, kBf16, x, w_gate, w_up, nullptr, nullptr, 0, act, M, I, K, ldx, ldw, ldact), p, kBf16,
             stream);
}

extern "C" int tn_gemm_midm_fp8(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                const long long* ldw, const float* const* scale, const void* const* bias, void* const* y,
                                const long long* ldy, const int* N, const void* cos_t, const void* sin_t, int head_dim,
                                int rope_mask, void* stream) {
  Params p;
  return run(linear_params(p, kMaxM, kFp8, x, ldx, M, K, nseg, w, ldw, reinterpret_cast<const void* const*>(scale), nullptr,
                           bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask),
             p, kFp8, stream);
}

extern "C" int tn_gemm_midm_swiglu_fp8(const void* x, const void* w_gate, const void* w_up, const float* scale_gate,
                                       const float* scale_up, void* act, int M, int I, int K, long long ldx, long long ldw,
                                       long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, kFp8, x, w_gate, w_up, scale_gate, scale_up, 0, act, M, I, K, ldx, ldw, ldact), p, kFp8,
             stream);
}

extern "C" int tn_gemm_midm_mxfp4(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                  const long long* ldw, const unsigned char* const* scales, const long long* lds,
                                  const void* const* bias, void* const* y, const long long* ldy, const int* N,
                                  const void* cos_t, const void* sin_t, int head_dim, int rope_mask, void* stream) {
  Params p;
  return run(linear_params(p, kMaxM, kMxfp4, x, ldx, M, K, nseg, w, ldw, reinterpret_cast<const void* const*>(scales), lds,
                           bias, y, ldy, N, cos_t, sin_t, head_dim, rope_mask),
             p, kMxfp4, stream);
}

extern "C" int tn_gemm_midm_swiglu_mxfp4(const void* x, const void* w_gate, const void* w_up, const unsigned char* scales_gate,
                                         const unsigned char* scales_up, void* act, int M, int I, int K, long long ldx,
                                         long long ldw, long long lds, long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kMaxM, kMxfp4, x, w_gate, w_up, scales_gate, scales_up, lds, act, M, I, K, ldx, ldw, ldact), p,
             kMxfp4, stream);
}
