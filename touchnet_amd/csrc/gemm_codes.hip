// Prefill GEMM on weight codes (gfx950): Y[m, n] = sum_k X[m, k] dequant(W)[n, k] (+ bias[n]) for any M >= 1 — the linear
// products of a quantised decoder at prefill and long-extend row counts (257 rows and up), where the two weight-streaming
// kernels (gemm_smallm.hip, gemm_midm.hip) stop and the route used to write a bf16 copy of every weight per call.  W stays
// FP8 (e4m3) or MXFP4 codes through HBM, L2 and LDS; a code becomes a bf16 number only on its way into the MFMA operand
// registers, with gemm_stream.h's exact expansions, so the arithmetic contract is that header's: bf16 products on
// v_mfma_f32_16x16x32_bf16, fp32 sums, (FP8: x row scale,) + bias, one rounding to bf16.  DESIGN.md §9.16.
//
//  * Work split.  A workgroup of four waves (2 x 2) owns a 128 x BN output tile, BN = 128 or 64 (the host picks 64 while 128
//    would leave CUs without a tile); a wave owns 64 rows x BN / 2 features = 4 x NB blocks of 16 x 16, NB = BN / 32, 16 NB
//    accumulator registers.  One workgroup per tile; gemm_kernel.h's XCD-aware tile map keeps the workgroups that share a
//    panel of W on one XCD's L2.  The n-tiles of up to three weights that share X (q / k / v) are one list.
//  * K is consumed in 128-deep chunks through a ring of three LDS stages, all by LDS-DMA (buffer_load ... lds, no staging
//    registers).  A stage = X [128 rows][256 B] bf16 + W codes [BN rows][128 B] (FP8) or [BN rows][64 B] + scale bytes
//    [BN rows][4 B] (MXFP4).  The DMA image is lane-linear, so the bank swizzles are applied to the lanes' SOURCE addresses:
//      X      16-byte slot s of row r at slot s ^ (r & 15)          (256-byte rows: the mid-M kernel's rule)
//      FP8    slot s of row r at slot s ^ ((r >> 1) & 7)            (128-byte rows: gemm_kernel.h's ROW rule)
//      MXFP4  slot s of row r at slot s ^ ((r >> 2) & 3)            (64-byte rows)
//    Each puts the sixteen rows a lane group reads into sixteen different 16-byte columns of the 256 bytes the banks span.
//    Rows behind M or N are zero-filled by the buffer descriptors' bounds check: no address outside a tensor is formed.
//  * One barrier per chunk: [wait for my pieces of chunk c] [barrier] [issue chunk c + 2 into the stage chunk c - 1 left]
//    [MFMAs of chunk c].  The wait is vmcnt(pieces of one stage) — chunk c + 1 stays in flight — except on the last chunk.
//  * Fragments: gemm_stream.h's lane pattern.  Lane l reads bytes 32 (l >> 4) .. + 31 (MXFP4: 16 (l >> 4) .. + 15, and scale
//    byte l >> 4) of code row l & 15 of a block, expands them to the operands of four MFMAs, and each feeds the four row
//    blocks of the wave tile: 32 (16 + 4) conversion instructions per 16 MFMAs.  X: slots 4 (l >> 4) + j of row l & 15.
//    Per accumulator the chunks and the four MFMAs of a chunk run in ascending order whatever M, N, BN or the tile: the
//    order of an output's K terms depends on K alone.
//  * Epilogues straight from the accumulators (a lane holds four consecutive features of one row: 8-byte stores).  SwiGLU:
//    the W tile interleaves 16-row blocks of gate_proj and up_proj, so accumulator blocks 2 p and 2 p + 1 of a lane are gate
//    and up of the same features; only act = silu(gate) * up is written, with gemm_stream.h's rule.  RoPE is not fused:
//    the callers run the rotary row kernel on the plain product, which is the same bits by the project's rule.
#include "gemm_kernel.h"
#include "gemm_stream.h"

namespace tn {
namespace prefill {
using namespace wstream;
using gemm::lds_ptr_t;

constexpr int BM = 128, kThreads = 256, kDepth = 128, kStages = 3;
constexpr int kXStage = BM * 2 * kDepth;               // 32 KB
constexpr int kXPieces = kXStage / 1024 / 4;           // 1 KB DMA instructions per wave and stage: 8

template <int BN, Format F>
struct Geo {
  static constexpr int NB = BN / 32;                             // 16-feature blocks per wave
  static constexpr int kRow = F == kMxfp4 ? 64 : 128;            // bytes of a code row's chunk
  // (MXFP4 scales: a 16-row block's 16 dwords in a 256-byte slot of their own — a DMA instruction writes 4 bytes for every
  //  lane, and lanes 16 .. 63 write zeros into the slot's padding instead of being masked off)
  static constexpr int kW = BN * kRow, kS = F == kMxfp4 ? BN / 16 * 256 : 0;
  static constexpr int kStage = kXStage + kW + kS;
  static constexpr int kPieces = kXPieces + NB;                  // DMA instructions per wave and stage (MXFP4: NB / 2 + NB / 2)
};

// the launch's n-tile list: end[i] = n-tiles of segments 0 .. i, n[i] = output features of segment i (SwiGLU: of act)
struct Tiles {
  int nbm, ntn;
  int end[kMaxSeg], n[kMaxSeg];
};

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The MXFP4 scale dwords are inline-asm LDS reads retired by wait_scales: hipcc puts `s_waitcnt vmcnt(0)` in front of a
// scalar-typed LDS read while an LDS-DMA is pending (the 16-byte vector reads it counts itself).
__device__ __forceinline__ uint32_t ds_b32(uint32_t addr) {
  uint32_t r;
  asm volatile("ds_read_b32 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
template <int NB> __device__ __forceinline__ void wait_scales(uint32_t (&sw)[NB]) {
  if constexpr (NB == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sw[0]), "+v"(sw[1]), "+v"(sw[2]), "+v"(sw[3]));
  else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sw[0]), "+v"(sw[1]));
}

template <int BN, Format F, bool SWIGLU>
__device__ __forceinline__ void body(const Params& p, const Tiles& tl, unsigned char* smem) {
  using G = Geo<BN, F>;
  constexpr bool F4 = F == kMxfp4;
  constexpr int NB = G::NB, kRow = G::kRow, kPer = SWIGLU ? BN / 2 : BN;   // output features per tile
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;

  int tm, tn, s = 0, first = 0;
  gemm::tile_of_block(blockIdx.x, tl.nbm, tl.ntn, tm, tn);
#pragma unroll
  for (int i = 0; i + 1 < kMaxSeg; ++i)
    if (tn >= tl.end[i]) {
      s = i + 1;
      first = tl.end[i];
    }
  const Seg& sg = p.seg[s];
  const int N = tl.n[s], m0 = tm * BM, n0 = (tn - first) * kPer;

  // descriptors over exactly the rows of this tile that exist: everything else reads zeros
  const int xrows = min(p.M - m0, BM), wrows = min(N - n0, kPer), ldx2 = (int)(2 * p.ldx), ldw = (int)sg.ldw;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.X + (long long)m0 * p.ldx), 0, (xrows - 1) * ldx2 + 2 * p.K, 0x00020000);
  const int wlen = (wrows - 1) * ldw + (F4 ? p.K / 2 : p.K);
  const __amdgpu_buffer_rsrc_t wrs0 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(static_cast<const uint8_t*>(sg.W) + (long long)n0 * ldw), 0, wlen, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs1 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(static_cast<const uint8_t*>(SWIGLU ? sg.W2 : sg.W) + (long long)n0 * ldw), 0, wlen, 0x00020000);
  const int lds = (int)sg.lds, slen = F4 ? (wrows - 1) * lds + p.K / 32 : 0;
  const __amdgpu_buffer_rsrc_t srs0 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(static_cast<const uint8_t*>(F4 ? sg.scale : sg.W) + (long long)n0 * lds), 0, slen, 0x00020000);
  const __amdgpu_buffer_rsrc_t srs1 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(static_cast<const uint8_t*>(F4 ? (SWIGLU ? sg.scale2 : sg.scale) : sg.W) + (long long)n0 * lds), 0, slen,
      0x00020000);

  // ---- the fill: per-lane source offsets of this wave's pieces (the image in LDS is lane-linear) ----
  // tile row t of W: plain = feature n0 + t; SwiGLU = block t >> 4 is gate (even) or up (odd) of features 16 (t >> 5) + (t & 15)
  auto src_row = [](int t) { return SWIGLU ? 16 * (t >> 5) + (t & 15) : t; };
  int xv[kXPieces], wv[NB], sv[F4 ? NB / 2 : 1];
#pragma unroll
  for (int q = 0; q < kXPieces; ++q) {       // piece q = rows 32 wave + 4 q + (lane >> 4), a lane = one 16-byte slot
    const int r = 32 * wave + 4 * q + (lane >> 4);
    xv[q] = r * ldx2 + (((lane & 15) ^ (r & 15)) << 4);
  }
  if constexpr (F4) {
#pragma unroll
    for (int q = 0; q < NB / 2; ++q) {       // piece q = block NB / 2 * wave + q: 16 rows of 64 bytes; and its 16 scale dwords
      const int blk = NB / 2 * wave + q, t = 16 * blk + (lane >> 2);
      wv[q] = src_row(t) * ldw + (((lane & 3) ^ ((t >> 2) & 3)) << 4);
      sv[q] = lane < 16 ? src_row(16 * blk + l15) * lds : slen;          // (behind the descriptor's end: zeros, no traffic)
    }
  } else {
#pragma unroll
    for (int q = 0; q < NB; ++q) {           // piece q = rows 8 (NB wave + q) + (lane >> 3) of 128 bytes
      const int t = 8 * (NB * wave + q) + (lane >> 3);
      wv[q] = src_row(t) * ldw + (((lane & 7) ^ ((t >> 1) & 7)) << 4);
    }
  }
  auto fill = [&](int stage, int c) {
    unsigned char* st = smem + stage * G::kStage;
#pragma unroll
    for (int q = 0; q < kXPieces; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_ptr_t)(st + (32 * wave + 4 * q) * 256), 16, xv[q], c * 256, 0, 0);
    if constexpr (F4) {
#pragma unroll
      for (int q = 0; q < NB / 2; ++q) {
        const int blk = NB / 2 * wave + q;
        const bool up = SWIGLU && (blk & 1);
        const lds_ptr_t wdst = (lds_ptr_t)(st + kXStage + blk * 1024), sdst = (lds_ptr_t)(st + kXStage + G::kW + blk * 256);
        if (up) {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs1, wdst, 16, wv[q], c * 64, 0, 0);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(srs1, sdst, 4, sv[q], c * 4, 0, 0);
        } else {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs0, wdst, 16, wv[q], c * 64, 0, 0);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(srs0, sdst, 4, sv[q], c * 4, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const bool up = SWIGLU && (((NB * wave + q) >> 1) & 1);
        const lds_ptr_t wdst = (lds_ptr_t)(st + kXStage + (NB * wave + q) * 1024);
        if (up) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs1, wdst, 16, wv[q], c * 128, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs0, wdst, 16, wv[q], c * 128, 0, 0);
      }
    }
  };

  // ---- the reads: X slots 4 g + j of row 64 wr + 16 mb + l15; code row BN / 2 wc + 16 nb + l15, its bytes (32 | 16) g .. ----
  int xrd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xrd[j] = (64 * wr + l15) * 256 + (((4 * g + j) ^ l15) << 4);
  const int wt = BN / 2 * wc + l15;
  const int wrd0 = kXStage + wt * kRow + (F4 ? (g ^ ((l15 >> 2) & 3)) << 4 : ((2 * g) ^ ((l15 >> 1) & 7)) << 4);
  const int wrd1 = kXStage + wt * kRow + (((2 * g + 1) ^ ((l15 >> 1) & 7)) << 4);      // (FP8: the second 16 bytes)
  const uint32_t srd = (uint32_t)(size_t)(lds_ptr_t)smem + kXStage + G::kW + NB * wc * 256 + l15 * 4;

  f32x4_t acc[4][NB];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto mac = [&](const unsigned char* st) {
    uint32_t sw[NB];
    if constexpr (F4) {
      const uint32_t sa = srd + (uint32_t)(st - smem);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) sw[nb] = ds_b32(sa + nb * 256);
    }
    u32x4_t x[4][4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int j = 0; j < 4; ++j) x[mb][j] = *reinterpret_cast<const u32x4_t*>(st + xrd[j] + mb * 16 * 256);
    if constexpr (F4) wait_scales<NB>(sw);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      u32x4_t e[4];
      if constexpr (F4) {
        const u32x4_t c = *reinterpret_cast<const u32x4_t*>(st + wrd0 + nb * 16 * kRow);
        expand32(c, (sw[nb] >> (8 * g)) & 0xffu, e);
      } else {
        expand16(*reinterpret_cast<const u32x4_t*>(st + wrd0 + nb * 16 * kRow), e[0], e[1]);
        expand16(*reinterpret_cast<const u32x4_t*>(st + wrd1 + nb * 16 * kRow), e[2], e[3]);
      }
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, e[j]),
                                                                __builtin_bit_cast(bf16x8_t, x[mb][j]), acc[mb][nb], 0, 0, 0);
    }
  };

  // (every condition below depends on K alone: all four waves reach every barrier)
  const int nch = p.K / kDepth;
  fill(0, 0);
  if (nch > 1) fill(1, 1);
  int stage = 0;
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) wait_vm<G::kPieces>();   // my pieces of chunk c have landed; chunk c + 1 may stay in flight
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();             // everybody's have; nobody reads the stage of chunk c - 1 any more
    if (c + 2 < nch) fill(stage >= 1 ? stage - 1 : kStages - 1, c + 2);
    mac(smem + stage * G::kStage);
    stage = stage + 1 == kStages ? 0 : stage + 1;
  }

  // ---- epilogue: gemm_stream.h's rule per lane: four features f .. f + 3 of row m ----
  auto bias_of = [&](int f, float (&b)[4]) {
    u32x2_t bv = {0, 0};
    if (sg.bias != nullptr) bv = *reinterpret_cast<const u32x2_t*>(sg.bias + f);
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = __uint_as_float(e & 1 ? bv[e >> 1] & 0xffff0000u : bv[e >> 1] << 16);
  };
  if constexpr (SWIGLU) {
#pragma unroll
    for (int pr = 0; pr < NB / 2; ++pr) {
      const int f = n0 + 16 * (wc * (NB / 2) + pr) + 4 * g;
      if (f >= N) continue;
      f32x4_t sg_v = {1.f, 1.f, 1.f, 1.f}, su_v = sg_v;
      if constexpr (F == kFp8) {
        sg_v = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(sg.scale) + f);
        su_v = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(sg.scale2) + f);
      }
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int m = m0 + 64 * wr + 16 * mb + l15;
        f32x4_t gv = acc[mb][2 * pr], uv = acc[mb][2 * pr + 1];
        if constexpr (F == kFp8) {
          gv *= sg_v;
          uv *= su_v;
        }
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gate = rbf(gv[e] + 0.f), up = rbf(uv[e] + 0.f);
          y[e] = rbf(gate * sigmoid_fast(gate)) * up;
        }
        if (m < p.M)
          *reinterpret_cast<u32x2_t*>(sg.Y + (long long)m * sg.ldy + f) = u32x2_t{pack2bf(y[0], y[1]), pack2bf(y[2], y[3])};
      }
    }
  } else {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int f = n0 + BN / 2 * wc + 16 * nb + 4 * g;
      if (f >= N) continue;
      float b[4];
      bias_of(f, b);
      f32x4_t sc = {1.f, 1.f, 1.f, 1.f};
      if constexpr (F == kFp8) sc = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(sg.scale) + f);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int m = m0 + 64 * wr + 16 * mb + l15;
        f32x4_t v = acc[mb][nb];
        if constexpr (F == kFp8) v *= sc;
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = rbf(v[e] + b[e]);
        if (m < p.M)
          *reinterpret_cast<u32x2_t*>(sg.Y + (long long)m * sg.ldy + f) = u32x2_t{pack2bf(y[0], y[1]), pack2bf(y[2], y[3])};
      }
    }
  }
}

template <int BN, Format F, bool SWIGLU>
__global__ __launch_bounds__(kThreads) void kernel(const Params p, const Tiles tl) {
  static_assert(F != kBf16 && kStages * Geo<BN, F>::kStage <= 160 * 1024, "codes only; the ring fits the LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[kStages * Geo<BN, F>::kStage];
  body<BN, F, SWIGLU>(p, tl, smem);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// The tile list for output features `per` wide per n-tile -> its length
static inline int tile_list(const Params& p, bool swiglu, int per, Tiles& tl) {
  tl.nbm = (p.M + BM - 1) / BM;
  int prev = 0, tiles = 0;
  for (int i = 0; i < kMaxSeg; ++i) {
    const bool used = i == 0 || prev < p.nstrip;
    tl.n[i] = used ? (swiglu ? 8 : 16) * (p.seg[i].strip_end - prev) : 0;
    tiles += (tl.n[i] + per - 1) / per;
    tl.end[i] = tiles;
    if (used) prev = p.seg[i].strip_end;
  }
  tl.ntn = tiles;
  return tl.nbm * tiles;
}

template <int BN, Format F>
static int launch_bn(const Params& p, bool swiglu, const Tiles& tl, hipStream_t st) {
  const dim3 grid(tl.nbm * tl.ntn), block(kThreads);
  if (swiglu)
    hipLaunchKernelGGL((kernel<BN, F, true>), grid, block, 0, st, p, tl);
  else
    hipLaunchKernelGGL((kernel<BN, F, false>), grid, block, 0, st, p, tl);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

// BN = 64 while 128-wide tiles would leave some of the 256 CUs without one (a prefill of a few hundred rows of a 4096-wide
// layer); the summation order does not depend on it
template <Format F>
static int launch(const Params& p, bool swiglu, hipStream_t st) {
  Tiles tl;
  if (tile_list(p, swiglu, swiglu ? 64 : 128, tl) >= 256) return launch_bn<128, F>(p, swiglu, tl, st);
  tile_list(p, swiglu, swiglu ? 32 : 64, tl);
  return launch_bn<64, F>(p, swiglu, tl, st);
}

// (a pitch or a contraction the kernel's 32-bit byte offsets could not span is refused with the rest)
static bool spans_ok(const Params& p) {
  constexpr long long kMax = 1LL << 23;
  for (int i = 0; i < kMaxSeg; ++i)
    if (p.seg[i].ldw >= kMax || p.seg[i].lds >= kMax) return false;
  return p.ldx < kMax && p.K < kMax;
}

static int run(int rc, const Params& p, Format f, bool swiglu, void* stream) {
  if (rc != TN_OK) return rc;
  if (!spans_ok(p)) return TN_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  return f == kMxfp4 ? launch<kMxfp4>(p, swiglu, st) : launch<kFp8>(p, swiglu, st);
}

constexpr int kAnyM = 0x7fffffff;

}  // namespace prefill
}  // namespace tn

using namespace tn;
using namespace tn::prefill;

extern "C" int tn_gemm_prefill_fp8(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                   const long long* ldw, const float* const* scale, const void* const* bias, void* const* y,
                                   const long long* ldy, const int* N, void* stream) {
  Params p;
  return run(linear_params(p, kAnyM, kFp8, x, ldx, M, K, nseg, w, ldw, reinterpret_cast<const void* const*>(scale), nullptr,
                           bias, y, ldy, N, nullptr, nullptr, 0, 0),
             p, kFp8, false, stream);
}

extern "C" int tn_gemm_prefill_mxfp4(const void* x, long long ldx, int M, int K, int nseg, const void* const* w,
                                     const long long* ldw, const unsigned char* const* scales, const long long* lds,
                                     const void* const* bias, void* const* y, const long long* ldy, const int* N,
                                     void* stream) {
  Params p;
  return run(linear_params(p, kAnyM, kMxfp4, x, ldx, M, K, nseg, w, ldw, reinterpret_cast<const void* const*>(scales), lds,
                           bias, y, ldy, N, nullptr, nullptr, 0, 0),
             p, kMxfp4, false, stream);
}

extern "C" int tn_gemm_prefill_swiglu_fp8(const void* x, const void* w_gate, const void* w_up, const float* scale_gate,
                                          const float* scale_up, void* act, int M, int I, int K, long long ldx,
                                          long long ldw, long long ldact, void* stream) {
  Params p;
  return run(swiglu_params(p, kAnyM, kFp8, x, w_gate, w_up, scale_gate, scale_up, 0, act, M, I, K, ldx, ldw, ldact), p, kFp8,
             true, stream);
}

extern "C" int tn_gemm_prefill_swiglu_mxfp4(const void* x, const void* w_gate, const void* w_up,
                                            const unsigned char* scales_gate, const unsigned char* scales_up, void* act,
                                            int M, int I, int K, long long ldx, long long ldw, long long lds, long long ldact,
                                            void* stream) {
  Params p;
  return run(swiglu_params(p, kAnyM, kMxfp4, x, w_gate, w_up, scales_gate, scales_up, lds, act, M, I, K, ldx, ldw, ldact), p,
             kMxfp4, true, stream);
}
