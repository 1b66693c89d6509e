// Hand-written bf16 MFMA GEMM for gfx950 (MI355X): every product of the linear layers of the decoder / audio-tower
// blocks — forward, input gradient and weight gradient — in the layout the tensors already have.
//
//     C[M, N] (bf16) = sum over segments s of  opA_s · opB_s^T   (+ bias[N]) (+ C)       fp32 accumulation, one rounding
//
// Each operand of each segment is stored either
//   ROW    X[R, K]  contraction-contiguous (row pitch ld)   — x in y = x W^T, W in y = x W^T, dY in dX = dY W
//   KMAJ   X[K, R]  contraction-major      (row pitch ld)   — W in dX = dY W, dY and x in dW = dY^T x
// so the three GEMMs of a linear layer (transformers' LlamaMLP / LlamaAttention projections as swapped at
// touchnet/models/llama/__init__.py:11-15) read nn.Linear's own tensors: no transposed copies of
// W, dY or x are ever made (a ROW-only kernel needed 480 standalone transpose launches per step).  Several segments = one
// accumulator over several (A, B) pairs: dX = dQ Wq + dK Wk + dV Wv is ONE launch without bf16 round trips.
//
// Two kernels, one stage ring, and nothing that selects among alternatives: which one a product runs on follows from its
// shape (`launch` below states the rule).
//   Kernel16  v_mfma_f32_16x16x32_bf16  row-stored A — every forward and input-gradient product, with the fused SwiGLU /
//                                       RoPE / GELU epilogues
//   Kernel    v_mfma_f32_32x32x16_bf16  contraction-major A (the weight gradients: plain, grouped — three
//                                       products from Params or any number from a table —, with the bias gradient, fp32 output), split-K units, products with a transposed copy
// The measured alternatives (a half-stage ring, a four-wave geometry with the accumulators in AGPRs, other DMA placements)
// are history: DESIGN.md 5.5 has what they showed.
//
// Structure of Kernel (MI355X-first; numbers from MI355X_MICROARCH.md; Kernel16 differs in the MFMA shape only, see there):
//  * 256 x 256 output tile per 512-thread workgroup (8 waves = 2(M) x 4(N), wave tile 128 x 64 = 4 x 2 blocks of
//    v_mfma_f32_32x32x16_bf16, 128 accumulator registers), one workgroup per CU, two waves per SIMD.
//  * K is consumed in 64-deep operand stages of 32 KB that reach LDS by LDS-DMA (buffer_load_dwordx4 ... lds: no staging
//    registers, no ds_write pass) in FULL 128-byte lines.  The DMA image is lane-linear, so every bank swizzle is
//    applied to the per-lane SOURCE address and undone on the read side:
//      ROW   image [256 r][128 B]: 16-byte chunk c of row r in slot c ^ ((r >> 1) & 7); fragment = one ds_read_b128
//      KMAJ  image [64 k][512 B] : 64-byte group g of row k in position g ^ (k & 3);    fragment = two
//            ds_read_b64_tr_b16 (gfx950 transpose read: the 16 lanes of a group point at 4 k-rows x 32 B and lane i
//            receives column i of that [4 k][16 r] block) — the four k-rows of a 32-lane service group sit in four
//            different 64-byte bank groups: conflict-free, same as the ROW image.
//    Both give a lane the contraction slots k = 8 * (lane >> 5) + (0..7) of row lane & 31, so the modes mix freely.
//  * 160 KB of LDS = ring of FIVE operand slots (operand-stage j = A(t) for j = 2t, B(t) for j = 2t+1, slot j % 5).
//    ONE barrier per stage, in front of its LAST 16-deep quarter (fragments of quarter q+1 are read while quarter q's
//    8 MFMAs run, so the matrix pipe does not drain across it).  The barrier of stage t frees two slots, which take
//    B(t+2) (due one stage later) and A(t+3) (due two stages later); their 8 pieces per wave are placed between the
//    MFMAs of the following quarters by a compile-time table (kPieceB / kPieceA) — never a vmcnt(0) in the loop:
//      wait at the barrier of stage t, in flight oldest first: A(t+1), B(t+1), A(t+2) -> vmcnt(4) = A(t+2) may remain.
//  * Out-of-range rows (M, N not multiples of 256) and exhausted operand streams are zero-filled by the buffer
//    descriptor's bounds check (an exhausted stream's descriptor has length 0: no memory traffic).
//  * XCD-aware bijective workgroup -> tile map (8-tall column-major groups per XCD: the 32 workgroups an XCD runs at
//    once share their A / B panels in its L2).
//  * Epilogue through LDS (the ring is dead by then): XOR-swizzled park per wave, full 128-byte lines out (bias,
//    accumulate-into-C, optional transposed copy).
#pragma once

#include <stdlib.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

namespace tn {
namespace gemm {

constexpr int BM = 256, BN = 256;
constexpr int SLOT = 32768;                          // one operand stage: 256 rows x 64 k bf16
constexpr int LDS_BYTES = 5 * SLOT;
constexpr int NT = 512;
constexpr int MAXSEG = 3;

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

struct Seg {
  const bf16_t* A;
  const bf16_t* B;
  long long lda, ldb;
  int K;
  int pad_;
};

struct Grp {
  bf16_t* C;
  long long ldc;
  int M, N, nbm, nbn;
  int start;           // index of the product's first tile in the launch's tile list (the running sum of nbm * nbn)
  int stages;          // ceil(K / 64)
};

// One product of a table-driven grouped launch (EPI_TABLE): the records lie in device memory, ordered by grp.start
struct Rec {
  Seg seg;
  Grp grp;
  bf16_t* bias_out;    // [M] column sums of A (the bias gradient), or null
};
// (the kernel reads them with scalar loads: the table is written by an earlier launch and never by this one)
typedef const __attribute__((address_space(4))) Rec* rec_ptr_t;
constexpr int MAXTAB = 1024;                         // products per table-driven launch
constexpr int TABCHUNK = 32;                         // records one upload launch carries in its kernel arguments

// What the epilogue does with a finished tile (Kernel: PLAIN, GROUPED, BIASG; Kernel16: PLAIN and the fused ones):
//   EPI_PLAIN       C = acc (+ bias) (+ C), optional transposed copy
//   EPI_GROUPED     the same per product of a grouped launch (no bias / transposed copy)
//   EPI_SWIGLU_FWD  the MLP's gate and up products as ONE launch: an output tile is 256 rows x (128 gate columns + 128 up
//                   columns), the B stage image interleaves 32-row runs of gate_proj and up_proj so that every wave holds
//                   gate (block j = 0) and up (j = 1) of the SAME 32 columns in the same lanes; it writes gate, up (the
//                   backward needs both) and act = silu(gate) * up — the separate SwiGLU pass (3 tensors through HBM) is gone
//   EPI_SWIGLU_BWD  the product is d(act) = dY W_down; the epilogue reads the gate / up tiles through the park and writes
//                   d(gate), d(up): d(act) never exists in HBM and the separate backward pass (5 tensors) is gone
// (transformers' LlamaMLP.forward behind touchnet/models/llama/__init__.py:11-15, where the reference swaps in liger's
//  fused SwiGLU)
//   EPI_BIASG       EPI_PLAIN for a weight gradient dW = dY^T x that ALSO returns the bias gradient: the column sums of
//                   dY (the A operand, contraction-major) are taken from the A fragments the MFMAs read anyway — wave
//                   (wr, wc) of the tiles in output column 0 sums its A block wc over the whole contraction (16 VALU
//                   adds per 8 MFMAs) — so the separate column-sum pass over dY (one more trip of dY through HBM per
//                   biased layer: 258 launches per Qwen2-Audio step) is gone
//   EPI_ROPE        a q / k projection whose epilogue applies the rotary embedding (transformers' apply_rotary_pos_emb,
//                   modeling_llama.py:113-160 behind LlamaAttention.forward): the rotation pairs column c with c + D/2 of a
//                   head; for D = 128 the B stage image is arranged per DMA wave so that a wave's two 32-column blocks
//                   are (c .. c + 31) and (c + 64 .. c + 95) of one head — both members of every pair in ONE lane (D = 64:
//                   the natural layout already has that).  (acc + bias) is rounded to bf16 first, as the separate
//                   projection leaves it, then rotated with the row kernel's arithmetic: bit-identical, one pass over
//                   q and k through HBM less per layer
//   EPI_GELU_FWD    (the audio tower's fc1) C = x W^T + bias AND C2 = gelu(C): the activation pass read C again
//   EPI_GELU_BWD    (the tower's fc2 input gradient) the product d(act) = dY W never reaches HBM: C = d(act) o gelu'(E1),
//                   E1 = the saved fc1 output (pitch lde) — the GELU backward pass read both and wrote C
constexpr int EPI_PLAIN = 0, EPI_GROUPED = 1, EPI_SWIGLU_FWD = 2, EPI_SWIGLU_BWD = 3, EPI_BIASG = 4, EPI_ROPE = 5;
//   EPI_TABLE       EPI_GROUPED over any number of products (up to MAXTAB): their records come from a table in device
//                   memory instead of from Params, a workgroup finds the product of its tile by binary search over the
//                   records' first tiles, and a record with a bias_out also gets EPI_BIASG's column sums — the audio
//                   tower's weight gradients of many layers as ONE unsplit tile list
constexpr int EPI_GELU_FWD = 6, EPI_GELU_BWD = 7, EPI_TABLE = 8;

struct Params {
  Seg seg[MAXSEG];
  int nseg;
  int M, N;
  bf16_t* C;
  bf16_t* Ct;          // optional transposed copy [N, M] (ldct), or null
  const bf16_t* bias;  // optional [N]
  long long ldc, ldct;
  int accumulate;      // C += result
  // C = result + ADDEND (the residual stream added in the o_proj / down_proj epilogue — `hidden_states = residual
  // + hidden_states` of the HF decoder layers — so that the norm behind it reads ONE tensor): same arithmetic as
  // accumulate (the product rounded to bf16, added in fp32, rounded), the other term read from here instead of from C
  const bf16_t* addend;
  long long ldadd;
  int nbm, nbn;
  int stages;          // sum over segments of K / 64
  // split-K (outputs of few tiles with a deep contraction: the tower's 1280 x 1280 weight gradients over 30000 frames are
  // 25 tiles for 256 CUs): unit u = (split u / tiles, tile u % tiles) contracts stages [split * kchunk, (split+1) * kchunk)
  // of the ONE segment and leaves fp32 partial sums in ws[split][M][N]; splitk_reduce_kernel adds them up
  int splitk, kchunk;
  float* ws;           // [splitk][ntiles][256 x 256] fp32, tile-local
  // the linear tile ids (XCD-aware order, tile_of_block) this launch covers: all of them, or — "tail split" — the whole
  // rounds [0, main) unsplit in one launch and the last partial round [main, tiles) split-K in a second one (688 tiles on
  // 256 CUs are 2 rounds + 176 tiles: whole, the 176 take a third round at 69 % occupancy; cut in 4 they take 0.75)
  int tile0, ntiles;
  // fp32 output (weight gradients written straight into the data-parallel engine's fp32 staging buffers, utils/zero_dp.py):
  // C is a float matrix (ldc in floats), no bias, no transposed copy; accumulate adds to what is there
  int c_f32;
  // EPI_GROUPED: several independent products of one operand mode in ONE persistent launch — product g = seg[g] (one
  // segment each) with its own output; the launch walks the concatenation of their tile lists (tile0 / ntiles index it)
  Grp grp[MAXSEG];
  int ngrp;
  // EPI_SWIGLU_FWD (B = rows of gate_proj AND up_proj, seg[0].B / seg[1].B): C = gate, C2 = up, C3 = silu(gate) * up
  // EPI_SWIGLU_BWD (product = d(act)): E1 = gate, E2 = up (row pitch lde) are read, C = d(gate), C2 = d(up) are written
  bf16_t* C2;
  bf16_t* C3;
  const bf16_t* E1;
  const bf16_t* E2;
  long long lde;
  // EPI_BIASG: bias_out[M] (bf16) = column sums of A; under split-K the units leave fp32 partial sums in
  // bias_ws[split][nbm * 256] and the reduce kernel adds them up
  bf16_t* bias_out;
  float* bias_ws;
  // EPI_ROPE: cos / sin tables [M, rope_d / 2] (bf16, one row per output row), head dimension 64 or 128
  const bf16_t* rope_cos;
  const bf16_t* rope_sin;
  int rope_d;
  // EPI_TABLE: the products' records (ngrp of them, in device memory) instead of seg[] / grp[]
  const Rec* table;
};

// XCD-aware, bijective workgroup -> tile map
//  step 1 (xcd_chunk): workgroups are dealt to the 8 XCDs round-robin, so unit `bid` of `total` runs on XCD bid & 7; it gets
//          position `bid >> 3` of that XCD's own contiguous eighth of the list — what an XCD runs at once is 32 neighbours
//  step 2 (panel_group): a position inside a product -> its tile, 8-tall column-major groups
__device__ __forceinline__ int xcd_chunk(int bid, int total) {
  const int xcd = bid & 7, local = bid >> 3;
  const int q = total >> 3, r = total & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

__device__ __forceinline__ void panel_group(int vid, int nbm, int nbn, int& tm, int& tn) {
  constexpr int GM = 8;
  const int per_group = GM * nbn;
  const int g = vid / per_group, w = vid - g * per_group;
  const int gm = min(GM, nbm - g * GM);  // rows in this (possibly short, last) group
  tm = g * GM + w % gm;
  tn = w / gm;
}

// both steps for one product: the 32 workgroups an XCD runs at once are (8 tall) x (4 wide) neighbours of it
__device__ __forceinline__ void tile_of_block(int bid, int nbm, int nbn, int& tm, int& tn) {
  panel_group(xcd_chunk(bid, nbm * nbn), nbm, nbn, tm, tn);
}

typedef f32x16_t Acc[4][2];

// Where the 8 DMA pieces a wave issues per stage go, as positions 0..31 in the stream of MFMAs that follows the barrier
// which freed their slots (0-7 = last quarter of stage t, 8-31 = quarters 0-2 of stage t+1; Kernel16: a position = two
// MFMAs).  B(t+2) is due one stage later: every other MFMA right behind the barrier; A(t+3) is due two stages later: spread
// over the following quarters instead of bunched behind the barrier.  All B positions must be below all A positions (the
// vmcnt arithmetic of the stage loop relies on B(t+2) being older than A(t+3)).
constexpr int kPieceB[4] = {0, 2, 4, 6}, kPieceA[4] = {14, 18, 22, 26};
static_assert(kPieceB[3] < kPieceA[0], "every B piece is issued before the first A piece");

// piece index issued at position `pos`, or -1
template <bool IS_A> constexpr int piece_at(int pos) {
  for (int i = 0; i < 4; ++i)
    if ((IS_A ? kPieceA[i] : kPieceB[i]) == pos) return i;
  return -1;
}
// pieces with positions 0..7: issued in one burst where no MFMA stream runs (prologue; behind a tile's epilogue)
constexpr int early_piece_count() {
  int n = 0;
  for (int i = 0; i < 4; ++i) n += (kPieceB[i] < 8) + (kPieceA[i] < 8);
  return n;
}

// ---- operand stream: which bytes the next operand stage comes from -------------------------------------------------------
// (M16: the stage image the 16x16x32 kernel reads — contraction-major images swap the two 32-byte halves of every 64-byte
//  group in the k-rows with bit 3 set, see Kernel16)
template <bool KMAJ, bool M16 = false>
struct Stream {
  __amdgpu_buffer_rsrc_t rs;
  int soff;      // byte offset of the next stage inside the descriptor
  int step;      // bytes per stage
  int left;      // stages left in the current segment
  int seg;
  int ld2;       // row pitch in bytes of the current segment
  int voff[4];   // per-lane byte offsets of this wave's 4 pieces

  // (re)derive the per-lane piece offsets from the lane id (also used to re-materialise them behind a tile's epilogue,
  // so that they are not kept alive — i.e. spilled — across it)
  __device__ __forceinline__ void set_voff(int wave, int lane) {
    if constexpr (!KMAJ) {
      // piece q = rows 32 wave + 8 q + (lane >> 3), the lane's 16-byte slot holds chunk (lane & 7) ^ ((row >> 1) & 7)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = wave * 32 + q * 8 + (lane >> 3);
        voff[q] = row * ld2 + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
      }
    } else {
      // piece q = k-rows 8 wave + 2 q + (lane >> 5) of the stage; the lane's 16-byte slot u = lane & 31 of the 512-byte
      // row holds 64-byte group (u >> 2) ^ (k & 3), chunk u & 3
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = wave * 8 + q * 2 + (lane >> 5);
        const int u = lane & 31;
        const int ch = M16 ? ((u & 3) ^ (((k >> 3) & 1) << 1)) : (u & 3);
        voff[q] = k * ld2 + ((((u >> 2) ^ (k & 3)) << 6) | (ch << 4));
      }
    }
  }

  // R = rows of the output dimension this operand spans (M or N), origin = first one of this tile
  __device__ __forceinline__ void open(const bf16_t* X, long long ld, int K, int R, int origin, int wave, int lane) {
    ld2 = (int)(ld * 2);
    if constexpr (!KMAJ) {
      // up to the END of the last row, which with overlapping rows (ld < K) lies behind (R - origin) * ld; rows >= R are
      // zero-filled for ld >= K and may read the last rows' own tails for ld < K: they feed accumulator rows / columns that
      // are never stored, as with a contraction-major operand  (origin >= R: nothing to read, all zeros)
      const long long bytes = R > origin ? (long long)(R - origin - 1) * ld2 + 2LL * K : 0LL;
      rs = __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long long)origin * ld), 0, (int)min(bytes, 0x7fffffffLL),
                                             0x00020000);
      step = 128;
    } else {
      const long long bytes = ((long long)(K - 1) * ld + (R - origin)) * 2;
      rs = __builtin_amdgcn_make_buffer_rsrc((void*)(X + origin), 0, (int)min(bytes, 0x7fffffffLL), 0x00020000);
      step = 64 * ld2;
    }
    set_voff(wave, lane);
    soff = 0;
    left = (K + 63) >> 6;
  }
  __device__ __forceinline__ void kill(const void* any) {
    rs = __builtin_amdgcn_make_buffer_rsrc((void*)any, 0, 0, 0x00020000);   // length 0: every piece reads zeros, no traffic
    soff = 0;
    step = 0;
    left = 0x7fffffff;
  }
};

// MFMA operand fragments of one 16-deep quarter.  ROW fragments are plain LDS loads the compiler counts itself; KMAJ
// fragments are inline-asm transpose reads (the builtin carries no alias metadata: with an LDS-DMA pending hipcc puts
// `s_waitcnt vmcnt(0)` in front of it, which would serialise the ring) that are retired by wait_frags() below.
template <bool KMAJ, int NB>
struct Frags {
  bf16x8_t v[NB];
  u32x2_t h[KMAJ ? NB : 1][2];
};

template <int OFF>
__device__ __forceinline__ u32x2_t ds_tr16(uint32_t addr) {
  u32x2_t r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}

template <bool AK, bool BK, bool HAS_CT, bool SPLITK = false, bool OUT_F32 = false, int EPI = EPI_PLAIN>
struct Kernel {
  static_assert(EPI == EPI_PLAIN || EPI == EPI_GROUPED || EPI == EPI_BIASG || EPI == EPI_TABLE,
                "Kernel: plain / grouped / bias-gradient epilogues (the fused ones are Kernel16's)");
  static constexpr bool MULTI = EPI == EPI_GROUPED || EPI == EPI_TABLE;   // several products in one tile list
  static constexpr bool BIASG = EPI == EPI_BIASG || EPI == EPI_TABLE;     // column sums of A beside the product
  static_assert(!MULTI || (!HAS_CT && !SPLITK), "grouped launch: whole tiles, no transposed copy");
  static_assert(!BIASG || (AK && BK && !HAS_CT), "bias gradient: weight-gradient mode");
  struct Out {
    bf16_t* C;
    long long ldc;
    int M, N;
  };
  // ---- per-lane LDS read offsets ------------------------------------------------------------------------------------------
  //  ROW : xr[q] = (row0 + l31) * 128 + (((2 q + hi) ^ ((l31 >> 1) & 7)) << 4); block b at + b * 4096
  //  KMAJ: xk[b] = (8 hi + j) * 512 + half * 32 + w * 8 + (((blk0 + b) ^ j) << 6); quarter q, half e at + (16 q + 4 e) * 512
  //        (s4 = lane & 15, j = s4 >> 2 = k-row inside the 4-row group, w = s4 & 3, half = (lane >> 4) & 1)
  template <bool KMAJ, int NB>
  struct Reader {
    int x[4];
    __device__ __forceinline__ Reader(int lane, int row0 /* first of the wave's rows inside the 256-row tile */) {
      const int l31 = lane & 31, hi = lane >> 5;
      if constexpr (!KMAJ) {
        const int f = (l31 >> 1) & 7;
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = (row0 + l31) * 128 + (((2 * q + hi) ^ f) << 4);
      } else {
        const int s4 = lane & 15, j = s4 >> 2, w = s4 & 3, half = (lane >> 4) & 1;
#pragma unroll
        for (int b = 0; b < 4; ++b)
          x[b] = (8 * hi + j) * 512 + half * 32 + w * 8 + ((((row0 >> 5) + (b < NB ? b : 0)) ^ j) << 6);
      }
    }
    // fragment `b` of quarter Q from the slot at byte offset `sbase`
    template <int Q, int B>
    __device__ __forceinline__ void read(const char* smem, int sbase, Frags<KMAJ, NB>& f) const {
      if constexpr (!KMAJ) {
        f.v[B] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(smem + sbase + x[Q] + B * 4096));
      } else {
        const uint32_t a = (uint32_t)(size_t)(lds_ptr_t)smem + (uint32_t)(sbase + x[B]);
        f.h[B][0] = ds_tr16<(16 * Q) * 512>(a);
        f.h[B][1] = ds_tr16<(16 * Q + 4) * 512>(a);
      }
    }
  };

  static __device__ __forceinline__ void wait_frags(Frags<AK, 4>& a, Frags<BK, 2>& b) {
    if constexpr (AK && BK) {
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(a.h[0][0]), "+v"(a.h[0][1]), "+v"(a.h[1][0]), "+v"(a.h[1][1]), "+v"(a.h[2][0]), "+v"(a.h[2][1]),
                     "+v"(a.h[3][0]), "+v"(a.h[3][1]), "+v"(b.h[0][0]), "+v"(b.h[0][1]), "+v"(b.h[1][0]), "+v"(b.h[1][1]));
    } else if constexpr (AK) {
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(a.h[0][0]), "+v"(a.h[0][1]), "+v"(a.h[1][0]), "+v"(a.h[1][1]), "+v"(a.h[2][0]), "+v"(a.h[2][1]),
                     "+v"(a.h[3][0]), "+v"(a.h[3][1]));
    } else if constexpr (BK) {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b.h[0][0]), "+v"(b.h[0][1]), "+v"(b.h[1][0]), "+v"(b.h[1][1]));
    }
    if constexpr (AK) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4_t t = {a.h[i][0].x, a.h[i][0].y, a.h[i][1].x, a.h[i][1].y};
        a.v[i] = __builtin_bit_cast(bf16x8_t, t);
      }
    }
    if constexpr (BK) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const u32x4_t t = {b.h[j][0].x, b.h[j][0].y, b.h[j][1].x, b.h[j][1].y};
        b.v[j] = __builtin_bit_cast(bf16x8_t, t);
      }
    }
  }

  // (The kernel enters its body through this one extra call level on purpose: hipcc's result depends on the inlining depth —
  //  called directly, the two unsplit EPI_BIASG kernels come out with the same instructions but two waits of the bias-sum
  //  store placed elsewhere.  Everything is inlined either way.)
  static __device__ __forceinline__ void run(const Params& p, char* smem) { body(p, smem); }

  static __device__ __forceinline__ void body(const Params& p, char* smem) {
    const int tid = threadIdx.x;
    int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;   // 2 x 4 waves

    // persistent: workgroup b of G owns tiles b, b + G, b + 2 G, ... of the XCD-aware order (G is a multiple of 8 or
    // the grid covers every tile at once, so a workgroup's tiles stay on its XCD)
    const int bid = blockIdx.x, G = gridDim.x;
    const int tiles = p.ntiles;
    const int mine = ((SPLITK ? tiles * p.splitk : tiles) - bid + G - 1) / G;
    // product g of a grouped launch: from Params, or (EPI_TABLE) from the table — g is the same in every lane, so these
    // are scalar loads; nothing of a record is kept across a tile, every use looks it up again
    const rec_ptr_t tab = (rec_ptr_t)p.table;
    auto seg_of = [&](int g) {
      if constexpr (EPI == EPI_TABLE) {
        Seg s;
        s.A = tab[g].seg.A;
        s.B = tab[g].seg.B;
        s.lda = tab[g].seg.lda;
        s.ldb = tab[g].seg.ldb;
        s.K = tab[g].seg.K;
        s.pad_ = 0;
        return s;
      } else {
        return p.seg[g];
      }
    };
    auto grp_of = [&](int g) {
      if constexpr (EPI == EPI_TABLE) {
        Grp r;
        r.C = tab[g].grp.C;
        r.ldc = tab[g].grp.ldc;
        r.M = tab[g].grp.M;
        r.N = tab[g].grp.N;
        r.nbm = tab[g].grp.nbm;
        r.nbn = tab[g].grp.nbn;
        r.start = tab[g].grp.start;
        r.stages = tab[g].grp.stages;
        return r;
      } else {
        return p.grp[g];
      }
    };
    // THE tile walk: unit k of this workgroup -> linear tile id -> (grouped launches) its product g -> the tile's origin
    auto origin_g = [&](int k, int& m0, int& n0, int& g) {
      int tm, tn, u = bid + k * G;
      if constexpr (SPLITK) u -= (u / tiles) * tiles;
      u += p.tile0;
      g = 0;
      if constexpr (EPI == EPI_TABLE) {
        // The XCD step of the tile map is taken over the WHOLE list, not inside each product: an XCD walks its own
        // contiguous eighth, so the 32 tiles it runs at once are neighbours in ONE product (two where a product ends) and
        // share their panels in its L2.  Inside each product — EPI_GROUPED's way — an XCD would hold an eighth of every
        // product in flight: 3 tiles of a 25-tile product, 12 of a 100-tile one, 1.5 - 2.6 tiles per panel fetched from
        // beyond the L2 where a product that fills the chip has 5.3.
        u = xcd_chunk(u, tiles);
        int hi = p.ngrp - 1;                               // the last record whose first tile is <= u
        while (g < hi) {
          const int mid = (g + hi + 1) >> 1;
          if (tab[mid].grp.start <= u) g = mid;
          else hi = mid - 1;
        }
      } else if constexpr (EPI == EPI_GROUPED) {
        if (p.ngrp > 1 && u >= p.grp[1].start) g = 1;
        if (p.ngrp > 2 && u >= p.grp[2].start) g = 2;
      }
      if constexpr (EPI == EPI_TABLE) {
        const Grp r = grp_of(g);
        panel_group(u - r.start, r.nbm, r.nbn, tm, tn);
      } else if constexpr (EPI == EPI_GROUPED) {
        const Grp r = grp_of(g);
        tile_of_block(u - r.start, r.nbm, r.nbn, tm, tn);
      } else {
        tile_of_block(u, p.nbm, p.nbn, tm, tn);
      }
      m0 = tm * BM;
      n0 = tn * BN;
    };
    auto origin = [&](int k, int& m0, int& n0) {
      int g;
      origin_g(k, m0, n0, g);
    };
    auto split_of = [&](int k) { return (bid + k * G) / tiles; };

    Stream<AK> sA;
    Stream<BK> sB;
    int ka = 0, kb = 0;                        // tile cursors of the two operand streams (they run 2-3 stages ahead)
    auto open_a = [&](int s) {
      int m0, n0;
      origin(ka, m0, n0);
      if constexpr (SPLITK) {
        // the unit's share of the contraction: `kchunk` stages from k0 on (a share that starts behind K reads nothing;
        // one that crosses K is cut by the descriptor — contraction-major operands only, the host sees to that)
        const int k0 = split_of(ka) * p.kchunk * 64, klen = min(p.seg[0].K - k0, p.kchunk * 64);
        if (klen > 0) sA.open(p.seg[0].A + (AK ? (long long)k0 * p.seg[0].lda : (long long)k0), p.seg[0].lda, klen, p.M,
                              m0, wave, lane);
        else sA.kill(p.C);
        sA.left = p.kchunk;
      } else if constexpr (MULTI) {
        int g;
        origin_g(ka, m0, n0, g);
        const Seg sg = seg_of(g);
        sA.open(sg.A, sg.lda, sg.K, grp_of(g).M, m0, wave, lane);
      } else {
        sA.open(p.seg[s].A, p.seg[s].lda, p.seg[s].K, p.M, m0, wave, lane);
      }
      sA.seg = s;
    };
    auto open_b = [&](int s) {
      int m0, n0;
      origin(kb, m0, n0);
      if constexpr (SPLITK) {
        const int k0 = split_of(kb) * p.kchunk * 64, klen = min(p.seg[0].K - k0, p.kchunk * 64);
        if (klen > 0) sB.open(p.seg[0].B + (BK ? (long long)k0 * p.seg[0].ldb : (long long)k0), p.seg[0].ldb, klen, p.N,
                              n0, wave, lane);
        else sB.kill(p.C);
        sB.left = p.kchunk;
      } else if constexpr (MULTI) {
        int g;
        origin_g(kb, m0, n0, g);
        const Seg sg = seg_of(g);
        sB.open(sg.B, sg.ldb, sg.K, grp_of(g).N, n0, wave, lane);
      } else {
        sB.open(p.seg[s].B, p.seg[s].ldb, p.seg[s].K, p.N, n0, wave, lane);
      }
      sB.seg = s;
    };
    auto adv_a = [&]() {
      sA.soff += sA.step;
      if (--sA.left == 0) {
        if (sA.seg + 1 < p.nseg) open_a(sA.seg + 1);
        else if (++ka < mine) open_a(0);
        else sA.kill(p.C);
      }
    };
    auto adv_b = [&]() {
      sB.soff += sB.step;
      if (--sB.left == 0) {
        if (sB.seg + 1 < p.nseg) open_b(sB.seg + 1);
        else if (++kb < mine) open_b(0);
        else sB.kill(p.C);
      }
    };
    auto piece_a = [&](int slot, int q) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(sA.rs, (lds_ptr_t)(smem + slot * SLOT + wave * 4096 + q * 1024), 16,
                                               sA.voff[q], sA.soff, 0, 0);
    };
    auto piece_b = [&](int slot, int q) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(sB.rs, (lds_ptr_t)(smem + slot * SLOT + wave * 4096 + q * 1024), 16,
                                               sB.voff[q], sB.soff, 0, 0);
    };
    open_a(0);
    open_b(0);

    Reader<AK, 4> ra(lane, wr * 128);
    Reader<BK, 2> rb(lane, wc * 64);

    Acc acc;
    auto zero_acc = [&]() {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };
    zero_acc();

    Frags<AK, 4> ae, ao;
    Frags<BK, 2> be, bo;

#define TN_PIN() __builtin_amdgcn_sched_barrier(0)
    // fragment f (0, 1 = B blocks; 2..5 = A blocks) of quarter Q
    auto read_frag = [&](auto QC, auto FC, int sa, int sb, Frags<AK, 4>& a, Frags<BK, 2>& b) {
      constexpr int Q = decltype(QC)::value, F = decltype(FC)::value;
      if constexpr (F < 2) rb.template read<Q, F>(smem, sb * SLOT, b);
      else ra.template read<Q, F - 2>(smem, sa * SLOT, a);
    };
    auto read_all = [&](auto QC, int sa, int sb, Frags<AK, 4>& a, Frags<BK, 2>& b) {
      read_frag(QC, std::integral_constant<int, 0>{}, sa, sb, a, b);
      read_frag(QC, std::integral_constant<int, 1>{}, sa, sb, a, b);
      read_frag(QC, std::integral_constant<int, 2>{}, sa, sb, a, b);
      read_frag(QC, std::integral_constant<int, 3>{}, sa, sb, a, b);
      read_frag(QC, std::integral_constant<int, 4>{}, sa, sb, a, b);
      read_frag(QC, std::integral_constant<int, 5>{}, sa, sb, a, b);
    };
    auto mma = [&](const Frags<AK, 4>& a, const Frags<BK, 2>& b, int i, int j) {
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b.v[j], a.v[i], acc[i][j], 0, 0, 0);
    };

    // EPI_BIASG: this wave's share of the A panel's column sums — block wc of the four A fragments (32 rows of dY^T), the
    // 8 contraction slots of the lane, every quarter of every stage (rows and depths beyond the operand are zero-filled)
    float bsum = 0.f;
    bool bias_on = false;
    auto bias_accum = [&](const Frags<AK, 4>& a) {
      auto add = [&](const bf16x8_t& v) {
        const u32x4_t w = __builtin_bit_cast(u32x4_t, v);
        bsum += ((__uint_as_float(w.x << 16) + __uint_as_float(w.x & 0xffff0000u)) +
                 (__uint_as_float(w.y << 16) + __uint_as_float(w.y & 0xffff0000u))) +
                ((__uint_as_float(w.z << 16) + __uint_as_float(w.z & 0xffff0000u)) +
                 (__uint_as_float(w.w << 16) + __uint_as_float(w.w & 0xffff0000u)));
      };
      if (wc == 0) add(a.v[0]);
      else if (wc == 1) add(a.v[1]);
      else if (wc == 2) add(a.v[2]);
      else add(a.v[3]);
    };

    // One quarter: the 8 MFMAs of (ca, cb); the fragments of quarter NQ of slots (nsa, nsb) are read into (na, nb), one
    // behind each of the first six MFMAs; the DMA pieces the placement table puts at positions P0 .. P0 + 7 go behind
    // their MFMA (P0 < 0: none).  dst_b / dst_a = slots the open piece set fills.
    auto quarter = [&](auto NQC, auto P0C, const Frags<AK, 4>& ca, const Frags<BK, 2>& cb, Frags<AK, 4>& na,
                       Frags<BK, 2>& nb, int nsa, int nsb, int dst_b, int dst_a) {
      constexpr int P0 = decltype(P0C)::value;
      if constexpr (BIASG) {
        if (bias_on) bias_accum(ca);
        TN_PIN();
      }
      auto step = [&](auto MC) {
        constexpr int m = decltype(MC)::value;
        mma(ca, cb, m >> 1, m & 1);
        TN_PIN();
        if constexpr (m < 6) {
          read_frag(NQC, std::integral_constant<int, m>{}, nsa, nsb, na, nb);
          TN_PIN();
        }
        constexpr int pb = P0 < 0 ? -1 : piece_at<false>(P0 + m);
        constexpr int pa = P0 < 0 ? -1 : piece_at<true>(P0 + m);
        if constexpr (pb >= 0) {
          piece_b(dst_b, pb);
          if constexpr (pb == 3) adv_b();
          TN_PIN();
        }
        if constexpr (pa >= 0) {
          piece_a(dst_a, pa);
          if constexpr (pa == 3) adv_a();
          TN_PIN();
        }
      };
      step(std::integral_constant<int, 0>{});
      step(std::integral_constant<int, 1>{});
      step(std::integral_constant<int, 2>{});
      step(std::integral_constant<int, 3>{});
      step(std::integral_constant<int, 4>{});
      step(std::integral_constant<int, 5>{});
      step(std::integral_constant<int, 6>{});
      step(std::integral_constant<int, 7>{});
    };
    // the pieces of positions 0..7 in one burst (prologue; behind a tile's epilogue)
    auto early_pieces = [&](int dst_b, int dst_a) {
      auto one = [&](auto MC) {
        constexpr int m = decltype(MC)::value;
        constexpr int pb = piece_at<false>(m), pa = piece_at<true>(m);
        if constexpr (pb >= 0) {
          piece_b(dst_b, pb);
          if constexpr (pb == 3) adv_b();
        }
        if constexpr (pa >= 0) {
          piece_a(dst_a, pa);
          if constexpr (pa == 3) adv_a();
        }
      };
      one(std::integral_constant<int, 0>{});
      one(std::integral_constant<int, 1>{});
      one(std::integral_constant<int, 2>{});
      one(std::integral_constant<int, 3>{});
      one(std::integral_constant<int, 4>{});
      one(std::integral_constant<int, 5>{});
      one(std::integral_constant<int, 6>{});
      one(std::integral_constant<int, 7>{});
    };
    auto next = [](int s, int d) { s += d; return s >= 5 ? s - 5 : s; };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using NONE = std::integral_constant<int, -1>;

    // prologue: A0 B0 A1 -> slots 0..2, then the piece set "opened at the barrier of stage -1" = {B(1) -> slot 3,
    // A(2) -> slot 4}: its pieces with positions < 8 are issued here, the later ones by the first trip
#pragma unroll
    for (int q = 0; q < 4; ++q) piece_a(0, q);
    adv_a();
#pragma unroll
    for (int q = 0; q < 4; ++q) piece_b(1, q);
    adv_b();
#pragma unroll
    for (int q = 0; q < 4; ++q) piece_a(2, q);
    adv_a();
    early_pieces(3, 4);
    // A(0), B(0) must have landed; everything issued behind them may stay in flight
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + early_piece_count()) : "memory");
    __builtin_amdgcn_s_barrier();
    int sa = 0, sb = 1;                         // slots of A(t), B(t)
    int pa = 4, pb = 3;                         // slots the piece set opened at the previous barrier fills (A part, B part)

    // One stage.  LAST = last stage of a tile: its final quarter neither opens the next piece set (the two slots it
    // frees first serve as the epilogue's park) nor reads the next stage's first fragments (nothing but the accumulators
    // is to stay alive across the epilogue).
    auto trip = [&](auto LASTC) {
      constexpr bool LAST = decltype(LASTC)::value;
      const int sa1 = next(sa, 2), sb1 = next(sb, 2);       // slots of stage t+1
      __builtin_amdgcn_s_setprio(1);
      // quarters 0..2 of stage t (positions 8..31 of the piece set opened at the previous barrier)
      quarter(I1{}, std::integral_constant<int, 8>{}, ae, be, ao, bo, sa, sb, pb, pa);
      wait_frags(ao, bo);
      TN_PIN();
      quarter(I2{}, std::integral_constant<int, 16>{}, ao, bo, ae, be, sa, sb, pb, pa);
      wait_frags(ae, be);
      TN_PIN();
      quarter(I3{}, std::integral_constant<int, 24>{}, ae, be, ao, bo, sa, sb, pb, pa);
      __builtin_amdgcn_s_setprio(0);
      wait_frags(ao, bo);                                 // (asm reads retired here; ROW reads by the next line)
      __builtin_amdgcn_s_waitcnt(0xc07f);                 // my reads of stage t are complete (quarter 3 is in registers)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");    // A(t+1), B(t+1) landed; A(t+2) may still be in flight
      __builtin_amdgcn_s_barrier();                       // stage t+1 visible; slots sa, sb free
      __builtin_amdgcn_s_setprio(1);
      if constexpr (!LAST) {
        // last quarter of stage t: the new piece set {B(t+2) -> slot sa, A(t+3) -> slot sb} opens (positions 0..7)
        quarter(I0{}, I0{}, ao, bo, ae, be, sa1, sb1, sa, sb);
        __builtin_amdgcn_s_setprio(0);
        wait_frags(ae, be);
        TN_PIN();
      } else {
        if constexpr (BIASG) {
          if (bias_on) bias_accum(ao);
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) mma(ao, bo, m >> 1, m & 1);
        __builtin_amdgcn_s_setprio(0);
      }
      pb = sa;
      pa = sb;
      sa = sa1;
      sb = sb1;
    };

    const int np_all = SPLITK ? p.kchunk : p.stages;
    for (int kc = 0; kc < mine; ++kc) {
      int np = np_all;
      if constexpr (BIASG) {
        int m0_, n0_, g_;
        origin_g(kc, m0_, n0_, g_);
        bias_on = n0_ == 0;                                // the tiles of output column 0 carry the bias gradient
        if constexpr (EPI == EPI_TABLE) bias_on = bias_on && tab[g_].bias_out != nullptr;   // (of the products that want one)
        bsum = 0.f;
      }
      if constexpr (MULTI) {                               // (the products of a group may differ in depth)
        int m0_, n0_, g_;
        origin_g(kc, m0_, n0_, g_);
        np = grp_of(g_).stages;
      }
      read_all(I0{}, sa, sb, ae, be);
      wait_frags(ae, be);
      TN_PIN();
      for (int t = 1; t < np; ++t) trip(std::false_type{});
      trip(std::true_type{});
      // Epilogue.  The streams are already inside the next tile (its stage 0 and A(1) are in the other three slots);
      // the two slots the last barrier freed (now pb / pa) are the park, then they take their deferred pieces.
      int m0, n0, grp;
      origin_g(kc, m0, n0, grp);
      if constexpr (BIASG) {
        if (bias_on) {
          // the lane pair (l, l + 32) holds the two halves of every 16-deep slice of row l
          const float tot = bsum + __shfl_xor(bsum, 32, 64);
          const int m = m0 + wr * 128 + wc * 32 + (lane & 31);
          if (lane < 32) {
            if constexpr (SPLITK) {
              p.bias_ws[(long long)split_of(kc) * (p.nbm * BM) + m] = tot;
            } else if constexpr (EPI == EPI_TABLE) {
              if (m < tab[grp].grp.M) tab[grp].bias_out[m] = f2bf(tot);
            } else if (m < p.M) {
              p.bias_out[m] = f2bf(tot);
            }
          }
        }
      }
      if constexpr (SPLITK) {
        const int u = bid + kc * G, sp = u / tiles;
        epilogue_ws(p, acc, sp * tiles + (u - sp * tiles), wr * 128, wc * 64, lane);
      } else if constexpr (OUT_F32) {
        if constexpr (MULTI) {
          const Grp r = grp_of(grp);
          const Out o = {r.C, r.ldc, r.M, r.N};
          epilogue_f32(p, o, acc, m0 + wr * 128, n0 + wc * 64, lane);
        } else {
          const Out o = {p.C, p.ldc, p.M, p.N};
          epilogue_f32(p, o, acc, m0 + wr * 128, n0 + wc * 64, lane);
        }
      } else if constexpr (MULTI) {
        const Grp r = grp_of(grp);
        const Out o = {r.C, r.ldc, r.M, r.N};
        epilogue(p, o, acc, smem + (wave < 4 ? pb : pa) * SLOT + (wave & 3) * 8192, m0 + wr * 128, n0 + wc * 64, lane);
      } else {
        const Out o = {p.C, p.ldc, p.M, p.N};
        epilogue(p, o, acc, smem + (wave < 4 ? pb : pa) * SLOT + (wave & 3) * 8192, m0 + wr * 128, n0 + wc * 64, lane);
      }
      zero_acc();
      __builtin_amdgcn_s_waitcnt(0xc07f);               // my park reads are done ...
      __builtin_amdgcn_s_barrier();                     // ... and everybody's: the slots may be refilled
      // lane constants are re-derived from an opaque copy of the lane id: the compiler must not carry (spill) the old
      // ones across the epilogue
      asm volatile("" : "+v"(lane));
      ra = Reader<AK, 4>(lane, wr * 128);
      rb = Reader<BK, 2>(lane, wc * 64);
      sA.set_voff(wave, lane);
      sB.set_voff(wave, lane);
      early_pieces(pb, pa);
    }
  }

  // fp32 output: the accumulators as they are, 16 bytes per lane and register quad (see epilogue_ws), clipped to M x N
  static __device__ __forceinline__ void epilogue_f32(const Params& p, const Out& o, Acc& acc, int wm0, int wn0, int lane) {
    const int l31 = lane & 31, hi = lane >> 5;
    float* C = reinterpret_cast<float*>(o.C);
    const bool add = p.accumulate != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = wm0 + i * 32 + l31;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = wn0 + j * 32 + 8 * g + 4 * hi;
          if (m < o.M && n < o.N) {                          // N is a multiple of 8: the quad is inside or outside
            f32x4_t* dst = reinterpret_cast<f32x4_t*>(C + (long long)m * o.ldc + n);
            f32x4_t v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
            if (add) v += *dst;
            *dst = v;
          }
        }
    }
  }

  // Split-K epilogue: the fp32 accumulators go to this unit's [256 x 256] slab of the workspace as they are (a lane holds 4
  // consecutive n of one m per register quad: 16-byte stores; the L2 merges the quads of a line before it is written back).
  // Slabs are whole tiles: no bounds checks here, the reduce kernel clips to M x N.
  static __device__ __forceinline__ void epilogue_ws(const Params& p, Acc& acc, int slab, int lm0, int ln0, int lane) {
    const int l31 = lane & 31, hi = lane >> 5;
    float* base = p.ws + (long long)slab * (BM * BN);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = lm0 + i * 32 + l31;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = ln0 + j * 32 + 8 * g + 4 * hi;
          const f32x4_t v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          *reinterpret_cast<f32x4_t*>(base + m * BN + n) = v;
        }
    }
  }

  // Epilogue through LDS: the wave parks its 128 x 64 tile, 64 rows at a time, in its own XOR-swizzled 8 KB
  // ([64 rows][64 cols] bf16, 128-byte rows, chunk ^= row & 7) and writes full 128-byte lines.
  static __device__ __forceinline__ void epilogue(const Params& p, const Out& o, Acc& acc, char* park, int wm0, int wn0,
                                                  int lane) {
    const int l31 = lane & 31, hi = lane >> 5;
    float bias_v[2][4][4];
    if (p.bias != nullptr) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = min(wn0 + j * 32 + 8 * g + 4 * hi, o.N - 4);    // (columns >= N are never stored)
          const uint2 w = *reinterpret_cast<const uint2*>(p.bias + n);
          bias_v[j][g][0] = __uint_as_float(w.x << 16);
          bias_v[j][g][1] = __uint_as_float(w.x & 0xffff0000u);
          bias_v[j][g][2] = __uint_as_float(w.y << 16);
          bias_v[j][g][3] = __uint_as_float(w.y & 0xffff0000u);
        }
    }
    const bool acc_c = p.accumulate != 0 || p.addend != nullptr;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      // result rows (registers) = n, result column (lane) = m: 4 consecutive n per register quad -> 8-byte packs
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = half * 2 + ii;
        const int row = ii * 32 + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e] + (p.bias != nullptr ? bias_v[j][g][e] : 0.f);
            const int chunk = (j * 4 + g) ^ (row & 7);
            // (vector-typed LDS accesses: hipcc puts `s_waitcnt vmcnt(0)` in front of an LDS access without alias
            //  metadata while an LDS-DMA is pending — here the next tile's prefetched stages)
            const u32x2_t pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
            *reinterpret_cast<u32x2_t*>(park + row * 128 + chunk * 16 + hi * 8) = pk;
          }
      }
      // (only this wave touches its park region: a wave-level wait is enough; LDS operations of one wave execute in
      //  order, so the next half's stores cannot overtake this half's reads)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
      for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3), c = lane & 7;
        const u32x4_t pv = *reinterpret_cast<const u32x4_t*>(park + row * 128 + ((c ^ (row & 7)) << 4));
        uint4 v = make_uint4(pv.x, pv.y, pv.z, pv.w);
        const int m = wm0 + half * 64 + row, n = wn0 + c * 8;
        if (m < o.M && n < o.N) {                            // N is a multiple of 8 (checked by the host)
          bf16_t* dst = o.C + (long long)m * o.ldc + n;
          if (acc_c) {
            Vec16<bf16_t> o, nw;
            o.load(p.addend != nullptr ? p.addend + (long long)m * p.ldadd + n : dst);
            nw.raw = v;
            float fo[8], fn[8];
            o.unpack(fo);
            nw.unpack(fn);
#pragma unroll
            for (int e = 0; e < 8; ++e) fn[e] += fo[e];
            nw.pack(fn);
            v = nw.raw;
          }
          *reinterpret_cast<uint4*>(dst) = v;
        }
      }
      if constexpr (HAS_CT) {
        // transposed copy: Ct[n, m]; a lane gathers 8 consecutive m of one n from the parked half tile (2-byte LDS
        // reads: this path trades LDS instructions for the HBM round trip of a separate transpose pass)
#pragma unroll 2
        for (int it = 0; it < 8; ++it) {
          const int n_l = it * 8 + (lane >> 3), mg = lane & 7;       // 64 n x 8 groups of 8 m
          uint32_t w[4];
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) {
            uint32_t lo, hi16;
            {
              const int row = mg * 8 + 2 * e2;
              lo = *reinterpret_cast<const uint16_t*>(park + row * 128 + ((((n_l >> 3) ^ (row & 7))) << 4) + (n_l & 7) * 2);
            }
            {
              const int row = mg * 8 + 2 * e2 + 1;
              hi16 = *reinterpret_cast<const uint16_t*>(park + row * 128 + ((((n_l >> 3) ^ (row & 7))) << 4) + (n_l & 7) * 2);
            }
            w[e2] = lo | (hi16 << 16);
          }
          const int n = wn0 + n_l, m = wm0 + half * 64 + mg * 8;
          if (n < o.N && m < o.M)     // M is a multiple of 8 when a transposed copy is requested (host check)
            *reinterpret_cast<uint4*>(p.Ct + (long long)n * p.ldct + m) = make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
    }
  }
};

template <bool AK, bool BK, bool HAS_CT, bool SPLITK = false, bool OUT_F32 = false, int EPI = EPI_PLAIN>
__global__ __launch_bounds__(NT, 2) void gemm_kernel(const Params p) {
  __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
  Kernel<AK, BK, HAS_CT, SPLITK, OUT_F32, EPI>::run(p, smem);
}

}  // namespace gemm
}  // namespace tn
