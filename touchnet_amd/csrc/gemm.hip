// The GEMM library's source file: Kernel16, the split-K reduce kernel, the rule that picks a kernel (`launch`) and the C
// entry points.  gemm_kernel.h has the description of the design, the shared device code and Kernel; gemm_host.h the
// host-side rules shared with gemm_table.hip (the table-driven grouped weight-gradient launch).
#include "gemm_host.h"

namespace tn {
namespace gemm {

// =====================================================================================================================
// Kernel16: the same workgroup geometry, stage ring, DMA placement and persistent tile walk as Kernel above, with
// v_mfma_f32_16x16x32_bf16 instead of v_mfma_f32_32x32x16_bf16.  Why (profiles/r05p_*): with operands in
// registers only the 32x32x16 shape SUSTAINS 1.73-1.78 PF on this chip — the 1.67 GHz the GEMM was always measured at —
// and the 16x16x32 shape 1.98-1.99 PF (half the accumulator register traffic per flop): the "power limit" of the
// kernel was its instruction shape (hipBLASLt's gfx950 kernels issue 16x16x32).  Products with a row-stored A gain 5-7 %
// (forward) / 2-3 % (input gradient); the weight-gradient mode (both operands through transpose reads) gains nothing and
// stays on Kernel.
//  * wave tile 128 x 64 = 8 x 4 blocks of 16 x 16, accumulators f32x4 [8][4] (the same 128 registers)
//  * a 64-deep stage = two 32-deep halves; a "quarter" = 16 MFMAs = A blocks 4 part .. 4 part + 3 (part = quarter & 1) of
//    half quarter >> 1 against the half's four B blocks.  Fragment sets: 4 A fragments per quarter (double buffered),
//    4 B fragments per half (double buffered); one fragment read behind every second MFMA.
//  * operand fragment of v_mfma_f32_16x16x32: lane l holds row l & 15, contraction slots 8 (l >> 4) .. + 7:
//      ROW   one ds_read_b128 at row * 128 + ((4 half + (l >> 4)) ^ ((row >> 1) & 7)) * 16   (same image as Kernel)
//      KMAJ  two ds_read_b64_tr_b16: the 16 lanes of group g4 = l >> 4 point at k-rows 32 half + 8 g4 + (0..3) [+ 4] x the
//            32 bytes of a 16-row block.  Lanes 0-15 and 16-31 are served together and would hit the same banks (their
//            k-rows are 8 apart: same (k & 3) group swizzle), so the IMAGE swaps the two 32-byte halves of every 64-byte
//            group in k-rows with bit 3 set (Stream<.., M16>): the second group reads the other half.
//  * result of mfma(b, a): lane holds column m = l & 15 of its 16 x 16 block, registers r = rows n = 4 (l >> 4) + r
// =====================================================================================================================
typedef f32x4_t Acc16[8][4];

template <bool AK, bool BK, int EPI = EPI_PLAIN>
struct Kernel16 {
  static_assert(EPI == EPI_PLAIN || EPI == EPI_SWIGLU_FWD || EPI == EPI_SWIGLU_BWD || EPI == EPI_ROPE ||
                    EPI == EPI_GELU_FWD || EPI == EPI_GELU_BWD,
                "Kernel16: plain / SwiGLU / RoPE / GELU epilogues (the weight-gradient modes stay on Kernel)");
  static_assert(EPI != EPI_GELU_FWD || !BK, "GELU forward: x W^T layout");
  static_assert(EPI != EPI_GELU_BWD || BK, "GELU backward: dY W layout");
  static_assert(!AK, "Kernel16: row-stored A (forward and input-gradient products)");
  static_assert(EPI != EPI_SWIGLU_FWD || !BK, "SwiGLU forward: x W^T layout");
  static_assert(EPI != EPI_SWIGLU_BWD || BK, "SwiGLU backward: dY W layout");
  static_assert(EPI != EPI_ROPE || !BK, "RoPE epilogue: x W^T layout");
  static constexpr int BN_EFF = EPI == EPI_SWIGLU_FWD ? 128 : BN;
  static __device__ __forceinline__ float sigm(float x) { return sigmoid_fast(x); }
  static __device__ __forceinline__ float lo16(uint32_t w) { return __uint_as_float(w << 16); }
  static __device__ __forceinline__ float hi16(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
  static __device__ __forceinline__ float rbf(float v) { return __uint_as_float(((uint32_t)f2bf(v)) << 16); }
  template <bool KMAJ>
  struct F4 {
    bf16x8_t v[4];
    u32x2_t h[KMAJ ? 4 : 1][2];
  };
  // per-lane LDS offsets.  ROW: x[half]; block b of the wave's rows at + b * 2048.  KMAJ: x[G] for the 64-byte group G of
  // the wave's 32-row pairs, x ^ 32 for the odd 16-row block of the pair; k-row offsets are compile-time.
  template <bool KMAJ, int NB /* 16-row blocks: 8 (A) or 4 (B) */>
  struct Reader {
    int x[KMAJ ? NB / 2 : 2];
    __device__ __forceinline__ Reader(int lane, int row0) {
      const int l15 = lane & 15, g4 = lane >> 4;
      if constexpr (!KMAJ) {
        const int f = (l15 >> 1) & 7;
#pragma unroll
        for (int h = 0; h < 2; ++h) x[h] = (row0 + l15) * 128 + (((4 * h + g4) ^ f) << 4);
      } else {
        const int j = l15 >> 2, w = l15 & 3;
#pragma unroll
        for (int g = 0; g < NB / 2; ++g)
          x[g] = (8 * g4 + j) * 512 + w * 8 + ((((row0 >> 5) + g) ^ j) << 6) + (g4 & 1) * 32;
      }
    }
    // fragment I (0..3) of the set: 16-row block BLK of the wave's rows, half H of the stage
    template <int H, int BLK, int I>
    __device__ __forceinline__ void read(const char* smem, int sbase, F4<KMAJ>& f) const {
      if constexpr (!KMAJ) {
        f.v[I] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(smem + sbase + x[H] + BLK * 2048));
      } else {
        const uint32_t a = (uint32_t)(size_t)(lds_ptr_t)smem + (uint32_t)(sbase + (x[BLK >> 1] ^ ((BLK & 1) * 32)));
        f.h[I][0] = ds_tr16<(32 * H) * 512>(a);
        f.h[I][1] = ds_tr16<(32 * H + 4) * 512>(a);
      }
    }
  };
  template <bool KMAJ>
  static __device__ __forceinline__ void retire(F4<KMAJ>& f) {
    if constexpr (KMAJ) {
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(f.h[0][0]), "+v"(f.h[0][1]), "+v"(f.h[1][0]), "+v"(f.h[1][1]), "+v"(f.h[2][0]), "+v"(f.h[2][1]),
                     "+v"(f.h[3][0]), "+v"(f.h[3][1]));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4_t t = {f.h[i][0].x, f.h[i][0].y, f.h[i][1].x, f.h[i][1].y};
        f.v[i] = __builtin_bit_cast(bf16x8_t, t);
      }
    }
  }

  static __device__ __forceinline__ void run(const Params& p, char* smem) {
    const int tid = threadIdx.x;
    int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int bid = blockIdx.x, G = gridDim.x;
    const int tiles = p.ntiles;
    const int mine = (tiles - bid + G - 1) / G;
    auto origin = [&](int k, int& m0, int& n0) {
      int tm, tn;
      tile_of_block(p.tile0 + bid + k * G, p.nbm, p.nbn, tm, tn);
      m0 = tm * BM;
      n0 = tn * BN_EFF;
    };
    Stream<AK, true> sA;
    Stream<BK, true> sB;
    int ka = 0, kb = 0;
    auto open_a = [&](int s) {
      int m0, n0;
      origin(ka, m0, n0);
      sA.open(p.seg[s].A, p.seg[s].lda, p.seg[s].K, p.M, m0, wave, lane);
      sA.seg = s;
    };
    // B stage images of the fused epilogues: which rows of B DMA wave w fetches into LDS rows [32 w, 32 w + 32) (per-lane
    // offsets as for wave 0: the bank swizzle only involves row bits below 32)
    //   SwiGLU forward   rows n0 + 32 (w >> 1) .. of gate_proj (w even) / up_proj (w odd)
    //   RoPE, D = 128    W rows of head n0 / 128 + (w >> 2), columns 64 (w & 1) + 32 ((w >> 1) & 1) ..: reader wave
    //                    wc = w >> 1 then holds (c, c + 64) pairs.  D = 64: the plain order.
    const bool b_wave0 = EPI == EPI_SWIGLU_FWD || (EPI == EPI_ROPE && p.rope_d == 128);
    auto open_b = [&](int s) {
      int m0, n0;
      origin(kb, m0, n0);
      if constexpr (EPI == EPI_SWIGLU_FWD) {
        sB.open((wave & 1) ? p.seg[1].B : p.seg[0].B, p.seg[0].ldb, p.seg[0].K, p.N, n0 + (wave >> 1) * 32, 0, lane);
      } else if constexpr (EPI == EPI_ROPE) {
        if (p.rope_d == 128)
          sB.open(p.seg[0].B, p.seg[0].ldb, p.seg[0].K, p.N, n0 + (wave >> 2) * 128 + (wave & 1) * 64 + ((wave >> 1) & 1) * 32,
                  0, lane);
        else
          sB.open(p.seg[0].B, p.seg[0].ldb, p.seg[0].K, p.N, n0, wave, lane);
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

    Reader<AK, 8> ra(lane, wr * 128);
    Reader<BK, 4> rb(lane, wc * 64);
    Acc16 acc;
    auto zero_acc = [&]() {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    };
    zero_acc();
    F4<AK> ae, ao;
    F4<BK> be, bo;
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;

    // read fragment R (0..3 = A blocks of quarter Q, 4..7 = the B blocks of half Q >> 1) of the quarter that follows
    auto read_frag = [&](auto QC, auto RC, int sa, int sb, F4<AK>& a, F4<BK>& b) {
      constexpr int Q = decltype(QC)::value, R = decltype(RC)::value;
      if constexpr (R < 4) ra.template read<(Q >> 1), (Q & 1) * 4 + R, R>(smem, sa * SLOT, a);
      else rb.template read<(Q >> 1), R - 4, R - 4>(smem, sb * SLOT, b);
    };
    // (Measured and dropped: B fragments read first and retired by a counted `lgkmcnt(4)` while the four younger A
    //  reads stay in flight — 0.7 % SLOWER than A first + lgkmcnt(0), profiles/r05s_*.)
    // One quarter: 16 MFMAs of A part PART (fragments ca) against the half's B fragments cb; fragment r of the NEXT quarter
    // NQ (4 A fragments, and with RB its half's 4 B fragments) is read behind MFMA 2 r; DMA pieces of positions
    // P0 .. P0 + 7 go behind MFMAs 0, 2, .. 14 (P0 < 0: none).
    auto quarter = [&](auto NQC, auto RBC, auto P0C, auto PARTC, const F4<AK>& ca, const F4<BK>& cb, F4<AK>& na,
                       F4<BK>& nb, int nsa, int nsb, int dst_b, int dst_a) {
      constexpr int P0 = decltype(P0C)::value, PART = decltype(PARTC)::value;
      constexpr bool RB = decltype(RBC)::value;
      auto step = [&](auto MC) {
        constexpr int m = decltype(MC)::value, i = m >> 2, j = m & 3;
        acc[PART * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cb.v[j], ca.v[i], acc[PART * 4 + i][j], 0, 0, 0);
        TN_PIN();
        // fragment reads behind the FIRST MFMAs of the quarter (reads 0..7 behind MFMAs 0..7, so the last one is 8+ MFMAs
        // old when the quarter's fragments are retired)
        if constexpr (m < 4 || (m < 8 && RB)) {
          read_frag(NQC, std::integral_constant<int, m>{}, nsa, nsb, na, nb);
          TN_PIN();
        }
        if constexpr ((m & 1) == 0) {
          constexpr int r = m >> 1;
          constexpr int pb = P0 < 0 ? -1 : piece_at<false>(P0 + r);
          constexpr int pa = P0 < 0 ? -1 : piece_at<true>(P0 + r);
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
      step(std::integral_constant<int, 8>{});
      step(std::integral_constant<int, 9>{});
      step(std::integral_constant<int, 10>{});
      step(std::integral_constant<int, 11>{});
      step(std::integral_constant<int, 12>{});
      step(std::integral_constant<int, 13>{});
      step(std::integral_constant<int, 14>{});
      step(std::integral_constant<int, 15>{});
    };
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
    using T_ = std::true_type;
    using F_ = std::false_type;

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
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + early_piece_count()) : "memory");
    __builtin_amdgcn_s_barrier();
    int sa = 0, sb = 1;
    int pa = 4, pb = 3;

    auto trip = [&](auto LASTC) {
      constexpr bool LAST = decltype(LASTC)::value;
      const int sa1 = next(sa, 2), sb1 = next(sb, 2);
      __builtin_amdgcn_s_setprio(1);
      // quarter 0 (half 0, A part 0): reads A of quarter 1
      quarter(I1{}, F_{}, std::integral_constant<int, 8>{}, I0{}, ae, be, ao, bo, sa, sb, pb, pa);
      retire(ao);
      TN_PIN();
      // quarter 1 (half 0, part 1): reads A of quarter 2 and B of half 1
      quarter(I2{}, T_{}, std::integral_constant<int, 16>{}, I1{}, ao, be, ae, bo, sa, sb, pb, pa);
      retire(ae);
      retire(bo);
      TN_PIN();
      // quarter 2 (half 1, part 0): reads A of quarter 3
      quarter(I3{}, F_{}, std::integral_constant<int, 24>{}, I0{}, ae, bo, ao, be, sa, sb, pb, pa);
      __builtin_amdgcn_s_setprio(0);
      retire(ao);
      __builtin_amdgcn_s_waitcnt(0xc07f);                 // my reads of stage t are complete
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");    // A(t+1), B(t+1) landed; A(t+2) may still be in flight
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(1);
      if constexpr (!LAST) {
        // quarter 3 (half 1, part 1): the new piece set opens; reads A of quarter 0 and B of half 0 of stage t + 1
        quarter(I0{}, T_{}, I0{}, I1{}, ao, bo, ae, be, sa1, sb1, sa, sb);
        __builtin_amdgcn_s_setprio(0);
        retire(ae);
        retire(be);
        TN_PIN();
      } else {
#pragma unroll
        for (int m = 0; m < 16; ++m)
          acc[4 + (m >> 2)][m & 3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bo.v[m & 3], ao.v[m >> 2], acc[4 + (m >> 2)][m & 3], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      pb = sa;
      pa = sb;
      sa = sa1;
      sb = sb1;
    };

    const int np = p.stages;
    for (int kc = 0; kc < mine; ++kc) {
      // quarter 0's fragments of the tile's first stage
      read_frag(I0{}, I0{}, sa, sb, ae, be);
      read_frag(I0{}, I1{}, sa, sb, ae, be);
      read_frag(I0{}, I2{}, sa, sb, ae, be);
      read_frag(I0{}, I3{}, sa, sb, ae, be);
      read_frag(I0{}, std::integral_constant<int, 4>{}, sa, sb, ae, be);
      read_frag(I0{}, std::integral_constant<int, 5>{}, sa, sb, ae, be);
      read_frag(I0{}, std::integral_constant<int, 6>{}, sa, sb, ae, be);
      read_frag(I0{}, std::integral_constant<int, 7>{}, sa, sb, ae, be);
      retire(ae);
      retire(be);
      TN_PIN();
      for (int t = 1; t < np; ++t) trip(F_{});
      trip(T_{});
      int m0, n0;
      origin(kc, m0, n0);
      char* park = smem + (wave < 4 ? pb : pa) * SLOT + (wave & 3) * 8192;
      if constexpr (EPI == EPI_SWIGLU_FWD) {
        epilogue16_swiglu_fwd(p, acc, park, m0 + wr * 128, n0 + wc * 32, lane);
      } else if constexpr (EPI == EPI_SWIGLU_BWD) {
        epilogue16_swiglu_bwd(p, acc, park, m0 + wr * 128, n0 + wc * 64, lane);
      } else if constexpr (EPI == EPI_ROPE) {
        const bool d128 = p.rope_d == 128;
        epilogue16_rope(p, acc, park, m0 + wr * 128, d128 ? n0 + (wc >> 1) * 128 + (wc & 1) * 32 : n0 + wc * 64,
                        d128 ? (wc & 1) * 32 : 0, lane);
      } else {
        epilogue16(p, acc, park, m0 + wr * 128, n0 + wc * 64, lane);
      }
      zero_acc();
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_s_barrier();
      asm volatile("" : "+v"(lane));
      ra = Reader<AK, 8>(lane, wr * 128);
      rb = Reader<BK, 4>(lane, wc * 64);
      sA.set_voff(wave, lane);
      sB.set_voff(b_wave0 ? 0 : wave, lane);
      early_pieces(pb, pa);
    }
  }

  // ---- park helpers: a 64-row half of the wave tile (A blocks 4 half .. 4 half + 3) <-> the [64 rows][64 columns] bf16 park.
  // Element (row = 16 bi + l15, columns 16 bj + 4 g4 .. + 3) = one 8-byte pack at chunk (2 bj + (g4 >> 1)) ^ (row & 7).
  static __device__ __forceinline__ char* park_at(char* park, int bi, int bj, int l15, int g4) {
    const int row = bi * 16 + l15;
    return park + row * 128 + (((bj * 2 + (g4 >> 1)) ^ (row & 7)) << 4) + (g4 & 1) * 8;
  }

  // ---- fused SwiGLU epilogues ------------------------------------------------------------------------------------------
  // Arithmetic = tn::swiglu_fwd_kernel / swiglu_bwd_kernel (csrc/norm_act.hip) on the bf16-ROUNDED products, as the
  // separate passes saw them: silu(gate) rounded to bf16 before the product (what the eager path materialises), so the
  // fused and the unfused MLP agree bit for bit.
  // Forward: blocks bj = 0, 1 of a lane are gate, bj = 2, 3 up of the SAME columns wn0 + 16 bj + 4 g4 ..  Three trips through
  // the wave's park:
  //   1, 2  rows half * 64 ..: columns 0-31 = gate, 32-63 = up  -> 64-byte row segments of C (gate) and C2 (up)
  //   3     act of ALL 128 rows: columns 0-31 = rows 0-63, columns 32-63 = rows 64-127 -> 64-byte row segments of C3
  static __device__ __forceinline__ void epilogue16_swiglu_fwd(const Params& p, Acc16& acc, char* park, int wm0, int wn0,
                                                               int lane) {
    const int l15 = lane & 15, g4 = lane >> 4;
    // (the per-lane choice between the two outputs as integer arithmetic on pointers held in registers: written as
    //  `c < 4 ? p.C : p.C2` hipcc selects between the two kernel-argument ADDRESSES and re-loads the pointer per store)
    const uintptr_t c_gate = (uintptr_t)p.C, c_up = (uintptr_t)p.C2;
    bf16_t* const gu_base = reinterpret_cast<bf16_t*>(c_gate + ((lane & 4) ? c_up - c_gate : (uintptr_t)0));
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) {
          const f32x4_t a = acc[half * 4 + bi][bj];
          *reinterpret_cast<u32x2_t*>(park_at(park, bi, bj, l15, g4)) = u32x2_t{pack2bf(a[0], a[1]), pack2bf(a[2], a[3])};
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
      for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3), c = lane & 7;
        const u32x4_t pv = *reinterpret_cast<const u32x4_t*>(park + row * 128 + ((c ^ (row & 7)) << 4));
        const int m = wm0 + half * 64 + row, n = wn0 + (c & 3) * 8;
        if (m < p.M && n < p.N)
          *reinterpret_cast<uint4*>(gu_base + (long long)m * p.ldc + n) = make_uint4(pv.x, pv.y, pv.z, pv.w);
      }
    }
#pragma unroll
    for (int bi = 0; bi < 8; ++bi)
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        float h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gf = rbf(acc[bi][bj][e]), uf = rbf(acc[bi][bj + 2][e]);
          h[e] = rbf(gf * sigm(gf)) * uf;
        }
        // columns 0-31 of the park = rows 0-63, columns 32-63 = rows 64-127
        *reinterpret_cast<u32x2_t*>(park_at(park, bi & 3, (bi >> 2) * 2 + bj, l15, g4)) =
            u32x2_t{pack2bf(h[0], h[1]), pack2bf(h[2], h[3])};
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
    for (int it = 0; it < 8; ++it) {
      const int row = it * 8 + (lane >> 3), c = lane & 7;
      const u32x4_t pv = *reinterpret_cast<const u32x4_t*>(park + row * 128 + ((c ^ (row & 7)) << 4));
      const int m = wm0 + (c >> 2) * 64 + row, n = wn0 + (c & 3) * 8;
      if (m < p.M && n < p.N)
        *reinterpret_cast<uint4*>(p.C3 + (long long)m * p.ldc + n) = make_uint4(pv.x, pv.y, pv.z, pv.w);
    }
  }

  // Backward.  acc = d(act) of the wave's 128 x 64 tile.  Per 64-row half: the gate and up rows come in as full 128-byte
  // lines (16 bytes per lane), go through the park into the accumulator layout, d(gate) / d(up) are formed in registers and
  // leave through the park like any other tile.
  static __device__ __forceinline__ void epilogue16_swiglu_bwd(const Params& p, Acc16& acc, char* park, int wm0, int wn0,
                                                               int lane) {
    const int l15 = lane & 15, g4 = lane >> 4;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint4 gv[8], uv[8];
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3), c = lane & 7;
        const int m = wm0 + half * 64 + row, n = wn0 + c * 8;
        const bool in = m < p.M && n < p.N;
        const long long off = (long long)m * p.lde + n;
        gv[it] = in ? *reinterpret_cast<const uint4*>(p.E1 + off) : make_uint4(0, 0, 0, 0);
        uv[it] = in ? *reinterpret_cast<const uint4*>(p.E2 + off) : make_uint4(0, 0, 0, 0);
      }
      u32x2_t gq[4][4], uq[4][4];
      auto through_park = [&](const uint4 (&src)[8], u32x2_t (&dst)[4][4]) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int row = it * 8 + (lane >> 3), c = lane & 7;
          const u32x4_t v = {src[it].x, src[it].y, src[it].z, src[it].w};
          *reinterpret_cast<u32x4_t*>(park + row * 128 + ((c ^ (row & 7)) << 4)) = v;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
          for (int bj = 0; bj < 4; ++bj) dst[bi][bj] = *reinterpret_cast<const u32x2_t*>(park_at(park, bi, bj, l15, g4));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      };
      through_park(gv, gq);
      through_park(uv, uq);
#pragma unroll
      for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) {
          float dg[4], du[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t wg = e < 2 ? gq[bi][bj].x : gq[bi][bj].y, wu = e < 2 ? uq[bi][bj].x : uq[bi][bj].y;
            const float gf = (e & 1) ? hi16(wg) : lo16(wg), uf = (e & 1) ? hi16(wu) : lo16(wu);
            const float d = rbf(acc[half * 4 + bi][bj][e]);
            const float sg = sigm(gf);
            const float silu = gf * sg;
            du[e] = d * silu;
            dg[e] = d * uf * (sg + silu * (1.f - sg));
          }
          gq[bi][bj] = u32x2_t{pack2bf(dg[0], dg[1]), pack2bf(dg[2], dg[3])};
          uq[bi][bj] = u32x2_t{pack2bf(du[0], du[1]), pack2bf(du[2], du[3])};
        }
      auto out_park = [&](const u32x2_t (&src)[4][4], bf16_t* C) {
#pragma unroll
        for (int bi = 0; bi < 4; ++bi)
#pragma unroll
          for (int bj = 0; bj < 4; ++bj) *reinterpret_cast<u32x2_t*>(park_at(park, bi, bj, l15, g4)) = src[bi][bj];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
        for (int it = 0; it < 8; ++it) {
          const int row = it * 8 + (lane >> 3), c = lane & 7;
          const u32x4_t pv = *reinterpret_cast<const u32x4_t*>(park + row * 128 + ((c ^ (row & 7)) << 4));
          const int m = wm0 + half * 64 + row, n = wn0 + c * 8;
          if (m < p.M && n < p.N)
            *reinterpret_cast<uint4*>(C + (long long)m * p.ldc + n) = make_uint4(pv.x, pv.y, pv.z, pv.w);
        }
      };
      out_park(gq, p.C);
      out_park(uq, p.C2);
    }
  }

  // RoPE: blocks bj = 0, 1 hold columns col_a + 16 bj + 4 g4 .., blocks bj = 2, 3 the partners half a head further
  // (col_a + D / 2 + ..): both members of every rotary pair in one lane; c0 = index of col_a's pair inside the head (table
  // column).  Every table / bias element of a 64-row half is requested up front (ONE wait per half) — issued one (row block,
  // column quad) at a time the epilogue paid a memory round trip per quad.
  static __device__ __forceinline__ void epilogue16_rope(const Params& p, Acc16& acc, char* park, int wm0, int col_a, int c0,
                                                         int lane) {
    const int l15 = lane & 15, g4 = lane >> 4;
    const int hd = p.rope_d >> 1;
    const int col_b = col_a + hd;
    uint2 bwa[2], bwb[2];
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const int q = 16 * bj + 4 * g4;
      bwa[bj] = bwb[bj] = make_uint2(0, 0);
      if (p.bias != nullptr) {
        bwa[bj] = *reinterpret_cast<const uint2*>(p.bias + min(col_a + q, p.N - 4));
        bwb[bj] = *reinterpret_cast<const uint2*>(p.bias + min(col_b + q, p.N - 4));
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint2 cw[4][2], sw[4][2];
#pragma unroll
      for (int bi = 0; bi < 4; ++bi) {
        const int m = min(wm0 + (half * 4 + bi) * 16 + l15, p.M - 1);
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
          const long long o = (long long)m * hd + c0 + 16 * bj + 4 * g4;
          cw[bi][bj] = *reinterpret_cast<const uint2*>(p.rope_cos + o);
          sw[bi][bj] = *reinterpret_cast<const uint2*>(p.rope_sin + o);
        }
      }
#pragma unroll
      for (int bi = 0; bi < 4; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
          const float ba[4] = {lo16(bwa[bj].x), hi16(bwa[bj].x), lo16(bwa[bj].y), hi16(bwa[bj].y)};
          const float bb[4] = {lo16(bwb[bj].x), hi16(bwb[bj].x), lo16(bwb[bj].y), hi16(bwb[bj].y)};
          const float cf[4] = {lo16(cw[bi][bj].x), hi16(cw[bi][bj].x), lo16(cw[bi][bj].y), hi16(cw[bi][bj].y)};
          const float sf[4] = {lo16(sw[bi][bj].x), hi16(sw[bi][bj].x), lo16(sw[bi][bj].y), hi16(sw[bi][bj].y)};
          float ya[4], yb[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            rope_rotate(rbf(acc[half * 4 + bi][bj][e] + ba[e]), rbf(acc[half * 4 + bi][bj + 2][e] + bb[e]), cf[e], sf[e],
                        ya[e], yb[e]);
          *reinterpret_cast<u32x2_t*>(park_at(park, bi, bj, l15, g4)) = u32x2_t{pack2bf(ya[0], ya[1]), pack2bf(ya[2], ya[3])};
          *reinterpret_cast<u32x2_t*>(park_at(park, bi, bj + 2, l15, g4)) = u32x2_t{pack2bf(yb[0], yb[1]), pack2bf(yb[2], yb[3])};
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
      for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3), c = lane & 7;
        const u32x4_t pv = *reinterpret_cast<const u32x4_t*>(park + row * 128 + ((c ^ (row & 7)) << 4));
        const int m = wm0 + half * 64 + row, n = (c < 4 ? col_a : col_b) + (c & 3) * 8;
        if (m < p.M && n < p.N)
          *reinterpret_cast<uint4*>(p.C + (long long)m * p.ldc + n) = make_uint4(pv.x, pv.y, pv.z, pv.w);
      }
    }
  }

  // Epilogue through LDS, as Kernel::epilogue: the wave parks its 128 x 64 tile 64 rows at a time in its XOR-swizzled 8 KB
  // ([64 rows m][64 columns n] bf16, 16-byte chunk ^= row & 7) and writes full 128-byte lines.  A lane holds, per 16 x 16
  // block, column m = l & 15 and the 4 consecutive n = 4 (l >> 4) ..: 8-byte packs.
  static __device__ __forceinline__ void epilogue16(const Params& p, Acc16& acc, char* park, int wm0, int wn0, int lane) {
    const int l15 = lane & 15, g4 = lane >> 4;
    float bias_v[4][4];
    if (p.bias != nullptr) {
#pragma unroll
      for (int bj = 0; bj < 4; ++bj) {
        const int n = min(wn0 + bj * 16 + 4 * g4, p.N - 4);
        const uint2 w = *reinterpret_cast<const uint2*>(p.bias + n);
        bias_v[bj][0] = __uint_as_float(w.x << 16);
        bias_v[bj][1] = __uint_as_float(w.x & 0xffff0000u);
        bias_v[bj][2] = __uint_as_float(w.y << 16);
        bias_v[bj][3] = __uint_as_float(w.y & 0xffff0000u);
      }
    }
    const bool acc_c = p.accumulate != 0 || p.addend != nullptr;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      // GELU backward: the pre-activation rows this lane will meet in the read-out loop, asked for before the tile is parked
      // (fetched row by row inside that loop every load's latency was exposed: one workgroup per CU, attn_bwd_dq_stream.hip)
      uint4 xpre[8];
      if constexpr (EPI == EPI_GELU_BWD) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int m = wm0 + half * 64 + it * 8 + (lane >> 3), n = wn0 + (lane & 7) * 8;
          xpre[it] = (m < p.M && n < p.N) ? *reinterpret_cast<const uint4*>(p.E1 + (long long)m * p.lde + n)
                                          : make_uint4(0, 0, 0, 0);
        }
      }
#pragma unroll
      for (int bi = 0; bi < 4; ++bi) {
        const int row = bi * 16 + l15;
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[half * 4 + bi][bj][e] + (p.bias != nullptr ? bias_v[bj][e] : 0.f);
          const int chunk = (bj * 2 + (g4 >> 1)) ^ (row & 7);
          const u32x2_t pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
          *reinterpret_cast<u32x2_t*>(park + row * 128 + chunk * 16 + (g4 & 1) * 8) = pk;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      constexpr int kReadOutUnroll = EPI == EPI_GELU_BWD ? 8 : 4;       // (xpre[it] must be a register, not an indexed array)
#pragma unroll kReadOutUnroll
      for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3), c = lane & 7;
        const u32x4_t pv = *reinterpret_cast<const u32x4_t*>(park + row * 128 + ((c ^ (row & 7)) << 4));
        uint4 v = make_uint4(pv.x, pv.y, pv.z, pv.w);
        const int m = wm0 + half * 64 + row, n = wn0 + c * 8;
        if (m < p.M && n < p.N) {
          bf16_t* dst = p.C + (long long)m * p.ldc + n;
          if constexpr (EPI == EPI_GELU_FWD) {
            // v = the rounded pre-activation: stored, and its GELU beside it (what the activation kernel made of it)
            *reinterpret_cast<uint4*>(dst) = v;
            Vec16<bf16_t> x;
            x.raw = v;
            float f[8];
            x.unpack(f);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              const gelu_f32x2 r = gelu_f2(gelu_f32x2{f[e], f[e + 1]});
              f[e] = r.x;
              f[e + 1] = r.y;
            }
            x.pack(f);
            *reinterpret_cast<uint4*>(p.C2 + (long long)m * p.ldc + n) = x.raw;
            continue;
          }
          if constexpr (EPI == EPI_GELU_BWD) {
            // v = the rounded d(act): times gelu'(pre), what the GELU backward kernel made of the two
            Vec16<bf16_t> x, d;
            x.raw = xpre[it];
            d.raw = v;
            float f[8], df[8];
            x.unpack(f);
            d.unpack(df);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              const gelu_f32x2 r = gelu_grad_f2(gelu_f32x2{f[e], f[e + 1]}, gelu_f32x2{df[e], df[e + 1]});
              df[e] = r.x;
              df[e + 1] = r.y;
            }
            d.pack(df);
            *reinterpret_cast<uint4*>(dst) = d.raw;
            continue;
          }
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
    }
  }
};

template <bool AK, bool BK, int EPI = EPI_PLAIN>
__global__ __launch_bounds__(NT, 2) void gemm16_kernel(const Params p) {
  __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
  Kernel16<AK, BK, EPI>::run(p, smem);
}

// ws[S][ntiles][256 x 256] fp32 partial sums -> C = bf16(sum_s ws[s] (+ bias) (+ C)) on the tiles [tile0, tile0 + ntiles);
// 32 blocks of 256 threads per tile, one thread per 8 consecutive columns
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, int S, int M, int N, int nbm,
                                                            int nbn, int tile0, int ntiles, bf16_t* __restrict__ C,
                                                            long long ldc, const bf16_t* __restrict__ bias,
                                                            int accumulate, int out_f32,
                                                            const float* __restrict__ bias_ws,
                                                            bf16_t* __restrict__ bias_out) {
  const int t = blockIdx.x >> 5, part = blockIdx.x & 31;
  int tm, tn;
  tile_of_block(tile0 + t, nbm, nbn, tm, tn);
  const int idx = part * 256 + threadIdx.x;                 // 0 .. 8191: (row, 8-column group) of the tile
  const int lm = idx >> 5, ln = (idx & 31) * 8;
  const int m = tm * BM + lm, n = tn * BN + ln;
  if (m >= M || n >= N) return;
  if (bias_out != nullptr && tn == 0 && ln == 0) {          // EPI_BIASG: the units' partial column sums of A, row m
    float b = 0.f;
    for (int sp = 0; sp < S; ++sp) b += bias_ws[(long long)sp * (nbm * BM) + m];
    bias_out[m] = f2bf(b);
  }
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float* src = ws + (long long)t * (BM * BN) + lm * BN + ln;
  const long long slab = (long long)ntiles * (BM * BN);
  for (int sp = 0; sp < S; ++sp) {
    const float4 x = *reinterpret_cast<const float4*>(src + sp * slab);
    const float4 y = *reinterpret_cast<const float4*>(src + sp * slab + 4);
    a[0] += x.x; a[1] += x.y; a[2] += x.z; a[3] += x.w;
    a[4] += y.x; a[5] += y.y; a[6] += y.z; a[7] += y.w;
  }
  if (out_f32) {                                           // (weight gradients into fp32 staging: no bias)
    float* d = reinterpret_cast<float*>(C) + (long long)m * ldc + n;
    float4 x = make_float4(a[0], a[1], a[2], a[3]), y = make_float4(a[4], a[5], a[6], a[7]);
    if (accumulate) {
      const float4 ox = *reinterpret_cast<const float4*>(d), oy = *reinterpret_cast<const float4*>(d + 4);
      x.x += ox.x; x.y += ox.y; x.z += ox.z; x.w += ox.w;
      y.x += oy.x; y.y += oy.y; y.z += oy.z; y.w += oy.w;
    }
    *reinterpret_cast<float4*>(d) = x;
    *reinterpret_cast<float4*>(d + 4) = y;
    return;
  }
  bf16_t* dst = C + (long long)m * ldc + n;
  if (bias != nullptr) {
    Vec16<bf16_t> b;
    float fb[8];
    b.load(bias + n);
    b.unpack(fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += fb[e];
  }
  if (accumulate) {
    Vec16<bf16_t> o;
    float fo[8];
    o.load(dst);
    o.unpack(fo);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += fo[e];
  }
  Vec16<bf16_t> out;
  out.pack(a);
  out.store(dst);
}

// Which kernel a product runs on, by its shape alone (first match; -1 = no kernel for this combination, the entry points
// answer TN_EINVAL):
//   1. bias gradient wanted (weight-gradient mode only): Kernel EPI_BIASG — split-K + reduce, fp32 output, or bf16 output
//   2. split-K (no transposed copy): Kernel SPLITK + splitk_reduce_kernel
//   3. fp32 output (weight-gradient mode only): Kernel OUT_F32
//   4. row-stored A without a transposed copy (forward and input-gradient products): Kernel16
//   5. everything else (weight-gradient mode; any product with a transposed copy): Kernel
// Weight-gradient mode = both operands contraction-major, no transposed copy.
template <bool AK, bool BK, bool HAS_CT>
static int launch(dim3 grid, hipStream_t st, const Params& p) {
  constexpr bool WGRAD = AK && BK && !HAS_CT;
  auto reduce = [&](const float* bias_ws, bf16_t* bias_out) {
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)p.ntiles * 32u), dim3(256), 0, st, p.ws, p.splitk, p.M, p.N,
                       p.nbm, p.nbn, p.tile0, p.ntiles, p.C, p.ldc, p.bias, p.accumulate, p.c_f32, bias_ws, bias_out);
  };
  if (p.bias_out != nullptr) {
    if constexpr (WGRAD) {
      if (p.splitk > 1) {
        hipLaunchKernelGGL((gemm_kernel<true, true, false, true, false, EPI_BIASG>), grid, dim3(NT), 0, st, p);
        reduce(p.bias_ws, p.bias_out);
      } else if (p.c_f32) {
        hipLaunchKernelGGL((gemm_kernel<true, true, false, false, true, EPI_BIASG>), grid, dim3(NT), 0, st, p);
      } else {
        hipLaunchKernelGGL((gemm_kernel<true, true, false, false, false, EPI_BIASG>), grid, dim3(NT), 0, st, p);
      }
    } else {
      return -1;
    }
  } else if (p.splitk > 1) {
    if constexpr (!HAS_CT) {
      hipLaunchKernelGGL((gemm_kernel<AK, BK, false, true>), grid, dim3(NT), 0, st, p);
      reduce(nullptr, nullptr);
    } else {
      return -1;
    }
  } else if (p.c_f32) {
    if constexpr (WGRAD) {
      hipLaunchKernelGGL((gemm_kernel<true, true, false, false, true>), grid, dim3(NT), 0, st, p);
    } else {
      return -1;
    }
  } else if constexpr (!AK && !HAS_CT) {
    hipLaunchKernelGGL((gemm16_kernel<AK, BK>), grid, dim3(NT), 0, st, p);
  } else {
    hipLaunchKernelGGL((gemm_kernel<AK, BK, HAS_CT>), grid, dim3(NT), 0, st, p);
  }
  return 0;
}

}  // namespace gemm
}  // namespace tn

// ---- host side: ONE owner per rule — the grid (grid_for), the argument checks (row_operand_ok, kmaj_operand_ok, out_ok),
// the split-K workspace layout (tn_gemm_splitk_workspace_bytes), the grouped launch's remainder split (grouped_split), one
// product of either grouped launch (grouped_product), the general launcher (gemm_launch) and the fused-epilogue launcher (launch_fused); the C entry points follow them --------------

extern "C" long long tn_gemm_splitk_workspace_bytes(int M, int N, int splitk, int with_bias_grad, int tail_only);

namespace {

// One workgroup per CU walking a fixed tile list (1, default) or one workgroup per tile (0).  A host that runs collectives
// beside the compute (RCCL kernels hold CUs) selects 0 — touchnet_amd/bin/train.py — instead of changing the process
// environment; TN_GEMM_PERSIST in the environment still overrides it.
int g_persistent = 1;

// ---- split-K workspaces: fp32 slabs of whole tiles, [parts][tiles][256 x 256] ---------------------------------------------
long long slab_floats(int parts, long long tiles) { return parts * tiles * BM * BN; }

// The grouped launch's remainder split: r = tiles of the last partial round; returns the parts it is cut into (1 = it runs
// as whole tiles: no whole round before it, more than half a round of it, or fewer than 16 stages somewhere)
int grouped_split(long long total, int min_stages, int& r) {
  const int ncu = num_cus();
  r = (int)(total % ncu);
  if (total <= ncu || r == 0 || r * 2 > ncu || min_stages < 16) return 1;
  return min(ncu / r, min_stages / 8);
}

// One call of the general launcher; an entry point sets the fields it means and leaves the rest.
struct GemmCall {
  // C[M,N] = sum_s opA_s · opB_s^T: arrays of nseg (1..3) entries; a_kmaj / b_kmaj: 0 = operand stored [rows, K]
  // (contraction-contiguous), 1 = stored [K, rows] (contraction-major)
  const void* const* A;
  const void* const* B;
  const long long* lda;
  const long long* ldb;
  const int* K;
  int nseg, a_kmaj, b_kmaj;
  void* C;
  long long ldc;
  int M, N;
  void* stream;
  const void* bias = nullptr;      // + bias[N]
  int accumulate = 0;              // + C
  void* Ct = nullptr;              // transposed copy [N, M], pitch ldct
  long long ldct = 0;
  int splitk = 1, tail_only = 0;   // split-K through `workspace` (tn_gemm_splitk_workspace_bytes)
  void* workspace = nullptr;
  long long workspace_bytes = 0;
  int c_f32 = 0;                   // C is float (weight-gradient mode)
  void* bias_grad = nullptr;       // bf16 [M] column sums of A (weight-gradient mode)
  const void* addend = nullptr;    // + addend[M, N], pitch ldadd
  long long ldadd = 0;
};

int launch_mode(bool a_kmaj, bool b_kmaj, bool ct, dim3 grid, hipStream_t st, const Params& p) {
  if (!a_kmaj && !b_kmaj) return ct ? launch<false, false, true>(grid, st, p) : launch<false, false, false>(grid, st, p);
  if (!a_kmaj) return ct ? launch<false, true, true>(grid, st, p) : launch<false, true, false>(grid, st, p);
  return ct ? launch<true, true, true>(grid, st, p) : launch<true, true, false>(grid, st, p);
}

// Requirements (else -22): the operand checks above per segment, N % 8 == 0, a_kmaj: M % 8 == 0; with Ct: M % 8 == 0,
// ldct % 8 == 0, no accumulate.
int gemm_launch(const GemmCall& c) {
  const int M = c.M, N = c.N;
  const bool wgrad_mode = c.a_kmaj && c.b_kmaj && c.nseg == 1 && c.Ct == nullptr && c.bias == nullptr;
  if (c.a_kmaj && !c.b_kmaj) return TN_EINVAL;       // (A contraction-major with B contraction-contiguous: no caller)
  // (the addend rides on the plain epilogue of an unsplit, single-output product)
  if (c.addend != nullptr && (c.accumulate || c.splitk > 1 || c.tail_only || c.Ct != nullptr || c.c_f32 ||
                              c.bias_grad != nullptr || !out_ok(c.addend, c.ldadd, N, 8)))
    return TN_EINVAL;
  if ((c.bias_grad != nullptr || c.c_f32) && (!wgrad_mode || c.tail_only)) return TN_EINVAL;
  if (!aligned(1, c.bias_grad)) return TN_EINVAL;
  if (M <= 0 || N <= 0 || c.nseg < 1 || c.nseg > MAXSEG || (N % 8) != 0 || (c.a_kmaj && (M % 8))) return TN_EINVAL;
  if (!out_ok(c.C, c.ldc, N, 8)) return TN_EINVAL;
  if (c.Ct != nullptr && ((M % 8) || c.accumulate || !out_ok(c.Ct, c.ldct, M, 8))) return TN_EINVAL;
  Params p;
  clear_params(p);
  for (int s = 0; s < c.nseg; ++s) {
    const int k = c.K[s];
    if (!(c.a_kmaj ? kmaj_operand_ok(c.A[s], c.lda[s], k, M, M) : row_operand_ok(c.A[s], c.lda[s], k, 1))) return TN_EINVAL;
    if (!(c.b_kmaj ? kmaj_operand_ok(c.B[s], c.ldb[s], k, N, 1) : row_operand_ok(c.B[s], c.ldb[s], k, 1))) return TN_EINVAL;
    set_seg(p.seg[s], c.A[s], c.B[s], c.lda[s], c.ldb[s], k);
    p.stages += (k + 63) / 64;
  }
  for (int s = c.nseg; s < MAXSEG; ++s) p.seg[s] = p.seg[0];
  p.nseg = c.nseg;
  p.M = M;
  p.N = N;
  p.C = (bf16_t*)c.C;
  p.Ct = (bf16_t*)c.Ct;
  p.bias = (const bf16_t*)c.bias;
  p.ldc = c.ldc;
  p.ldct = c.ldct;
  p.accumulate = c.accumulate;
  p.addend = (const bf16_t*)c.addend;
  p.ldadd = c.ldadd;
  p.nbm = (M + BM - 1) / BM;
  p.nbn = (N + BN - 1) / BN;
  p.ntiles = p.nbm * p.nbn;
  p.c_f32 = c.c_f32;
  p.bias_out = (bf16_t*)c.bias_grad;
  const int ncu = num_cus();
  int main_tiles = 0;                                // tail split: tiles [0, main_tiles) run unsplit first
  if (c.splitk > 1) {
    // one segment, no transposed copy; a contraction-contiguous operand cannot be cut inside a stage or read behind K
    if (c.nseg != 1 || c.Ct != nullptr) return TN_EINVAL;
    if (!(c.a_kmaj && c.b_kmaj) && (p.stages % c.splitk) != 0) return TN_EINVAL;
    const long long need = tn_gemm_splitk_workspace_bytes(M, N, c.splitk, c.bias_grad != nullptr, c.tail_only);
    if (need < 0 || c.workspace == nullptr || !aligned(15, c.workspace) || c.workspace_bytes < need) return TN_EINVAL;
    if (c.tail_only) main_tiles = p.ntiles / ncu * ncu;
    p.splitk = c.splitk;
    p.kchunk = (p.stages + c.splitk - 1) / c.splitk;
    p.ws = (float*)c.workspace;
    if (c.bias_grad != nullptr) p.bias_ws = p.ws + slab_floats(c.splitk, p.ntiles);   // [splitk][nbm * 256] behind the slabs
  }
  hipStream_t st = (hipStream_t)c.stream;
  int rc = 0;
  if (main_tiles > 0) {                              // whole rounds first, unsplit, one workgroup per CU ...
    Params pm = p;
    pm.splitk = 1;
    pm.ntiles = main_tiles;
    rc |= launch_mode(c.a_kmaj, c.b_kmaj, c.Ct != nullptr, dim3(ncu), st, pm);
    p.tile0 = main_tiles;                            // ... then the last partial round, split
    p.ntiles -= main_tiles;
  }
  rc |= launch_mode(c.a_kmaj, c.b_kmaj, c.Ct != nullptr, grid_for(p.ntiles * p.splitk), st, p);
  if (rc != 0) return TN_EINVAL;
  TN_LAUNCH_CHECK();
  return TN_OK;
}

// THE launcher of the fused-epilogue products (Kernel16, row-stored A, one accumulator, whole tiles): the entry has checked
// its arguments and set the segments it uses (seg[0]; SwiGLU forward also seg[1]), the outputs and the epilogue's extra
// inputs.  col_tile: output columns per tile — 256, or 128 where a tile is 128 gate + 128 up columns.
template <int EPI, bool B_KMAJ>
int launch_fused(Params& p, int M, int N, long long ldc, int col_tile, void* stream) {
  for (int s = 1; s < MAXSEG; ++s)
    if (p.seg[s].K == 0) p.seg[s] = p.seg[0];
  p.stages = p.seg[0].K / 64;
  p.M = M;
  p.N = N;
  p.ldc = ldc;
  p.nbm = (M + BM - 1) / BM;
  p.nbn = (N + col_tile - 1) / col_tile;
  p.ntiles = p.nbm * p.nbn;
  hipLaunchKernelGGL((gemm16_kernel<false, B_KMAJ, EPI>), grid_for(p.ntiles), dim3(NT), 0, (hipStream_t)stream, p);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // namespace

extern "C" {

void tn_gemm_set_persistent(int on) { g_persistent = on ? 1 : 0; }
int tn_gemm_get_persistent(void) { return g_persistent; }

long long tn_gemm_splitk_workspace_bytes(int M, int N, int splitk, int with_bias_grad, int tail_only) {
  if (splitk <= 1) return 0;
  if (M <= 0 || N <= 0) return -1;
  const long long nbm = (M + BM - 1) / BM;
  long long tiles = nbm * ((N + BN - 1) / BN);
  if (tail_only) {                                   // whole rounds run unsplit: only the last partial round is split
    const int ncu = num_cus();
    if (tiles < ncu || tiles % ncu == 0) return -1;
    tiles %= ncu;
  }
  return (slab_floats(splitk, tiles) + (with_bias_grad ? splitk * nbm * BM : 0)) * (long long)sizeof(float);
}

// General entry: C[M,N] = sum_s opA_s · opB_s^T (+ bias) (+ C if accumulate); optional transposed copy Ct[N,M].
int tn_gemm_bf16(const void* const* A, const void* const* B, const long long* lda, const long long* ldb, const int* K,
                 int nseg, int a_kmaj, int b_kmaj, void* C, void* Ct, const void* bias, int M, int N, long long ldc,
                 long long ldct, int accumulate, void* stream) {
  GemmCall c{A, B, lda, ldb, K, nseg, a_kmaj, b_kmaj, C, ldc, M, N, stream};
  c.bias = bias;
  c.accumulate = accumulate;
  c.Ct = Ct;
  c.ldct = ldct;
  return gemm_launch(c);
}

// C = A B^T (+ bias) + addend: the residual stream added in the producing GEMM's epilogue (addend [M, N] bf16, pitch ldadd;
// it may NOT alias C).  One segment; the product is rounded to bf16 before the addition — the bits of the two-kernel form
// (GEMM, then the norm kernel's residual add: modeling_llama.py / modeling_qwen2.py `hidden_states = residual +
// hidden_states`).
int tn_gemm_bf16_addend(const void* A, const void* B, long long lda, long long ldb, int K, int a_kmaj, int b_kmaj, void* C,
                        const void* bias, const void* addend, long long ldadd, int M, int N, long long ldc, void* stream) {
  if (addend == nullptr || addend == C) return TN_EINVAL;
  GemmCall c{&A, &B, &lda, &ldb, &K, 1, a_kmaj, b_kmaj, C, ldc, M, N, stream};
  c.bias = bias;
  c.addend = addend;
  c.ldadd = ldadd;
  return gemm_launch(c);
}

// The same product with the contraction cut into `splitk` parts that run as independent units; fp32 partial sums go through
// `workspace` (tn_gemm_splitk_workspace_bytes, 16-byte aligned) and a second kernel adds them up (+ bias, + C).
// tail_only = 0: every tile is split (outputs of few tiles with a deep contraction); tail_only = 1: the whole rounds of
// tiles (floor(tiles / CUs) * CUs) run unsplit, only the last partial round is split (-22 when there is no whole round or
// no remainder).  One segment, no transposed copy; with a contraction-contiguous operand the number of 64-deep stages must
// be a multiple of splitk (else -22).
int tn_gemm_bf16_splitk(const void* A, const void* B, long long lda, long long ldb, int K, int a_kmaj, int b_kmaj,
                        void* C, const void* bias, int M, int N, long long ldc, int accumulate, int splitk, int tail_only,
                        void* workspace, long long workspace_bytes, void* stream) {
  if (splitk < 2) return TN_EINVAL;
  GemmCall c{&A, &B, &lda, &ldb, &K, 1, a_kmaj, b_kmaj, C, ldc, M, N, stream};
  c.bias = bias;
  c.accumulate = accumulate;
  c.splitk = splitk;
  c.tail_only = tail_only;
  c.workspace = workspace;
  c.workspace_bytes = workspace_bytes;
  return gemm_launch(c);
}

// Weight gradient AND (bias_grad != NULL) bias gradient of a linear layer y = x W^T + b in one launch: C[M, N] (bf16, or
// float with ldc in floats when c_f32; += when accumulate) = A[K, M]^T . B[K, N] and bias_grad[M] (bf16) = column sums of
// A — A = dY [tokens, M], B = x [tokens, N] as stored, both contraction-major.  The sums come from the A fragments the matrix
// pipe reads anyway (EPI_BIASG above): no separate pass over dY.  splitk <= 1: plain; >= 2: split-K through `workspace`
// (tn_gemm_splitk_workspace_bytes).
static int wgrad(const void* A, const void* B, long long lda, long long ldb, int K, void* C, void* bias_grad, int M, int N,
                 long long ldc, int accumulate, int c_f32, int splitk, void* workspace, long long workspace_bytes,
                 void* stream) {
  GemmCall c{&A, &B, &lda, &ldb, &K, 1, 1, 1, C, ldc, M, N, stream};
  c.accumulate = accumulate;
  c.c_f32 = c_f32;
  c.bias_grad = bias_grad;
  c.splitk = splitk > 1 ? splitk : 1;
  c.workspace = workspace;
  c.workspace_bytes = workspace_bytes;
  return gemm_launch(c);
}

int tn_gemm_bf16_wgrad_f32(const void* A, const void* B, long long lda, long long ldb, int K, float* C, int M, int N,
                           long long ldc, int accumulate, int splitk, void* workspace, long long workspace_bytes,
                           void* stream) {
  return wgrad(A, B, lda, ldb, K, C, nullptr, M, N, ldc, accumulate, 1, splitk, workspace, workspace_bytes, stream);
}

int tn_gemm_bf16_wgrad_bias(const void* A, const void* B, long long lda, long long ldb, int K, void* C, void* bias_grad,
                            int M, int N, long long ldc, int accumulate, int c_f32, int splitk, void* workspace,
                            long long workspace_bytes, void* stream) {
  if (bias_grad == nullptr) return TN_EINVAL;
  return wgrad(A, B, lda, ldb, K, C, bias_grad, M, N, ldc, accumulate, c_f32, splitk, workspace, workspace_bytes, stream);
}

// Several independent products of ONE operand mode in one persistent launch (`ngrp` = 1..3; product g:
// C_g[M_g, N_g] (+)= opA_g · opB_g^T, one segment each, no bias).  What it is for: the MLP's three weight gradients are 688
// output tiles each = 2.69 rounds on 256 CUs, i.e. three launches idle a third of the chip in their last rounds; as one
// tile list they are 2064 tiles = 8 whole rounds + 16.  That remainder (grouped_split) runs split-K — `workspace` >=
// tn_gemm_grouped_workspace_bytes(...) — so it costs a fraction of a round instead of a whole one.  c_f32: fp32 outputs
// (ldc in floats; both operands contraction-major).
long long tn_gemm_grouped_workspace_bytes(const int* M, const int* N, const int* K, int ngrp) {
  if (ngrp < 1 || ngrp > MAXSEG) return -1;
  long long tiles = 0;
  int min_stages = 0x7fffffff, r;
  for (int g = 0; g < ngrp; ++g) {
    tiles += (long long)((M[g] + BM - 1) / BM) * ((N[g] + BN - 1) / BN);
    min_stages = min(min_stages, (K[g] + 63) / 64);
  }
  const int S = grouped_split(tiles, min_stages, r);
  return S > 1 ? slab_floats(S, r) * (long long)sizeof(float) : 0;
}

int tn_gemm_bf16_grouped(const void* const* A, const void* const* B, const long long* lda, const long long* ldb,
                         const int* K, void* const* C, const long long* ldc, const int* M, const int* N, int ngrp,
                         int a_kmaj, int b_kmaj, int accumulate, int c_f32, void* workspace, long long workspace_bytes,
                         void* stream) {
  if (ngrp < 1 || ngrp > MAXSEG) return TN_EINVAL;
  if (!(a_kmaj && b_kmaj)) return TN_EINVAL;               // (weight-gradient mode: the one caller)
  Params p;
  clear_params(p);
  int total = 0, min_stages = 0x7fffffff;
  for (int g = 0; g < ngrp; ++g) {
    if (!grouped_product(A[g], B[g], lda[g], ldb[g], K[g], C[g], ldc[g], M[g], N[g], c_f32, total, p.seg[g], p.grp[g]))
      return TN_EINVAL;
    min_stages = min(min_stages, p.grp[g].stages);
    total += p.grp[g].nbm * p.grp[g].nbn;
  }
  for (int g = ngrp; g < MAXSEG; ++g) {
    p.seg[g] = p.seg[0];
    p.grp[g] = p.grp[0];
    p.grp[g].start = 0x7fffffff;
  }
  p.ngrp = ngrp;
  p.accumulate = accumulate;
  p.c_f32 = c_f32;
  hipStream_t st = (hipStream_t)stream;
  int r, S = grouped_split(total, min_stages, r);
  if (S > 1 && (workspace == nullptr || !aligned(15, workspace) ||
                workspace_bytes < slab_floats(S, r) * (long long)sizeof(float)))
    S = 1;                                                  // (no workspace: the remainder runs as whole tiles)
  const int main_tiles = S > 1 ? total - r : total;
  p.tile0 = 0;
  p.ntiles = main_tiles;
  if (c_f32)
    hipLaunchKernelGGL((gemm_kernel<true, true, false, false, true, EPI_GROUPED>), grid_for(main_tiles), dim3(NT), 0, st, p);
  else
    hipLaunchKernelGGL((gemm_kernel<true, true, false, false, false, EPI_GROUPED>), grid_for(main_tiles), dim3(NT), 0, st, p);
  if (S > 1) {
    float* ws = (float*)workspace;
    for (int g = 0; g < ngrp; ++g) {
      const int end = p.grp[g].start + p.grp[g].nbm * p.grp[g].nbn;
      const int lo = max(main_tiles, p.grp[g].start), hi = end;
      if (lo >= hi) continue;
      Params q;
      clear_params(q);
      q.seg[0] = p.seg[g];
      q.seg[1] = q.seg[2] = q.seg[0];
      q.M = p.grp[g].M;
      q.N = p.grp[g].N;
      q.C = p.grp[g].C;
      q.ldc = p.grp[g].ldc;
      q.accumulate = accumulate;
      q.nbm = p.grp[g].nbm;
      q.nbn = p.grp[g].nbn;
      q.stages = p.grp[g].stages;
      q.splitk = S;
      q.kchunk = (q.stages + S - 1) / S;
      q.ws = ws;
      q.tile0 = lo - p.grp[g].start;
      q.ntiles = hi - lo;
      q.c_f32 = c_f32;
      hipLaunchKernelGGL((gemm_kernel<true, true, false, true>), grid_for(q.ntiles * S), dim3(NT), 0, st, q);
      hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)q.ntiles * 32u), dim3(256), 0, st, q.ws, q.splitk, q.M, q.N,
                         q.nbm, q.nbn, q.tile0, q.ntiles, q.C, q.ldc, (const bf16_t*)nullptr, q.accumulate, q.c_f32,
                         (const float*)nullptr, (bf16_t*)nullptr);
      ws += slab_floats(S, q.ntiles);
    }
  }
  TN_LAUNCH_CHECK();
  return TN_OK;
}
// The MLP's gate and up products with the SwiGLU fused into the epilogue (transformers' LlamaMLP.forward; liger's fused
// SwiGLU at touchnet/models/llama/__init__.py:11-15): gate[M, I] = x Wg^T, up[M, I] = x Wu^T, act = silu(gate) * up, all
// bf16 with row pitch ldc; x [M, K] (pitch ldx), Wg / Wu [I, K] (pitch ldw).  -22 unless K % 64 == 0, I % 8 == 0, pitches % 8.
int tn_gemm_bf16_swiglu_fwd(const void* x, const void* wg, const void* wu, void* gate, void* up, void* act, int M, int I,
                            int K, long long ldx, long long ldw, long long ldc, void* stream) {
  if (M <= 0 || I <= 0 || (I % 8) || !row_operand_ok(x, ldx, K, K) || !row_operand_ok(wg, ldw, K, K) ||
      !row_operand_ok(wu, ldw, K, K) || !out_ok(gate, ldc, I, 8) || !aligned(15, up, act))
    return TN_EINVAL;
  Params p;
  clear_params(p);
  set_seg(p.seg[0], x, wg, ldx, ldw, K);
  set_seg(p.seg[1], x, wu, ldx, ldw, K);
  p.C = (bf16_t*)gate;
  p.C2 = (bf16_t*)up;
  p.C3 = (bf16_t*)act;
  return launch_fused<EPI_SWIGLU_FWD, false>(p, M, I, ldc, 128, stream);
}

// Its backward counterpart: d(act) = dY W_down (dY [M, H] pitch lddy, W_down [H, I] read contraction-major, pitch ldw) is
// formed in the accumulators only; the epilogue reads gate / up [M, I] (pitch ld) and writes d(gate), d(up) (pitch ld).
// -22 unless H % 64 == 0, I % 8 == 0, pitches % 8.
int tn_gemm_bf16_swiglu_bwd(const void* dy, const void* wd, const void* gate, const void* up, void* dgate, void* dup,
                            int M, int I, int H, long long lddy, long long ldw, long long ld, void* stream) {
  if (M <= 0 || I <= 0 || (I % 8) || !row_operand_ok(dy, lddy, H, H) || !kmaj_operand_ok(wd, ldw, H, I, I) ||
      !out_ok(dgate, ld, I, 8) || !aligned(15, dup, gate, up))
    return TN_EINVAL;
  Params p;
  clear_params(p);
  set_seg(p.seg[0], dy, wd, lddy, ldw, H);
  p.C = (bf16_t*)dgate;
  p.C2 = (bf16_t*)dup;
  p.E1 = (const bf16_t*)gate;
  p.E2 = (const bf16_t*)up;
  p.lde = ld;
  return launch_fused<EPI_SWIGLU_BWD, true>(p, M, I, ld, BN, stream);
}

// A q / k projection with the rotary embedding in the epilogue: out[M, N] = rope(x W^T + bias), N = heads x head_dim
// (head_dim 64 or 128; N % 256 == 0 for 128, N % 64 == 0 for 64), cos / sin [M, head_dim / 2] bf16 = one table row per
// output row (tn_rope_table).  -22 unless K % 64 == 0 and the pitches are multiples of 8.
int tn_gemm_bf16_rope(const void* x, const void* w, const void* bias, const void* cos_t, const void* sin_t, void* out, int M,
                      int N, int K, long long ldx, long long ldw, long long ldc, int head_dim, void* stream) {
  if (M <= 0 || N <= 0 || !row_operand_ok(x, ldx, K, K) || !row_operand_ok(w, ldw, K, K) || !out_ok(out, ldc, N, 8))
    return TN_EINVAL;
  if (!((head_dim == 128 && N % 256 == 0) || (head_dim == 64 && N % 64 == 0))) return TN_EINVAL;
  // (the epilogue reads the tables and the bias in 8-byte pieces)
  if (cos_t == nullptr || sin_t == nullptr || !aligned(7, cos_t, sin_t, bias)) return TN_EINVAL;
  Params p;
  clear_params(p);
  set_seg(p.seg[0], x, w, ldx, ldw, K);
  p.C = (bf16_t*)out;
  p.bias = (const bf16_t*)bias;
  p.rope_cos = (const bf16_t*)cos_t;
  p.rope_sin = (const bf16_t*)sin_t;
  p.rope_d = head_dim;
  return launch_fused<EPI_ROPE, false>(p, M, N, ldc, BN, stream);
}

// The audio tower's MLP, first half: pre[M, N] = x[M, K] W[N, K]^T + bias AND act = gelu(pre) from one launch (exact-erf
// GELU, common.h gelu_f: the bits of tn_gelu_fwd on the rounded pre).  -22 unless K % 64 == 0, N % 8 == 0, pitches % 8 and
// >= the rows they span, 16-byte aligned bases.
int tn_gemm_bf16_gelu_fwd(const void* x, const void* w, const void* bias, void* pre, void* act, int M, int N, int K,
                          long long ldx, long long ldw, long long ldc, void* stream) {
  if (M <= 0 || N <= 0 || (N % 8) || !row_operand_ok(x, ldx, K, K) || !row_operand_ok(w, ldw, K, K) ||
      !out_ok(pre, ldc, N, 8) || !aligned(15, act) || !aligned(7, bias))
    return TN_EINVAL;
  if (pre == act) return TN_EINVAL;                  // (this entry alone has two outputs of one meaning to mix up)
  Params p;
  clear_params(p);
  set_seg(p.seg[0], x, w, ldx, ldw, K);
  p.C = (bf16_t*)pre;
  p.C2 = (bf16_t*)act;
  p.bias = (const bf16_t*)bias;
  return launch_fused<EPI_GELU_FWD, false>(p, M, N, ldc, BN, stream);
}

// ... and the backward of its second half: d(pre)[M, I] = (dY[M, H] W2[H, I]) o gelu'(pre) — the product d(act) is formed in
// the accumulators only (W2 read contraction-major, pitch ldw; pre and d(pre) with pitch ld).  -22 unless H % 64 == 0,
// I % 8 == 0, pitches % 8.
int tn_gemm_bf16_gelu_bwd(const void* dy, const void* w2, const void* pre, void* dpre, int M, int I, int H, long long lddy,
                          long long ldw, long long ld, void* stream) {
  if (M <= 0 || I <= 0 || (I % 8) || !row_operand_ok(dy, lddy, H, H) || !kmaj_operand_ok(w2, ldw, H, I, I) ||
      !out_ok(dpre, ld, I, 8) || !aligned(15, pre))
    return TN_EINVAL;
  Params p;
  clear_params(p);
  set_seg(p.seg[0], dy, w2, lddy, ldw, H);
  p.C = (bf16_t*)dpre;
  p.E1 = (const bf16_t*)pre;
  p.lde = ld;
  return launch_fused<EPI_GELU_BWD, true>(p, M, I, ld, BN, stream);
}

// C[M,N] = A[M,K] · B[N,K]^T (+ bias) (+ C if accumulate); optional transposed copy Ct[N,M]: the single-segment,
// both-operands-contraction-contiguous case of tn_gemm_bf16.
int tn_gemm_bf16_tn(const void* A, const void* B, void* C, void* Ct, const void* bias, int M, int N, int K,
                    long long lda, long long ldb, long long ldc, long long ldct, int accumulate, void* stream) {
  return tn_gemm_bf16(&A, &B, &lda, &ldb, &K, 1, 0, 0, C, Ct, bias, M, N, ldc, ldct, accumulate, stream);
}

}  // extern "C"
