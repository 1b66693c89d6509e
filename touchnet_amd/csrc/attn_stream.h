// What the two "stream" attention kernels share (attn_fwd_stream.hip, attn_bwd_dq_stream.hip): a workgroup owns 128 query
// rows of one head and walks the 64-row KV tiles that can meet them — the stored list of attn_common.h (klist), or a list it
// builds in chunks from the tile metadata — with K / V tiles travelling global -> LDS by LDS-DMA into a two-slot ring, one
// stage ahead.  Here: the geometry of that ring, the list builder, the K / V stage DMA and the per-trip predicates.  Each
// kernel keeps what is its own: how its Q (and dO) rows reach registers, its MFMA chains, its softmax arithmetic and the
// retire schedules of its operand reads.
//
// TileLister and KVStage are structs of REFERENCES to the kernel's own variables, as the lambdas they replace captured
// them: handed the same state by value, hipcc folds the address arithmetic of issue() differently (v_lshl_or_b32 becomes
// s_lshl_b32 + v_or_b32, registers renumbered) and the kernels' assembly changes.
#pragma once
#include "attn_common.h"

namespace tn {

template <int D>
struct StreamGeom {
  static constexpr int BM = 128, BN = 64, NST = 2;
  static constexpr int KSTEPS = D / 16, DBLK = D / 32;
  using Tile = PTile<BN, D>;
  static constexpr int IMGB = Tile::SIZE * 2;          // bytes of one panel image
  static constexpr int NPC = Tile::NP * (BN / 16);     // 1-KiB DMA pieces per image: 16 rows of one panel each
  static constexpr int PPW = NPC / 4;                  // pieces per wave and image
  static constexpr int IPS = 2 * PPW + 1;              // DMA instructions per wave and stage
  static constexpr int STAGE_KV = 2 * IMGB + 4 * 256;  // {K image | V image | doc ids[64] per wave}
  static constexpr int OUTB = 4 * WholeRows<D>::BYTES;  // a slot also stages the four waves' 32 output rows each
  static constexpr int STAGEB = STAGE_KV > OUTB ? STAGE_KV : OUTB;
  static constexpr int CAP = 192;                      // tile-list chunk
  // ONE LDS variable (attn_bwd.hip explains why two would serialise the DMA ring): {ring | tile list | wave counts}
  static constexpr int LIST = NST * STAGEB, WCOUNT = LIST + (CAP + 4) * 16, SMEM = WCOUNT + 16;
};

// Tiles of [lo, hi_t] that may interact with the query tile -> list entries {tile, min id, max id, min positive id} in
// `tlist`, four end marks behind them; returns their number.  keep(j): a further test of tile j — the forward's key-chunk
// restriction (QView::kv_tile_on); the dQ pass keeps every tile: no backward entry point sets a restriction.
struct EveryKeyChunk {
  __device__ __forceinline__ bool kv_tile_on(int) const { return true; }
};
template <class Chunks>
struct TileLister {
  const int& tid;
  const int *const &m_min, *const &m_max, *const &m_minpos;
  const int &bminpos, &bmax;
  Chunks chunks;
  const int& lane;
  int* const& wcount;
  const int& wave;
  i32x4_t* const& tlist;
  const int& j_hi;
  __device__ __forceinline__ int operator()(int lo, int hi_t) const {
    const int j = lo + tid;
    int mn = 0, mx = 0, mp = 0;
    bool ok = false;
    if (j <= hi_t) {
      mn = m_min[j];
      mx = m_max[j];
      mp = m_minpos[j];
      ok = tile_may_interact(bminpos, bmax, mp, mx) && chunks.kv_tile_on(j);
    }
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wcount[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (ok) tlist[before + __popcll(bal & ((1ull << lane) - 1ull))] = i32x4_t{j, mn, mx, mp};
    const int n = __builtin_amdgcn_readfirstlane(total);
    if (tid < 4) tlist[n + tid] = i32x4_t{j_hi + 1, 0, 0, 0};
    __syncthreads();
    return n;
  }
};

// K / V tile j -> ring slot `slot`: always IPS instructions per wave (the counted waits of the ring rely on it)
template <int D>
struct KVStage {
  using G = StreamGeom<D>;
  static constexpr uint32_t OOB = 0x80000000u;       // >= num_records: the load returns 0 and touches no memory
  char* const smem;
  const int &T, &Nkv, &hk, &wave, &lane, &rr;
  const size_t& krow_elems;
  const uint32_t& voff;
  const __amdgpu_buffer_rsrc_t &rk, &rv, &rdoc;
  __device__ __forceinline__ void operator()(int j, int slot) const {
    using Tile = typename G::Tile;
    char* st = smem + slot * G::STAGEB;
    const int k0 = j * G::BN;
    const int left = min(T - k0, G::BN);
    const uint32_t base = (uint32_t)(((size_t)k0 * Nkv + hk) * D * 2);
#pragma unroll
    for (int i = 0; i < G::PPW; ++i) {
      const int pc = wave + 4 * i, panel = pc % Tile::NP, rh = pc / Tile::NP;
      const uint32_t vo = (16 * rh + rr < left) ? voff : OOB;
      const uint32_t so = base + (uint32_t)((16 * rh * krow_elems + 32 * panel) * 2);
      char* dst = st + panel * (Tile::PSTRIDE * 2) + rh * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_ptr_t)dst, 16, vo, so, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_ptr_t)(dst + G::IMGB), 16, vo, so, 0, 0);
    }
    const uint32_t va = lane < left ? (uint32_t)lane * 4 : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rdoc, (lds_ptr_t)(st + 2 * G::IMGB + 256 * wave), 4, va, (uint32_t)k0 * 4,
                                             0, 0);
  }
};

// K "row" operand fragments kf[buf][0..3] have arrived (KEEP younger LDS reads may stay in flight).  A macro: an asm
// operand cannot name an array captured from an enclosing scope.
#define TN_K_RETIRE(buf, keep)                                                                                        \
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(kf[buf][0]), "+v"(kf[buf][1]), "+v"(kf[buf][2]), "+v"(kf[buf][3])       \
               : "n"(keep))

}  // namespace tn
