// Shared pieces of the packed (document-masked, causal) attention kernels for gfx950.
//
// Mask predicate (bit-exact restatement of transformers/integrations/flex_attention.py:190-201 as
// invoked at touchnet/models/kimi_audio/modeling_kimi_audio.py:582-585 for the packers' document ids,
// touchnet/models/llama/processing_llama.py:38-40):
//     allow(b, q, kv) = (q >= kv) && (doc[b,q] > 0) && (doc[b,q] == doc[b,kv])
// Rows with no allowed key (pad rows, doc == 0) produce 0 output / 0 gradient (flex semantics).
//
// MFMA conventions used everywhere (v_mfma_f32_32x32x16_bf16, wave64):
//   operand A[i][k] / B[k][j]: lane holds i (resp. j) = lane & 31 and 8 contraction slots selected by
//     (lane >> 5, e) — the same slot function for A and B, so any consistent choice of which logical
//     index feeds slot (hi, e) is valid;
//   result  C[i][j]: lane holds column j = lane & 31, register r holds row
//     i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace tn {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
// LDS reads in kernels that fill LDS by LDS-DMA (buffer_load ... lds) must go through these ext_vector_type pointers,
// NOT through HIP's uint4 / int4 / float4 structs: hipcc's waitcnt insertion puts an `s_waitcnt vmcnt(0)` in front of
// any LDS access that carries no alias metadata while an LDS-DMA is pending (it cannot tell the slots of a ring apart),
// which silently serialises a hand-counted vmcnt(N) pipeline; loads through vector-typed pointers carry TBAA metadata
// and are left alone (checked in the ISA: scripts/check_dma_waits.sh).

__device__ __forceinline__ f32x16_t mfma32(bf16x8_t a, bf16x8_t b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// max of three: compiles to ONE v_max3_f32 when the file is built with -fno-honor-nans (touchnet_amd/build.py does
// that for the attention forward kernels; without the flag every MFMA output is canonicalised first: 2x the VALU
// work, still correct).  Deliberately NOT inline asm: hipcc's hazard recognizer does not look inside asm blocks, and
// a v_max3 that reads a just-issued MFMA's registers without the required wait states returns stale data —
// run-to-run 1-ulp differences in the D = 64 kernel were exactly that.
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ bf16x8_t as_bf16x8(uint4 v) {
  u32x4_t t = {v.x, v.y, v.z, v.w};
  return __builtin_bit_cast(bf16x8_t, t);
}
__device__ __forceinline__ bf16x8_t as_bf16x8(uint2 lo, uint2 hi) {
  u32x4_t t = {lo.x, lo.y, hi.x, hi.y};
  return __builtin_bit_cast(bf16x8_t, t);
}
// row index inside a 32x32 MFMA result tile held by register r of a lane with hi = lane >> 5
__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ---- Inline-asm pieces of the kernels that count their own waits: hipcc serialises compiler-visible reads of an LDS-DMA
// ring (above) and pairs every MFMA of a chain with its own read, so those kernels issue LDS reads as asm statements and
// retire them with hand-counted s_waitcnt statements that name the registers they release.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int OFF>
__device__ __forceinline__ u32x2_t ds_tr16(uint32_t addr) {
  u32x2_t r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
// (V: any 16-byte vector — the fused dK / dV pass reads float and int rows straight into the type it computes with)
template <int OFF, class V = u32x4_t>
__device__ __forceinline__ V ds_b128(uint32_t addr) {
  V r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant expression (asm
// immediates, register-array indices)
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

constexpr int kTile = 64;  // granularity of the document-range metadata

// Per-64-position tile metadata (all int32 [B, nt], nt = ceil(T/64)):
//   tmax    max document id in the tile (positions >= T count as 0)
//   tminpos min over the POSITIVE ids of the tile (INT_MAX if the tile is all pad)
//   tmin    min over all ids (0 if the tile contains pad)
//   q_lo    first kv tile j <= t that can interact with q tile t        (t + 1 if none)
//   kv_hi   last  q  tile t >= j that can interact with kv tile j       (j - 1 if none)
// Behind them (round 6), what a workgroup used to derive itself through dependent memory round trips at its start:
//   qstat [B, nq32, 4]   {min positive id, max id, 1 if a pad id occurs, 0} of every 32 positions (one wave's query rows)
//   klist [B, nq128, 4 + 4 * kListPre]   the KV tiles a 128-position CAUSAL query tile meets, all chunks:
//                        {count, query tile, 0, 0} then min(count, kListPre) entries {tile, min id, max id, min positive
//                        id}; count > kListPre: the kernel builds its list itself (long documents).
//                        (Records SORTED by count, heaviest workgroups first, were measured and dropped: the launch
//                        balances better — a scheduling model says 0.92 -> 0.97 of the CU slots busy — but neighbouring
//                        query tiles no longer run side by side, their shared K / V tiles fall out of the XCD's L2 and
//                        the wait for a tile grows by 40 %: 233 -> 242 us, profiles/r06a_*.)
//   qlist [B, nq128, 4 + 4 * kListPre]   the mirror image for the dK / dV pass: the 64-position QUERY tiles a 128-position
//                        KV tile meets under the causal mask, {count, kv tile, 0, 0} + entries {q tile, min id, max id,
//                        min positive id}
constexpr int kListPre = 64;
struct AttnMeta {
  const int* tmin;
  const int* tmax;
  const int* tminpos;
  const int* q_lo;
  const int* kv_hi;
  int nt;
  const int* qstat;
  const int* klist;
  int nq32, nq128;
  const int* qlist;
};
__host__ inline int attn_meta_ints(int B, int T) {
  const int nt = (T + kTile - 1) / kTile, nq32 = (T + 31) / 32, nq128 = (T + 127) / 128;
  return 5 * B * nt + 4 * B * nq32 + 2 * (4 + 4 * kListPre) * B * nq128;
}
__host__ inline AttnMeta make_attn_meta(const int* meta, int B, int T) {
  const int nt = (T + kTile - 1) / kTile, n = B * nt, nq32 = (T + 31) / 32, nq128 = (T + 127) / 128;
  return AttnMeta{meta, meta + n, meta + 2 * n, meta + 3 * n, meta + 4 * n, nt,
                  meta + 5 * n, meta + 5 * n + 4 * B * nq32, nq32, nq128,
                  meta + 5 * n + 4 * B * nq32 + (4 + 4 * kListPre) * B * nq128};
}

// Which rows of the (possibly sequence-sharded) query-side buffers a launch covers.  Q / O / dO / dQ are
// [B, rpb, Nh, D] and LSE / delta are [B, Nh, rpb]; segment s = local rows [row0, row0 + rows) holding GLOBAL
// positions [off, off + rows) of the packed row (K / V / doc ids / metadata are always global, [B, T, ...]).
// Plain attention: one segment {0, T, 0}, rpb = T.  Context parallel with head/tail load balancing
// (touchnet/utils/distributed.py:292-315 -> torch's round-robin CP sharding): two segments per rank.
// Segment offsets and all but the last segment's length must be multiples of 128; seg_view() below holds the whole
// contract of what the kernels can serve.
struct QView {
  int nseg;
  int row0[2], rows[2], off[2];
  int rpb;
  // optional restriction of the KEY side to a set of sequence chunks (context parallel: the forward runs once on the
  // rank's own chunks while the remote ones travel, once on the remote ones, and the two are merged by their LSE):
  // kv_tpc = 64-position tiles per chunk (0 = no restriction), bit c of kv_mask = chunk c takes part
  int kv_tpc;
  unsigned long long kv_mask;
  // 0 = causal inside a document (every decoder; Qwen2-Audio's tower), 1 = BIDIRECTIONAL inside a document (the Whisper
  // speech encoder of Kimi-Audio: transformers' WhisperEncoder has no causal mask,
  // touchnet/models/kimi_audio/modeling_kimi_audio.py:933-960): the key range of a query tile then runs to the LAST
  // tile that shares a document with it and the predicate loses its `kv <= q` term
  int bidir;
  // plain attention: the one segment is the whole row, every key chunk, causal
  __host__ static QView whole(int T) { return QView{1, {0, 0}, {T, 0}, {0, 0}, T, 0, ~0ull, 0}; }
  __device__ __forceinline__ bool kv_tile_on(int j) const { return kv_tpc == 0 || ((kv_mask >> (j / kv_tpc)) & 1ull); }
  __host__ __device__ int tiles(int s, int bm) const { return s < nseg ? (rows[s] + bm - 1) / bm : 0; }
  // tile `idx` of size bm over all segments -> local first row, global first position, rows left in segment
  __device__ __forceinline__ void tile(int idx, int bm, int& l0, int& g0, int& left) const {
    const int n0 = tiles(0, bm);
    const int s = idx >= n0 ? 1 : 0;
    const int lt = idx - (s ? n0 : 0);
    l0 = row0[s] + lt * bm;
    g0 = off[s] + lt * bm;
    left = rows[s] - lt * bm;
  }
};

// What every attention entry point asks of its shape: whole GQA groups, a head size the kernels are built for.
__host__ inline bool attn_shape_ok(int B, int T, int Nh, int Nkv, int D) {
  return B > 0 && T > 0 && Nh > 0 && Nkv > 0 && Nh % Nkv == 0 && (D == 64 || D == 128);
}

// The QView of a tn_attn_*_seg* call, or TN_EINVAL for a description the kernels cannot serve (the contract stated in
// include/touchnet_amd.h) — checked on the host, before any launch: the kernels index the local buffers with
// row0 + (rows of the segment) and K / V / the ids with off + (rows of the segment) and trust both.  `segs` = host
// int[3 * nseg] {row0, rows, off} per segment.  The segments may come in any order of their global positions.
__host__ inline int seg_view(int nseg, const int* segs, int rows_per_batch, int T, QView* out) {
  if (nseg < 1 || nseg > 2 || segs == nullptr || rows_per_batch <= 0 || T <= 0) return TN_EINVAL;
  QView qv = {nseg, {0, 0}, {0, 0}, {0, 0}, rows_per_batch, 0, ~0ull, 0};
  for (int s = 0; s < nseg; ++s) {
    const int row0 = segs[3 * s], rows = segs[3 * s + 1], off = segs[3 * s + 2];
    if (rows <= 0 || off < 0 || row0 < 0) return TN_EINVAL;
    if ((long long)off + rows > T || (long long)row0 + rows > rows_per_batch) return TN_EINVAL;
    // a 128-row tile of the kernels never straddles two segments, and its global position is a multiple of 128 (the
    // stored tile lists and the per-32-row statistics are indexed by it)
    if (off % 128 || row0 % 128 || (s + 1 < nseg && rows % 128)) return TN_EINVAL;
    qv.row0[s] = row0;
    qv.rows[s] = rows;
    qv.off[s] = off;
  }
  if (nseg == 2) {
    // disjoint local rows (two tiles would write the same O / dQ rows) and disjoint global positions (a query would be
    // counted twice in dK / dV)
    if (qv.row0[0] < qv.row0[1] + qv.rows[1] && qv.row0[1] < qv.row0[0] + qv.rows[0]) return TN_EINVAL;
    if (qv.off[0] < qv.off[1] + qv.rows[1] && qv.off[1] < qv.off[0] + qv.rows[0]) return TN_EINVAL;
  }
  *out = qv;
  return TN_OK;
}

// Workgroup -> (head, tile) mapping shared by the attention kernels.  Launch grids are (heads, tiles, batch):
//  * blockIdx.x = head slot.  Workgroups go to XCDs round-robin by linear id (MI355X_MICROARCH.md "Workgroup
//    dispatch"), so with the TILE index in x (the first version) XCD k received tiles {k, k+8, ..}: under a causal
//    mask XCD 7 had 21 % (256-row tiles) more work than the average and every XCD's L2 fetched the K/V of every
//    head.  With the head in x all tiles of a head run on ONE XCD: balanced work, K/V of a head read into one L2.
//    GQA: slot x -> head (x % Nkv) * G + x / Nkv, so that the G query heads of a kv head share its XCD(s).
//  * blockIdx.y = tile rank, heaviest first (q tiles: last rows first; kv tiles of dK/dV: first rows first), so
//    that the tail of the launch is made of the light workgroups.
__device__ __forceinline__ int head_of_slot(int x, int Nh, int Nkv) {
  const int G = Nh / Nkv;
  return (x % Nkv) * G + x / Nkv;
}

// Can any (q, kv) pair with q in a set having positive-id range [qminpos, qmax] and kv in tile j be
// allowed?  Conservative on purpose: false only when the id ranges are disjoint.
__device__ __forceinline__ bool tile_may_interact(int qminpos, int qmax, int kminpos, int kmax) {
  return !(qminpos == 0x7fffffff || kminpos == 0x7fffffff || kmax < qminpos || kminpos > qmax);
}

// a list entry as four scalars (4 readfirstlane)
__device__ __forceinline__ int4 scalarize(i32x4_t e) {
  return make_int4(__builtin_amdgcn_readfirstlane(e.x), __builtin_amdgcn_readfirstlane(e.y),
                   __builtin_amdgcn_readfirstlane(e.z), __builtin_amdgcn_readfirstlane(e.w));
}
__device__ __forceinline__ int4 scalarize(int4 e) {
  return make_int4(__builtin_amdgcn_readfirstlane(e.x), __builtin_amdgcn_readfirstlane(e.y),
                   __builtin_amdgcn_readfirstlane(e.z), __builtin_amdgcn_readfirstlane(e.w));
}

// v_permlane32_swap: {a with its upper half replaced by b's lower half, b with its lower half replaced by a's upper half}
__device__ __forceinline__ u32x2_t swap32(uint32_t a, uint32_t b) {
  const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  return u32x2_t{r[0], r[1]};
}
// sum / max over the two 32-lane halves of a wave without an LDS round trip (ds_bpermute queues behind other waves'
// operand reads)
__device__ __forceinline__ float half_sum(float x) {
  const u32x2_t r = swap32(__float_as_uint(x), __float_as_uint(x));
  return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float half_max(float x) {
  const u32x2_t r = swap32(__float_as_uint(x), __float_as_uint(x));
  return fmaxf(__uint_as_float(r.x), __uint_as_float(r.y));
}
// half_max as inline asm, for attn_fwd_pp.hip alone: with the builtin its assembly changes (the pads around the swap go and
// the registers of the tile loop are renumbered), so the kernel keeps the form it was measured with.
__device__ __forceinline__ float half_swap_max(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}

// Positive-id range of a wave's 32 rows (both 32-lane halves hold the same rows), returned in SGPRs so that
// every tile decision derived from it is a scalar branch and not an exec-mask region.
__device__ __forceinline__ void wave_id_range(int id, int& minpos, int& mx) {
  int a = id > 0 ? id : 0x7fffffff, b = id;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    a = min(a, __shfl_xor(a, o, 64));
    b = max(b, __shfl_xor(b, o, 64));
  }
  minpos = __builtin_amdgcn_readfirstlane(a);
  mx = __builtin_amdgcn_readfirstlane(b);
}

// A wave-uniform predicate as a real scalar (SGPR) bool: `if (uniform(c))` compiles to s_cbranch_scc and both
// arms stay free of exec-mask bookkeeping.  (hipcc otherwise turns a mask-typed bool that it cannot prove
// uniform into one s_and_saveexec region PER ELEMENT of the unrolled softmax loops.)
__device__ __forceinline__ bool uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

// ---- Panel image: ONE LDS copy of an [R rows][D] bf16 tile that serves both MFMA operand shapes ------------------
// The tile is cut into D/32 column panels of [R][32] (64-byte rows, panel stride R*64 + 64 bytes); inside a row the
// four 16-byte chunks are permuted by XOR with (row >> 2) & 3:
//   element (r, d) lives at  (d >> 5) * PSTRIDE + r * 32 + 8 * (((d >> 3) & 3) ^ ((r >> 2) & 3)) + (d & 7)
// * "row" operand (lane = tile row, 8 consecutive d per contraction slot group): one ds_read_b128; the 16 lanes of a
//   b128 service group hold 16 distinct (r & 15) -> 16 distinct 16-byte slots of the 256-byte bank row;
// * "transposed" operand (lane = d, contraction slots = tile rows): two ds_read_b64_tr_b16 (gfx950 transpose read: the
//   16 lanes of a group each point at 4 consecutive d of one row, rows 4 apart in groups of 4; lane i of the group
//   receives column i of the [4 rows][16 d] block — measured with scripts/microbench/tr_read_probe.hip).  The 32 lanes
//   of a service group cover 4 consecutive rows x 64 bytes = one contiguous 256-byte bank row: conflict free;
// * fill: 16-byte stores; 8 consecutive lanes write chunks 8p..8p+7 of one row = two neighbouring panels, whose
//   addresses differ by 64 bytes mod 128: conflict free for ds_write_b128's 8-lane groups.
// Replaces the row-major + transposed image pairs (the transposed ones were written with 8-byte transposing stores:
// 16 v_perm per 4x8 unit and 24-36 % LDS bank-conflict cycles, profiles/r02_attention_pmc_final.md).
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

template <int R, int D>
struct PTile {
  static constexpr int NP = D / 32, PSTRIDE = R * 32 + 32, SIZE = NP * PSTRIDE;   // elements
  static __device__ __forceinline__ int chunk_off(int r, int c) {                  // c = d >> 3
    return (c >> 2) * PSTRIDE + r * 32 + 8 * ((c & 3) ^ ((r >> 2) & 3));
  }
};

// "row" operand reads: zero address VALU inside the tile loops (lane part: two VGPRs; the rest is a compile-time offset)
template <int R, int D>
struct PRowReader {
  int a[2];
  __device__ __forceinline__ PRowReader(int l31, int hi) {
    const int x = (l31 >> 2) & 3;
    a[0] = l31 * 32 + 8 * (hi ^ x);
    a[1] = l31 * 32 + 8 * ((2 + hi) ^ x);
  }
  // contraction slots d = 16 * s + 8 * hi + (0..7) of row rb + l31 (rb a multiple of 16)
  __device__ __forceinline__ bf16x8_t operand(const bf16_t* img, int rb, int s) const {
    return __builtin_bit_cast(
        bf16x8_t, *reinterpret_cast<const u32x4_t*>(img + (s >> 1) * PTile<R, D>::PSTRIDE + rb * 32 + a[s & 1]));
  }
};

// "transposed" operand reads: lane = d (32 * db + (lane & 31)), slots (hi, i) = rows kb + 8 * (i >> 2) + 4 * hi + (i & 3)
// (kb a multiple of 16) — exactly the rows a lane of a 32x32 MFMA result holds in registers 8 * sp .. 8 * sp + 7.
template <int R, int D>
struct PTrReader {
  int t[2];
  __device__ __forceinline__ PTrReader(int lane) {
    const int s4 = lane & 15, half = (lane >> 4) & 1, hi = lane >> 5;
    const int j = s4 >> 2, q = 2 * half + ((s4 & 3) >> 1);
    t[0] = (4 * hi + j) * 32 + 8 * (q ^ hi) + 4 * (s4 & 1);
    t[1] = (4 * hi + j) * 32 + 8 * ((q ^ hi) ^ 2) + 4 * (s4 & 1);
  }
  static __device__ __forceinline__ s16x4_t tr(const bf16_t* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
  }
  __device__ __forceinline__ bf16x8_t operand(const bf16_t* img, int db, int kb) const {
    const bf16_t* base = img + db * PTile<R, D>::PSTRIDE + kb * 32;
    const s16x4_t lo = tr(base + t[(kb >> 3) & 1]);
    const s16x4_t up = tr(base + 8 * 32 + t[((kb >> 3) & 1) ^ 1]);
    return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, up, 0, 1, 2, 3, 4, 5, 6, 7));
  }
};

// (With LDS-DMA in flight hipcc puts `s_waitcnt vmcnt(0)` in front of the transpose-read builtin as well — the builtin
// carries no alias metadata.  At the prefetch distance the dK/dV kernel can afford, one stage, that wait costs nothing;
// an inline-asm read with hand-placed lgkmcnt waits removes it and measured 1-5 % slower, so the builtin stays.)

// Wave-uniform buffer descriptor over the first `rows_valid` rows of a [rows][ld] bf16 tile starting at
// `base`: loads past the last valid row return 0 in hardware (no exec-mask branches around tile edges).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const bf16_t* base, size_t ld, int rows_valid, int D) {
  const uint64_t p = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
  const uint32_t bytes = rows_valid > 0 ? (uint32_t)(((size_t)(rows_valid - 1) * ld + D) * 2) : 0u;
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0,
                                           __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
// Batch row b of a [B][rows][row_elems] bf16 tensor (K / V: rows = T, row_elems = Nkv D; Q / dO: rows = rpb, row_elems =
// Nh D) as an LDS-DMA source: rsrc(X) = the descriptor over X's slice.  An offset at or past the slice's bytes (capped at
// 2^31 - 1) reads zeros and touches no memory.  (Constructor arguments by reference: taken by value hipcc groups the byte
// count's product differently and the stream kernels' assembly changes.  In the two dK / dV kernels this form does so too:
// attn_bwd.hip and attn_bwd_fused.hip write the same arithmetic out.)
struct BatchRows {
  int b, rows;
  size_t row_elems;
  uint32_t bytes;
  __device__ __forceinline__ BatchRows(const int& b_, const int& rows_, const size_t& row_elems_)
      : b(b_), rows(rows_), row_elems(row_elems_),
        bytes((uint32_t)min((size_t)rows_ * row_elems_ * 2, (size_t)0x7fffffff)) {}
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const bf16_t* base) const {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (size_t)b * rows * row_elems), 0, bytes, 0x00020000);
  }
};
__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// The TRANSPOSED rotary rotation — what tn_rope_apply(backward = 1) applies to the gradient of a rotated q / k row — of one
// 16-byte chunk of a gradient row in a backward kernel's epilogue: `own` = the lane's 8 columns, `other` = the same 8
// columns of the row's other half, c4 / s4 = the 8 table entries of the row (bf16 [rows, D / 2] tables of tn_rope_table),
// upper = the lane's columns are >= D / 2.  rope_rotate itself on the bf16-rounded values: the bits the row kernel produces.
__device__ __forceinline__ u32x4_t rope_grad_chunk(u32x4_t own, u32x4_t other, u32x4_t c4, u32x4_t s4, bool upper) {
  // rope_rotate(a, b, c, -sin): lower half ya = fma(-b, -sin, a c) = fma(other, sin, own c); upper half yb = fma(a, -sin, b c)
  // = fma(other, -sin, own c) — sign flips of a factor are exact, so ONE form with the table's sign bits flipped for the upper
  // lanes gives the row kernel's bits at a third of its instructions (an epilogue's VALU time is exposed: 1-2 waves per SIMD)
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  const uint32_t flip = upper ? 0x80008000u : 0u;
  u32x4_t out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t sj = s4[j] ^ flip;
    const f32x2 x = {__uint_as_float(own[j] << 16), __uint_as_float(own[j] & 0xffff0000u)};
    const f32x2 y = {__uint_as_float(other[j] << 16), __uint_as_float(other[j] & 0xffff0000u)};
    const f32x2 c = {__uint_as_float(c4[j] << 16), __uint_as_float(c4[j] & 0xffff0000u)};
    const f32x2 sv = {__uint_as_float(sj << 16), __uint_as_float(sj & 0xffff0000u)};
    const f32x2 t = x * c;
    const f32x2 r = __builtin_elementwise_fma(y, sv, t);
    out[j] = pack2bf(r.x, r.y);
  }
  return out;
}

// ---- Whole-row store: how a wave's 32 x D accumulator block (MFMA result layout: lane = row l31, 8-byte runs of columns)
// leaves as whole rows.  The wave writes the block into a private staging image (32 rows at stride OSTR: conflict-free
// 8-byte stores) and reads it back as 16-byte chunks — 16-byte stores, RPI rows per instruction, instead of 8 bytes per
// lane at a row stride (store-issue bound: MI355X_MICROARCH.md "attention epilogue store tail").  The layout has this one
// definition; the two loops around it stay in each kernel's epilogue: as a shared function, whatever way its arguments
// are handed over, hipcc pairs the staging stores and schedules the scaling differently, and the assembly changes.
template <int D>
struct WholeRows {
  static constexpr int OSTR = 2 * D + 16;              // row stride (bytes) of the staging image
  static constexpr int BYTES = 32 * OSTR;              // ... and its size
  static constexpr int CPR = D / 8, RPI = 64 / CPR;    // 16-byte chunks per row, rows per store instruction
  static constexpr int NI = 32 / RPI;                  // store instructions per block
  // where registers 4 r4 .. 4 r4 + 3 of accumulator block db (an 8-byte run of row l31) go in the image at ob
  static __device__ __forceinline__ u32x2_t* put(char* ob, int l31, int hi, int db, int r4) {
    return reinterpret_cast<u32x2_t*>(ob + l31 * OSTR + (32 * db + 8 * r4 + 4 * hi) * 2);
  }
  // ... and of 16-byte chunk cc of row `row`: lane L takes chunk L % CPR of row i RPI + L / CPR in store instruction i
  static __device__ __forceinline__ const u32x4_t* get(const char* ob, int row, int cc) {
    return reinterpret_cast<const u32x4_t*>(ob + row * OSTR + cc * 16);
  }
};

}  // namespace tn
