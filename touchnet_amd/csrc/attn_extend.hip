// Extend attention (gfx950): several NEW rows per sequence attend to keys that are already in a KV cache and, causally, to
// each other — the shape between the packed forward (recomputes everything) and tn_attn_decode (one new row per cache
// row).  Rescoring N-best lists behind cached prompts, a second chat turn behind a cached conversation, chunked prefill.
//
//   q      bf16 [T, Nh, D]          rotated queries of the new rows of R sequences, packed one after another
//   k_new, v_new bf16 [T, Nkv, D]   their rotated keys / values
//   seq_start int32 [R + 1]         ascending, seq_start[0] = 0, seq_start[R] = T; n_r = seq_start[r + 1] - seq_start[r]
//   k_cache, v_cache bf16 [B, S_max, Nkv, D]   read only
//   prefix_len int32 [R], kv_row int32 [R] or null (row r)
//   o      bf16 [T, Nh, D]
//
// New row i of sequence r sits at position prefix_len[r] + i and sees cache[kv_row[r], 0 .. prefix_len[r]) and the new rows
// j <= i of its own sequence; nothing else.  Sequences may share a kv_row.  The kernel writes o alone and never reads a
// cache slot at or past prefix_len[r]; a prefix_len outside [0, S_max] or a kv_row outside [0, B) poisons the sequence's
// rows with NaN without consulting the cache.
//
// Work split: one workgroup of four waves per (sequence, tile of 16 new positions, kv head); the G query heads of the group
// are dealt to the waves (head g -> wave g & 3, at most four per wave), so ONE pass over the keys serves the whole group.
// Workgroups are numbered heaviest tile first inside a sequence.  The key stream of a tile is virtual: index j < P is
// cache[kv_row, j], index j >= P is k_new[seq_start + j - P], up to the tile's last row; rows past its end are zero.  It
// moves in 64-key stages: while stage s is computed from LDS, stage s + 1 is in flight from global memory into registers.
// A stage is stored ONCE, in attn_common.h's panel image, for K and for V: K is read as the 16-row operand (ds_read_b128),
// V as the transposed operand (ds_read_b64_tr_b16), so there is no second, transposed copy of V.
//
// MFMA: v_mfma_f32_16x16x32_bf16.  S^T = K Q^T — lane l holds query position l & 15 and, of key block kb, keys
// 16 kb + 4 (l >> 4) + r in register r — then O^T += V^T P^T with the contraction slot (l >> 4, e) of step c standing for
// key 32 c + 16 (e >> 2) + 4 (l >> 4) + (e & 3): exactly the registers the lane already holds, so P goes from the softmax
// into the next MFMA without leaving the lane.  A wave reads every K / V operand once per stage and uses it for all its
// heads.  Online softmax in fp32, log2 domain (scale * log2(e)), one rescale per stage, P rounded to bf16, row sums from the
// unrounded P: the packed forward's arithmetic.  Only stages that hold a key beyond the tile's first position take the
// mask (one compare per score); whole prefix stages run unmasked.  No atomics, no cross-workgroup reduction.
//
// FP8 (tn_attn_extend_fp8; KV = kvq::fp8_t): the cache AND the new rows arrive as e4m3 codes uint8 with one fp32
// power-of-two scale per key (kv_fp8.h; the caller quantises k_new / v_new once with tn_kv_quantize), so the per-chunk
// choice between cache, new rows and zero stays a choice between like sources.  A thread's chunk of a stage is 8 bytes of
// codes and the key's scale instead of 16 bytes: half the global bytes are in flight in registers (12 instead of 16
// registers per stage at D = 64, 24 instead of 32 at D = 128; the freed registers are left free).  The chunk is expanded
// to bf16 — exactly — on its way into the SAME panel image; from the image on this is the bf16 kernel: lane layout,
// head sharing, masks, one rescale per stage.
#include <type_traits>

#include "attn_common.h"
#include "kv_fp8.h"

namespace tn {
namespace extend {

constexpr int kThreads = 256;
constexpr int kRows = 16;      // new positions per workgroup
constexpr int kStage = 64;     // keys per stage

__device__ __forceinline__ f32x4_t mfma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

struct NoScales {};                  // the bf16 kernel's scales: an empty argument, so its code is what it was
struct Scales {                      // fp32, one per key: new rows [T, Nkv], caches [B, S_max, Nkv]
  const float* __restrict__ k_new;
  const float* __restrict__ v_new;
  const float* __restrict__ k_cache;
  const float* __restrict__ v_cache;
};

template <int D, int HPW, typename KV = bf16_t>
__global__ void __launch_bounds__(kThreads) attn_extend_kernel(
    const bf16_t* __restrict__ q, const KV* __restrict__ k_new, const KV* __restrict__ v_new,
    const KV* __restrict__ k_cache, const KV* __restrict__ v_cache, const int* __restrict__ seq_start,
    const int* __restrict__ prefix_len, const int* __restrict__ kv_row, bf16_t* __restrict__ o, int T, int R, int B,
    int S_max, int Nh, int Nkv, float scale_log2, std::conditional_t<std::is_same_v<KV, bf16_t>, NoScales, Scales> sc) {
  constexpr bool FP8 = !std::is_same_v<KV, bf16_t>;
  using Raw = std::conditional_t<FP8, uint2, u32x4_t>;     // a 8-element chunk of a key as it is loaded
  using PT = PTile<kStage, D>;
  constexpr int CPR = D / 8;                          // 16-byte chunks per key row
  constexpr int NLD = kStage * CPR / kThreads;        // chunks of K (and of V) per thread and stage
  constexpr int NS = D / 32, NDB = D / 16;            // contraction steps of S, 16-column blocks of O
  __shared__ __attribute__((aligned(16))) bf16_t ks[PT::SIZE];
  __shared__ __attribute__((aligned(16))) bf16_t vs[PT::SIZE];

  const int tid = threadIdx.x, lane = tid & 63, s4 = lane & 15, g4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kvh = blockIdx.y, G = Nh / Nkv;

  // ---- workgroup -> (sequence, tile): tiles are counted sequence by sequence, the last (heaviest) tile first.  The
  //      launch has at least as many workgroups as there are tiles; the rest leave here.
  int w = blockIdx.x, r = 0, n = 0, s0 = 0;
  for (; r < R; ++r) {
    s0 = seq_start[r];
    n = s0 >= 0 ? min(seq_start[r + 1], T) - s0 : 0;  // (a malformed table can shorten a sequence, never leave q / o)
    const int nt = n > 0 ? (n + kRows - 1) / kRows : 0;
    if (w < nt) {
      w = nt - 1 - w;
      break;
    }
    w -= nt;
  }
  if (r == R) return;
  const int i0 = w * kRows, rows = min(kRows, n - i0);
  const int P = prefix_len[r], cr = kv_row != nullptr ? kv_row[r] : r;
  const size_t orow = ((size_t)(s0 + i0) * Nh + (size_t)kvh * G) * D;       // the group's heads are contiguous in a row of o
  if (P < 0 || P > S_max || cr < 0 || cr >= B) {
    // poisoned sequence: no cache slot is consulted
    const int per_row = G * D;
    for (int i = tid; i < rows * per_row; i += kThreads)
      o[orow + (size_t)(i / per_row) * Nh * D + i % per_row] = 0x7fc0;      // bf16 quiet NaN
    return;
  }
  const int L = P + i0 + rows;                        // keys of the tile's stream
  const int nst = (L + kStage - 1) / kStage;
  const size_t kv_ld = (size_t)Nkv * D;
  const KV* kc = k_cache + (size_t)cr * S_max * kv_ld + (size_t)kvh * D;
  const KV* vc = v_cache + (size_t)cr * S_max * kv_ld + (size_t)kvh * D;
  const KV* kn = k_new + (size_t)s0 * kv_ld + (size_t)kvh * D;
  const KV* vn = v_new + (size_t)s0 * kv_ld + (size_t)kvh * D;
  [[maybe_unused]] const float *kcs = nullptr, *vcs = nullptr, *kns = nullptr, *vns = nullptr;     // scales of key 0
  if constexpr (FP8) {
    kcs = sc.k_cache + (size_t)cr * S_max * Nkv + kvh;
    vcs = sc.v_cache + (size_t)cr * S_max * Nkv + kvh;
    kns = sc.k_new + (size_t)s0 * Nkv + kvh;
    vns = sc.v_new + (size_t)s0 * Nkv + kvh;
  }

  // ---- Q fragments of the wave's heads: lane = position s4, slots (g4, e) = d 32 s + 8 g4 + e
  bool on[HPW];
  bf16x8_t qf[HPW][NS];
#pragma unroll
  for (int hh = 0; hh < HPW; ++hh) {
    on[hh] = hh * 4 + wave < G;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      u32x4_t t = {0u, 0u, 0u, 0u};
      if (on[hh] && s4 < rows)
        t = *reinterpret_cast<const u32x4_t*>(q + orow + ((size_t)s4 * Nh + hh * 4 + wave) * D + 32 * s + 8 * g4);
      qf[hh][s] = __builtin_bit_cast(bf16x8_t, t);
    }
  }
  f32x4_t acc[HPW][NDB];
  float m[HPW], l[HPW];
#pragma unroll
  for (int hh = 0; hh < HPW; ++hh) {
    m[hh] = -INFINITY;
    l[hh] = 0.f;
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[hh][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // ---- lane parts of the LDS addresses (elements).  K: row 16 kb + s4, chunk 4 s + g4.  V (transpose read): the lane
  //      points at 4 consecutive d of row 4 g4 + (s4 >> 2) and receives column s4 of its 16-lane group's [4 rows][16 d]
  //      block, i.e. d = 16 db + s4 of rows base + 4 g4 + 0..3.
  const int ka = s4 * 32 + 8 * (g4 ^ ((s4 >> 2) & 3));
  int va[2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
    va[p] = (4 * g4 + (s4 >> 2)) * 32 + 8 * ((2 * p + ((s4 & 3) >> 1)) ^ g4) + 4 * (s4 & 1);

  Raw kr[NLD], vr[NLD];
  [[maybe_unused]] float ksc[NLD], vsc[NLD];          // FP8: the scale of each chunk's key (0 for a zero row)
  auto fetch = [&](int st) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + kThreads * i, row = idx / CPR, c = idx % CPR;
      const int j = st * kStage + row;
      kr[i] = Raw{};
      vr[i] = Raw{};
      if constexpr (FP8) ksc[i] = vsc[i] = 0.f;
      if (j < P) {
        kr[i] = *reinterpret_cast<const Raw*>(kc + (size_t)j * kv_ld + c * 8);
        vr[i] = *reinterpret_cast<const Raw*>(vc + (size_t)j * kv_ld + c * 8);
        if constexpr (FP8) {
          ksc[i] = kcs[(size_t)j * Nkv];
          vsc[i] = vcs[(size_t)j * Nkv];
        }
      } else if (j < L) {
        kr[i] = *reinterpret_cast<const Raw*>(kn + (size_t)(j - P) * kv_ld + c * 8);
        vr[i] = *reinterpret_cast<const Raw*>(vn + (size_t)(j - P) * kv_ld + c * 8);
        if constexpr (FP8) {
          ksc[i] = kns[(size_t)(j - P) * Nkv];
          vsc[i] = vns[(size_t)(j - P) * Nkv];
        }
      }
    }
  };
  // a chunk as the 8 bf16 of the panel image
  auto image = [](const Raw& r, [[maybe_unused]] float s) -> u32x4_t {
    if constexpr (FP8) {
      const uint4 t = kvq::decode8_bf16(r, s);
      return u32x4_t{t.x, t.y, t.z, t.w};
    } else {
      return r;
    }
  };

  fetch(0);
  for (int st = 0; st < nst; ++st) {
    __syncthreads();                                  // every wave is done with the previous stage's image
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + kThreads * i, off = PT::chunk_off(idx / CPR, idx % CPR);
      if constexpr (FP8) {
        *reinterpret_cast<u32x4_t*>(ks + off) = image(kr[i], ksc[i]);
        *reinterpret_cast<u32x4_t*>(vs + off) = image(vr[i], vsc[i]);
      } else {
        *reinterpret_cast<u32x4_t*>(ks + off) = kr[i];
        *reinterpret_cast<u32x4_t*>(vs + off) = vr[i];
      }
    }
    __syncthreads();
    if (st + 1 < nst) fetch(st + 1);                  // in flight while this stage is computed

    // ---- S^T = K Q^T for all heads of the wave: one read of every K operand
    f32x4_t sc[HPW][4];
#pragma unroll
    for (int hh = 0; hh < HPW; ++hh)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) sc[hh][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const bf16x8_t a =
            __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(ks + s * PT::PSTRIDE + kb * 16 * 32 + ka));
#pragma unroll
        for (int hh = 0; hh < HPW; ++hh)
          if (on[hh]) sc[hh][kb] = mfma16(a, qf[hh][s], sc[hh][kb]);
      }

    // ---- mask (stages that hold a key beyond the tile's first position), online softmax in the log2 domain
    const bool masked = st * kStage + kStage - 1 > P + i0;
    const int lim = P + i0 + s4 - st * kStage;        // last visible key of this lane's row, stage-local
    bf16x8_t pb[HPW][2];
#pragma unroll
    for (int hh = 0; hh < HPW; ++hh) {
      if (!on[hh]) continue;
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = sc[hh][kb][e] * scale_log2;
          if (masked) v = kb * 16 + 4 * g4 + e <= lim ? v : -INFINITY;
          sc[hh][kb][e] = v;
          mx = fmaxf(mx, v);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m[hh], mx);           // finite from stage 0 on: every row sees key 0
      const float alpha = fast_exp2(m[hh] - m_new);
      float ps = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = fast_exp2(sc[hh][kb][e] - m_new);
          sc[hh][kb][e] = p;
          ps += p;
        }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l[hh] = l[hh] * alpha + ps;
      m[hh] = m_new;
#pragma unroll
      for (int db = 0; db < NDB; ++db) acc[hh][db] *= alpha;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const u32x4_t t = {pack2bf(sc[hh][2 * c][0], sc[hh][2 * c][1]), pack2bf(sc[hh][2 * c][2], sc[hh][2 * c][3]),
                           pack2bf(sc[hh][2 * c + 1][0], sc[hh][2 * c + 1][1]),
                           pack2bf(sc[hh][2 * c + 1][2], sc[hh][2 * c + 1][3])};
        pb[hh][c] = __builtin_bit_cast(bf16x8_t, t);
      }
    }

    // ---- O^T += V^T P^T: one transposed read of every V operand
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bf16_t* base = vs + (db >> 1) * PT::PSTRIDE + 32 * c * 32 + va[db & 1];
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)base);
        const s16x4_t up =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base + 16 * 32));
        const bf16x8_t a = __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, up, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
        for (int hh = 0; hh < HPW; ++hh)
          if (on[hh]) acc[hh][db] = mfma16(a, pb[hh][c], acc[hh][db]);
      }
  }

  // ---- epilogue: register e of acc[hh][db] is O[s4][16 db + 4 g4 + e]: one 8-byte store per block
  if (s4 >= rows) return;
#pragma unroll
  for (int hh = 0; hh < HPW; ++hh) {
    if (!on[hh]) continue;
    const float inv = 1.f / l[hh];
    bf16_t* dst = o + orow + ((size_t)s4 * Nh + hh * 4 + wave) * D + 4 * g4;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
      *reinterpret_cast<u32x2_t*>(dst + 16 * db) =
          u32x2_t{pack2bf(acc[hh][db][0] * inv, acc[hh][db][1] * inv), pack2bf(acc[hh][db][2] * inv, acc[hh][db][3] * inv)};
  }
}

template <int D, int HPW, typename KV>
static int launch(const void* q, const void* k_new, const void* v_new, const void* k_cache, const void* v_cache,
                  const float* const* scales, const int* seq_start, const int* prefix_len, const int* kv_row, void* o,
                  int T, int R, int B, int S_max, int Nh, int Nkv, float scale, hipStream_t st) {
  // sum_r ceil(n_r / 16) <= (T + 15 R) / 16: the host does not read seq_start
  const long long tiles = ((long long)T + 15ll * R) / kRows;
  std::conditional_t<std::is_same_v<KV, bf16_t>, NoScales, Scales> sc{};
  if constexpr (!std::is_same_v<KV, bf16_t>) sc = Scales{scales[0], scales[1], scales[2], scales[3]};
  hipLaunchKernelGGL((attn_extend_kernel<D, HPW, KV>), dim3((unsigned)tiles, Nkv), dim3(kThreads), 0, st, (const bf16_t*)q,
                     (const KV*)k_new, (const KV*)v_new, (const KV*)k_cache, (const KV*)v_cache, seq_start, prefix_len,
                     kv_row, (bf16_t*)o, T, R, B, S_max, Nh, Nkv, scale * kLog2e, sc);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

static inline bool al(const void* p, uintptr_t a) { return p != nullptr && ((uintptr_t)p & (a - 1)) == 0; }

// scales: null for the bf16 kernel, else {k_new, v_new, k_cache, v_cache} scales and k / v hold codes
static int entry(const void* q, const void* k_new, const void* v_new, const void* k_cache, const void* v_cache,
                 const float* const* scales, const int* seq_start, const int* prefix_len, const int* kv_row, void* o, int T,
                 int R, int B, int S_max, int Nh, int Nkv, int D, float scale, void* stream) {
  if (T < 0 || R < 0 || B <= 0 || S_max <= 0 || Nh <= 0 || Nkv <= 0 || (D != 64 && D != 128) || Nh % Nkv || Nh / Nkv > 16)
    return TN_EINVAL;
  if (kv_row == nullptr && R > B) return TN_EINVAL;
  if (Nkv > 65535 || ((long long)T + 15ll * R) / kRows > 0x7fffffffll) return TN_EINVAL;
  if (T == 0) return TN_OK;
  if (R == 0) return TN_EINVAL;                       // rows that belong to no sequence
  if (!al(q, 16) || !al(k_new, 16) || !al(v_new, 16) || !al(k_cache, 16) || !al(v_cache, 16) || !al(o, 16) ||
      !al(seq_start, 4) || !al(prefix_len, 4) || (kv_row != nullptr && !al(kv_row, 4)))
    return TN_EINVAL;
  if (scales != nullptr && (!al(scales[0], 4) || !al(scales[1], 4) || !al(scales[2], 4) || !al(scales[3], 4)))
    return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int hpw = (Nh / Nkv + 3) / 4;
#define TN_EXTEND(d, h)                                                                                                   \
  if (D == d && hpw == h)                                                                                                 \
    return scales != nullptr                                                                                              \
               ? launch<d, h, kvq::fp8_t>(q, k_new, v_new, k_cache, v_cache, scales, seq_start, prefix_len, kv_row, o, T, \
                                          R, B, S_max, Nh, Nkv, scale, st)                                                \
               : launch<d, h, bf16_t>(q, k_new, v_new, k_cache, v_cache, scales, seq_start, prefix_len, kv_row, o, T, R,  \
                                      B, S_max, Nh, Nkv, scale, st);
  TN_EXTEND(64, 1) TN_EXTEND(64, 2) TN_EXTEND(64, 3) TN_EXTEND(64, 4)
  TN_EXTEND(128, 1) TN_EXTEND(128, 2) TN_EXTEND(128, 3) TN_EXTEND(128, 4)
#undef TN_EXTEND
  return TN_EINVAL;
}

}  // namespace extend
}  // namespace tn

extern "C" int tn_attn_extend(const void* q, const void* k_new, const void* v_new, const void* k_cache, const void* v_cache,
                              const int* seq_start, const int* prefix_len, const int* kv_row, void* o, int T, int R, int B,
                              int S_max, int Nh, int Nkv, int D, float scale, void* stream) {
  return tn::extend::entry(q, k_new, v_new, k_cache, v_cache, nullptr, seq_start, prefix_len, kv_row, o, T, R, B, S_max, Nh,
                           Nkv, D, scale, stream);
}

// tn_attn_extend on FP8 keys / values: k_new / v_new uint8 codes [T, Nkv, D] with k_new_scale / v_new_scale fp32 [T, Nkv],
// k_cache / v_cache uint8 codes [B, S_max, Nkv, D] with k_scale / v_scale fp32 [B, S_max, Nkv]
extern "C" int tn_attn_extend_fp8(const void* q, const void* k_new, const void* v_new, const float* k_new_scale,
                                  const float* v_new_scale, const void* k_cache, const void* v_cache, const float* k_scale,
                                  const float* v_scale, const int* seq_start, const int* prefix_len, const int* kv_row,
                                  void* o, int T, int R, int B, int S_max, int Nh, int Nkv, int D, float scale,
                                  void* stream) {
  const float* scales[4] = {k_new_scale, v_new_scale, k_scale, v_scale};
  return tn::extend::entry(q, k_new, v_new, k_cache, v_cache, scales, seq_start, prefix_len, kv_row, o, T, R, B, S_max, Nh,
                           Nkv, D, scale, stream);
}
