// Block-causal self-attention forward of the Kimi-Audio / GLM-4-voice speech tokenizer (WhisperVQEncoder,
// touchnet/models/kimi_audio/modeling_kimi_audio.py:226-242 builds the mask, :293-301 applies it in every layer):
//     allowed(i, j) = m[j] && (j <= i || j / block == i / block)  ==  m[j] && j / block <= i / block
// with m[j] = "post-conv frame j of the clip is valid".  Padded query rows are ordinary rows: they see every valid key
// of their block range.  The tokenizer is frozen: forward only, no LSE.
//
// Layout: q / k / v / o bf16 [B, T, Nh, 64] (Nh == Nkv, D = 64 = whisper-large-v3's 1280 / 20).  A batch row may hold
// several clips back to back (the packed, per-clip trimmed schedule) or one clip (the padded schedule).  Position t of
// row b belongs to the clip that starts at seg_start[b, t] (row-local) and whose valid keys end at key_end[b, t]
// (exclusive); the valid keys of a clip are a prefix of it.  Then, with s = seg_start, query i attends to exactly
//     keys [s, min(key_end, s + ((i - s) / block + 1) * block))
// — an interval per row.  A row with an empty interval writes 0.
//
// One workgroup = 4 waves = 128 query rows of one (b, head).  The key range of the workgroup is the union of its rows'
// intervals; keys run through LDS in tiles of 64 (K as is, V transposed), each wave holds its 32 rows' S^T = K Q^T
// (lane = query row, 32 keys per lane across the two 32x32 MFMA results) so the row max / sum need one cross-half
// shuffle, and O^T = V^T P^T accumulates in fp32 with the online-softmax rescale (exp2 domain).
#include <limits.h>

#include "attn_common.h"

namespace tn {

constexpr int kBcRows = 128, kBcKeys = 64, kBcD = 64, kBcPad = 8;

__global__ __launch_bounds__(256) void attn_block_causal_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                                    const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
                                                                    const int* __restrict__ seg_start,
                                                                    const int* __restrict__ key_end, int T, int Nh, int block,
                                                                    float scale_log2) {
  constexpr int D = kBcD;
  __shared__ __attribute__((aligned(16))) bf16_t ks[kBcKeys][D + kBcPad];
  __shared__ __attribute__((aligned(16))) bf16_t vt[D][kBcKeys + kBcPad];
  __shared__ int red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, col = lane & 31;
  const int b = blockIdx.z, h = blockIdx.y;
  const size_t rs = (size_t)Nh * D;                                 // elements between consecutive positions
  const size_t base = (size_t)b * T * rs + (size_t)h * D;
  const int qi = blockIdx.x * kBcRows + wave * 32 + col;           // this lane's query row (both halves of the wave)
  const bool qok = qi < T;

  // ---- this row's key interval [lo, kend)
  int lo = INT_MAX, kend = 0;
  if (qok) {
    const int s = seg_start[(size_t)b * T + qi], e = key_end[(size_t)b * T + qi];
    const long long bend = (long long)s + ((long long)(qi - s) / block + 1) * block;
    const int hk = (int)(bend < (long long)e ? bend : (long long)e);
    if (hk > s) {
      lo = s;
      kend = hk;
    }
  }
  int wlo = lo, whi = kend;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    wlo = min(wlo, __shfl_xor(wlo, off, 64));
    whi = max(whi, __shfl_xor(whi, off, 64));
  }
  if (lane == 0) {
    red[0][wave] = wlo;
    red[1][wave] = whi;
  }
  __syncthreads();
  const int tlo = max(0, min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3])));
  const int thi = min(T, max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));

  // ---- Q as the B operand of S^T = K Q^T: lane = query row, slots (hi, e) = d = 16 c + 8 hi + e
  bf16x8_t qop[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    uint4 t = {0u, 0u, 0u, 0u};
    if (qok) t = *reinterpret_cast<const uint4*>(q + base + (size_t)qi * rs + 16 * c + 8 * hi);
    qop[c] = as_bf16x8(t);
  }

  f32x16_t acc_o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_o[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int kt = (tlo < thi ? tlo / kBcKeys * kBcKeys : thi); kt < thi; kt += kBcKeys) {
    // ---- K tile as is, V tile transposed: 64 keys x 64 d = 512 16-byte chunks each, 2 per thread
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i, key = idx >> 3, d8 = (idx & 7) * 8;
      uint4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
      if (kt + key < T) {
        const size_t off = base + (size_t)(kt + key) * rs + d8;
        kv = *reinterpret_cast<const uint4*>(k + off);
        vv = *reinterpret_cast<const uint4*>(v + off);
      }
      *reinterpret_cast<uint4*>(&ks[key][d8]) = kv;
      const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vt[d8 + 2 * e][key] = (bf16_t)(w[e] & 0xffffu);
        vt[d8 + 2 * e + 1][key] = (bf16_t)(w[e] >> 16);
      }
    }
    __syncthreads();

    // ---- S^T for the two 32-key halves: lane holds query col, register r holds key crow(r, hi) + 32 kb
    f32x16_t s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8_t a = as_bf16x8(*reinterpret_cast<const uint4*>(&ks[kb * 32 + col][16 * c + 8 * hi]));
        s[kb] = mfma32(a, qop[c], s[kb]);
      }
    }
    // ---- mask, online softmax (exp2 domain)
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt + kb * 32 + crow(r, hi);
        const float sv = (key >= lo && key < kend) ? s[kb][r] * scale_log2 : -INFINITY;
        s[kb][r] = sv;
        mx = fmaxf(mx, sv);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = fast_exp2(m - m_use);
    float ps = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = fast_exp2(s[kb][r] - m_use);
        s[kb][r] = p;
        ps += p;
      }
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = m_new;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_o[db][r] *= alpha;

    // ---- O^T += V^T P^T.  Contraction chunk (kb, c): slot (hi, e) = register 8 c + e of S^T half kb, i.e.
    //      key 32 kb + 16 c + 4 hi + (e & 3) + 8 (e >> 2)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int r0 = 8 * c;
        const bf16x8_t pb = as_bf16x8(make_uint2(pack2bf(s[kb][r0 + 0], s[kb][r0 + 1]), pack2bf(s[kb][r0 + 2], s[kb][r0 + 3])),
                                      make_uint2(pack2bf(s[kb][r0 + 4], s[kb][r0 + 5]), pack2bf(s[kb][r0 + 6], s[kb][r0 + 7])));
        const int kc = 32 * kb + 16 * c + 4 * hi;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const int d = 32 * db + col;
          const uint2 lo4 = *reinterpret_cast<const uint2*>(&vt[d][kc]);
          const uint2 hi4 = *reinterpret_cast<const uint2*>(&vt[d][kc + 8]);
          acc_o[db] = mfma32(as_bf16x8(lo4, hi4), pb, acc_o[db]);
        }
      }
    __syncthreads();
  }

  // ---- epilogue: register r of acc_o[db] holds O[qi][32 db + crow(r, hi)]; four consecutive d per 8-byte store
  if (!qok) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  bf16_t* orow = o + base + (size_t)qi * rs;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * db + 8 * g + 4 * hi;
      const uint2 w = make_uint2(pack2bf(acc_o[db][4 * g] * inv, acc_o[db][4 * g + 1] * inv),
                                 pack2bf(acc_o[db][4 * g + 2] * inv, acc_o[db][4 * g + 3] * inv));
      *reinterpret_cast<uint2*>(orow + d) = w;
    }
}

}  // namespace tn

extern "C" int tn_attn_block_causal_fwd(const void* q, const void* k, const void* v, void* o, const int* seg_start,
                                        const int* key_end, int B, int T, int Nh, int D, int block, float scale, void* stream) {
  if (B < 0 || T < 0 || Nh <= 0 || D != tn::kBcD || block < 1) return TN_EINVAL;
  if (B == 0 || T == 0) return TN_OK;
  if (!q || !k || !v || !o || !seg_start || !key_end) return TN_EINVAL;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) || ((uintptr_t)o & 7)) return TN_EINVAL;
  if ((long long)B * T > INT_MAX || B > 65535 || Nh > 65535) return TN_EINVAL;
  dim3 grid((T + tn::kBcRows - 1) / tn::kBcRows, Nh, B), blk(256);
  hipLaunchKernelGGL(tn::attn_block_causal_fwd_kernel, grid, blk, 0, (hipStream_t)stream, (const tn::bf16_t*)q,
                     (const tn::bf16_t*)k, (const tn::bf16_t*)v, (tn::bf16_t*)o, seg_start, key_end, T, Nh, block,
                     scale * tn::kLog2e);
  TN_LAUNCH_CHECK();
  return TN_OK;
}
