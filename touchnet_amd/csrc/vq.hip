// Nearest-code search of the Kimi-Audio / GLM-4-voice speech tokenizer's vector quantiser
// (`vector_quantize`, touchnet/models/kimi_audio/modeling_kimi_audio.py:85-98):
//     ids[r] = argmin_c ( |c|^2 - 2 x_r . c )      (|x_r|^2 is the same for every c and is dropped)
// first index on ties, like torch.min.  x bf16 [M, d], codebook bf16 [V, d], |c|^2 fp32 [V] (computed once: the
// codebook is frozen), d % 64 == 0.
//
// A GEMM with an argmin epilogue: the [M, V] distance matrix never leaves the registers.  One workgroup = 4 waves =
// 128 rows x a chunk of 128-code tiles; the operands run through LDS 64 contraction elements at a time and every
// wave accumulates a 64-code x 64-row block of C^T = codes . x^T on v_mfma_f32_32x32x16_bf16 (fp32).  In that
// orientation a lane owns two rows and 16 codes of each 32-code half, so the epilogue keeps a running best per row
// without shuffles.  The best of a row is a 64-bit key (order-preserving distance bits << 32 | code index): the
// lexicographic (distance, index) minimum.  Workgroups of different code chunks meet in one 64-bit atomic min per row
// on the output buffer itself, which is order-independent — the id of a row does not depend on M, on its neighbours,
// on the chunking or on the launch.  A last pass drops the distance bits.
#include <limits.h>

#include <algorithm>

#include "attn_common.h"

namespace tn {

constexpr int kVqRows = 128, kVqCodes = 128, kVqK = 64, kVqPad = 8;

__device__ __forceinline__ unsigned long long vq_key(float dist, int idx) {
  uint32_t u = __float_as_uint(dist);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);            // float order == unsigned order
  return ((unsigned long long)u << 32) | (uint32_t)idx;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void vq_nearest_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ cb,
                                                         const float* __restrict__ cnorm, unsigned long long* __restrict__ best,
                                                         int M, int V, int d, int tiles_per_chunk) {
  __shared__ __attribute__((aligned(16))) bf16_t xs[kVqRows][kVqK + kVqPad];
  __shared__ __attribute__((aligned(16))) bf16_t cs[kVqCodes][kVqK + kVqPad];
  __shared__ unsigned long long red[kVqRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, col = lane & 31;
  const int wr = wave & 1, wc = wave >> 1;                        // the wave's 64-row half and 64-code half
  const int m0 = blockIdx.x * kVqRows;
  const int ntiles = (V + kVqCodes - 1) / kVqCodes;
  const int ct0 = blockIdx.y * tiles_per_chunk, ct1 = min(ntiles, ct0 + tiles_per_chunk);
  unsigned long long bk[2] = {~0ull, ~0ull};                      // rows m0 + 64 wr + 32 j + col

  for (int ct = ct0; ct < ct1; ++ct) {
    const int c0 = ct * kVqCodes;
    f32x16_t acc[2][2];                                             // [code half][row half]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int k0 = 0; k0 < d; k0 += kVqK) {
      // 128 x 64 tiles of x and of the codebook: 1024 16-byte chunks each, 4 per thread
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 3, c8 = (idx & 7) * 8;
        uint4 xv = {0u, 0u, 0u, 0u}, cv = {0u, 0u, 0u, 0u};
        if (m0 + r < M) xv = *reinterpret_cast<const uint4*>(x + (size_t)(m0 + r) * d + k0 + c8);
        if (c0 + r < V) cv = *reinterpret_cast<const uint4*>(cb + (size_t)(c0 + r) * d + k0 + c8);
        *reinterpret_cast<uint4*>(&xs[r][c8]) = xv;
        *reinterpret_cast<uint4*>(&cs[r][c8]) = cv;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kVqK; kk += 16) {
        bf16x8_t a[2], bx[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          a[j] = as_bf16x8(*reinterpret_cast<const uint4*>(&cs[64 * wc + 32 * j + col][kk + 8 * hi]));
          bx[j] = as_bf16x8(*reinterpret_cast<const uint4*>(&xs[64 * wr + 32 * j + col][kk + 8 * hi]));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(a[i], bx[j], acc[i][j]);
      }
      __syncthreads();
    }
    // epilogue: acc[i][j] register r = x_row . c for row 64 wr + 32 j + col, code c0 + 64 wc + 32 i + crow(r, hi)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int code = c0 + 64 * wc + 32 * i + crow(r, hi);
        if (code < V) {
          const float cn = cnorm[code];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const unsigned long long key = vq_key(__builtin_fmaf(-2.f, acc[i][j][r], cn), code);
            bk[j] = key < bk[j] ? key : bk[j];
          }
        }
      }
  }
  // the two lane halves hold the same rows; then the two code-half waves; then one atomic per row and workgroup
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const unsigned long long o = shfl_xor_u64(bk[j], 32);
    bk[j] = o < bk[j] ? o : bk[j];
  }
  if (wc == 1 && hi == 0) {
    red[64 * wr + col] = bk[0];
    red[64 * wr + 32 + col] = bk[1];
  }
  __syncthreads();
  if (wc == 0 && hi == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = 64 * wr + 32 * j + col;
      const unsigned long long o = red[row];
      const unsigned long long key = o < bk[j] ? o : bk[j];
      if (m0 + row < M) atomicMin(best + m0 + row, key);
    }
  }
}

__global__ void vq_init_kernel(unsigned long long* __restrict__ best, int M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) best[i] = ~0ull;
}

__global__ void vq_finish_kernel(unsigned long long* __restrict__ best, int M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) best[i] &= 0xffffffffull;
}

}  // namespace tn

extern "C" int tn_vq_nearest(const void* x, const void* codebook, const float* cnorm, long long* ids, int M, int V, int d,
                             void* stream) {
  if (M < 0 || V <= 0 || d <= 0 || d % tn::kVqK != 0) return TN_EINVAL;
  if (M == 0) return TN_OK;
  if (!x || !codebook || !cnorm || !ids) return TN_EINVAL;
  if ((((uintptr_t)x | (uintptr_t)codebook) & 15) || ((uintptr_t)ids & 7)) return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  auto* best = reinterpret_cast<unsigned long long*>(ids);
  const int row_tiles = (M + tn::kVqRows - 1) / tn::kVqRows, code_tiles = (V + tn::kVqCodes - 1) / tn::kVqCodes;
  // split the codes until the launch has ~2048 workgroups (8 per CU); the result does not depend on the split
  int chunks = std::max(1, std::min(code_tiles, (2048 + row_tiles - 1) / row_tiles));
  const int per = (code_tiles + chunks - 1) / chunks;
  chunks = (code_tiles + per - 1) / per;
  hipLaunchKernelGGL(tn::vq_init_kernel, dim3((M + 255) / 256), dim3(256), 0, st, best, M);
  hipLaunchKernelGGL(tn::vq_nearest_kernel, dim3(row_tiles, chunks), dim3(256), 0, st, (const tn::bf16_t*)x,
                     (const tn::bf16_t*)codebook, cnorm, best, M, V, d, per);
  hipLaunchKernelGGL(tn::vq_finish_kernel, dim3((M + 255) / 256), dim3(256), 0, st, best, M);
  TN_LAUNCH_CHECK();
  return TN_OK;
}
