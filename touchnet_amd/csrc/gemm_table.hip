// The table-driven grouped weight-gradient launch (EPI_TABLE of Kernel, gemm_kernel.h): its two kernel instantiations, the
// kernel that carries the table to the device, and the C entry point.  A source file of its own: gemm.hip holds exactly
// the kernels its `launch` rule and the fused entry points reach.
#include "gemm_host.h"

namespace tn {
namespace gemm {

// EPI_TABLE's table reaches the device in the kernel arguments of this launch, TABCHUNK records at a time: stream-ordered
// in front of the GEMM that reads it, with no pinned host buffer and no wait on the host (a copy from pageable memory may
// hold the host until the stream has drained).  One thread per 8-byte word.
struct RecChunk {
  Rec r[TABCHUNK];
};
static_assert(sizeof(Rec) % 8 == 0 && sizeof(RecChunk) <= 3072, "a chunk of records fits the kernel-argument segment");
constexpr int REC_WORDS = (int)(sizeof(Rec) / 8);

__global__ __launch_bounds__(TABCHUNK * REC_WORDS) void table_upload_kernel(const RecChunk c, Rec* dst, int n) {
  const int t = threadIdx.x;
  if (t < n * REC_WORDS)
    reinterpret_cast<unsigned long long*>(dst)[t] = reinterpret_cast<const unsigned long long*>(&c)[t];
}

}  // namespace gemm
}  // namespace tn

extern "C" {

// The grouped launch for ANY number of weight gradients (n = 1..MAXTAB; both operands contraction-major): product g is
// C_g[M_g, N_g] (+)= A_g^T B_g and, where bias_grad[g] is not null, bias_grad[g][M_g] (bf16) = column sums of A_g.  What it
// is for: the audio tower's linear layers are 300 output tiles per layer — 1.17 rounds on 256 CUs, so every per-layer
// form either idles most of a round or cuts the contraction (workspace, reduce); a weight gradient is consumed by nobody
// before the gradient norm, so the products of MANY layers can wait and run as one tile list: 11 layers are 3300 tiles =
// 12.9 rounds.  Whole tiles only — every output has the bits of the single-product unsplit launch (tn_gemm_bf16_wgrad_bias /
// tn_gemm_bf16_wgrad_f32 with splitk = 1): no workspace, no reduce.  The products' records travel through `table`, device
// memory of the caller's (>= tn_gemm_grouped_table_bytes(n), 16-byte aligned) that must stay untouched until the launch
// has run; outputs of different products may not overlap.
long long tn_gemm_grouped_table_bytes(int n) { return n < 1 || n > MAXTAB ? -1 : (long long)n * (long long)sizeof(Rec); }

int tn_gemm_bf16_grouped_table(const void* const* A, const void* const* B, const long long* lda, const long long* ldb,
                               const int* K, void* const* C, const long long* ldc, const int* M, const int* N,
                               void* const* bias_grad, int n, int accumulate, int c_f32, void* table, long long table_bytes,
                               void* stream) {
  if (n < 1 || n > MAXTAB) return TN_EINVAL;
  if (table == nullptr || !aligned(15, table) || table_bytes < tn_gemm_grouped_table_bytes(n)) return TN_EINVAL;
  std::vector<RecChunk> chunks((n + TABCHUNK - 1) / TABCHUNK);
  long long total = 0;
  for (int g = 0; g < n; ++g) {
    Rec& r = chunks[g / TABCHUNK].r[g % TABCHUNK];
    if (total > 0x7fffffff) return TN_EINVAL;                                      // (tile ids are ints)
    if (!grouped_product(A[g], B[g], lda[g], ldb[g], K[g], C[g], ldc[g], M[g], N[g], c_f32, (int)total, r.seg, r.grp))
      return TN_EINVAL;
    r.bias_out = bias_grad != nullptr ? (bf16_t*)bias_grad[g] : nullptr;
    if (!aligned(1, r.bias_out)) return TN_EINVAL;
    total += (long long)r.grp.nbm * r.grp.nbn;
  }
  if (total > 0x7fffffff) return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  for (int c = 0; c * TABCHUNK < n; ++c)
    hipLaunchKernelGGL(table_upload_kernel, dim3(1), dim3(TABCHUNK * REC_WORDS), 0, st, chunks[c],
                       (Rec*)table + c * TABCHUNK, min(TABCHUNK, n - c * TABCHUNK));
  Params p;
  clear_params(p);
  p.table = (const Rec*)table;
  p.ngrp = n;
  p.accumulate = accumulate;
  p.c_f32 = c_f32;
  p.ntiles = (int)total;
  if (c_f32)
    hipLaunchKernelGGL((gemm_kernel<true, true, false, false, true, EPI_TABLE>), grid_for(p.ntiles), dim3(NT), 0, st, p);
  else
    hipLaunchKernelGGL((gemm_kernel<true, true, false, false, false, EPI_TABLE>), grid_for(p.ntiles), dim3(NT), 0, st, p);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
