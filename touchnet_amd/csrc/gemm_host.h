// Host-side rules of the GEMM entry points that more than one source file needs (gemm.hip, gemm_table.hip), ONE owner
// each: the grid (grid_for), the argument checks (row_operand_ok, kmaj_operand_ok, out_ok), one product of a grouped
// launch (grouped_product).  Internal linkage: every source file that includes this gets its own copy of the code, the
// one piece of state — persistent or not — lives in gemm.hip behind tn_gemm_get_persistent.
#pragma once

#include "gemm_kernel.h"

using namespace tn::gemm;
using tn::bf16_t;

extern "C" int tn_gemm_get_persistent(void);

namespace {

int num_cus() {
  static const int ncu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n >= 8 ? n / 8 * 8 : 8;
  }();
  return ncu;
}

bool persistent_now() {
  const char* pe = getenv("TN_GEMM_PERSIST");        // (the environment wins: kernel-development A/B)
  return pe ? atoi(pe) != 0 : tn_gemm_get_persistent() != 0;
}

// THE grid rule — persistent: one workgroup per CU walks its units (tiles x split-K parts); else one workgroup per unit
dim3 grid_for(int units) {
  const int ncu = num_cus();
  return dim3(persistent_now() && units > ncu ? ncu : units);
}

void clear_params(Params& p) {
  p = Params{};
  p.splitk = 1;
  p.nseg = 1;
}

void set_seg(Seg& s, const void* A, const void* B, long long lda, long long ldb, int K) {
  s.A = (const bf16_t*)A;
  s.B = (const bf16_t*)B;
  s.lda = lda;
  s.ldb = ldb;
  s.K = K;
  s.pad_ = 0;
}

// ---- THE argument checks: every entry point below refuses (-22) what these refuse, before anything is launched ----------
template <typename... P>
bool aligned(uintptr_t mask, P... ps) {
  return ((... | (uintptr_t)ps) & mask) == 0;
}

// per-tile DMA offsets are 32-bit: what one buffer descriptor spans stays below 2 GB
constexpr long long DMA_SPAN = 0x7fffffffLL;

// Row-stored operand X[rows, K] (pitch ld): whole 64-deep stages (behind K a stage would read the row's own next columns),
// 16-byte base, pitch % 8, the 288 rows a tile's descriptor spans below 2 GB.  min_ld is the entries' one difference: the
// fused ones pass K; the general entry passes 1, because it also takes OVERLAPPING rows (ld < K) — the im2col view of a
// k = 3 convolution over a channels-last sequence, row r = 3 C elements from r * stride * C on.  Every row is read in
// full, the last ones too: a tile's descriptor ends with the last row's last element, (rows - 1) * ld + K (Stream::open).
bool row_operand_ok(const void* X, long long ld, int K, long long min_ld) {
  return K > 0 && (K % 64) == 0 && aligned(15, X) && (ld % 8) == 0 && ld >= min_ld && 288 * ld * 2 < DMA_SPAN;
}

// Contraction-major operand X[K, rows] (pitch ld): any depth K (beside a row-stored operand, that one's check holds K to
// whole stages; two contraction-major descriptors both zero-fill the rows k >= K), 16-byte base, pitch % 8, the whole
// operand below 2 GB.  min_ld: `rows` for A and for the fused entries' B; 1 where the general and the grouped entry have
// always taken a B with overlapping rows.
bool kmaj_operand_ok(const void* X, long long ld, int K, int rows, long long min_ld) {
  return K > 0 && aligned(15, X) && (ld % 8) == 0 && ld >= min_ld && ((long long)(K - 1) * ld + rows) * 2 < DMA_SPAN;
}

// Output (or same-shape epilogue input) of `cols` columns: 16-byte base, pitch >= cols.  ld_mult: 8 elements everywhere
// (fp32 outputs of the general entry included) except the grouped launch's fp32 outputs, which need 4 floats = 16 bytes.
bool out_ok(const void* C, long long ld, int cols, int ld_mult) { return aligned(15, C) && (ld % ld_mult) == 0 && ld >= cols; }

// One product of a grouped launch (both entries; weight-gradient mode): THE checks — false = the entry answers -22 — and
// its segment and its place in the launch's tile list, which begins at tile `start` for it
bool grouped_product(const void* A, const void* B, long long lda, long long ldb, int k, void* C, long long ldc, int m, int n,
                     int c_f32, int start, Seg& s, Grp& g) {
  if (m <= 0 || n <= 0 || (m % 8) || (n % 8) || !kmaj_operand_ok(A, lda, k, m, m) || !kmaj_operand_ok(B, ldb, k, n, 1) ||
      !out_ok(C, ldc, n, c_f32 ? 4 : 8))
    return false;
  set_seg(s, A, B, lda, ldb, k);
  g.C = (bf16_t*)C;
  g.ldc = ldc;
  g.M = m;
  g.N = n;
  g.nbm = (m + BM - 1) / BM;
  g.nbn = (n + BN - 1) / BN;
  g.start = start;
  g.stages = (k + 63) / 64;
  return true;
}

}  // namespace
