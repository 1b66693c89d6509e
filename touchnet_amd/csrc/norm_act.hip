// HBM-bound row kernels: (add+)RMSNorm, (add+)LayerNorm, SwiGLU, GELU, RoPE.
//
// Reference arithmetic being replaced (all executed as un-fused eager aten ops on the
// packed path):
//   RMSNorm  transformers/models/llama/modeling_llama.py:62-67  (fp32 stats, cast, then * w)
//   residual transformers/models/llama/modeling_llama.py:306-324
//   SwiGLU   transformers/models/llama/modeling_llama.py:174-176
//   RoPE     transformers/models/llama/modeling_llama.py:113-160 with the packers'
//            restart-per-sentence position_ids (touchnet/models/llama/processing_llama.py:96-97)
//   LayerNorm/GELU: Whisper-style encoder layer driven by touchnet/models/qwen2_audio/__init__.py:18-133
//
// Layout: activations are row-major [rows, H] (rows = B*T of the packed buffer).  One wave64
// owns one row: every lane keeps its 16-byte vectors of the row in registers, statistics are
// wave-shuffle reductions (no LDS, no barrier), one HBM read + one write per element.
// Algorithmic bytes per row: see DESIGN.md §5.
//
// One definition per rule: `norm_fwd_kernel` / `norm_bwd_kernel` are the row shells of both norms (a `LN` flag
// selects the statistics and the affine formula), `norm_fwd_t` / `norm_bwd_t` their host checks and grids,
// `colsum_partials` every second-stage column sum, `swiglu_fwd_vec` / `swiglu_bwd_vec` the SwiGLU arithmetic of
// the plain and the transposing kernels, `ew_launch` the four element-wise entries, `rope_apply_kernel` the vector
// and the scalar RoPE walk.
#include "common.h"

namespace tn {

constexpr int kRowWaves = 4;  // rows per 256-thread block

// ------------------------------------------------------------------------------------------
// (residual-add +) norm forward, one wave per row.
//   h = x (+ res_in)              rounded to T (HF adds in the activation dtype); res_out = h when given
//   RMSNorm   (LN = false):  y = T( w * T(h * rstd) )             rstd = rsqrt(mean(h^2) + eps) in fp32
//   LayerNorm (LN = true):   y = T((h - mean) * rstd * w + b)     two-pass fp32 mean and variance
// `b` and `mean_out` are read / written by LayerNorm only; RMSNorm's `rstd_out` may be null.
// The guarded vector loop (`v = i * stride + thread; if (v < nvec)`) stays written out at each of its sites here and
// in the backward: as one helper that takes the body as a lambda it cost registers (fp32 LayerNorm forward MAXV 16:
// 112 -> 135 VGPRs, 4 -> 3 waves per SIMD; bf16 LayerNorm backward MAXV 4: 204 -> 234).
// ------------------------------------------------------------------------------------------
template <typename T, bool LN, int MAXV>
__global__ __launch_bounds__(256) void norm_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res_in,
                                                       const T* __restrict__ w, const T* __restrict__ b,
                                                       T* __restrict__ y, T* __restrict__ res_out,
                                                       float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                       int rows, int H, float eps) {
  constexpr int N = Vec16<T>::N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nvec = H / N;
  const size_t base = (size_t)row * H;
  float hv[MAXV][N];
  float s = 0.f;  // sum of h^2 (RMSNorm) / of h (LayerNorm)
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int v = i * 64 + lane;
    if (v < nvec) {
      Vec16<T> a;
      a.load(x + base + (size_t)v * N);
      a.unpack(hv[i]);
      if (res_in) {
        Vec16<T> r;
        float rf[N];
        r.load(res_in + base + (size_t)v * N);
        r.unpack(rf);
#pragma unroll
        for (int j = 0; j < N; ++j) hv[i][j] += rf[j];
        a.pack(hv[i]);  // round the sum to T ...
        a.unpack(hv[i]);  // ... and norm the rounded value, as the eager path does
        if (res_out) a.store(res_out + base + (size_t)v * N);
      }
#pragma unroll
      for (int j = 0; j < N; ++j) s += LN ? hv[i][j] : hv[i][j] * hv[i][j];
    }
  }
  float mean = 0.f;
  if constexpr (LN) {
    mean = wave_sum(s) / (float)H;
    s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = i * 64 + lane;
      if (v < nvec) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const float d = hv[i][j] - mean;
          s += d * d;
        }
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(s) / (float)H + eps);
  if (lane == 0) {
    if constexpr (LN) mean_out[row] = mean;
    if (LN || rstd_out) rstd_out[row] = rstd;
  }
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int v = i * 64 + lane;
    if (v < nvec) {
      Vec16<T> wv, o;
      float wf[N], of[N];
      wv.load(w + (size_t)v * N);
      wv.unpack(wf);
      if constexpr (LN) {
        Vec16<T> bv;
        float bf[N];
        bv.load(b + (size_t)v * N);
        bv.unpack(bf);
#pragma unroll
        for (int j = 0; j < N; ++j) of[j] = (hv[i][j] - mean) * rstd * wf[j] + bf[j];
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) of[j] = hv[i][j] * rstd;
        o.pack(of);  // T(h * rstd)
        o.unpack(of);
#pragma unroll
        for (int j = 0; j < N; ++j) of[j] *= wf[j];
      }
      o.pack(of);
      o.store(y + base + (size_t)v * N);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Norm backward.  g = dy*w;
//   RMSNorm:    xhat = T(h*rstd);       dh = rstd * (g - xhat * mean(g*xhat))
//   LayerNorm:  xhat = (h-mean)*rstd;   dh = rstd * (g - mean(g) - xhat * mean(g*xhat));   db = sum dy
//   both:       dh += dres (gradient arriving on the residual stream);   dw = sum dy * xhat
//   dw_partial / db_partial[block][c] = sum over the block's rows            (deterministic 2-stage)
// ------------------------------------------------------------------------------------------
// block-wide sum of two values at once (one barrier pair); `sm` holds >= 2 * blockDim.x/64 floats.  Per value the
// order is block_sum's (common.h): wave shuffle, then the waves in index order.
__device__ __forceinline__ void block_sum2(float& a, float& b, float* sm) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) {
    sm[2 * w] = a;
    sm[2 * w + 1] = b;
  }
  __syncthreads();
  a = b = 0.f;
  for (int i = 0; i < nw; ++i) {
    a += sm[2 * i];
    b += sm[2 * i + 1];
  }
}

// The one-value form, for a block of exactly four waves (the norm backward's 256 threads): a lane reads one partial
// and the sum takes them from lanes 0-3 as scalars, in the same order.  block_sum (common.h) is left alone: it reads the
// four partials as one 16-byte LDS load, four VGPRs at the point where the backward holds most, and the fp32 MAXV = 4
// instantiation came out at 98 VGPRs where 96 keep five waves per SIMD.
__device__ __forceinline__ float block_sum_4waves(float a, float* sm) {
  a = wave_sum(a);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[w] = a;
  __syncthreads();
  const int p = __float_as_int(sm[lane & 3]);
  a = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) a += __int_as_float(__builtin_amdgcn_readlane(p, i));
  return a;
}

// One 256-thread block walks rows (grid-stride); thread t owns 16-byte vectors t, t+256, ... of every row,
// so its slice of dw (and db) accumulates in registers across rows and is written once per block.
// `mean_in` and `db_partial` are LayerNorm's only.
template <typename T, bool LN, int MAXV>
__global__ __launch_bounds__(256) void norm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h,
                                                       const T* __restrict__ w, const float* __restrict__ mean_in,
                                                       const float* __restrict__ rstd_in, const T* __restrict__ dres,
                                                       T* __restrict__ dh, float* __restrict__ dw_partial,
                                                       float* __restrict__ db_partial, int rows, int H) {
  constexpr int N = Vec16<T>::N;
  __shared__ float sm[8];
  const int tid = threadIdx.x;
  const int nvec = H / N;
  float wf[MAXV][N], dwacc[MAXV][N] = {}, dbacc[MAXV][N] = {};
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int v = i * 256 + tid;
    if (v < nvec) {
      Vec16<T> wv;
      wv.load(w + (size_t)v * N);
      wv.unpack(wf[i]);
    }
  }
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const size_t base = (size_t)row * H;
    const float rstd = rstd_in[row];
    float mean = 0.f;
    if constexpr (LN) mean = mean_in[row];
    float g[MAXV][N], xh[MAXV][N];
    float s1 = 0.f, s2 = 0.f;  // sum of g (LayerNorm only) and of g * xhat
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = i * 256 + tid;
      if (v < nvec) {
        Vec16<T> a, b;
        float dyf[N];
        a.load(dy + base + (size_t)v * N);
        a.unpack(dyf);
        b.load(h + base + (size_t)v * N);
        b.unpack(xh[i]);
        if constexpr (LN) {
#pragma unroll
          for (int j = 0; j < N; ++j) xh[i][j] = (xh[i][j] - mean) * rstd;
        } else {
#pragma unroll
          for (int j = 0; j < N; ++j) xh[i][j] *= rstd;
          b.pack(xh[i]);
          b.unpack(xh[i]);  // xhat as the forward rounded it
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
          dwacc[i][j] += dyf[j] * xh[i][j];
          if constexpr (LN) dbacc[i][j] += dyf[j];
          g[i][j] = dyf[j] * wf[i][j];
          if constexpr (LN) s1 += g[i][j];
          s2 += g[i][j] * xh[i][j];
        }
      }
    }
    if constexpr (LN) {
      block_sum2(s1, s2, sm);
      s1 /= (float)H;
    } else {
      s2 = block_sum_4waves(s2, sm);
    }
    s2 /= (float)H;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = i * 256 + tid;
      if (v < nvec) {
        float o[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
          if constexpr (LN) o[j] = rstd * (g[i][j] - s1 - xh[i][j] * s2);
          else o[j] = rstd * (g[i][j] - xh[i][j] * s2);
        }
        if (dres) {
          Vec16<T> r;
          float rf[N];
          r.load(dres + base + (size_t)v * N);
          r.unpack(rf);
#pragma unroll
          for (int j = 0; j < N; ++j) o[j] += rf[j];
        }
        Vec16<T> ov;
        ov.pack(o);
        ov.store(dh + base + (size_t)v * N);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int v = i * 256 + tid;
    if (v < nvec) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        dw_partial[(size_t)blockIdx.x * H + v * N + j] = dwacc[i][j];
        if constexpr (LN) db_partial[(size_t)blockIdx.x * H + v * N + j] = dbacc[i][j];
      }
    }
  }
}

// out[c] = sum_p partial[p][c]  (second stage of every weight/bias gradient).
// 16 columns per block (64-byte row segments), 16 row groups summed through LDS.  (The first version gave a block 64
// columns x 4 row groups: 64 workgroups for a 4096-wide gradient, 16 us per launch x 451 launches per step — most of
// the chip idle; with cols/16 workgroups the 1-4 MB of partials take a third of that.)
template <typename T>
__global__ __launch_bounds__(256) void colsum_partials_kernel(const float* __restrict__ partial, T* __restrict__ out,
                                                              int P, int H) {
  __shared__ float sm[16][16 + 1];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cx;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < H) {
    int p = ry;
    for (; p + 48 < P; p += 64) {
      s0 += partial[(size_t)p * H + c];
      s1 += partial[(size_t)(p + 16) * H + c];
      s2 += partial[(size_t)(p + 32) * H + c];
      s3 += partial[(size_t)(p + 48) * H + c];
    }
    for (; p < P; p += 16) s0 += partial[(size_t)p * H + c];
  }
  sm[ry][cx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ry == 0 && c < H) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sm[k][cx];
    Elem<T>::st(out + c, t);
  }
}

// Bias gradient, stage 1:  partial[p][c] = sum over the rows of slab p of x[r][c]   (x bf16 [rows, ld], fp32 sums).
// Block = 256 columns (32 threads x 16-byte vectors) x 8 row lanes; slab p = rows [p*rps, (p+1)*rps).  torch's
// column reduction of a [30000, 1280] bf16 gradient runs at 1.8 TB/s; this pair of kernels is HBM-bound.
__global__ __launch_bounds__(256) void colsum_rows_kernel(const bf16_t* __restrict__ x, float* __restrict__ partial,
                                                          int rows, int cols, long long ld, int rps) {
  __shared__ float sm[8][256 + 8];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 256 + cx * 8;
  const int r_beg = blockIdx.y * rps, r_end = min(r_beg + rps, rows);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < cols) {
    for (int r = r_beg + ry; r < r_end; r += 8) {
      Vec16<bf16_t> v;
      float f[8];
      v.load(x + (size_t)r * ld + c0);
      v.unpack(f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sm[ry][cx * 8 + j] = acc[j];
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += sm[k][threadIdx.x];
    partial[(size_t)blockIdx.y * cols + c] = t;
  }
}

// ------------------------------------------------------------------------------------------
// Element-wise: SwiGLU and exact (erf) GELU, forward and backward, 16-byte vectors, grid-stride.
// The four kernels keep their own grid-stride loops: they differ in the number of tensors they read and write, and a
// shell over that (an operation type with its own argument list per kernel) is longer than the four three-line loops.
// ------------------------------------------------------------------------------------------
// SwiGLU on one 16-byte vector, for the plain and the transposing kernels alike (sigmoid_fast: common.h, shared with
// the GEMM epilogues).  Forward: T( T(silu(g)) * u ), silu rounded to T as the eager path materialises it.
template <typename T>
__device__ __forceinline__ Vec16<T> swiglu_fwd_vec(const Vec16<T>& g, const Vec16<T>& u) {
  constexpr int N = Vec16<T>::N;
  Vec16<T> o;
  float gf[N], uf[N];
  g.unpack(gf);
  u.unpack(uf);
#pragma unroll
  for (int j = 0; j < N; ++j) gf[j] = gf[j] * sigmoid_fast(gf[j]);
  o.pack(gf);  // T(silu(g))
  o.unpack(gf);
#pragma unroll
  for (int j = 0; j < N; ++j) gf[j] *= uf[j];
  o.pack(gf);
  return o;
}

// Backward: dup = d * silu(g);  dgate = d * u * (s + silu(g) * (1 - s)),  s = sigmoid(g)
template <typename T>
__device__ __forceinline__ void swiglu_bwd_vec(const Vec16<T>& d, const Vec16<T>& g, const Vec16<T>& u,
                                               Vec16<T>& dgate, Vec16<T>& dup) {
  constexpr int N = Vec16<T>::N;
  float df[N], gf[N], uf[N], dg[N], du[N];
  d.unpack(df);
  g.unpack(gf);
  u.unpack(uf);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float s = sigmoid_fast(gf[j]);
    const float silu = gf[j] * s;
    du[j] = df[j] * silu;
    dg[j] = df[j] * uf[j] * (s + silu * (1.f - s));
  }
  dgate.pack(dg);
  dup.pack(du);
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ gate, const T* __restrict__ up,
                                                         T* __restrict__ out, size_t nvec) {
  constexpr int N = Vec16<T>::N;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    Vec16<T> g, u;
    g.load(gate + v * N);
    u.load(up + v * N);
    swiglu_fwd_vec(g, u).store(out + v * N);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ gate,
                                                         const T* __restrict__ up, T* __restrict__ dgate,
                                                         T* __restrict__ dup, size_t nvec) {
  constexpr int N = Vec16<T>::N;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    Vec16<T> d, g, u, og, ou;
    d.load(dout + v * N);
    g.load(gate + v * N);
    u.load(up + v * N);
    swiglu_bwd_vec(d, g, u, og, ou);
    og.store(dgate + v * N);
    ou.store(dup + v * N);
  }
}

// ---- SwiGLU with transposed second outputs (bf16): the MLP's weight-gradient GEMMs want act^T, d_gate^T and d_up^T
// (forward-layout GEMMs).  Writing them here costs one extra store of each tensor; the standalone
// transpose pass costs a load and a store.  A thread owns an 8 x 8 block (same tiling as transpose.hip): 16-byte row
// loads (8 adjacent lanes = one 128-byte line), v_perm register transposes, 16-byte stores both ways.
__device__ __forceinline__ void transpose8x8_store(const uint4 (&in)[8], bf16_t* dst, long long dst_ld) {
  const uint32_t w[8][4] = {{in[0].x, in[0].y, in[0].z, in[0].w}, {in[1].x, in[1].y, in[1].z, in[1].w},
                            {in[2].x, in[2].y, in[2].z, in[2].w}, {in[3].x, in[3].y, in[3].z, in[3].w},
                            {in[4].x, in[4].y, in[4].z, in[4].w}, {in[5].x, in[5].y, in[5].z, in[5].w},
                            {in[6].x, in[6].y, in[6].z, in[6].w}, {in[7].x, in[7].y, in[7].z, in[7].w}};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int wi = c >> 1;
    const uint32_t sel = (c & 1) ? 0x07060302u : 0x05040100u;
    uint4 o;
    o.x = __builtin_amdgcn_perm(w[1][wi], w[0][wi], sel);
    o.y = __builtin_amdgcn_perm(w[3][wi], w[2][wi], sel);
    o.z = __builtin_amdgcn_perm(w[5][wi], w[4][wi], sel);
    o.w = __builtin_amdgcn_perm(w[7][wi], w[6][wi], sel);
    *reinterpret_cast<uint4*>(dst + (long long)c * dst_ld) = o;
  }
}

__global__ __launch_bounds__(256) void swiglu_fwd_t_kernel(const bf16_t* __restrict__ gate, const bf16_t* __restrict__ up,
                                                           bf16_t* __restrict__ out, bf16_t* __restrict__ out_t, int rows,
                                                           int cols) {
  const int cx = threadIdx.x & 7, rb = threadIdx.x >> 3;
  const int c0 = (blockIdx.x * 8 + cx) * 8, r0 = (blockIdx.y * 32 + rb) * 8;
  if (c0 >= cols || r0 >= rows) return;
  uint4 o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    Vec16<bf16_t> g, u;
    const size_t off = (size_t)(r0 + i) * cols + c0;
    g.load(gate + off);
    u.load(up + off);
    const Vec16<bf16_t> a = swiglu_fwd_vec(g, u);
    a.store(out + off);
    o[i] = a.raw;
  }
  transpose8x8_store(o, out_t + (size_t)c0 * rows + r0, rows);
}

__global__ __launch_bounds__(256) void swiglu_bwd_t_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ gate,
                                                           const bf16_t* __restrict__ up, bf16_t* __restrict__ dgate,
                                                           bf16_t* __restrict__ dup, bf16_t* __restrict__ dgu_t, int rows,
                                                           int cols) {
  const int cx = threadIdx.x & 7, rb = threadIdx.x >> 3;
  const int c0 = (blockIdx.x * 8 + cx) * 8, r0 = (blockIdx.y * 32 + rb) * 8;
  if (c0 >= cols || r0 >= rows) return;
  uint4 og[8], ou[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    Vec16<bf16_t> d, g, u, a, b;
    const size_t off = (size_t)(r0 + i) * cols + c0;
    d.load(dout + off);
    g.load(gate + off);
    u.load(up + off);
    swiglu_bwd_vec(d, g, u, a, b);
    a.store(dgate + off);
    b.store(dup + off);
    og[i] = a.raw;
    ou[i] = b.raw;
  }
  transpose8x8_store(og, dgu_t + (size_t)c0 * rows + r0, rows);                    // rows [0, cols): d_gate^T
  transpose8x8_store(ou, dgu_t + (size_t)(cols + c0) * rows + r0, rows);           // rows [cols, 2 cols): d_up^T
}

template <typename T>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, size_t nvec) {
  constexpr int N = Vec16<T>::N;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    Vec16<T> a;
    float f[N];
    a.load(x + v * N);
    a.unpack(f);
#pragma unroll
    for (int j = 0; j < N; j += 2) {
      const gelu_f32x2 r = gelu_f2(gelu_f32x2{f[j], f[j + 1]});
      f[j] = r.x;
      f[j + 1] = r.y;
    }
    a.pack(f);
    a.store(out + v * N);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ x,
                                                       T* __restrict__ dx, size_t nvec) {
  constexpr int N = Vec16<T>::N;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (size_t)gridDim.x * blockDim.x) {
    Vec16<T> a, d;
    float f[N], df[N];
    a.load(x + v * N);
    d.load(dout + v * N);
    a.unpack(f);
    d.unpack(df);
#pragma unroll
    for (int j = 0; j < N; j += 2) {
      const gelu_f32x2 r = gelu_grad_f2(gelu_f32x2{f[j], f[j + 1]}, gelu_f32x2{df[j], df[j + 1]});
      df[j] = r.x;
      df[j + 1] = r.y;
    }
    d.pack(df);
    d.store(dx + v * N);
  }
}

// ------------------------------------------------------------------------------------------
// RoPE.  Table: cos/sin[n, D/2] = cos/sin(position_ids[n] * inv_freq[i]) computed in fp32 and
// stored in T (the eager path casts its fp32 table to the activation dtype).
// Apply (out of place or in place when y == x, half-split convention): for i < D/2
//   y[i]       = x[i]*c[i] - x[i+D/2]*s[i]
//   y[i+D/2]   = x[i+D/2]*c[i] + x[i]*s[i]
// `sign` = +1 forward, -1 backward (the transpose rotation).
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void rope_table_kernel(const int64_t* __restrict__ pos, const float* __restrict__ inv_freq,
                                  T* __restrict__ cos_t, T* __restrict__ sin_t, int n, int half, float scaling) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n * half) return;
  const int i = idx % half;
  const float ang = (float)pos[idx / half] * inv_freq[i];
  float s, c;
  sincosf(ang, &s, &c);
  Elem<T>::st(cos_t + idx, c * scaling);
  Elem<T>::st(sin_t + idx, s * scaling);
}

// x: [n, heads, D] contiguous, the q heads of a token in xq / yq and its k heads in xk / yk.  One thread rotates W
// adjacent pairs (x[i], x[i + D/2]): W = Vec16<T>::N moves 16-byte vectors, W = 1 is the scalar form for tiny head dims
// (D/2 not a multiple of the vector width).
template <typename T, int W>
__global__ __launch_bounds__(256) void rope_apply_kernel(const T* xq, const T* xk, T* yq, T* yk,
                                                         const T* __restrict__ cos_t, const T* __restrict__ sin_t,
                                                         int n, int hq, int hk, int D, float sign) {
  const int half = D / 2, per = half / W;  // threads per half head
  const int heads = hq + hk;
  const size_t total = (size_t)n * heads * per;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int v = idx % per;
    const int hd = (idx / per) % heads;
    const size_t tok = idx / ((size_t)per * heads);
    const size_t off = (hd < hq) ? (tok * hq + hd) * D : (tok * hk + (hd - hq)) * D;
    const T* p = ((hd < hq) ? xq : xk) + off;
    T* o = ((hd < hq) ? yq : yk) + off;
    if constexpr (W == 1) {
      const float a = Elem<T>::ld(p + v), b = Elem<T>::ld(p + half + v);
      const float c = Elem<T>::ld(cos_t + tok * half + v), s = sign * Elem<T>::ld(sin_t + tok * half + v);
      float ya, yb;
      rope_rotate(a, b, c, s, ya, yb);
      Elem<T>::st(o + v, ya);
      Elem<T>::st(o + half + v, yb);
    } else {
      static_assert(W == Vec16<T>::N, "a thread moves one element or one 16-byte vector per half");
      Vec16<T> lo, hi, cv, sv;
      float a[W], b[W], c[W], s[W], ya[W], yb[W];
      lo.load(p + v * W);
      hi.load(p + half + v * W);
      cv.load(cos_t + tok * half + v * W);
      sv.load(sin_t + tok * half + v * W);
      lo.unpack(a);
      hi.unpack(b);
      cv.unpack(c);
      sv.unpack(s);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        rope_rotate(a[j], b[j], c[j], sign * s[j], ya[j], yb[j]);
      }
      lo.pack(ya);
      hi.pack(yb);
      lo.store(o + v * W);
      hi.store(o + half + v * W);
    }
  }
}

// ------------------------------------------------------------------------------------------
// host-side dispatch
// ------------------------------------------------------------------------------------------
static inline int pick_maxv(int H, int N) {   // vectors per lane when a wave holds a row (forward)
  const int per_lane = (H / N + 63) / 64;
  if (per_lane <= 1) return 1;
  if (per_lane <= 2) return 2;
  if (per_lane <= 4) return 4;
  if (per_lane <= 8) return 8;
  if (per_lane <= 16) return 16;
  return -1;
}

static inline int pick_maxv_block(int H, int N) {   // vectors per thread when 256 threads share a row (backward)
  const int per = (H / N + 255) / 256;
  return per <= 1 ? 1 : (per <= 2 ? 2 : (per <= 4 ? 4 : -1));
}

// Each norm kernel is instantiated for exactly the values its picker returns: the forward for 1 ... 16, the backward
// for 1, 2, 4 (at 8 and 16 it would need 300-512 VGPRs and scratch, and nothing could launch it).  A width past the
// widest instantiation is refused.
#define TN_MAXV_CASE(n, ...) case n: { constexpr int MAXV = n; __VA_ARGS__; } break;
#define TN_DISPATCH_MAXV(mv, ...)                                                                                   \
  switch (mv) {                                                                                                     \
    TN_MAXV_CASE(1, __VA_ARGS__) TN_MAXV_CASE(2, __VA_ARGS__) TN_MAXV_CASE(4, __VA_ARGS__)                          \
    TN_MAXV_CASE(8, __VA_ARGS__) TN_MAXV_CASE(16, __VA_ARGS__)                                                      \
    default: return TN_EINVAL;                                                                                      \
  }
#define TN_DISPATCH_MAXV_BLOCK(mv, ...)                                                                             \
  switch (mv) {                                                                                                     \
    TN_MAXV_CASE(1, __VA_ARGS__) TN_MAXV_CASE(2, __VA_ARGS__) TN_MAXV_CASE(4, __VA_ARGS__)                          \
    default: return TN_EINVAL;                                                                                      \
  }

// out[c] = sum_p partial[p][c]: the second stage of dw, db and the bias gradient
template <typename T>
static int colsum_partials(const float* partial, void* out, int P, int H, hipStream_t st) {
  hipLaunchKernelGGL((colsum_partials_kernel<T>), dim3((H + 15) / 16), dim3(256), 0, st, partial, (T*)out, P, H);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

// The norm entries' contract (include/touchnet_amd.h): rows > 0, H > 0 a whole number of 16-byte vectors and no wider
// than the widest instantiation.  Forward: one wave per row, kRowWaves rows per block.
template <typename T, bool LN>
static int norm_fwd_t(const void* x, const void* res_in, const void* w, const void* b, void* y, void* res_out,
                      float* mean, float* rstd, int rows, int H, float eps, hipStream_t st) {
  constexpr int N = Vec16<T>::N;
  if (rows <= 0 || H <= 0 || H % N) return TN_EINVAL;
  dim3 grid((rows + kRowWaves - 1) / kRowWaves), block(256);
  TN_DISPATCH_MAXV(pick_maxv(H, N), hipLaunchKernelGGL((norm_fwd_kernel<T, LN, MAXV>), grid, block, 0, st,
                                                       (const T*)x, (const T*)res_in, (const T*)w, (const T*)b, (T*)y,
                                                       (T*)res_out, mean, rstd, rows, H, eps));
  TN_LAUNCH_CHECK();
  return TN_OK;
}

static inline int norm_bwd_blocks(int rows) { return rows < 1024 ? rows : 1024; }

// Backward: norm_bwd_blocks(rows) blocks walk the rows; `ws` holds their dw partials, then (LayerNorm) their db partials
template <typename T, bool LN>
static int norm_bwd_t(const void* dy, const void* h, const void* w, const float* mean, const float* rstd,
                      const void* dres, void* dh, void* dw, void* db, float* ws, int rows, int H, hipStream_t st) {
  constexpr int N = Vec16<T>::N;
  if (rows <= 0 || H <= 0 || H % N) return TN_EINVAL;
  const int nb = norm_bwd_blocks(rows);
  float* ws_b = ws + (size_t)nb * H;
  TN_DISPATCH_MAXV_BLOCK(pick_maxv_block(H, N),
                         hipLaunchKernelGGL((norm_bwd_kernel<T, LN, MAXV>), dim3(nb), dim3(256), 0, st, (const T*)dy,
                                            (const T*)h, (const T*)w, mean, rstd, (const T*)dres, (T*)dh, ws, ws_b,
                                            rows, H));
  TN_LAUNCH_CHECK();
  if (int e = colsum_partials<T>(ws, dw, nb, H, st)) return e;
  return LN ? colsum_partials<T>(ws_b, db, nb, H, st) : TN_OK;
}

static inline int ew_grid(size_t nvec) {
  size_t b = (nvec + 255) / 256;
  return (int)(b < 4096 ? (b ? b : 1) : 4096);
}

// The element-wise entries: n >= 0 a whole number of 16-byte vectors; `kernel` takes `args...` and the vector count
template <typename T, typename K, typename... A>
static int ew_launch(K kernel, long long n, void* stream, A... args) {
  constexpr int N = Vec16<T>::N;
  if (n < 0 || n % N) return TN_EINVAL;
  const size_t nvec = (size_t)n / N;
  hipLaunchKernelGGL(kernel, dim3(ew_grid(nvec)), dim3(256), 0, (hipStream_t)stream, args..., nvec);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // namespace tn

using namespace tn;

#define TN_DTYPE_SWITCH(dtype, ...)                                  \
  if ((dtype) == 0) { typedef float T; __VA_ARGS__; }                \
  else if ((dtype) == 1) { typedef bf16_t T; __VA_ARGS__; }          \
  else return TN_EINVAL;

extern "C" {

int tn_norm_bwd_workspace_floats(int rows, int H) { return 2 * norm_bwd_blocks(rows) * H; }

int tn_rmsnorm_fwd(const void* x, const void* res_in, const void* w, void* y, void* res_out, float* rstd, int rows,
                   int H, float eps, int dtype, void* stream) {
  TN_DTYPE_SWITCH(dtype, return (norm_fwd_t<T, false>)(x, res_in, w, nullptr, y, res_out, nullptr, rstd, rows, H, eps,
                                                       (hipStream_t)stream));
}

int tn_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, void* dh,
                   void* dw, float* workspace, int rows, int H, int dtype, void* stream) {
  TN_DTYPE_SWITCH(dtype, return (norm_bwd_t<T, false>)(dy, h, w, nullptr, rstd, dres, dh, dw, nullptr, workspace, rows,
                                                       H, (hipStream_t)stream));
}

int tn_layernorm_fwd(const void* x, const void* res_in, const void* w, const void* b, void* y, void* res_out,
                     float* mean, float* rstd, int rows, int H, float eps, int dtype, void* stream) {
  TN_DTYPE_SWITCH(dtype, return (norm_fwd_t<T, true>)(x, res_in, w, b, y, res_out, mean, rstd, rows, H, eps,
                                                      (hipStream_t)stream));
}

int tn_layernorm_bwd(const void* dy, const void* h, const void* w, const float* mean, const float* rstd,
                     const void* dres, void* dh, void* dw, void* db, float* workspace, int rows, int H, int dtype,
                     void* stream) {
  TN_DTYPE_SWITCH(dtype, return (norm_bwd_t<T, true>)(dy, h, w, mean, rstd, dres, dh, dw, db, workspace, rows, H,
                                                      (hipStream_t)stream));
}

int tn_swiglu_fwd(const void* gate, const void* up, void* out, long long n, int dtype, void* stream) {
  TN_DTYPE_SWITCH(dtype, return ew_launch<T>(swiglu_fwd_kernel<T>, n, stream, (const T*)gate, (const T*)up, (T*)out));
}

int tn_swiglu_bwd(const void* dout, const void* gate, const void* up, void* dgate, void* dup, long long n, int dtype,
                  void* stream) {
  TN_DTYPE_SWITCH(dtype, return ew_launch<T>(swiglu_bwd_kernel<T>, n, stream, (const T*)dout, (const T*)gate,
                                             (const T*)up, (T*)dgate, (T*)dup));
}

// bf16 only; rows, cols multiples of 8; out_t [cols, rows]; dgu_t [2 cols, rows] = [d_gate^T ; d_up^T]
int tn_swiglu_fwd_t(const void* gate, const void* up, void* out, void* out_t, int rows, int cols, void* stream) {
  if (rows <= 0 || cols <= 0 || (rows | cols) & 7) return TN_EINVAL;
  dim3 grid((cols + 63) / 64, (rows + 255) / 256);
  hipLaunchKernelGGL(swiglu_fwd_t_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)gate,
                     (const bf16_t*)up, (bf16_t*)out, (bf16_t*)out_t, rows, cols);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

int tn_swiglu_bwd_t(const void* dout, const void* gate, const void* up, void* dgate, void* dup, void* dgu_t, int rows,
                    int cols, void* stream) {
  if (rows <= 0 || cols <= 0 || (rows | cols) & 7) return TN_EINVAL;
  dim3 grid((cols + 63) / 64, (rows + 255) / 256);
  hipLaunchKernelGGL(swiglu_bwd_t_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout,
                     (const bf16_t*)gate, (const bf16_t*)up, (bf16_t*)dgate, (bf16_t*)dup, (bf16_t*)dgu_t, rows, cols);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

int tn_gelu_fwd(const void* x, void* out, long long n, int dtype, void* stream) {
  TN_DTYPE_SWITCH(dtype, return ew_launch<T>(gelu_fwd_kernel<T>, n, stream, (const T*)x, (T*)out));
}

int tn_gelu_bwd(const void* dout, const void* x, void* dx, long long n, int dtype, void* stream) {
  TN_DTYPE_SWITCH(dtype, return ew_launch<T>(gelu_bwd_kernel<T>, n, stream, (const T*)dout, (const T*)x, (T*)dx));
}

int tn_rope_table(const long long* position_ids, const float* inv_freq, void* cos_t, void* sin_t, int n, int half,
                  float attention_scaling, int dtype, void* stream) {
  if (n <= 0 || half <= 0) return TN_EINVAL;
  TN_DTYPE_SWITCH(dtype, {
    const size_t total = (size_t)n * half;
    hipLaunchKernelGGL((rope_table_kernel<T>), dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)position_ids, inv_freq, (T*)cos_t, (T*)sin_t, n, half, attention_scaling);
    TN_LAUNCH_CHECK();
    return TN_OK;
  });
}

int tn_rope_apply(const void* q, const void* k, void* q_out, void* k_out, const void* cos_t, const void* sin_t, int n,
                  int hq, int hk, int D, int backward, int dtype, void* stream) {
  if (n <= 0 || hq <= 0 || hk < 0 || D <= 0 || D % 2) return TN_EINVAL;
  const float sign = backward ? -1.f : 1.f;
  TN_DTYPE_SWITCH(dtype, {
    constexpr int N = Vec16<T>::N;
    const bool vec = (D / 2) % N == 0;                                        // whole 16-byte vectors per half head
    const size_t total = (size_t)n * (hq + hk) * (D / 2 / (vec ? N : 1));     // one thread each
    hipLaunchKernelGGL((vec ? rope_apply_kernel<T, N> : rope_apply_kernel<T, 1>), dim3(ew_grid(total)), dim3(256), 0,
                       (hipStream_t)stream, (const T*)q, (const T*)k, (T*)q_out, (T*)k_out, (const T*)cos_t,
                       (const T*)sin_t, n, hq, hk, D, sign);
    TN_LAUNCH_CHECK();
    return TN_OK;
  });
}

// out[c] = sum_r x[r][c]  for a bf16 [rows, cols] matrix with row stride ld (bias gradient of a linear layer):
// two deterministic stages through `ws` (tn_colsum_workspace_floats(rows, cols) floats).
// slabs: enough workgroups to keep HBM busy (~4096; the first version used 64 slabs = 320 workgroups on a
// [30000, 1280] gradient and ran at 1.8 TB/s, PMC-confirmed), at least 16 rows each
static int colsum_slabs(int rows, int cols) {
  const int cb = (cols + 255) / 256;
  int s = (4096 + cb - 1) / cb;
  const int smax = rows / 16 > 0 ? rows / 16 : 1;
  s = s > 1024 ? 1024 : s;
  s = s > smax ? smax : s;
  return s < 1 ? 1 : s;
}

long long tn_colsum_workspace_floats(int rows, int cols) { return (long long)colsum_slabs(rows, cols) * cols; }

int tn_colsum_bf16(const void* x, void* out, float* ws, int rows, int cols, long long ld, void* stream) {
  if (rows <= 0 || cols <= 0 || cols % 8 || ld % 8 || ld < cols || ((uintptr_t)x & 15)) return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int slabs = colsum_slabs(rows, cols);
  const int rps = (rows + slabs - 1) / slabs;
  hipLaunchKernelGGL(colsum_rows_kernel, dim3((cols + 255) / 256, slabs), dim3(256), 0, st, (const bf16_t*)x, ws, rows,
                     cols, ld, rps);
  TN_LAUNCH_CHECK();
  return colsum_partials<bf16_t>(ws, out, slabs, cols, st);
}

}  // extern "C"
