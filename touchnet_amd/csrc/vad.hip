// Voice-activity detection on the GPU: the energy rule of Kaldi's `compute-vad-energy`, for recordings longer than one
// utterance (touchnet_amd/longform.py).  The reference's inference scripts know no such step: they cut every waveform at
// 30 s (touchnet/models/qwen2_audio/inference_qwen2_audio.py:101, touchnet/models/kimi_audio/processing_kimi_audio.py:73).
//
// Framing as in kaldi_feats.hip (snip_edges): frame t covers the samples [t shift, t shift + win), T = 1 + (N - win) /
// shift.  Log-energy of a frame (Kaldi's raw energy: after DC removal, before pre-emphasis and window, no dither): the
// samples on the int16 scale (int16 PCM as is, fp32 times 32768: exact, so both sources give the same bits), minus the
// frame's mean, E = sum d^2, loge = log(max(E, FLT_EPSILON)).  Two passes over the frame in LDS, mean first and then the
// squared deviations: sum x^2 - n mean^2 cancels in fp32 at this scale.
//
// tn_vad_log_energy: one workgroup owns `fpb` consecutive frames (tn_vad_frames_per_block) and stages the samples they
// cover through LDS once, converted.  Neighbouring frames overlap (2.5x at 25 / 10 ms), so each sample leaves HBM once,
// up to the win - shift samples two neighbouring workgroups share.  For shift < win the span is contiguous and is read
// in 16-byte vectors from the 16-byte boundary at or below its first sample; for shift >= win the frames are packed
// next to each other in LDS and the samples between them are never read.  A wave owns every fourth frame; lane l sums the
// samples l, l + 64, ... and the wave reduces by butterfly, so the order of every sum is fixed.  The workgroup's
// fp64 sum of its frames' loge goes to partials[block], summed in frame order by one thread.
//
// tn_vad_runs: thr = energy_threshold + mean_scale * sum(partials) / T in fp64; voiced[t] = (num >= den * proportion)
// with den the frames of [t - ctx, t + ctx] inside [0, T) and num those with loge > thr (compared and multiplied in fp64:
// the rule as a float64 restatement evaluates it); runs = the maximal intervals of voiced frames as (start, end) pairs in
// order.  Four launches, each ordered behind the one before by the stream alone — no workgroup waits on another:
//   1. one workgroup sums the partials (256 strided fp64 sums, then a fixed tree) and stores thr;
//   2. a workgroup per 1024 frames votes, writes voiced and counts the runs that START in its frames;
//   3. one workgroup turns the counts into exclusive offsets and the total;
//   4. a workgroup per 1024 frames writes the starts and the ends of its frames: the i-th start and the i-th end
//      belong to the same run, and the ends in front of a workgroup's frames are the starts in front of them minus the
//      one run that is open across the boundary.
// No floating-point atomics anywhere: two calls give the same bits.
#include <float.h>

#include "common.h"

namespace tn {

constexpr int kVadMaxWin = 4096, kVadMaxCtx = 64;
constexpr int kVadLdsFloats = 12288;          // 48 KiB of staged samples per workgroup at the most
constexpr int kVadMaxFpb = 64;                // frames of one workgroup of tn_vad_log_energy at the most
constexpr int kVadUnroll = 4;                // frames a wave of tn_vad_log_energy sums side by side
constexpr int kVadRunFrames = 1024;           // frames of one workgroup of tn_vad_runs: 4 per thread
constexpr float kLogFltEpsilon = -15.942385152878742f;       // log(2^-23), rounded to fp32

static int vad_frames_per_block(int win, int shift) {
  const int ls = shift < win ? shift : win;                  // LDS distance of two neighbouring frames
  const int fit = 1 + (kVadLdsFloats - win) / ls;
  return fit < kVadMaxFpb ? fit : kVadMaxFpb;
}

template <typename T> struct VadWave;
template <> struct VadWave<int16_t> {
  static constexpr int V = 8;
  static __device__ __forceinline__ float one(const int16_t* x, long long k) { return (float)x[k]; }
  static __device__ __forceinline__ void vec(const int16_t* p, float* out) {
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      out[2 * i] = (float)(int16_t)(w[i] & 0xffffu);
      out[2 * i + 1] = (float)(int16_t)(w[i] >> 16);
    }
  }
};
template <> struct VadWave<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ float one(const float* x, long long k) { return x[k] * 32768.f; }
  static __device__ __forceinline__ void vec(const float* p, float* out) {
    const float4 raw = *reinterpret_cast<const float4*>(p);
    out[0] = raw.x * 32768.f, out[1] = raw.y * 32768.f, out[2] = raw.z * 32768.f, out[3] = raw.w * 32768.f;
  }
};

// LDS: xs [span + 16] staged samples, then les [fpb] the workgroup's loge
template <typename T>
__global__ __launch_bounds__(256) void vad_log_energy_kernel(const T* __restrict__ x, float* __restrict__ loge,
                                                             double* __restrict__ partials, long long n,
                                                             long long frames, int win, int shift, int fpb, int span) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  float* les = xs + span + 16;
  constexpr int V = VadWave<T>::V;
  const long long f0 = (long long)blockIdx.x * fpb;
  const int nf = (int)(frames - f0 < fpb ? frames - f0 : fpb);
  const long long base = f0 * shift;
  int lead = 0, ls = win;
  if (shift < win) {
    // contiguous span [base, base + (nf - 1) shift + win), all below n; read from the 16-byte boundary at or below it
    ls = shift;
    lead = (int)(((uintptr_t)(x + base) / sizeof(T)) & (V - 1));
    const long long start = base - lead;
    const int total = lead + (nf - 1) * shift + win;           // <= span + V - 1
    for (int g = threadIdx.x * V; g < total; g += 256 * V) {
      const long long k = start + g;
      if (k >= 0 && k + V <= n) {
        float v[V];
        VadWave<T>::vec(x + k, v);
#pragma unroll
        for (int j = 0; j < V; ++j) xs[g + j] = v[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) xs[g + j] = (k + j >= 0 && k + j < n) ? VadWave<T>::one(x, k + j) : 0.f;
      }
    }
  } else {
    for (int s = threadIdx.x; s < nf * win; s += 256) {
      const int f = s / win;
      xs[s] = VadWave<T>::one(x, base + (long long)f * shift + (s - f * win));     // < n: frame f0 + f exists
    }
  }
  __syncthreads();
  // a wave takes kVadUnroll of its frames at a time: their sums are independent, so the reductions' latencies overlap;
  // every frame's own arithmetic and order are those of one frame at a time (a frame past the last repeats the last)
  const int lane = threadIdx.x & 63;
  for (int f = threadIdx.x >> 6; f < nf; f += 4 * kVadUnroll) {
    const float* fr[kVadUnroll];
    float s[kVadUnroll], e[kVadUnroll];
#pragma unroll
    for (int u = 0; u < kVadUnroll; ++u) {
      const int fu = f + 4 * u < nf ? f + 4 * u : nf - 1;
      fr[u] = xs + lead + fu * ls;
      s[u] = 0.f, e[u] = 0.f;
    }
    for (int j = lane; j < win; j += 64) {
#pragma unroll
      for (int u = 0; u < kVadUnroll; ++u) s[u] += fr[u][j];
    }
#pragma unroll
    for (int u = 0; u < kVadUnroll; ++u) s[u] = wave_sum(s[u]) / (float)win;        // the frame's mean
    for (int j = lane; j < win; j += 64) {
#pragma unroll
      for (int u = 0; u < kVadUnroll; ++u) {
        const float d = fr[u][j] - s[u];
        e[u] = fmaf(d, d, e[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kVadUnroll; ++u) {
      const float sum = wave_sum(e[u]);
      const float le = sum <= FLT_EPSILON ? kLogFltEpsilon : logf(sum);
      if (lane == 0 && f + 4 * u < nf) {
        loge[f0 + f + 4 * u] = le;
        les[f + 4 * u] = le;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = 0.0;
    for (int f = 0; f < nf; ++f) p += (double)les[f];
    partials[blockIdx.x] = p;
  }
}

// ---------------------------------------------------------------------------------------------------- runs
// exclusive scan of one int per thread over a workgroup of 256; `sm` holds 4 ints; -> (the scan, the total in `total`)
__device__ __forceinline__ int block_scan_excl(int v, int* sm, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();
  if (lane == 63) sm[w] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    before += i < w ? sm[i] : 0;
    total += sm[i];
  }
  return before + inc - v;
}

__global__ __launch_bounds__(256) void vad_threshold_kernel(const double* __restrict__ partials, long long n_partials,
                                                            long long frames, double energy_threshold,
                                                            double mean_scale, double* __restrict__ thr) {
  __shared__ double sm[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n_partials; i += 256) s += partials[i];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) thr[0] = energy_threshold + mean_scale * (sm[0] / (double)frames);
}

__global__ __launch_bounds__(256) void vad_vote_kernel(const float* __restrict__ loge, long long frames,
                                                       const double* __restrict__ thr_p, int ctx, double proportion,
                                                       unsigned char* __restrict__ voiced, int* __restrict__ counts) {
  // frames t0 - 1 .. t0 + 1024 are voted on (the neighbours decide where runs start), so the flags cover ctx more
  __shared__ unsigned char flag[kVadRunFrames + 2 + 2 * kVadMaxCtx];
  __shared__ unsigned char vote[kVadRunFrames + 2];
  __shared__ int sm[4];
  const double thr = thr_p[0];
  const long long t0 = (long long)blockIdx.x * kVadRunFrames;
  const int nflag = kVadRunFrames + 2 + 2 * ctx;
  for (int i = threadIdx.x; i < nflag; i += 256) {
    const long long t = t0 - 1 - ctx + i;
    flag[i] = (t >= 0 && t < frames && (double)loge[t] > thr) ? 1 : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kVadRunFrames + 2; i += 256) {
    const long long t = t0 - 1 + i;
    unsigned char v = 0;
    if (t >= 0 && t < frames) {
      const long long lo = t - ctx < 0 ? 0 : t - ctx, hi = t + ctx > frames - 1 ? frames - 1 : t + ctx;
      int num = 0;
      for (long long u = lo; u <= hi; ++u) num += flag[(int)(u - t0 + 1 + ctx)];
      v = (double)num >= (double)(hi - lo + 1) * proportion ? 1 : 0;
      if (i >= 1 && i <= kVadRunFrames) voiced[t] = v;
    }
    vote[i] = v;
  }
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 1 + threadIdx.x * 4 + j;           // a frame outside [0, frames) votes 0
    c += vote[i] && !vote[i - 1];
  }
  int total;
  block_scan_excl(c, sm, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void vad_offsets_kernel(const int* __restrict__ counts, int* __restrict__ offsets,
                                                          int nb, int* __restrict__ count) {
  __shared__ int sm[4];
  int carry = 0;
  for (int c0 = 0; c0 < nb; c0 += 256) {
    const int i = c0 + threadIdx.x;
    int total;
    const int ex = block_scan_excl(i < nb ? counts[i] : 0, sm, total);
    if (i < nb) offsets[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) count[0] = carry;
}

__global__ __launch_bounds__(256) void vad_emit_kernel(const unsigned char* __restrict__ voiced, long long frames,
                                                       const int* __restrict__ offsets, int* __restrict__ runs,
                                                       long long capacity) {
  __shared__ unsigned char vote[kVadRunFrames + 2];
  __shared__ int sm[4];
  const long long t0 = (long long)blockIdx.x * kVadRunFrames;
  for (int i = threadIdx.x; i < kVadRunFrames + 2; i += 256) {
    const long long t = t0 - 1 + i;
    vote[i] = (t >= 0 && t < frames) ? voiced[t] : 0;
  }
  __syncthreads();
  int c = 0;                                         // starts in the low half, ends in the high half (<= 1024 each)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 1 + threadIdx.x * 4 + j;
    c += (vote[i] && !vote[i - 1]) + ((vote[i] && !vote[i + 1]) << 16);
  }
  int total;
  const int ex = block_scan_excl(c, sm, total);
  const int first = offsets[blockIdx.x];
  long long rs = first + (ex & 0xffff);
  long long re = first - (vote[0] && vote[1]) + (ex >> 16);          // one run is open across the boundary
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 1 + threadIdx.x * 4 + j;
    const long long t = t0 - 1 + i;
    if (vote[i] && !vote[i - 1]) {
      if (rs < capacity) runs[2 * rs] = (int)t;
      ++rs;
    }
    if (vote[i] && !vote[i + 1]) {
      if (re < capacity) runs[2 * re + 1] = (int)(t + 1);
      ++re;
    }
  }
}

static long long vad_frames(long long n, int win, int shift) { return n < win ? 0 : 1 + (n - win) / shift; }

}  // namespace tn

using namespace tn;

extern "C" {

// frames one workgroup of tn_vad_log_energy owns: partials holds ceil(T / this) doubles.  -1 outside the limits.
int tn_vad_frames_per_block(int win, int shift) {
  if (win < 1 || win > kVadMaxWin || shift < 1) return -1;
  return vad_frames_per_block(win, shift);
}

// bytes of tn_vad_runs' workspace for T frames (thr, then the counts and the offsets of every 1024 frames); -1 for T
// outside [0, 2^31)
long long tn_vad_runs_workspace_bytes(long long T) {
  if (T < 0 || T > 0x7fffffffLL) return -1;
  const long long nb = (T + kVadRunFrames - 1) / kVadRunFrames;
  return 8 + 8 * (nb > 0 ? nb : 1);
}

int tn_vad_log_energy(const void* x, int x_is_pcm16, float* loge, double* partials, long long n, int win, int shift,
                      void* stream) {
  if (win < 1 || win > kVadMaxWin || shift < 1 || n < 0) return TN_EINVAL;
  const long long T = vad_frames(n, win, shift);
  if (T > 0x7fffffffLL) return TN_EINVAL;
  if (T == 0) return TN_OK;
  const uintptr_t elem = x_is_pcm16 ? 2 : 4;
  if (x == nullptr || loge == nullptr || partials == nullptr || (const void*)loge == x || ((uintptr_t)x & (elem - 1)) ||
      ((uintptr_t)loge & 3) || ((uintptr_t)partials & 7))
    return TN_EINVAL;
  const int fpb = vad_frames_per_block(win, shift);
  const int ls = shift < win ? shift : win;
  const int span = (fpb - 1) * ls + win;                      // <= kVadLdsFloats
  const long long blocks = (T + fpb - 1) / fpb;
  const dim3 grid((unsigned)blocks), block(256);
  const size_t lds = (size_t)(span + 16 + fpb) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (x_is_pcm16)
    hipLaunchKernelGGL(vad_log_energy_kernel<int16_t>, grid, block, lds, st, (const int16_t*)x, loge, partials, n, T,
                       win, shift, fpb, span);
  else
    hipLaunchKernelGGL(vad_log_energy_kernel<float>, grid, block, lds, st, (const float*)x, loge, partials, n, T, win,
                       shift, fpb, span);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

int tn_vad_runs(const float* loge, long long T, const double* partials, long long n_partials, double energy_threshold,
                double mean_scale, int ctx, double proportion, unsigned char* voiced_u8, int* runs, int* count,
                long long capacity, void* workspace, void* stream) {
  if (T < 0 || T > 0x7fffffffLL || ctx < 0 || ctx > kVadMaxCtx || !(proportion > 0.0 && proportion <= 1.0) ||
      !(energy_threshold == energy_threshold) || !(mean_scale == mean_scale) || capacity < T / 2 + 1 || count == nullptr ||
      ((uintptr_t)count & 3))
    return TN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (T == 0) {
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int), st);
    return e == hipSuccess ? TN_OK : (int)e;
  }
  if (loge == nullptr || partials == nullptr || n_partials < 1 || voiced_u8 == nullptr || runs == nullptr ||
      workspace == nullptr || ((uintptr_t)loge & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)runs & 3) ||
      ((uintptr_t)workspace & 7))
    return TN_EINVAL;
  const int nb = (int)((T + kVadRunFrames - 1) / kVadRunFrames);
  double* thr = (double*)workspace;
  int* counts = (int*)(thr + 1);
  int* offsets = counts + nb;
  hipLaunchKernelGGL(vad_threshold_kernel, dim3(1), dim3(256), 0, st, partials, n_partials, T, energy_threshold,
                     mean_scale, thr);
  TN_LAUNCH_CHECK();
  hipLaunchKernelGGL(vad_vote_kernel, dim3((unsigned)nb), dim3(256), 0, st, loge, T, (const double*)thr, ctx, proportion,
                     voiced_u8, counts);
  TN_LAUNCH_CHECK();
  hipLaunchKernelGGL(vad_offsets_kernel, dim3(1), dim3(256), 0, st, (const int*)counts, offsets, nb, count);
  TN_LAUNCH_CHECK();
  hipLaunchKernelGGL(vad_emit_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const unsigned char*)voiced_u8, T,
                     (const int*)offsets, runs, capacity);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
