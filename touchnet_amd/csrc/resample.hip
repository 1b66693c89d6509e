// Sample-rate conversion on the GPU: the `audio_resample` stage, touchnet/data/functions.py:83-96
// (`torchaudio.transforms.Resample(orig, new)(waveform)` with torchaudio's defaults: sinc_interp_hann,
// lowpass_filter_width 6, rolloff 0.99).
//
// torchaudio's algorithm is a closed formula — a Hann-windowed sinc evaluated per output phase and applied as a strided
// convolution over the zero-padded waveform — so, unlike libsox's speed perturbation (below), it can be restated
// exactly.  With o = orig / gcd, n = new / gcd, output m sits at input position (m o) / n: integer part i,
// phase r = (m o) mod n, and
//     y[m] = sum_j tab[r][j] * x[i - ntap / 2 + 1 + j],          x = 0 outside [0, n_in)
// where tab [n][ntap] holds the non-zero columns of torchaudio's kernel, rounded to float32 by the host
// (touchnet_amd/functional.py::sinc_resample_table).  The products are summed in the order j = 0 .. ntap - 1 by fused
// multiply-adds; the waveform is fp32 or int16 PCM read as v * 2^-15 (exact, so both sources give the same bits).
//
// One output per thread, `per` <= 256 outputs per workgroup.  The outputs of a workgroup read the samples
// [i(m0) - ntap / 2 + 1, i(m0 + per - 1) + ntap / 2], at most (per - 1) o / n + 2 + ntap of them; the workgroup stages
// that span through LDS once, converted, with the part outside [0, n_in) zero-filled, so the tap loop has neither bounds
// checks nor conversions and neighbouring outputs share their samples on chip.  Measured against the same sum read
// straight from global memory, one bounds-checked load per tap, the staging is 1.5x - 3x faster on 30 s clips
// (profiles/resample_bench_plain_vs_lds.log) and 3.4x - 4.0x on speed perturbation's 68 and 76 taps
// (profiles/frontend_one_kernel.log), so it is the one kernel: functional.py::speed_perturb runs on it with its own
// table, o / n = the speed p / q.
// Every position is 64-bit: m * o passes 2^31 after five minutes of 44.1 kHz audio.
//
// Speed perturbation, touchnet/data/functions.py:99-114: sox `speed s` + `rate sr` = the waveform resampled by the
// factor 1 / s (pitch and tempo change together).  libsox's polyphase resampler is a third-party binary algorithm that
// cannot be restated bit for bit, so the host builds the table of the band-limited interpolation
//     y[m] = sum_k x[k] h(m s - k),   h(t) = c sinc(c t) kaiser(t / W),  c = 0.95 min(1, 1 / s)
// in float64 for the rational speed p / q (functional.py::speed_filter_bank) and this kernel sums it.  PARITY UNPINNED
// against libsox (stated in DESIGN.md); held to a float64 evaluation of the same formula (oracle/frontend.py).
#include "common.h"

namespace tn {

template <typename T> __device__ __forceinline__ float wave_sample(const T* x, long long k);
template <> __device__ __forceinline__ float wave_sample<float>(const float* x, long long k) { return x[k]; }
template <> __device__ __forceinline__ float wave_sample<int16_t>(const int16_t* x, long long k) {
  return (float)x[k] * (1.f / 32768.f);
}

template <typename T>
__global__ __launch_bounds__(256) void resample_sinc_kernel(const T* __restrict__ x, float* __restrict__ y,
                                                            const float* __restrict__ tab, long long n_in,
                                                            long long n_out, int o, int n, int ntap, int per, int span) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const long long m0 = (long long)blockIdx.x * per;
  const long long i0 = (m0 * o) / n;
  const long long base = i0 - ntap / 2 + 1;
  for (int s = threadIdx.x; s < span; s += 256) {
    const long long k = base + s;
    xs[s] = (k >= 0 && k < n_in) ? wave_sample<T>(x, k) : 0.f;
  }
  __syncthreads();
  const long long m = m0 + threadIdx.x;
  if ((int)threadIdx.x >= per || m >= n_out) return;
  const long long pos = m * o;
  const long long i = pos / n;
  const int r = (int)(pos - i * n);
  const float* t = tab + (size_t)r * ntap;
  const float* w = xs + (int)(i - i0);        // i - i0 <= (per - 1) o / n + 1, so i - i0 + ntap - 1 < span
  float acc = 0.f;
  for (int j = 0; j < ntap; ++j) acc = fmaf(w[j], t[j], acc);
  y[m] = acc;
}

static int gcd_int(int a, int b) {
  while (b) {
    const int c = a % b;
    a = b, b = c;
  }
  return a;
}

}  // namespace tn

using namespace tn;

constexpr long long kLdsFloats = 12288;      // 48 KiB of staged samples per workgroup at the most

extern "C" {

// x [n_in] (fp32, or int16 PCM when x_is_pcm16) -> y [n_out] fp32 at new_ / orig times the rate;
// tab: device float [new_ / gcd(orig, new_)][ntap], ntap even.
int tn_resample_sinc(const void* x, int x_is_pcm16, float* y, const float* tab, long long n_in, long long n_out,
                     int orig, int new_, int ntap, void* stream) {
  if (x == nullptr || y == nullptr || tab == nullptr || n_in < 1 || n_out < 1 || orig < 1 || new_ < 1 || ntap < 2 ||
      (ntap & 1) || x == (const void*)y || ntap + 2 > kLdsFloats)
    return TN_EINVAL;
  const __int128 most = ((__int128)n_in * new_ + orig - 1) / orig;       // ceil(n_in new_ / orig)
  if ((__int128)n_out > most) return TN_EINVAL;
  const int g = gcd_int(orig, new_), o = orig / g, n = new_ / g;
  // outputs per workgroup: 256, or as many as keep the span (per - 1) o / n + 2 + ntap inside the LDS budget
  const long long room = kLdsFloats - 2 - ntap;
  const int per = 255LL * o / n <= room ? 256 : (int)(room * n / o) + 1;
  const long long span = (long long)(per - 1) * o / n + 2 + ntap;
  const long long blocks = (n_out + per - 1) / per;
  if (blocks > 0x7fffffffLL) return TN_EINVAL;
  const dim3 grid((unsigned)blocks), block(256);
  const size_t lds = (size_t)span * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (x_is_pcm16)
    hipLaunchKernelGGL(resample_sinc_kernel<int16_t>, grid, block, lds, st, (const int16_t*)x, y, tab, n_in, n_out, o,
                       n, ntap, per, (int)span);
  else
    hipLaunchKernelGGL(resample_sinc_kernel<float>, grid, block, lds, st, (const float*)x, y, tab, n_in, n_out, o, n,
                       ntap, per, (int)span);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
