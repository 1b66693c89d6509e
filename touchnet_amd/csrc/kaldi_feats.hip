// Kaldi log-fbank and MFCC at any sample rate and frame geometry: the `audio_compute_fbank` / `audio_compute_mfcc` stages,
// touchnet/data/functions.py:117-156 (`torchaudio.compliance.kaldi.fbank` / `.mfcc`, snip_edges, dither 0, waveform * 32768,
// use_energy false).  The one Kaldi feature kernel: the recipes' 16 kHz 25 ms / 10 ms fbank is one geometry among the rest.
//
// Per frame f (one workgroup of 256 threads, grid-stride over the frames):
//     x[n]   = wav[f shift + n] * 32768,  n < win                       win = int(sr frame_length_ms / 1000)
//     x     -= mean(x)
//     y[n]   = (x[n] - 0.97 x[max(n - 1, 0)]) * window[n]               Povey window, from the host
//     Y      = FFT_padded(y, zeros)                                     padded = next power of two >= win, radix 2 in LDS
//     p[k]   = |Y[k]|^2,  k < padded / 2                                (the Nyquist bin carries no mel weight)
//     e[b]   = sum_j bank_w[off_b + j] p[first_b + j],  j < count_b     sparse mel triangles, from the host
//     lm[b]  = log(max(e[b], FLT_EPSILON))                              -> the fbank row [num_mel_bins]
//     c[k]   = sum_b dct[k][b] lm[b]                                    -> the MFCC row [num_ceps]; dct = lifter . DCT-II
// Both output modes are ONE template: everything down to lm[] in LDS is the same code with contraction off and every fused
// multiply-add written out, so the fbank rows of the two modes carry the same bits; the sums run in ascending index order.
//
// The tables (touchnet_amd/functional.py::kaldi_feature_tables, float64 rounded to float32) are read-only device memory.
// Every index taken from them is checked against the LDS / table extent before it is used, so that a table that does not
// belong to the geometry cannot make the kernel read outside its buffers.
//
// LDS (dynamic, 4.5 padded + 260 floats = 37.9 KB at padded 2048, 10.2 KB at 512): re / im [padded] each, twiddle cos / sin
// [padded / 2] each, window [padded], power [padded / 2], log energies [256], 4 floats for the block sum.
#include "common.h"
#include <float.h>

namespace tn {

constexpr int kFeatThreads = 256, kFeatMaxPadded = 2048, kFeatMinPadded = 32, kFeatMaxBins = 256, kFeatGridCap = 2048;

template <bool MFCC>
__global__ __launch_bounds__(256) void kaldi_feats_kernel(const float* __restrict__ wav, float* __restrict__ out,
                                                          const float* __restrict__ window,
                                                          const int* __restrict__ bank_idx,
                                                          const float* __restrict__ bank_w,
                                                          const float* __restrict__ dct, int n_frames, int win, int shift,
                                                          int log2p, int n_mels, int n_ceps, int n_bank_w) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int P = 1 << log2p, half = P >> 1;
  float* re = lds;
  float* im = re + P;
  float* twc = im + P;
  float* tws = twc + half;
  float* wn = tws + half;
  float* pw = wn + P;
  float* lm = pw + half;
  float* red = lm + kFeatMaxBins;
  const int tid = threadIdx.x;
  for (int k = tid; k < half; k += kFeatThreads) {  // per-workgroup constants: e^{-2 pi i k / P}
    float s, c;
    sincospif(2.f * (float)k / (float)P, &s, &c);
    twc[k] = c;
    tws[k] = -s;
  }
  for (int n = tid; n < win; n += kFeatThreads) wn[n] = window[n];
  __syncthreads();

  for (int f = blockIdx.x; f < n_frames; f += gridDim.x) {
    const float* src = wav + (size_t)f * (size_t)shift;
    float part = 0.f;
    for (int n = tid; n < win; n += kFeatThreads) {
      const float x = src[n] * 32768.f;
      im[n] = x;  // raw samples parked in `im`
      part += x;
    }
    const float mean = block_sum(part, red) / (float)win;  // (contains the barriers that publish im[])
    for (int n = tid; n < P; n += kFeatThreads) {
      float y = 0.f;
      if (n < win) {
        const float cur = im[n] - mean;
        const float prev = (n > 0 ? im[n - 1] : im[0]) - mean;
        y = (cur - 0.97f * prev) * wn[n];
      }
      re[(int)(__brev((unsigned)n) >> (32 - log2p))] = y;
    }
    __syncthreads();
    for (int n = tid; n < P; n += kFeatThreads) im[n] = 0.f;
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s <= log2p; ++s) {
      const int hs = 1 << (s - 1);
      for (int b = tid; b < half; b += kFeatThreads) {  // butterflies of one stage touch disjoint pairs
        const int pos = b & (hs - 1);
        const int i = ((b >> (s - 1)) << s) + pos;
        const int j = i + hs;
        const int tw = pos << (log2p - s);
        const float c = twc[tw], sn = tws[tw];
        const float rj = re[j], ij = im[j];
        const float br = __builtin_fmaf(rj, c, -(ij * sn)), bi = __builtin_fmaf(rj, sn, ij * c);
        const float ar = re[i], ai = im[i];
        re[i] = ar + br;
        im[i] = ai + bi;
        re[j] = ar - br;
        im[j] = ai - bi;
      }
      __syncthreads();
    }
    for (int k = tid; k < half; k += kFeatThreads) pw[k] = __builtin_fmaf(re[k], re[k], im[k] * im[k]);
    __syncthreads();
    if (tid < n_mels) {
      const int first = bank_idx[3 * tid], count = bank_idx[3 * tid + 1], off = bank_idx[3 * tid + 2];
      float acc = 0.f;
      if (first >= 0 && count > 0 && first + count <= half && off >= 0 && off + count <= n_bank_w)
        for (int j = 0; j < count; ++j) acc = __builtin_fmaf(bank_w[off + j], pw[first + j], acc);
      const float v = logf(fmaxf(acc, FLT_EPSILON));
      if (MFCC)
        lm[tid] = v;
      else
        out[(size_t)f * n_mels + tid] = v;
    }
    if (MFCC) {
      __syncthreads();
      if (tid < n_ceps) {
        const float* row = dct + (size_t)tid * n_mels;
        float acc = 0.f;
        for (int b = 0; b < n_mels; ++b) acc = __builtin_fmaf(row[b], lm[b], acc);
        out[(size_t)f * n_ceps + tid] = acc;
      }
    }
    __syncthreads();  // the next frame overwrites im[] / lm[]
  }
}

}  // namespace tn

using namespace tn;

extern "C" {

int tn_kaldi_feats(const float* wav, float* out, long long n_samples, int sample_rate, int win, int shift, int padded,
                   int num_mel_bins, int num_ceps, float low_freq, float high_freq, const float* window,
                   const int* bank_idx, const float* bank_w, int n_bank_w, const float* dct, void* stream) {
  if (window == nullptr || bank_idx == nullptr || n_samples < 0 || sample_rate < 1 || shift < 1) return TN_EINVAL;
  if (padded < kFeatMinPadded || padded > kFeatMaxPadded || (padded & (padded - 1)) || win > padded || 2 * win <= padded)
    return TN_EINVAL;                                              // padded = the next power of two of win
  if (num_mel_bins < 4 || num_mel_bins > kFeatMaxBins || num_ceps < 0 || num_ceps > num_mel_bins) return TN_EINVAL;
  if (num_ceps > 0 && dct == nullptr) return TN_EINVAL;
  if (n_bank_w < 0 || n_bank_w > padded || (n_bank_w > 0 && bank_w == nullptr)) return TN_EINVAL;
  const float nyquist = 0.5f * (float)sample_rate;
  const float high = high_freq > 0.f ? high_freq : nyquist + high_freq;
  if (!(low_freq >= 0.f && low_freq < high && high <= nyquist)) return TN_EINVAL;
  const long long nf = n_samples < win ? 0 : 1 + (n_samples - win) / shift;   // snip_edges
  if (nf > 0x7fffffffLL) return TN_EINVAL;
  if (nf == 0) return TN_OK;                                       // (an empty output has no address to check)
  if (wav == nullptr || out == nullptr || (const void*)wav == (const void*)out) return TN_EINVAL;
  int log2p = 0;
  while ((1 << log2p) < padded) ++log2p;
  const size_t lds = (size_t)(4 * padded + padded / 2 + kFeatMaxBins + 4) * sizeof(float);
  const dim3 grid((unsigned)(nf < kFeatGridCap ? nf : kFeatGridCap)), block(kFeatThreads);
  hipStream_t st = (hipStream_t)stream;
  if (num_ceps > 0)
    hipLaunchKernelGGL(kaldi_feats_kernel<true>, grid, block, lds, st, wav, out, window, bank_idx, bank_w, dct, (int)nf,
                       win, shift, log2p, num_mel_bins, num_ceps, n_bank_w);
  else
    hipLaunchKernelGGL(kaldi_feats_kernel<false>, grid, block, lds, st, wav, out, window, bank_idx, bank_w, dct, (int)nf,
                       win, shift, log2p, num_mel_bins, num_ceps, n_bank_w);
  TN_LAUNCH_CHECK();
  return TN_OK;
}

}  // extern "C"
