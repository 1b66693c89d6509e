/* touchnet_amd — C ABI of the MI355X (gfx950) packed-sequence training kernels.
 *
 * One shared library, libtouchnet_amd.so (hipcc --offload-arch=gfx950), plain pointers and sizes,
 * no torch / C++ types.  This is the drop-in boundary: the reference is pure Python
 * (SURVEY.md §0 fact 1), so the binding a TouchNet maintainer adds is a ctypes stub — see
 * INTEGRATION.md and touchnet_amd/_C.py (the binding this repo ships).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless named host_*; buffers are dense row-major
 *   - `dtype`: 0 = float32, 1 = bfloat16 (raw uint16 bits)
 *   - `stream`: hipStream_t cast to void* (NULL = default stream); all entry points only ENQUEUE work
 *     on that stream, never synchronise, never allocate; safe under hipGraph capture and from
 *     autograd worker threads (no global mutable state)
 *   - return value: 0 on success, a positive hipError_t from the launch, or -22 (EINVAL) for
 *     unsupported arguments.  Callers must treat non-zero as fatal (the reference has no per-op
 *     recovery either: touchnet/bin/train.py:639-648)
 *   - ownership: the caller owns every buffer; outputs are fully overwritten unless stated
 */
#ifndef TOUCHNET_AMD_H_
#define TOUCHNET_AMD_H_

#ifdef __cplusplus
extern "C" {
#endif

/* ---- build identification -------------------------------------------------------------------- */
const char* tn_version(void);   /* "touchnet_amd <ver> gfx950" */

/* ---- RMSNorm (+ fused residual add)  — replaces LlamaRMSNorm / Qwen2RMSNorm forward+backward
 *      transformers/models/llama/modeling_llama.py:62-67 and the residual adds at :306-324,
 *      swapped in the way liger does at touchnet/models/llama/__init__.py:11-15.
 * fwd:  h = x (+ res_in);  res_out = h (if res_in);  y = w * T(h * rsqrt(mean(h^2) + eps));  rstd[rows] fp32
 * bwd:  dh = rmsnorm'(dy) (+ dres);  dw[H]     workspace: tn_norm_bwd_workspace_floats(rows, H) floats
 * -22 (before any launch) unless rows > 0, H > 0, H a multiple of the 16-byte vector (8 bf16 / 4 fp32), H <= 8192 (bf16) /
 * 4096 (fp32), dtype 0 (fp32) or 1 (bf16); the same contract holds for the LayerNorm entries. */
int tn_norm_bwd_workspace_floats(int rows, int H);
int tn_rmsnorm_fwd(const void* x, const void* res_in, const void* w, void* y, void* res_out, float* rstd,
                   int rows, int H, float eps, int dtype, void* stream);
int tn_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, void* dh,
                   void* dw, float* workspace, int rows, int H, int dtype, void* stream);

/* ---- LayerNorm (+ fused residual add) — Whisper-style encoder layers of the Qwen2-Audio tower
 *      (touchnet/models/qwen2_audio/__init__.py:18-133 drives transformers' Qwen2AudioEncoderLayer). */
int tn_layernorm_fwd(const void* x, const void* res_in, const void* w, const void* b, void* y, void* res_out,
                     float* mean, float* rstd, int rows, int H, float eps, int dtype, void* stream);
int tn_layernorm_bwd(const void* dy, const void* h, const void* w, const float* mean, const float* rstd,
                     const void* dres, void* dh, void* dw, void* db, float* workspace, int rows, int H, int dtype,
                     void* stream);

/* ---- SwiGLU / GELU — transformers/models/llama/modeling_llama.py:174-176; encoder fc1 activation
 *      -22 (before any launch) unless n >= 0, n a multiple of the 16-byte vector (8 bf16 / 4 fp32), dtype 0 or 1. */
int tn_swiglu_fwd(const void* gate, const void* up, void* out, long long n, int dtype, void* stream);
int tn_swiglu_bwd(const void* dout, const void* gate, const void* up, void* dgate, void* dup, long long n,
                  int dtype, void* stream);
/* bf16 variants that ALSO write the transposed tensors the MLP's weight-gradient GEMMs consume (rows, cols multiples
 * of 8): out_t [cols, rows] = out^T;  dgu_t [2*cols, rows] = [dgate^T ; dup^T].  Same arithmetic as the two above.
 * -22 (before any launch) unless rows > 0, cols > 0 and both are multiples of 8. */
int tn_swiglu_fwd_t(const void* gate, const void* up, void* out, void* out_t, int rows, int cols, void* stream);
int tn_swiglu_bwd_t(const void* dout, const void* gate, const void* up, void* dgate, void* dup, void* dgu_t, int rows,
                    int cols, void* stream);
int tn_gelu_fwd(const void* x, void* out, long long n, int dtype, void* stream);
int tn_gelu_bwd(const void* dout, const void* x, void* dx, long long n, int dtype, void* stream);

/* ---- RoPE from packed position_ids — transformers/models/llama/modeling_llama.py:113-160 with
 *      position_ids restarting per sentence (touchnet/models/llama/processing_llama.py:96-97).
 * table: cos/sin [n, half] in `dtype` = cos/sin(position_ids[n] * inv_freq[half]) * attention_scaling
 * apply: q [n, hq, D] -> q_out, k [n, hk, D] -> k_out (may alias; half-split rotate_half convention);
 *        backward = 1 applies the transpose rotation to gradients
 * -22 (before any launch) unless n > 0, half > 0 (table); n > 0, hq > 0, hk >= 0, D > 0 and even (apply); dtype 0 or 1. */
int tn_rope_table(const long long* position_ids, const float* inv_freq, void* cos_t, void* sin_t, int n, int half,
                  float attention_scaling, int dtype, void* stream);
int tn_rope_apply(const void* q, const void* k, void* q_out, void* k_out, const void* cos_t, const void* sin_t,
                  int n, int hq, int hk, int D, int backward, int dtype, void* stream);

/* ---- packed cross-entropy + accuracy — touchnet/loss/__init__.py:7-28,
 *      touchnet/loss/cross_entropy.py:12-50, touchnet/utils/metrics.py:26-50.
 * logits [n, V]; labels, sentence_lens int64 [n]; num_sentence, grad_out: device float[1]
 * forward: nll[n], lse[n] fp32, hit[n] int32, out[4] = {loss_per_sample, loss_per_token, accuracy, n_valid}
 * backward: dlogits (may alias logits) = (softmax - onehot) * grad_out / (sentence_lens * num_sentence) */
int tn_ce_forward(const void* logits, const long long* labels, const long long* sentence_lens,
                  const float* num_sentence, float* nll, float* lse, int* hit, float* out, int n, int V,
                  long long ignore_index, int dtype, void* stream);
int tn_ce_reduce(const float* nll, const int* hit, const long long* labels, const long long* sentence_lens,
                 const float* num_sentence, float* out, int n, long long ignore_index, void* stream);
int tn_ce_backward(const void* logits, void* dlogits, const long long* labels, const long long* sentence_lens,
                   const float* lse, const float* num_sentence, const float* grad_out, int n, int V,
                   long long ignore_index, int dtype, void* stream);

/* ---- packed (document-masked causal) attention — replaces flex_attention / SDPA
 *      (transformers/integrations/flex_attention.py:190-201,264-340 as selected by
 *      "attn_implementation": "flex_attention", examples/text/pretrain/fineweb-edu/config/Llama-3_2-1B.json:7;
 *      mask built from the packers' document ids, touchnet/models/llama/processing_llama.py:38-40).
 * q [B,T,Nh,D], k/v [B,T,Nkv,D], o [B,T,Nh,D] bf16, D in {64,128}; doc int32 [B,T] (0 = pad);
 * lse2, delta fp32 [B,Nh,T]; meta: int32[tn_attn_meta_ints(B,T)] filled by tn_attn_build_meta once per batch */
int tn_attn_meta_ints(int B, int T);
int tn_attn_build_meta(const int* doc, int* meta, int B, int T, void* stream);
int tn_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc, const int* meta,
                int B, int T, int Nh, int Nkv, int D, float scale, void* stream);
int tn_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2,
                float* delta, void* dq, void* dk, void* dv, const int* doc, const int* meta, int B, int T, int Nh,
                int Nkv, int D, float scale, void* stream);
/* tn_attn_bwd for q / k that carry the rotary embedding (tn_gemm_bf16_rope's epilogue or tn_rope_apply put it there): dq / dk
 * are returned as gradients of the UN-rotated projections — tn_attn_bwd followed by tn_rope_apply(dq, dk, backward = 1), bit
 * for bit, with the transposed rotation done in the backward kernels' epilogues (D = 128) instead of one more pass over
 * dq / dk.  Replaces the autograd backward of transformers' apply_rotary_pos_emb inside the reference's decoder layers
 * (modeling_qwen2.py Qwen2Attention.forward as patched by touchnet/models/llama/__init__.py:11-15; flex_attention's
 * backward at touchnet/models/llama/parallelize_llama.py).  cos_t / sin_t: bf16 [B * T, D / 2] from tn_rope_table. */
int tn_attn_bwd_rope(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2,
                     float* delta, void* dq, void* dk, void* dv, const int* doc, const int* meta, int B, int T, int Nh,
                     int Nkv, int D, float scale, const void* cos_t, const void* sin_t, void* stream);
/* The same pair with the mask BIDIRECTIONAL inside a document (allowed = same positive document id; no causal term):
 * transformers' WhisperEncoder layers, which the reference's Kimi-Audio speech encoder runs on every 30 s clip
 * (touchnet/models/kimi_audio/modeling_kimi_audio.py:933-960; one clip = one document).  Same tensors, same metadata. */
int tn_attn_fwd_bidir(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc, const int* meta,
                      int B, int T, int Nh, int Nkv, int D, float scale, void* stream);
int tn_attn_bwd_bidir(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2,
                      float* delta, void* dq, void* dk, void* dv, const int* doc, const int* meta, int B, int T, int Nh,
                      int Nkv, int D, float scale, void* stream);

/* Sequence-sharded query side — context parallelism (replaces torch's experimental ring-attention CP that the
 * reference enters at touchnet/utils/distributed.py:292-346 / touchnet/bin/train.py:354-389, which intercepts
 * SDPA only and cannot carry the document mask).  q/o/dout/dq are [B, rows_per_batch, Nh, D] and lse2/delta
 * [B, Nh, rows_per_batch]: segment i = local rows [row0_i, row0_i+rows_i) holding GLOBAL positions
 * [off_i, off_i+rows_i) (head/tail load balancing = 2 segments per rank); `segs` = host int[6]
 * {row0_a, rows_a, off_a, row0_b, rows_b, off_b}.  k/v/doc/meta are global ([B, T, ...], all-gathered by the
 * caller); dk/dv come back as this rank's partial sums over [B, T, Nkv, D] for the caller to reduce-scatter.
 * The segment contract, checked on the host by all three *_seg* entry points (TN_EINVAL, nothing is launched):
 *   - nseg is 1 or 2, host_segs is not null, rows_per_batch > 0; every segment has rows > 0, row0 >= 0, off >= 0,
 *     off + rows <= T and row0 + rows <= rows_per_batch;
 *   - row0 and off are multiples of 128, and so is rows of every segment but the last, which may have any length (a
 *     contiguous split's last shard, a ragged T);
 *   - two segments overlap neither in their local rows nor in their global positions.  They need not be equal, adjacent
 *     or in ascending order, and one segment {0, T, 0} with rows_per_batch = T is the plain tn_attn_fwd / tn_attn_bwd.
 * Local rows that no segment covers are neither read nor written (o, lse2, delta and dq keep what they held).  dk / dv
 * are written for all T rows: rows that no local query may see come back as zeros. */
int tn_attn_fwd_seg(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                    const int* meta, int B, int T, int Nh, int Nkv, int D, float scale, int nseg,
                    const int* host_segs, int rows_per_batch, void* stream);
/*      Key side restricted to the sequence chunks whose bit is set in `chunk_mask` (chunk c = positions
 *      [c*chunk_len, (c+1)*chunk_len), chunk_len % 64 == 0, at most 64 chunks): rows that see no key there get
 *      O = 0, LSE2 = +inf.  With tn_attn_merge this is the local / remote split of context-parallel attention: the
 *      own-chunk part runs while the halo travels (replaces the per-step (out, lse) merge of torch's ring attention,
 *      torch/distributed/tensor/experimental/_context_parallel/_attention.py:182-183 entered from
 *      touchnet/utils/distributed.py:292-315). */
int tn_attn_fwd_seg_chunks(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc,
                           const int* meta, int B, int T, int Nh, int Nkv, int D, float scale, int nseg, const int* segs,
                           int rows_per_batch, int chunk_len, unsigned long long chunk_mask, void* stream);
/*      lse = log2(2^lse_a + 2^lse_b), O = (2^lse_a O_a + 2^lse_b O_b) / 2^lse for two partial results over DISJOINT key
 *      sets; o may alias o_a, lse2 may alias lse2_a.  o_* [B, rows, Nh, D] bf16, lse2_* [B, Nh, rows] fp32. */
int tn_attn_merge(const void* o_a, const float* lse2_a, const void* o_b, const float* lse2_b, void* o, float* lse2,
                  int B, int rows, int Nh, int D, void* stream);
int tn_attn_bwd_seg(const void* q, const void* k, const void* v, const void* o, const void* dout,
                    const float* lse2, float* delta, void* dq, void* dk, void* dv, const int* doc, const int* meta,
                    int B, int T, int Nh, int Nkv, int D, float scale, int nseg, const int* host_segs,
                    int rows_per_batch, void* stream);

/* ---- audio frontend on device — touchnet/data/functions.py:159-190 (whisper log-mel), :258-286 (stack / stride /
 *      normalise); Kaldi fbank / MFCC (:117-156) is tn_kaldi_feats below, at any sample rate and frame geometry.
 * logmel: wav fp32 [n_samples] -> feat fp32 [n_samples/160, n_mels]; `mel_fb` = slaney filter bank
 *         fp32 [n_mels, 201] supplied by the host (it is a constant table)
 * stack:  feat fp32 [T, F] -> out fp32 [ceil(T/stride), F*stack], optional per-row normalisation */
int tn_log_mel(const float* wav, const float* mel_fb, float* feat, float* scratch_max, int n_samples, int n_mels,
               void* stream);
int tn_audiofeat_stack(const float* feat, float* out, int T, int F, int stack, int stride, int normalize,
                       void* stream);
/* Feature-level augmentation of the reference's datapipe, touchnet/data/functions.py:193-255 (audiofeat_spec_aug,
 * audiofeat_spec_sub, audiofeat_spec_trim), applied in ONE gather pass: x [T, F] -> y [out_rows, F].  The random draws
 * are the caller's (host arrays): t_masks / f_masks = n x [start, end) stripes set to zero, subs = n x (start, end, pos):
 * rows [start, end) take rows [start - pos, end - pos) of x (later entries win), out_rows <= T drops the tail.  At most 16
 * entries each; y must not alias x. */
int tn_feat_augment(const float* x, float* y, int T, int F, int out_rows, const int* t_masks, int n_t,
                    const int* f_masks, int n_f, const int* subs, int n_sub, void* stream);
/* Sample-rate conversion, touchnet/data/functions.py:83-96 (`torchaudio.transforms.Resample(orig, new)`, torchaudio's
 * defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): x [n_in] -> y [n_out] fp32.  With o = orig / gcd,
 * n = new_ / gcd, output m sits at input position m o / n (integer part i, phase r = (m o) mod n) and
 * y[m] = sum_j tab[r][j] x[i - ntap / 2 + 1 + j], x = 0 outside [0, n_in); tab: device float [n][ntap], torchaudio's
 * kernel in float32 without its zero columns (touchnet_amd/functional.py::sinc_resample_table).  x is fp32, or int16 PCM
 * read as v * 2^-15 when x_is_pcm16 (exact: the same bits as converting first).  One launch, no allocation, no
 * synchronisation; all index arithmetic is 64-bit.
 * Waveform-level speed perturbation, touchnet/data/functions.py:99-114 (sox `speed s` + `rate`), is the same sum with
 * orig / new_ = the speed p / q and the band-limited interpolation table tab [q][ntap] of
 * touchnet_amd/functional.py::speed_filter_bank.  Not bit-comparable with libsox.
 * -22 (before any launch) for a null pointer, y == x, n_in < 1, n_out outside [1, ceil(n_in new_ / orig)], orig < 1,
 * new_ < 1, ntap < 2, odd or above 12286 (a workgroup stages the samples of its outputs, ntap of them for one, in
 * 48 KiB of LDS). */
int tn_resample_sinc(const void* x, int x_is_pcm16, float* y, const float* tab, long long n_in, long long n_out,
                     int orig, int new_, int ntap, void* stream);
/* Kaldi log-fbank / MFCC at any sample rate and frame geometry, touchnet/data/functions.py:117-156
 * (`torchaudio.compliance.kaldi.fbank` / `.mfcc`: snip_edges, dither 0, waveform * 32768, DC removal, pre-emphasis 0.97,
 * Povey window, power spectrum of the frame zero-padded to `padded`, mel triangles in 1127 ln(1 + f / 700),
 * log(max(e, FLT_EPSILON)); use_energy false).  wav fp32 [n_samples] in [-1, 1) -> out fp32 [frames, C],
 * frames = n_samples < win ? 0 : 1 + (n_samples - win) / shift; C = num_mel_bins when num_ceps == 0 (fbank rows),
 * else num_ceps (MFCC rows: out = dct . log energies).  The fbank rows behind both modes carry the same bits.
 * Tables, device memory, built by touchnet_amd/functional.py::kaldi_feature_tables in float64 and rounded to float32:
 *   window   float [win]                      the Povey window
 *   bank_idx int   [num_mel_bins][3]          (first FFT bin, count, offset into bank_w) of each mel triangle's
 *                                             non-zero weights; count 0 = no FFT bin inside it: log(FLT_EPSILON)
 *   bank_w   float [n_bank_w]                 the non-zero weights, packed; n_bank_w <= padded
 *   dct      float [num_ceps][num_mel_bins]   lifter[k] * DCT-II[k][n], orthonormal (row 0 sqrt(1/N), row k
 *                                             sqrt(2/N) cos(pi/N (n + 1/2) k)), lifter 1 + 11 sin(pi k / 22); MFCC only
 * sample_rate, low_freq and high_freq (<= 0: offset from Nyquist) are checked, not used: the tables carry them.
 * One launch (none for 0 frames), no allocation, no synchronisation.
 * -22 (before any launch) unless: padded a power of two in [32, 2048] with padded / 2 < win <= padded; shift >= 1;
 * 4 <= num_mel_bins <= 256; 0 <= num_ceps <= num_mel_bins; 0 <= low_freq < high <= sample_rate / 2;
 * 0 <= n_bank_w <= padded; no null table that the mode reads; frames < 2^31; with at least one frame, wav and out
 * non-null and out != wav. */
int tn_kaldi_feats(const float* wav, float* out, long long n_samples, int sample_rate, int win, int shift, int padded,
                   int num_mel_bins, int num_ceps, float low_freq, float high_freq, const float* window,
                   const int* bank_idx, const float* bank_w, int n_bank_w, const float* dct, void* stream);
/* Voice-activity detection for recordings longer than one utterance: the energy rule of Kaldi's `compute-vad-energy`.
 * This goes beyond the reference, whose inference scripts cut every waveform at 30 s
 * (touchnet/models/qwen2_audio/inference_qwen2_audio.py:101, touchnet/models/kimi_audio/processing_kimi_audio.py:73).
 * Framing as tn_kaldi_feats: frame t = samples [t shift, t shift + win), T = n < win ? 0 : 1 + (n - win) / shift.
 * vad_log_energy: x [n] fp32 in [-1, 1) or int16 PCM (x_is_pcm16) -> loge fp32 [T] = log(max(sum_j (s_j - mean)^2,
 *      FLT_EPSILON)) over the frame's samples s on the int16 scale (int16 as is, fp32 times 32768: the same bits), mean
 *      first and squared deviations second, in fp32 in a fixed order; a frame of equal samples is log(FLT_EPSILON)
 *      exactly.  partials double [ceil(T / tn_vad_frames_per_block(win, shift))]: each workgroup's fp64 sum of its frames'
 *      loge.  A workgroup stages the samples of its frames through LDS once; all sample positions are 64-bit.  One
 *      launch (none for T == 0, whatever the pointers), no allocation, no synchronisation.
 *      -22 before any launch for win outside [1, 4096], shift < 1 (shift > win is legal), n < 0, T >= 2^31, and with
 *      T > 0 a NULL pointer, loge == x, or x / loge / partials not aligned to their elements.
 * vad_runs: thr = energy_threshold + mean_scale * sum(partials[0 .. n_partials)) / T (fp64, fixed order); for every t,
 *      den = the frames of [t - ctx, t + ctx] inside [0, T), num = those with loge > thr, voiced_u8[t] = (num >=
 *      den * proportion), evaluated in fp64; runs int [capacity][2] = the maximal intervals of voiced frames as ordered
 *      (start, end) pairs, end exclusive, count[0] their number; rows from count on are not written.  loge is an input:
 *      any decision pattern can be handed in, with partials = {its sum}.  workspace: tn_vad_runs_workspace_bytes(T)
 *      bytes, 8-byte aligned.  Four launches ordered by the stream (threshold; vote and per-workgroup run counts;
 *      exclusive scan; starts and ends): no workgroup waits on another, no floating-point atomics, bit-identical repeats.
 *      T == 0: count[0] = 0, nothing else is read or written.
 *      -22 before any launch for T outside [0, 2^31), ctx outside [0, 64], proportion outside (0, 1], a NaN threshold or
 *      scale, capacity < T / 2 + 1, count NULL, and with T > 0 any other NULL or misaligned pointer or n_partials < 1.
 * tn_vad_frames_per_block: the frames one workgroup of vad_log_energy owns (at most 64; fewer when their samples pass
 *      48 KiB of LDS); -1 outside the limits of win and shift.  tn_vad_runs_workspace_bytes: -1 for T outside [0, 2^31). */
int tn_vad_frames_per_block(int win, int shift);
long long tn_vad_runs_workspace_bytes(long long T);
int tn_vad_log_energy(const void* x, int x_is_pcm16, float* loge, double* partials, long long n, int win, int shift,
                      void* stream);
int tn_vad_runs(const float* loge, long long T, const double* partials, long long n_partials, double energy_threshold,
                double mean_scale, int ctx, double proportion, unsigned char* voiced_u8, int* runs, int* count,
                long long capacity, void* workspace, void* stream);

/* ---- fused AdamW on fp32 master weights with bf16 shadow write-back and device-side
 *      skip-on-nonfinite — touchnet/utils/optimizer.py:157-172 + touchnet/bin/train.py:458-474.
 * step 1: tn_sumsq accumulates sum(g^2) of one (flat) tensor into norm_sq[0] (fp32, zeroed by the caller);
 *         deterministic two-stage reduction through `scratch` (tn_sumsq_scratch_floats() floats)
 * step 2: tn_adamw_step updates p/m/v (fp32) from g, scaling g by min(1, max_norm/(sqrt(norm_sq)+1e-6));
 *         if norm_sq is NaN/Inf nothing is written (the reference skips the step, train.py:467-473)
 * -22 (before any launch) unless n > 0 and the (gradient) dtype is 0 (fp32) or 1 (bf16); tn_sumsq ADDS to norm_sq[0]. */
int tn_sumsq_scratch_floats(void);
int tn_sumsq(const void* g, float* scratch, float* norm_sq, long long n, int dtype, void* stream);
/* multi-tensor step 1 (one launch for all gradient tensors of one dtype): device tables ptrs[t], sizes[t]
 * (elements), first_chunk[t] = sum_{u<t} ceil(sizes[u] / tn_sumsq_multi_chunk()); partial: nchunks floats.
 * ADDS to norm_sq[0].  -22 (before any launch) unless ntensors > 0, 0 < nchunks < 2^31, dtype 0 or 1. */
long long tn_sumsq_multi_chunk(void);
int tn_sumsq_multi(const void* const* ptrs, const long long* sizes, const long long* first_chunk, int ntensors,
                   long long nchunks, float* partial, float* norm_sq, int dtype, void* stream);
int tn_adamw_step(float* p, float* m, float* v, const void* g, void* p_shadow_bf16, const float* norm_sq,
                  long long n, float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                  float bias_corr1, float bias_corr2, int g_dtype, void* stream);

/* multi-tensor step 2 (one launch per gradient dtype for ALL parameters — FSDP shards are 1/N of each tensor, a launch
 * per tensor would dominate).  tn_adamw_prepare turns norm_sq into the device-side step state (8 floats owned by the
 * caller, zeroed once): step count — advanced only when the norm is finite, like torch's AdamW on a skipped step —
 * bias corrections, clip coefficient, skip flag; no host round trip.  Tables as in tn_sumsq_multi with
 * first_chunk over tn_adamw_multi_chunk(); shadows[t] may be NULL.
 * -22 (before any launch) unless state != NULL (all three entries), ntensors > 0, 0 < nchunks < 2^31, g_dtype 0 or 1,
 * max_workgroups >= 0.  norm_sq may be NULL in tn_adamw_prepare: no clip, no skip, the step advances. */
long long tn_adamw_multi_chunk(void);
int tn_adamw_prepare(const float* norm_sq, float* state, float beta1, float beta2, float max_norm, void* stream);
int tn_adamw_multi(void* const* ps, void* const* ms, void* const* vs, const void* const* gs, void* const* shadows,
                   const long long* sizes, const long long* first_chunk, int ntensors, long long nchunks,
                   const float* state, float lr, float beta1, float beta2, float eps, float weight_decay, int g_dtype,
                   void* stream);
/* The same update from at most `max_workgroups` workgroups (0 = one per chunk = tn_adamw_multi), each striding over the
 * chunks: the form for a SIDE stream, where the update runs beside the next forward's kernels and must leave them the
 * machine — the unbounded launch takes the whole HBM bandwidth and the MFMA kernels beside it run at half speed
 * (profiles/r04e_*).  Same arithmetic per element. */
int tn_adamw_multi_bounded(void* const* ps, void* const* ms, void* const* vs, const void* const* gs, void* const* shadows,
                           const long long* sizes, const long long* first_chunk, int ntensors, long long nchunks,
                           const float* state, float lr, float beta1, float beta2, float eps, float weight_decay,
                           int g_dtype, int max_workgroups, void* stream);

/* ---- bf16 transpose for the weight-gradient GEMMs of the linear layers: dst[c*dst_ld + r] = src[r*src_ld + c].
 *      Replaces the implicit operand transposes of torch.nn.functional.linear's backward (every nn.Linear of the
 *      decoder blocks the reference trains, touchnet/bin/train.py:440-470): dW = dY^T X is run with BOTH operands
 *      contraction-contiguous (the forward GEMM's layout), which hipBLASLt executes ~1.4x faster on MI355X.
 *      rows, cols, leading dimensions: multiples of 8; base addresses 16-byte aligned (else -22). */
int tn_transpose_bf16(const void* src, void* dst, int rows, int cols, long long src_ld, long long dst_ld,
                      void* stream);

/* ---- bias gradient of a linear layer: out[c] = sum_r x[r*ld + c], x bf16 [rows, cols] (cols, ld multiples of 8),
 *      out bf16 [cols]; fp32 accumulation, deterministic two-stage reduction through ws
 *      (tn_colsum_workspace_floats(rows, cols) floats).  Replaces the `grad_output.sum(0)` of
 *      torch.nn.functional.linear's backward for the biased projections (Qwen2 q/k/v, the audio tower).
 *      -22 (before any launch) unless rows > 0, cols > 0, cols % 8 == 0, ld % 8 == 0, ld >= cols, x 16-byte aligned. */
long long tn_colsum_workspace_floats(int rows, int cols);
int tn_colsum_bf16(const void* x, void* out, float* ws, int rows, int cols, long long ld, void* stream);

/* ---- int16 PCM of a TouchDataset audio shard -> float32 [-1, 1) on the device (x / 32768, exact): the conversion
 *      the reference does on a CPU worker, touchnet/data/datapipe.py:163-165 */
int tn_pcm16_to_f32(const void* pcm_int16, float* out, long long n, void* stream);

/* ---- BEST-RQ labels: codes[t] = argmin_v || normalize(feat[t] @ quantizer) - codebook[v] ||_2 —
 *      BestRQTokenizer.tokenize, touchnet/tokenizer/tokenizer.py:289-299 (called per utterance from
 *      batch_audio_packed, touchnet/models/touch_audio/processing_touch_audio.py:97).
 *      feat [T, F], quantizer [F, E], codebook [V, E] (already L2-normalised, 16-byte aligned) fp32; codes int64 [T];
 *      E in {8, 16, 32} (else -22).  First index wins ties, like torch.argmin.  A frame with no finite winner (a NaN
 *      or inf feature: every distance is NaN) gets code 0, as torch.argmin gives; every code lies in [0, V). */
int tn_bestrq_tokenize(const float* feat, const float* quantizer, const float* codebook, long long* codes, int T,
                       int F, int E, int V, void* stream);

/* ---- greedy first-fit sequence packing on the device: the placement + scatter of
 *      touchnet/models/llama/processing_llama.py:24-104 (batch_text) and
 *      touchnet/models/touch_audio/processing_touch_audio.py:117-214 (batch_pairaudio_pairtext_packed), bit-identical.
 * plan: lens int32 [n] (slots per segment: tokens + 1, plus feature rows for audio+text) -> row / col / sent (document
 *       index inside the row, from 1) / batch int32 [n]; counts int32 [3] = {batches with >= 1 segment, segments longer
 *       than T, error flag (set when such a segment exists and skip_too_long == 0)}; skipped segments get row = -1.
 * fill: writes the five int64 [B, T] buffers (pad / -100 / 0 / 0 / 1 elsewhere) and, when feats != NULL, the fp32
 *       [B, T, F] feature buffer of batch `which_batch`; segment i = alen[i] feature rows then bos + ntok[i] tokens
 *       (labels pre-shifted: tokens + eos); tok_off / feat_off: offsets of segment i in `tokens` / `feat_src` rows. */
int tn_pack_plan(const int* lens, int n, int B, int T, int skip_too_long, int* row, int* col, int* sent, int* batch,
                 int* counts, void* stream);
int tn_pack_fill(const int* row, const int* col, const int* sent, const int* batch, int which_batch, int n,
                 const int* ntok, const long long* tok_off, const long long* tokens, const int* alen,
                 const long long* feat_off, const float* feat_src, int F, int B, int T, long long bos, long long eos,
                 long long pad, long long* input_ids, long long* labels, long long* position_ids, long long* doc,
                 long long* sentence_lens, float* feats, int* nsent, void* stream);

/* ---- hand-written bf16 MFMA GEMM for the linear layers (q/k/v/o/gate/up/down/lm_head of the decoder blocks,
 *      fc1/fc2/out_proj of the audio tower): replaces torch.nn.functional.linear / liger's MLP swap,
 *      touchnet/models/llama/__init__.py:11-15 — forward, input-gradient and weight-gradient
 *      products alike, each reading nn.Linear's own tensors (no transposed copies):
 *        C[M,N] = sum_{s < nseg} opA_s . opB_s^T (+ bias[N]) (+ C when accumulate != 0)
 *      bf16 in/out, fp32 accumulation over ALL segments, ONE rounding.
 *      a_kmaj / b_kmaj = 0: the operand is stored [rows, K] (contraction-contiguous: x and W in y = x W^T, dY in
 *      dX = dY W); = 1: stored [K, rows] (contraction-major: W in dX = dY W; dY and x in dW = dY^T x).
 *      (a_kmaj = 1, b_kmaj = 0) has no caller and returns -22.  A, B, lda, ldb, K are arrays of nseg (1..3) entries;
 *      Ct (optional, may be NULL): transposed copy [N, M] written by the same epilogue.
 *      -22 unless: every K % 64 == 0 (any K > 0 when both operands are contraction-major), N % 8 == 0, every ld % 8 == 0 and >= the operand's contiguous extent, 16-byte
 *      aligned bases; row-stored operands 288 * ld * 2 < 2^31, contraction-major operands ((K-1) * ld + rows) * 2 < 2^31;
 *      a_kmaj: M % 8 == 0; with Ct: M % 8 == 0, ldct % 8 == 0, accumulate == 0. */
int tn_gemm_bf16(const void* const* A, const void* const* B, const long long* lda, const long long* ldb, const int* K,
                 int nseg, int a_kmaj, int b_kmaj, void* C, void* Ct, const void* bias, int M, int N, long long ldc,
                 long long ldct, int accumulate, void* stream);
/*      C = A B^T (+ bias) + addend: the residual stream added in the epilogue of the producing GEMM — `hidden_states =
 *      residual + hidden_states` behind o_proj / down_proj (transformers' LlamaDecoderLayer / Qwen2DecoderLayer.forward as
 *      driven by touchnet/models/llama/__init__.py; WhisperEncoderLayer.forward for the audio tower) — so that the norm
 *      behind it reads one tensor instead of two.  One segment; addend [M, N] bf16 with pitch ldadd (>= N, % 8), 16-byte
 *      aligned, must not alias C; the product is rounded to bf16 before the addition (the bits of GEMM + residual add). */
int tn_gemm_bf16_addend(const void* A, const void* B, long long lda, long long ldb, int K, int a_kmaj, int b_kmaj, void* C,
                        const void* bias, const void* addend, long long ldadd, int M, int N, long long ldc, void* stream);
/*      The same product (one segment, no transposed copy) with the contraction cut into `splitk` >= 2 parts that run as
 *      independent units.  tail_only = 0: every tile is split — outputs of few 256 x 256 tiles with a deep contraction (the
 *      audio tower's 1280 x 1280 weight gradients contract 30000 frames: 25 tiles for 256 CUs).  tail_only = 1: the whole
 *      rounds of tiles run unsplit and only the last partial round is split (the MLP weight gradients are 688 tiles = 2
 *      rounds + 176: cut in 4 the remainder costs 0.75 of a round instead of 1).  fp32 partial sums travel through
 *      `workspace` (>= tn_gemm_splitk_workspace_bytes(M, N, splitk, 0, tail_only) bytes, 16-byte aligned); a second kernel
 *      adds them (+ bias, + C when accumulate).  -22 additionally when an operand is contraction-contiguous and
 *      ceil(K / 64) % splitk != 0, or tail_only without a whole round / without a remainder. */
int tn_gemm_bf16_splitk(const void* A, const void* B, long long lda, long long ldb, int K, int a_kmaj, int b_kmaj,
                        void* C, const void* bias, int M, int N, long long ldc, int accumulate, int splitk, int tail_only,
                        void* workspace, long long workspace_bytes, void* stream);
/*      Weight gradient with FP32 output — for a data-parallel engine that reduces gradients in fp32 (the reference's
 *      MixedPrecisionPolicy(reduce_dtype=float32), touchnet/models/helper_func.py:165) and wants dW written straight into its
 *      reduce-scatter input instead of cast-copied there: C[M,N] (float, ldc in floats) = (+= when accumulate)
 *      A[K,M]^T . B[K,N], both operands contraction-major as stored (dY [tokens, M], x [tokens, N]).  splitk <= 1: one
 *      launch; >= 2: split-K through `workspace` (tn_gemm_splitk_workspace_bytes(M, N, splitk, 0, 0)).  Same -22 rules as
 *      tn_gemm_bf16. */
int tn_gemm_bf16_wgrad_f32(const void* A, const void* B, long long lda, long long ldb, int K, float* C, int M, int N,
                           long long ldc, int accumulate, int splitk, void* workspace, long long workspace_bytes,
                           void* stream);
/*      Weight gradient AND bias gradient of y = x W^T + b (nn.Linear with bias: Qwen2's q/k/v projections,
 *      transformers' Qwen2Attention behind touchnet/models/qwen2_audio/__init__.py; every Whisper-tower layer) in ONE launch:
 *      C[M, N] (bf16; float with ldc in floats when c_f32; += when accumulate) = A[K, M]^T . B[K, N], bias_grad[M] (bf16)
 *      = column sums of A (A = dY [tokens, M], B = x [tokens, N] as stored).  The sums are taken from the dY fragments
 *      the matrix pipe reads anyway: the separate column-sum pass (tn_colsum_bf16, one more trip of dY through HBM) is
 *      not needed.  splitk >= 2: split-K through `workspace` (tn_gemm_splitk_workspace_bytes(M, N, splitk, 1, 0)).
 *      -22 as for tn_gemm_bf16 with both operands contraction-major; bias_grad must not be NULL. */
int tn_gemm_bf16_wgrad_bias(const void* A, const void* B, long long lda, long long ldb, int K, void* C, void* bias_grad,
                            int M, int N, long long ldc, int accumulate, int c_f32, int splitk, void* workspace,
                            long long workspace_bytes, void* stream);
/*      The split-K workspace of tn_gemm_bf16_splitk, tn_gemm_bf16_wgrad_f32 and tn_gemm_bf16_wgrad_bias, stated here
 *      ONCE — in floats: splitk x split_tiles x 256 x 256 partial-sum slabs of whole tiles (split_tiles = every 256 x 256
 *      output tile, or with tail_only the tiles of the last partial round, tiles mod CUs), then — with a bias gradient —
 *      splitk x ceil(M / 256) x 256 partial column sums.  Returns its size in bytes: 0 for splitk <= 1 (no workspace
 *      needed), -1 where the launch itself answers -22 (M or N <= 0; tail_only without a whole round / a remainder). */
long long tn_gemm_splitk_workspace_bytes(int M, int N, int splitk, int with_bias_grad, int tail_only);
/*      Several INDEPENDENT products of one operand mode as one persistent launch (ngrp = 1..3, weight-gradient mode
 *      a_kmaj = b_kmaj = 1 only): C_g[M_g, N_g] (+= when accumulate) A_g[K_g, M_g]^T . B_g[K_g, N_g], bf16 outputs (ldc in
 *      elements) or, c_f32 = 1, float outputs (ldc in floats).  The three weight gradients of transformers' LlamaMLP
 *      (gate / up / down_proj, swapped at touchnet/models/llama/__init__.py:11-15) are 688 output tiles each — 2.69
 *      rounds on 256 CUs; as ONE tile list they are 8 whole rounds + 16 tiles, and that remainder (tiles mod CUs, when at
 *      most half the CUs and every contraction >= 16 stages) runs split-K through `workspace`
 *      (>= tn_gemm_grouped_workspace_bytes(M, N, K, ngrp) bytes, 16-byte aligned; NULL / too small: the remainder runs as
 *      whole tiles).  -22: shapes as for tn_gemm_bf16 with both operands contraction-major. */
long long tn_gemm_grouped_workspace_bytes(const int* M, const int* N, const int* K, int ngrp);
int tn_gemm_bf16_grouped(const void* const* A, const void* const* B, const long long* lda, const long long* ldb,
                         const int* K, void* const* C, const long long* ldc, const int* M, const int* N, int ngrp,
                         int a_kmaj, int b_kmaj, int accumulate, int c_f32, void* workspace, long long workspace_bytes,
                         void* stream);
/*      The same for ANY number of weight gradients (n = 1..1024, both operands contraction-major), whole tiles only:
 *      C_g[M_g, N_g] (+= when accumulate) A_g[K_g, M_g]^T . B_g[K_g, N_g] and, where bias_grad is not NULL and
 *      bias_grad[g] is not NULL, bias_grad[g][M_g] (bf16) = column sums of A_g.  The linear layers of the Whisper-style
 *      audio tower (q / k / v / out_proj, fc1, fc2 of transformers' Qwen2AudioEncoderLayer) are 300 output tiles per layer
 *      = 1.17 rounds on 256 CUs; nothing reads a weight gradient before the gradient norm, so the products of many layers
 *      run as ONE tile list (11 layers: 3300 tiles = 12.9 rounds).  Every output has the bits of the unsplit single-product
 *      launch (tn_gemm_bf16_wgrad_bias / tn_gemm_bf16_wgrad_f32 with splitk <= 1).  The products' records reach the
 *      device through `table` (device memory, >= tn_gemm_grouped_table_bytes(n) bytes, 16-byte aligned), written
 *      stream-ordered by the call: the caller keeps it untouched until the launch has run.  Outputs of different products
 *      may not overlap.  -22: n out of range (tn_gemm_grouped_table_bytes: -1), no / a misaligned / a short table, shapes
 *      as for tn_gemm_bf16_grouped. */
long long tn_gemm_grouped_table_bytes(int n);
int tn_gemm_bf16_grouped_table(const void* const* A, const void* const* B, const long long* lda, const long long* ldb,
                               const int* K, void* const* C, const long long* ldc, const int* M, const int* N,
                               void* const* bias_grad, int n, int accumulate, int c_f32, void* table,
                               long long table_bytes, void* stream);
/*      The MLP's gate and up products with SwiGLU in the epilogue (LlamaMLP.forward: down(silu(gate(x)) * up(x));
 *      the reference swaps in liger's fused SwiGLU at touchnet/models/llama/__init__.py:11-15): one launch computes
 *      gate[M, I] = x Wg^T, up[M, I] = x Wu^T and act = silu(gate) * up (all bf16, row pitch ldc; gate and up are kept
 *      for the backward) from x [M, K] (pitch ldx) and Wg, Wu [I, K] (pitch ldw) — an output tile is 256 rows x (128 gate
 *      + 128 up columns), no separate SwiGLU pass.  Arithmetic = tn_swiglu_fwd on the bf16-rounded products (bit-identical).
 *      -22 unless K % 64 == 0, I % 8 == 0, pitches % 8 == 0, 16-byte aligned bases. */
int tn_gemm_bf16_swiglu_fwd(const void* x, const void* wg, const void* wu, void* gate, void* up, void* act, int M, int I,
                            int K, long long ldx, long long ldw, long long ldc, void* stream);
/*      Its backward counterpart: d(act) = dY W_down (dY [M, H], pitch lddy; W_down [H, I] read contraction-major, pitch
 *      ldw) stays in the accumulators; the epilogue reads gate / up [M, I] and writes d(gate), d(up) (pitch ld) =
 *      tn_swiglu_bwd on the bf16-rounded d(act) (bit-identical).  -22 unless H % 64 == 0, I % 8 == 0, pitches % 8 == 0. */
int tn_gemm_bf16_swiglu_bwd(const void* dy, const void* wd, const void* gate, const void* up, void* dgate, void* dup,
                            int M, int I, int H, long long lddy, long long ldw, long long ld, void* stream);
/*      The audio tower's MLP (transformers' WhisperEncoderLayer.forward: fc2(gelu(fc1(x))), exact-erf GELU, as driven by
 *      touchnet/models/qwen2_audio/__init__.py:18-133): pre[M, N] = x W^T + bias AND act = gelu(pre) from one launch
 *      (bit-identical to tn_gemm_bf16 followed by tn_gelu_fwd on the rounded pre).  -22 unless K % 64 == 0, N % 8 == 0,
 *      pitches % 8 == 0 and >= the rows they span, 16-byte aligned bases, pre != act. */
int tn_gemm_bf16_gelu_fwd(const void* x, const void* w, const void* bias, void* pre, void* act, int M, int N, int K,
                          long long ldx, long long ldw, long long ldc, void* stream);
/*      ... and the backward of its second half: d(pre)[M, I] = (dY[M, H] W2[H, I]) o gelu'(pre): d(act) lives in the
 *      accumulators only (W2 read contraction-major, pitch ldw; pre / d(pre) with pitch ld) = tn_gemm_bf16 (b_kmaj) followed
 *      by tn_gelu_bwd on the rounded d(act) (bit-identical).  -22 unless H % 64 == 0, I % 8 == 0, pitches % 8 == 0. */
int tn_gemm_bf16_gelu_bwd(const void* dy, const void* w2, const void* pre, void* dpre, int M, int I, int H, long long lddy,
                          long long ldw, long long ld, void* stream);
/*      A q / k projection with the rotary embedding in the epilogue (transformers' LlamaAttention.forward: q_proj /
 *      k_proj followed by apply_rotary_pos_emb, modeling_llama.py:113-160): out[M, N] = rope(x W^T + bias), N = heads x
 *      head_dim (64 or 128), cos / sin [M, head_dim / 2] bf16 = one table row per output row (tn_rope_table).  Bit-identical
 *      to tn_gemm_bf16 followed by tn_rope_apply.  -22 unless K % 64 == 0, pitches % 8 == 0, N % 256 == 0 (head_dim 128) /
 *      N % 64 == 0 (head_dim 64). */
int tn_gemm_bf16_rope(const void* x, const void* w, const void* bias, const void* cos_t, const void* sin_t, void* out, int M,
                      int N, int K, long long ldx, long long ldw, long long ldc, int head_dim, void* stream);
/*      Single segment, both operands contraction-contiguous (the round-2 entry point): */
int tn_gemm_bf16_tn(const void* A, const void* B, void* C, void* Ct, const void* bias, int M, int N, int K,
                    long long lda, long long ldb, long long ldc, long long ldct, int accumulate, void* stream);

/*      Launch form of the GEMMs above: 1 (default) = persistent, one workgroup per CU walking a fixed tile list; 0 = one
 *      workgroup per tile, for a host that runs collectives beside the compute (an RCCL kernel holding CUs would leave a
 *      persistent workgroup's whole tile list waiting: the FSDP2 / context-parallel schedule of
 *      touchnet/models/helper_func.py:134-202, touchnet/utils/distributed.py:292-346).  Process-wide, takes effect at the
 *      next launch; TN_GEMM_PERSIST in the environment overrides it (kernel-development A/B).  Returns nothing / the value. */
void tn_gemm_set_persistent(int on);
int tn_gemm_get_persistent(void);

/* ---- Greedy decoding with a KV cache — touchnet/models/touch_audio/inference_touch_audio.py:177-192 (HF generate() with
 *      use_cache=True, do_sample=False, num_beams=1, repetition_penalty, no_repeat_ngram_size; the per-token attention of
 *      transformers/models/llama/modeling_llama.py:243-285 over past_key_values).
 * attn_decode: q bf16 [B, Nh, D] and k_new / v_new bf16 [B, Nkv, D] of the new token (q, k_new rotated); caches bf16
 *      [B, S_max, Nkv, D]; cache_len int32 [B] = entries valid before this call.  Writes k_new / v_new into slot
 *      cache_len[b], attends over cache_len[b] + 1 keys (scale = softmax scale), writes o bf16 [B, Nh, D]; does NOT advance
 *      cache_len.  cache_len[b] outside [0, S_max): row b's output is NaN, its cache untouched.  workspace: >=
 *      tn_attn_decode_workspace_bytes(..) bytes, 16-byte aligned (NULL when that is 0).  -22 before any launch for NULL or
 *      non-16-byte-aligned tensors, D not 64 / 128, Nh % Nkv != 0, Nh / Nkv > 16. */
long long tn_attn_decode_workspace_bytes(int B, int Nh, int Nkv, int D, int S_max);
int tn_attn_decode(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_len,
                   void* o, void* workspace, int B, int Nh, int Nkv, int D, int S_max, float scale, void* stream);
/* greedy_step: logits [B, V] (`dtype`), V <= 262144; hist int32 [B, S_hist] with hist_len [B]; finished int32 [B];
 *      n_unfinished int32[1].  Per row: fp32 logits, repetition penalty over the ids of hist[b, :hist_len[b]]
 *      (l < 0 ? l * penalty : l / penalty, once per id), -inf on ids that complete an `ngram`-gram of the history
 *      (0 = off), argmax (lowest id on ties); a finished row emits `pad`.  Then hist[b, hist_len[b]] = token,
 *      hist_len[b]++, cache_len[b]++, and on `eos` finished[b] = 1, n_unfinished -= 1.  No host synchronisation.
 *      -22 before any launch for NULL or misaligned pointers, V or S_hist out of range, ngram < 0, penalty <= 0. */
int tn_greedy_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* finished, int* n_unfinished, int B,
                   int V, int S_hist, float penalty, int ngram, int eos, int pad, int dtype, void* stream);
/* sample_step: one decoding step of HF generate() with the sampling warpers — what a Qwen2-Audio checkpoint's
 *      generation_config.json asks of touchnet/models/qwen2_audio/inference_qwen2_audio.py (model.generate(**inputs,
 *      max_length=..., use_cache=True)); transformers/generation/logits_process.py RepetitionPenaltyLogitsProcessor,
 *      TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, then generation/utils.py's multinomial draw.
 *      logits [B, V] (`dtype`), V <= 262144; hist / hist_len / cache_len / finished / n_unfinished as for greedy_step.
 *      Per row: fp32 logits, repetition penalty over hist[b, :hist_len[b]] (each id once); with do_sample: l / temperature,
 *      top_k (0 = off; ties at the k-th value stay), top_p (keep a token iff the softmax mass strictly above it is < top_p;
 *      1 = off), then the first kept token in id order whose running sum of exp(l - max) exceeds u * (sum over the kept),
 *      u in [0, 1) from Philox4x32-10 keyed by `seed` with counter (hist_len[b], row_key[b]) — or uniforms[b] when
 *      `uniforms` (fp32 [B]) is not NULL; row_key int64 [B] (NULL: the row index).  Without do_sample: argmax (lowest id
 *      on ties).  A finished row emits `pad`; then the bookkeeping of greedy_step, with up to 8 `eos_ids` (host array)
 *      finishing a row.  n_kept (int32 [B], may be NULL): tokens left after top-k / top-p — exact whenever the threshold
 *      lies less than 1023/16 below the row's maximum (after penalty and temperature); when the k-th largest value lies
 *      farther down, every token below that distance is counted too (weight zero: they can be kept but are never drawn),
 *      so the count is between the exact one and V and the token is unaffected.  1 for a row without a finite maximum or
 *      without do_sample, 0 for a finished row.  No host synchronisation.
 *      -22 before any launch for NULL or misaligned pointers, V or S_hist out of range, penalty <= 0, n_eos outside
 *      [0, 8], and with do_sample temperature <= 0, top_k < 0 or top_p outside (0, 1]. */
int tn_sample_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* finished, int* n_unfinished,
                   const long long* row_key, const float* uniforms, int* n_kept, int B, int V, int S_hist, float penalty,
                   int do_sample, float temperature, int top_k, float top_p, unsigned long long seed, const int* eos_ids,
                   int n_eos, int pad, int dtype, void* stream);
/* kimi_text_step: one text-stream step of Kimi-Audio's decoding loop — KimiASampler.sample_text_logits and the per-row
 *      bookkeeping of MoonshotKimiaForCausalLM._generate_loop (touchnet/models/kimi_audio/modeling_kimi_audio.py:797-844
 *      and :1153-1214) — in one launch, without the loop's per-row `.item()` synchronisations.
 *      logits [B, V] (`dtype`), V <= 262144; hist / hist_len / cache_len / finished / n_unfinished as for greedy_step;
 *      prompt_len int32 [B]; embed bf16 [V, H], x_next bf16 [B, H], H % 8 == 0, both 16-byte aligned.
 *      Per row: with penalty > 1 and hist_len[b] - prompt_len[b] > window, every id of the last `window` (1..64) entries
 *      of the history, once: l < 0 ? l * penalty : l / penalty, rounded to the logits' dtype.  temperature <= 1e-6: argmax,
 *      lowest id on ties (the argmax of the reference's log_softmax wherever that has no tie of its own).  Otherwise, with
 *      1 <= top_k <= 64: the top_k largest in descending order (ties to the lower id), fp32 weights exp((l - max) /
 *      temperature) (the reference's exp((l - lse) / temperature) up to a factor common to all candidates), the first
 *      candidate whose running weight exceeds u * total; u from uniforms[b] (fp32 [B]) or from Philox4x32-10 keyed by
 *      `seed` with counter (hist_len[b], row_key[b]) as in sample_step (row_key int64 [B], NULL: the row index).
 *      A finished row emits `blank`.  Then the bookkeeping of greedy_step with `eos`, and
 *      x_next[b] = bf16(float(embed[token]) + float(embed[audio_token])) — the next step's input row, bit-equal to
 *      torch's bf16 add.  A row with no room in hist (hist_len[b] >= S_hist) does not advance, as in greedy_step; its
 *      x_next is still written.  No host synchronisation.
 *      -22 before any launch for NULL or misaligned pointers, V, S_hist, window or top_k out of range, penalty <= 0,
 *      H not a multiple of 8, blank or audio_token outside [0, V), and temperature > 1e-6 with top_k == 0 (the
 *      full-vocabulary multinomial: out of scope). */
int tn_kimi_text_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* finished, int* n_unfinished,
                      const int* prompt_len, const void* embed, void* x_next, const long long* row_key,
                      const float* uniforms, int B, int V, int S_hist, int H, float penalty, int window, float temperature,
                      int top_k, unsigned long long seed, int eos, int blank, int audio_token, int dtype, void* stream);

/* ---- Beam search on a KV cache shared between beams — the search mode of HF generate() that
 *      touchnet/models/touch_audio/inference_touch_audio.py:177-192 switches off by hand (num_beams=1) and
 *      touchnet/models/qwen2_audio/inference_qwen2_audio.py takes from the checkpoint's generation_config.json;
 *      transformers/generation/utils.py `_beam_search` (_get_top_k_continuations, _get_running_beams_for_next_iteration,
 *      _update_finished_beams, _check_early_stop_heuristic).  R = B * K rows, utterance b owns rows b K .. b K + K - 1.
 * attn_decode_beam: tn_attn_decode on R rows, plus src int32 [R, S_max]: key / value s < cache_len[r] of row r is read at
 *      cache[src[r, s], s] — keys and values stay where they were written, beams share their ancestors' rows.  The new
 *      key / value go to cache[r, cache_len[r]] (src is not consulted for that slot).  An entry outside [0, R) among the
 *      consulted ones: row r's output is NaN, nothing is read out of bounds.  Key splits, workspace
 *      (tn_attn_decode_workspace_bytes with B = R) and limits as for attn_decode; with a table that names a dense cache
 *      the result equals attn_decode's on that cache bit for bit.  Precondition: no consulted entry names a slot that is
 *      written in the same call, i.e. never src[r, s] == r' with s == cache_len[r'] and s < cache_len[r] (that slot is
 *      being stored by another workgroup: the read would race).  Rows that share one cache_len, as the beams of an
 *      utterance do, and a table that stays inside the utterance — what beam_step maintains — cannot violate it.
 *      -22 as for attn_decode, and for a NULL or misaligned src. */
int tn_attn_decode_beam(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                        const int* cache_len, const int* src, void* o, void* workspace, int R, int Nh, int Nkv, int D,
                        int S_max, float scale, void* stream);
/* beam_step: one step of `_beam_search` for every utterance that is not done.  logits [B * K_in, V] (`dtype`), K_in = 1
 *      right after the prefill (row b K live) or K; hist / fin_ids / src int32 [R, S_hist]; hist_len / cache_len / fin_len /
 *      fin_flag / out_ids / out_parent int32 [R]; run_score / fin_score fp32 [R] (an empty finished slot scores -1e9);
 *      gen / unsat / done int32 [B]; n_unfinished int32 [1]; workspace >= tn_beam_step_workspace_bytes(B, K) bytes.
 *      keep = max(2, 1 + n_eos) K.  acc = processors(log_softmax(fp32 logits)) + run_score[row]: repetition penalty
 *      (lp < 0 ? lp * penalty : lp / penalty, each id of the row's history once) and -inf on ids completing an
 *      `ngram`-gram (0 = off), both applied to the log-probabilities.  The top `keep` candidates of the utterance, ties to
 *      the lower row * V + id; hit = id in eos_ids or gen + 1 >= n_new.  The first K that did not hit become the running
 *      beams: run_score, out_ids, out_parent (absolute row); hist and src rows are permuted by parent, the id appended,
 *      src[row, cache_len] = parent row, hist_len and cache_len advance.  Hits among the first K candidates enter the
 *      finished set (fin_ids = the whole sequence, prompt included, fin_len its length) at acc / (gen + 1) ^ length_penalty;
 *      the best K are kept, descending.  unsat &= run_score[0] / L ^ length_penalty > worst finished score (L = n_new for
 *      early_stopping 2 = "never" with length_penalty > 0, else gen + 1); the utterance is done when !unsat, when the set
 *      is full under early_stopping 1 = True (0 = False), or when every candidate hit; then done[b] = 1, n_unfinished -= 1
 *      and later calls leave all its state untouched.  An utterance whose rows have no room for the appended id
 *      (hist_len[b K] outside [1, S_hist) or cache_len[b K] outside [0, S_hist)) is skipped whole: nothing of it changes,
 *      it does not advance and n_unfinished does not drop — the caller grows hist / fin_ids / src before the step, as
 *      it grows the caches.  No host synchronisation.  -22 before any launch for NULL or
 *      misaligned pointers, K outside [2, 8], K_in not 1 or K, n_eos outside [0, 3], V outside [64, 262144], penalty <= 0,
 *      ngram < 0, n_new < 1, early_stopping outside [0, 2]. */
long long tn_beam_step_workspace_bytes(int B, int K);
int tn_beam_step(const void* logits, int* hist, int* hist_len, int* cache_len, int* src, float* run_score, int* fin_ids,
                 int* fin_len, float* fin_score, int* fin_flag, int* gen, int* unsat, int* done, int* n_unfinished,
                 int* out_ids, int* out_parent, void* workspace, int B, int K, int K_in, int V, int S_hist, float penalty,
                 int ngram, const int* eos_ids, int n_eos, int n_new, float length_penalty, int early_stopping, int dtype,
                 void* stream);
/* logits_constrain: hotword biasing and forbidden sequences — transformers/generation/logits_process.py
 *      SequenceBiasLogitsProcessor and MinNewTokensLengthLogitsProcessor, the `sequence_bias` and `min_new_tokens` of a
 *      generation_config.json (touchnet/models/qwen2_audio/inference_qwen2_audio.py hands that file to model.generate()).
 *      hist int32 [R, S_hist], hist_len / prompt_len int32 [R] (prompt_len may be NULL when min_new == 0).  Logits row
 *      `row_in` of R_in belongs to history row (row_in / K_in) K + row_in % K_in (greedy and sampling: K = K_in = 1; beam
 *      search: K_in = 1 right after the prefill, K afterwards).
 *      The table: seq_off int32 [n_seq + 1] and seq_ids int32 [n_ids] (the sequences' ids, packed), seq_bias fp32 [n_seq]
 *      (finite or -inf); grp_off int32 [n_grp + 1], grp_tok int32 [n_grp], grp_eos int32 [n_grp]: the sequences grouped by
 *      their last id, grp_tok ascending, within a group the length-1 sequence first and then the longer ones in the order
 *      of the caller's dict — HF's order of summation; grp_eos marks eos ids (such a group may be empty).
 *      With n = hist_len[r]: a sequence of length L matches when L == 1, or L <= n and hist[r, n-L+1 .. n-1] equals its
 *      first L - 1 ids.  total(t) = the fp32 sum of the matching biases of t's group in listed order, each addition rounded
 *      on its own; -inf for an eos id while n - prompt_len[r] < min_new.
 *      mode 0 (apply): logits [R_in, V] (`dtype`), logits[row_in, t] = T(fp32(logits[row_in, t]) + total(t)) for every t
 *      with a matching sequence or under the eos rule; no other element is written.  mode 1 (emit): logits is not read
 *      (NULL allowed); edit_ids int32 [R_in, n_grp] = t where apply would write, else -1 - t; edit_val fp32 [R_in, n_grp] =
 *      total(t); edit_cnt int32 [R_in] = the number of ids apply would write — the list tn_beam_step_edits takes.
 *      Every id has one writer: no atomics, bit-identical repeats.  Finished rows and rows of done utterances are edited
 *      like any other (the step kernels ignore them).  Limits: n_seq <= 16384, every sequence 1 .. 64 ids, V <= 262144;
 *      a sequence outside them or a group id outside [0, V) is ignored by the kernel (the Python plan refuses it).
 *      -22 before any launch for NULL or misaligned pointers, counts outside those limits, n_grp outside [1, n_seq + 8],
 *      K_in not 1 or K, R_in % K_in != 0, min_new < 0, mode outside [0, 1]. */
int tn_logits_constrain(void* logits, const int* hist, const int* hist_len, const int* prompt_len, const int* seq_off,
                        const int* seq_ids, const float* seq_bias, const int* grp_off, const int* grp_tok,
                        const int* grp_eos, int* edit_ids, float* edit_val, int* edit_cnt, int R_in, int K, int K_in, int V,
                        int S_hist, int n_seq, int n_ids, int n_grp, int min_new, int mode, int dtype, void* stream);
/* beam_step_edits: beam_step with the edit list of logits_constrain's emit mode (edit_ids / edit_val [B * K_in, n_edit],
 *      edit_cnt [B * K_in]): lp[t] = log_softmax(..)[t] + edit_val of t's slot for every slot with edit_ids >= 0, BEFORE
 *      the repetition penalty — HF's processor order on the log-probabilities (editing the logits instead would move the
 *      normaliser).  All three NULL: exactly beam_step.  -22 as for beam_step, and for a partly NULL or misaligned list or
 *      n_edit < 1. */
int tn_beam_step_edits(const void* logits, int* hist, int* hist_len, int* cache_len, int* src, float* run_score,
                       int* fin_ids, int* fin_len, float* fin_score, int* fin_flag, int* gen, int* unsat, int* done,
                       int* n_unfinished, int* out_ids, int* out_parent, void* workspace, int B, int K, int K_in, int V,
                       int S_hist, float penalty, int ngram, const int* eos_ids, int n_eos, int n_new, float length_penalty,
                       int early_stopping, int dtype, const int* edit_ids, const float* edit_val, const int* edit_cnt,
                       int n_edit, void* stream);
/* token_scores: per-token confidences — transformers' compute_transition_scores(sequences, out.logits,
 *      normalize_logits=True) of a generate(output_logits=True) call (the generate() of
 *      touchnet/models/touch_audio/inference_touch_audio.py:177-192 returns ids only), plus the row's entropy and its k
 *      most likely tokens.  logits [R, V] (`dtype`: 0 fp32, 1 bf16) contiguous, read in fp32; row r starts at
 *      r * V * sizeof(T) and needs no more than its element's alignment.  The scored token t is named in one of two ways:
 *      token mode: tok int32 [R] (hist and hist_len NULL, S_hist ignored); outputs logp / entropy fp32 [R], alt_id int32 and
 *      alt_logp fp32 [R, k].  history mode: tok NULL, hist int32 [R, S_hist], hist_len int32 [R]: with n = hist_len[r],
 *      t = hist[r, n - 1] (the id a step kernel has just appended) and the outputs go to column n - 1 of logp / entropy
 *      [R, S_hist] and alt_id / alt_logp [R, S_hist, k]; a row with n outside [1, S_hist] writes nothing.
 *      With lse = log sum_v exp(l_v): logp = l_t - lse; entropy = lse - sum_v p_v l_v (a -inf logit contributes 0);
 *      alt_id = the ids of the k largest logits, descending, ties to the lower id, alt_logp their logp; for k > V the tail
 *      is id -1, logp -inf (k == 0: alt_id / alt_logp may be NULL).  t outside [0, V): logp = NaN, nothing is read out of
 *      bounds, entropy and the alternatives are still written.  A row that holds a NaN or +inf, or only -inf: every fp32
 *      output of the row is NaN and the ids are -1.  One workgroup per row; which thread sums which id depends on the id
 *      alone and the reduction order is fixed: repeats are bit-identical and a row scores the same in any batch and at any
 *      address.  No atomics; nothing but the outputs is written.  -22 before any launch for NULL or misaligned pointers
 *      (logits to its element, all others to 4 bytes), V outside [1, 262144], k outside [0, 8], R < 0, both or neither of
 *      tok and (hist, hist_len), S_hist < 1 in history mode, dtype outside [0, 1].  R == 0: 0, nothing launched. */
int tn_token_scores(const void* logits, const int* tok, const int* hist, const int* hist_len, float* logp, float* entropy,
                    int* alt_id, float* alt_logp, int R, int V, int S_hist, int k, int dtype, void* stream);

/* ---- Kimi-Audio's speech tokenizer (GLM-4-voice WhisperVQEncoder, touchnet/models/kimi_audio/modeling_kimi_audio.py:140-319,
 *      run by MoonshotKimiaForCausalLM.prepare_audio_input_embs under no_grad, :957-963).  Forward only: it is frozen.
 * attn_block_causal_fwd: the layers' self-attention under get_block_causal_attention_mask (:226-242, applied :293-301):
 *      allowed(i, j) = m[j] && j / block <= i / block.  q / k / v / o bf16 [B, T, Nh, D], D = 64, Nh == Nkv; position t of
 *      row b belongs to the clip starting at seg_start[b, t] (row-local) whose valid keys end at key_end[b, t] (exclusive;
 *      int32 [B, T] each): query i attends to keys [s, min(key_end, s + ((i - s) / block + 1) * block)), s = seg_start;
 *      fp32 softmax; a row with no such key writes 0.  -22 before any launch for D != 64, block < 1, NULL or misaligned
 *      (q / k / v 16-byte, o 8-byte) pointers. */
int tn_attn_block_causal_fwd(const void* q, const void* k, const void* v, void* o, const int* seg_start, const int* key_end,
                             int B, int T, int Nh, int D, int block, float scale, void* stream);
/* vq_nearest: `vector_quantize` (:85-98): ids[r] = argmin_c (cnorm[c] - 2 x[r] . c), the first index on ties (torch.min);
 *      x bf16 [M, d], codebook bf16 [V, d] (16-byte aligned), cnorm fp32 [V] = |c|^2, d % 64 == 0; bf16 MFMA products
 *      with fp32 accumulation, no [M, V] buffer; ids int64 [M] (also the scratch of the cross-workgroup 64-bit min, so
 *      the result is deterministic).  -22 before any launch for d % 64 != 0, V < 1, NULL or misaligned pointers. */
int tn_vq_nearest(const void* x, const void* codebook, const float* cnorm, long long* ids, int M, int V, int d, void* stream);

/* ---- scoring: edit-distance alignment of token sequences --------------------------------------
 * `EditDistance` and `CountEdits` of the recipe's scorer, touchnet/bin/error_rate_zh:44-149,192-205, for P (reference,
 * hypothesis) pairs at once: match 0, substitution / insertion / deletion 1 each, and the reference's tie rule (its
 * backpointer is updated in the order diagonal, deletion, insertion, each with `>=`): the insertion arc wins if it is at
 * least as good as both others, otherwise the deletion arc if it is at least as good as the diagonal, otherwise the
 * diagonal; first row insertions only, first column deletions only, backtrace from (R, H).
 *   ref_tok  int [n_ref], hyp_tok int [n_hyp]   packed token ids
 *   host_desc int [P][6] on the HOST            {ref_start, R, hyp_start, H, ws_base, ops_base} per pair
 *   desc_dev int [P][6]                         device room for the table: the entry uploads it, stream-ordered
 *   ws       unsigned [ws_words]                scratch: pair p owns tn_edit_align_ws_words(R, H) words from ws_base
 *                                               (2 bits of direction per cell, 16 rows of a column per word, the columns
 *                                               padded to a multiple of 64; + R words when R > 2048)
 *   ops      unsigned char [n_ops]              0 = C, 1 = S, 2 = I, 3 = D: pair p's arcs in path order, RIGHT-aligned in
 *                                               its R + H bytes from ops_base; the bytes to their left are not written
 *   counts   int [P][5]                         C, S, I, D, number of arcs; the reference's score is -(S + I + D)
 * Two launches (one wave per pair forward, one lane per pair back), no atomics, no synchronisation; deterministic.
 * -22 before the upload and any launch unless, for every pair: 1 <= R <= 16383, 0 <= H <= 16383, the token ranges lie
 * inside the two arrays, the workspace ranges lie inside ws_words and ascend without overlap in table order, the ops
 * ranges lie inside n_ops without overlap; and no buffer that is used is NULL.  P == 0: 0, nothing launched.
 * tn_edit_align_ws_words: the words of one pair, -1 for lengths outside those limits. */
long long tn_edit_align_ws_words(int R, int H);
int tn_edit_align(const int* ref_tok, long long n_ref, const int* hyp_tok, long long n_hyp, const int* host_desc,
                  int* desc_dev, int P, unsigned int* ws, long long ws_words, unsigned char* ops, long long n_ops,
                  int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TOUCHNET_AMD_H_ */
