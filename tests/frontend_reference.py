"""The data-side kernels restated in float64 — what csrc/frontend.hip (tn_log_mel, tn_audiofeat_stack, tn_feat_augment) and
csrc/tokenizer.hip (tn_bestrq_tokenize) are held to at their edges — with the error budgets of their fp32 arithmetic and
the named cases.  Plain numpy, written from the operations' definitions; no kernel, no oracle, no device.

log_mel / log_mel_budget     audio_compute_log_mel_spectrogram, touchnet/data/functions.py:159-190
stack / stack_budget         audiofeat_stack, touchnet/data/functions.py:258-286
augment                      audiofeat_spec_aug / _sub / _trim, touchnet/data/functions.py:193-255 (exact: no budget)
bestrq / bestrq_bound        BestRQTokenizer.tokenize, touchnet/tokenizer/tokenizer.py:289-299
LOG_MEL_CASES, STACK_CASES, AUGMENT_CASES, AUGMENT_REFUSALS, BESTRQ_CASES and CASES (all of them by kind): named, seeded,
small; tests/test_frontend_reference_cpu.py shows that the budgets tell a right kernel from a wrong one on them,
tests/test_frontend_edges_gpu.py runs them on the device.

u = 2^-24 is fp32's unit roundoff throughout; gamma_n stands for n u (1 + O(n u)), Higham's constant of an n-term sum.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 1e-3                      # the O(n u) second-order terms of every gamma_n used below (n <= 600)
NFFT, HOP, NFREQ = 400, 160, 201
GROUP = 4                               # frames per DFT group of the kernel (its masked tail: frame counts 4k+1 .. 4k+3)


# ================================================================================================== log-mel
@functools.lru_cache(maxsize=None)
def slaney_filters(n_mels):
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels) (functions.py:179-182) in float64, [n_mels, 201]: the Slaney scale
    (linear, 200/3 Hz per mel, below 1 kHz; logarithmic above, 27 mels per factor 6.4), triangles between neighbouring
    centres, each scaled by 2 / (its width in Hz)."""
    lin, knee_hz, per_log = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    knee = knee_hz / lin

    def mel(hz):
        return knee + math.log(hz / knee_hz) / per_log if hz >= knee_hz else hz / lin

    def hz(m):
        return knee_hz * math.exp(per_log * (m - knee)) if m >= knee else lin * m
    edges = np.array([hz(m) for m in np.linspace(mel(0.0), mel(8000.0), n_mels + 2)])
    bins = np.arange(NFREQ) * (16000.0 / NFFT)
    w = np.zeros((n_mels, NFREQ))
    for m in range(n_mels):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        rise, fall = (bins - lo) / (mid - lo), (hi - bins) / (hi - mid)
        w[m] = np.maximum(0.0, np.minimum(rise, fall)) * 2.0 / (hi - lo)
    return w


def hann():
    """torch.hann_window(400): periodic."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)


def frames(wav):
    """The frames torch.stft(center=True, pad_mode="reflect") cuts, without the last one (functions.py:172-177):
    float64 [N // 160, 400], unwindowed."""
    x = np.asarray(wav, dtype=np.float64).reshape(-1)
    assert x.size > NFFT // 2, "reflect padding needs more than 200 samples"
    padded = np.pad(x, NFFT // 2, mode="reflect")
    n = x.size // HOP
    return padded[HOP * np.arange(n)[:, None] + np.arange(NFFT)[None, :]]


def power(wav):
    """|rfft(frame * hann)|^2, float64 [frames, 201]."""
    return np.abs(np.fft.rfft(frames(wav) * hann(), axis=1)) ** 2


def _finish(logspec, gmax):
    return (np.maximum(logspec, gmax - 8.0) + 4.0) / 4.0


def log_mel(wav, n_mels):
    """float64 [N // 160, n_mels]: filters @ power, log10 of max(., 1e-10), max(., global max - 8), (x + 4) / 4
    (functions.py:183-189)."""
    logspec = np.log10(np.maximum(power(wav) @ slaney_filters(n_mels).T, 1e-10))
    return _finish(logspec, logspec.max())


# The device's sincospif and log10f carry no stated bound of their own; OCML is built to OpenCL's full-profile ceilings
# (sincospi 4 ulp, log10 3 ulp; HIP's own table reports 1 and 2), and 4 ulp is what the budget assumes for both.  Nothing
# in the budget is fitted to an output of the kernel or of its emulation.
ULP_TRIG = 4.0
ULP_LOG = 4.0
RUNNING_FRAMES = 64


@functools.lru_cache(maxsize=None)
def _dft_error(wav_bytes):
    """d of log_mel_budget, float64 [frames, 201] (one waveform serves both filter banks)."""
    fr = frames(np.frombuffer(wav_bytes, dtype=np.float64))
    xw = fr * hann()
    s1w, s1 = np.abs(xw).sum(axis=1), np.abs(fr).sum(axis=1)
    acc = np.repeat((NFFT * s1w)[:, None], NFREQ, axis=1)
    T = fr.shape[0]
    ends = np.unique(np.concatenate([np.arange(min(T, RUNNING_FRAMES)), np.arange(max(T - RUNNING_FRAMES, 0), T)]))
    ang = 2.0 * np.pi * np.outer(np.arange(NFFT), np.arange(NFREQ)) / NFFT
    tabs = (np.cos(ang), np.sin(ang))
    for i in range(0, ends.size, 32):
        t = ends[i:i + 32]
        run = [np.abs(np.cumsum(xw[t][:, :, None] * tab[None, :, :], axis=1)).sum(axis=1) for tab in tabs]
        acc[t] = np.minimum(acc[t], np.maximum(run[0], run[1]) + s1w[t][:, None])
    return U * SLACK * (acc + (12.0 * s1w + 6.0 * s1)[:, None])


def log_mel_budget(wav, n_mels):
    """Per-element bound on |tn_log_mel - log_mel| in fp32 arithmetic, float64 [frames, n_mels].

    Window and twiddles.  The angle 2 n / 400 is rounded once (relative u, at most 2 pi u in the argument of cos / sin)
    and the function errs by ULP_TRIG ulp of a value <= 1: |dc|, |ds| <= (2 pi + 4) u < 11 u.  hann = 0.5 - 0.5 c inherits
    half of it plus its own rounding, < 6 u; the product x[n] hann[n] rounds once more, u |x hann|.
    DFT.  re = sum_n xw[n] c[n k] over 400 terms in ascending n.  Each step rounds the running sum once (and the product
    once more where the compiler does not fuse them), so the sum errs by u (sum_n |s_n| + S1w) over its partial sums s_n
    — the running error bound of a recursive sum (Higham, Accuracy and Stability, 4.3), evaluated on the float64
    partial sums — and in any order by gamma_400 S1w, with S1w = sum_n |x[n] hann[n]| the frame's windowed l1 energy:
    either way in proportion to the frame, whatever the bin's own power.  The running form (some 7 times smaller on
    noise) is evaluated for the first and the last RUNNING_FRAMES frames of a clip, which covers every clip here but
    the two long ones; their quiet middle, clamped to max - 8, takes the order-free form.  With the table errors
          d := |d re|, |d im| <= u (min(sum_n |s_n| + S1w, 400 S1w) + 12 S1w + 6 S1) (1 + O(400 u)),   S1 = sum_n |x[n]|.
    Power.  P = re^2 + im^2: |dP| <= 2 (|re| + |im|) d + 2 d^2 + 3 u P <= 2 sqrt(2 P) d + 2 d^2 + 3 u P.
    Mel.  M = sum_k w[m, k] P[k] over 201 terms in sequence, the fp32 weights rounded once from float64:
          |dM| <= sum_k w[m, k] |dP[k]| + gamma_203 M — in proportion to the filter row's weights.
    Logarithm, floor and clamp by intervals: v lies in [log10 max(M - dM, 1e-10), log10 max(M + dM, 1e-10)] widened by
    ULP_LOG ulp of |v| (and u for the fp32 constant 1e-10f); the global maximum lies between the largest lower and the
    largest upper end; (max(v, g - 8) + 4) / 4 rises with both v and g, so its value lies between the expression at the
    lower ends and at the upper ends.  Linearised: a relative mel error r becomes r / (4 ln 10); floor and clamp only
    shrink the interval.  The last subtraction, addition and product round to 2 u (|y| + 1) more.
    On the cases of this file the fp32 emulation of test_frontend_reference_cpu.py uses at most 0.035 of this budget
    (the tone; 0.03 on noise): a worst case over 400 roundings and two 4-ulp tables against errors that mostly cancel."""
    w = slaney_filters(n_mels)
    d = _dft_error(np.asarray(wav, dtype=np.float64).tobytes())
    p = power(wav)
    dp = 2.0 * np.sqrt(2.0 * p) * d + 2.0 * d * d + 3.0 * U * p
    m = p @ w.T
    dm = dp @ w.T + (NFREQ + 2.0) * U * SLACK * m
    lo = np.log10(np.maximum(m - dm, 1e-10))
    hi = np.log10(np.maximum(m + dm, 1e-10))
    lo = lo - (ULP_LOG * 2.0 * U * np.abs(lo) + U)
    hi = hi + (ULP_LOG * 2.0 * U * np.abs(hi) + U)
    rnd = 2.0 * U * 20.0                               # g - 8 in fp32, |g - 8| < 20
    y = log_mel(wav, n_mels)
    y_lo, y_hi = _finish(lo, lo.max() - rnd), _finish(hi, hi.max() + rnd)
    return np.maximum(y_hi - y, y - y_lo) + 2.0 * U * (np.abs(y) + 1.0)


# ================================================================================================== stack
def stack_rows(feat, stack, stride):
    """Row r of the stacked matrix holds frames r*stride - lp ... r*stride - lp + stack - 1 with lp = (stack - 1) // 2,
    frames in front of 0 being copies of frame 0 and frames past T - 1 copies of the last (functions.py:267-281):
    [ceil(T / stride), stack * F]."""
    x = np.asarray(feat)
    T = x.shape[0]
    rows = -(-T // stride)
    t = np.arange(rows)[:, None] * stride + np.arange(stack)[None, :] - (stack - 1) // 2
    return x[np.clip(t, 0, T - 1)].reshape(rows, stack * x.shape[1])


def stack(feat, stack, stride, normalize):
    """float64 audiofeat_stack: the gather of stack_rows, then (y - mean) / (std + 1e-5) per row with torch's unbiased
    std (functions.py:282-284).  n = 1 with normalize gives NaN (0 / 0 in the variance), as torch.std does."""
    y = stack_rows(np.asarray(feat, dtype=np.float64), stack, stride)
    if not normalize:
        return y
    n = y.shape[1]
    mean = y.mean(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((y - mean) ** 2).sum(axis=1, keepdims=True) / np.float64(n - 1))
        return (y - mean) / (std + 1e-5)


def stack_budget(feat, stack, stride, normalize):
    """Per-element bound on |tn_audiofeat_stack - stack|, float64, zero without normalisation (a gather: bit-equal).

    One wave sums a row of n = stack F values: each lane ceil(n / 64) of them in sequence, then six shuffle levels, so
    every value passes through at most depth = ceil(n / 64) + 6 additions.
    Mean: |e| = |mean^ - mean| <= dmu := (depth + 2) u mean|x| (gamma_depth sum|x| / n, the division, second order) —
    of order n u max|x| / 64.
    Variance of the shifted values: sum (x_i - mean - e)^2 = sum (x_i - mean)^2 + n e^2 exactly (the deviations sum to
    zero), so the computed std lies in
          [ std (1 - r),  sqrt(std^2 + n dmu^2 / (n - 1)) (1 + r) ],    r = (depth + 6) u
    (two roundings per deviation, gamma_depth for the sum, the division, half of it all under the root, the root).
    Output (x_i - mean^) / (std^ + 1e-5): with d_i = x_i - mean and the two ends s- <= s+ of that interval
          |dy_i| <= |d_i| max(1/(std + eps) - 1/(s+ + eps), 1/(s- + eps) - 1/(std + eps))
                    + dmu / (s- + eps) + 4 u (|d_i| + dmu) / (s- + eps)
    — the mean's error amplified by 1 / (std + 1e-5), which is what near-constant rows show: at mean 1000 and std 1e-3
    dmu is about the std itself and the budget about 1: there the kernel is only held to the rule's own conditioning.
    Rows of one repeated value have d_i = 0 and sums that are exact in any order for the value used here (0.5): the test
    asks for exact zeros.  n = 1: NaN (no budget; the test asks for NaN)."""
    y = stack_rows(np.asarray(feat, dtype=np.float64), stack, stride)
    if not normalize:
        return np.zeros_like(y)
    n = y.shape[1]
    if n == 1:
        return np.full_like(y, np.nan)
    depth = -(-n // 64) + 6
    dmu = (depth + 2) * U * np.abs(y).mean(axis=1, keepdims=True)
    d = np.abs(y - y.mean(axis=1, keepdims=True))
    std = np.sqrt((d ** 2).sum(axis=1, keepdims=True) / (n - 1))
    r = (depth + 6) * U
    s_lo = std * (1.0 - r)
    s_hi = np.sqrt(std ** 2 + n * dmu ** 2 / (n - 1)) * (1.0 + r)
    eps = 1e-5
    scale = np.maximum(1.0 / (std + eps) - 1.0 / (s_hi + eps), 1.0 / (s_lo + eps) - 1.0 / (std + eps))
    return d * scale + dmu / (s_lo + eps) + 4.0 * U * (d + dmu) / (s_lo + eps)


# ================================================================================================== augment
def augment(feat, t_masks=(), f_masks=(), subs=(), out_rows=None):
    """The reference's chain spec_aug -> spec_sub -> spec_trim with the draws given (processing_touch_audio.py:468-473),
    stage by stage: zero the time stripes [start, end) and the frequency stripes (functions.py:205-215); then every
    substitution (start, end, pos) in order copies rows [start - pos, end - pos) of the stage's INPUT over rows
    [start, end) (:231-237); then keep the first out_rows rows (:250-253).  Same dtype out: an exact gather."""
    a = np.array(feat, copy=True)
    for s, e in t_masks:
        a[s:e, :] = 0
    for s, e in f_masks:
        a[:, s:e] = 0
    b = a.copy()
    for s, e, pos in subs:
        b[s:e, :] = a[s - pos:e - pos, :]
    return b[:a.shape[0] if out_rows is None else out_rows]


# ================================================================================================== BEST-RQ
def bestrq(feat, quantizer, codebook):
    """(codes int64 [T], margin float64 [T]) of BestRQTokenizer.tokenize (tokenizer.py:292-298) in float64:
    x = feat @ quantizer; x /= max(||x||, 1e-8); code = first argmin_v ||x - codebook[v]||.  margin is the gap between the
    best distance and the best among the rows that are not bit-for-bit copies of the winning row (inf if there is none).
    A frame whose projection is not finite has only NaN distances: code 0, as torch.argmin gives, margin NaN."""
    f, q, c = (np.asarray(a, dtype=np.float64) for a in (feat, quantizer, codebook))
    T, V = f.shape[0], c.shape[0]
    codes = np.zeros(T, dtype=np.int64)
    margin = np.full(T, np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        p = f @ q
    for t in range(T):
        if not np.isfinite(p[t]).all():
            continue
        x = p[t] / max(math.sqrt(float((p[t] ** 2).sum())), 1e-8)
        d = np.sqrt(((x[None, :] - c) ** 2).sum(axis=1))
        codes[t] = int(np.argmin(d))
        others = ~(c == c[codes[t]]).all(axis=1)
        margin[t] = d[others].min() - d[codes[t]] if others.any() else np.inf
    return codes, margin


def bestrq_bound(feat, quantizer):
    """Bound on the fp32 error of ONE distance ||x - codebook[v]|| of a frame, float64 [T] (NaN for a non-finite frame);
    two distances compare right when their gap exceeds twice this, and the cases keep ten times it.

    Projection.  p_e = sum_k f_k q_ke by one fma per k in ascending k (chunking the k range does not reorder it): each
    step rounds the running sum once, so |dp_e| <= u sum_k |s_k| over the partial sums s_k — the running error bound of
    a recursive sum (Higham, Accuracy and Stability, 4.3), evaluated here on the float64 partial sums.  It is the
    worst case for THIS order; the order-free form gamma_F sum_k |f_k q_ke| ~ F u |feat| |q_e| is some sqrt(F) larger
    (1.6e-3 at F = 560, no smaller than the gaps between neighbouring codebook rows) and would decide nothing.
    Normalisation.  ||a/|a| - b/|b||| <= 2 ||a - b|| / (|a| + |b|) (Dunkl-Williams), and x -> x / 1e-8 below the floor:
    both within ||dp|| / (max(||p||, 1e-8) - ||dp||).  The norm's own arithmetic (E fmas, root, division) scales x by
    1 + (E / 2 + 3) u, ||x|| <= 1.
    Distance.  Differences, E fmas and the root: (E / 2 + 2) u d with d <= 2.
          bound = ||dp|| / (max(||p||, 1e-8) - ||dp||) + (1.5 E + 7) u."""
    f, q = np.asarray(feat, dtype=np.float64), np.asarray(quantizer, dtype=np.float64)
    E = q.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        partial = np.cumsum(f[:, :, None] * q[None, :, :], axis=1)          # [T, F, E]
        p = partial[:, -1, :]
        ndp = np.sqrt(((U * SLACK * np.abs(partial).sum(axis=1)) ** 2).sum(axis=1))
        den = np.maximum(np.sqrt((p ** 2).sum(axis=1)), 1e-8) - ndp
        bound = ndp / den + (1.5 * E + 7.0) * U
    return np.where(np.isfinite(p).all(axis=1), bound, np.nan)


# ================================================================================================== cases
def _rng(*key):
    return np.random.default_rng([7321, *key])


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


# ---- log-mel: content x sample count; every waveform carries its full level in its first and last 200 samples
LOG_MEL_SAMPLES = {          # name -> (samples, what the count places)
    "201": 201,              # 1 frame (4k+1) that reflects at both ends
    "320": 320,              # 2 frames, shorter than a window
    "399": 399,
    "400": 400,
    "799": 640 + 159,        # 4 frames: one full group
    "1121": 7 * 160 + 1,     # 7 frames (4k+3): the group's masked tail
    "16077": 16000 + 77,     # 100 frames
}
LONG = 4100 * 160 + 5        # 4100 frames = 1025 groups: workgroup 0 of 1024 takes a second lap


def _content(kind, n, seed):
    g = _rng(1, seed, n)
    t = np.arange(n)
    if kind == "noise":                 # Gaussian noise at 0.1
        return 0.1 * g.standard_normal(n)
    if kind == "tone":                  # 1 kHz at 0.9: exactly bin 25, leaks into two neighbours only -> clamp active
        return 0.9 * np.sin(2 * np.pi * 1000.0 * t / 16000.0 + 0.3)
    if kind == "tone_noise":
        return 0.9 * np.sin(2 * np.pi * 1000.0 * t / 16000.0 + 0.3) + 1e-5 * g.standard_normal(n)
    if kind == "quiet":                 # noise at 1e-3: every log-mel value, the maximum too, is negative
        return 1e-3 * g.standard_normal(n)
    if kind == "quiet_ends":            # maximum in (-2, 0), so negative AND the clamp active: 0.1 noise at both ends,
        x = np.zeros(n)                 # silence (log10 1e-10 = -10 < max - 8) between
        x[:200] = 0.1 * g.standard_normal(200)
        x[-200:] = 0.1 * g.standard_normal(200)
        return x
    if kind == "impulse_head":          # one sample: the left reflection shows it twice to frame 0
        x = np.zeros(n)
        x[1] = 1.0
        return x
    if kind == "impulse_tail":
        x = np.zeros(n)
        x[n - 2] = 1.0
        return x
    if kind == "zeros":                 # the answer is -1.5 everywhere
        return np.zeros(n)
    if kind in ("loud_last", "loud_first"):   # 1e-5 noise with full-scale ends, the louder one in the last / first group
        x = 1e-5 * g.standard_normal(n)
        a, b = (0.45, 0.9) if kind == "loud_last" else (0.9, 0.45)
        x[:200] += a * g.standard_normal(200)
        x[-200:] += b * g.standard_normal(200)
        return x
    raise KeyError(kind)


def _log_mel_cases():
    cases = {}
    for sname, n in LOG_MEL_SAMPLES.items():
        cases[f"noise-{sname}"] = ("noise", n)
    for kind in ("tone", "tone_noise", "quiet", "quiet_ends", "impulse_head", "impulse_tail", "zeros"):
        for sname in ("201", "1121", "16077") if kind in ("tone", "quiet_ends") else ("320", "1121"):
            cases[f"{kind}-{sname}"] = (kind, LOG_MEL_SAMPLES[sname])
    cases["loud_last-long"] = ("loud_last", LONG)
    cases["loud_first-long"] = ("loud_first", LONG)
    return cases


LOG_MEL_CASES = _log_mel_cases()
LOG_MEL_BINS = (80, 128)


@functools.lru_cache(maxsize=None)
def log_mel_wave(name):
    """The fp32 waveform of a log-mel case (what the kernel, the emulation and the restatement all read)."""
    kind, n = LOG_MEL_CASES[name]
    return _f32(_content(kind, n, sorted(LOG_MEL_CASES).index(name)))


# ---- stack: name -> (stack, stride, T, F, content)
def _stack_cases():
    c = {}
    geo = [(1, 1, 1, 2), (1, 1, 33, 64), (4, 4, 1, 16), (4, 4, 3, 16), (4, 4, 17, 140), (7, 6, 2, 9), (7, 6, 6, 9),
           (7, 6, 25, 80), (5, 4, 4, 13), (5, 4, 17, 13), (5, 4, 33, 112), (3, 5, 2, 21), (3, 5, 21, 21), (3, 5, 33, 1),
           (7, 1, 1, 80), (7, 1, 5, 9), (7, 1, 33, 80), (2, 1, 33, 1)]
    for stack, stride, T, F in geo:     # stack * F: 2, 3, 63, 64, 65, 560 and the n = 1 row at (1, 1, T, 1) below
        c[f"s{stack}x{stride}-T{T}-F{F}"] = (stack, stride, T, F, "normal")
    c["n1-s1x1-T2-F1"] = (1, 1, 2, 1, "normal")                 # n = 1: NaN with normalize
    c["offset1000-s5x4-T17-F13"] = (5, 4, 17, 13, "offset")     # mean 1000, std 1e-3: 1 / (std + 1e-5) amplifies
    c["small_std-s7x6-T25-F80"] = (7, 6, 25, 80, "small")       # mean 0, std 1e-3: tells sqrt(var) + eps from sqrt(var + eps)
    c["constant-s4x4-T17-F16"] = (4, 4, 17, 16, "constant")     # 0.5 everywhere: exact zeros
    c["constant-s7x1-T5-F9"] = (7, 1, 5, 9, "constant")
    return c


STACK_CASES = _stack_cases()


@functools.lru_cache(maxsize=None)
def stack_input(name):
    stack, stride, T, F, kind = STACK_CASES[name]
    g = _rng(2, sorted(STACK_CASES).index(name))
    x = g.standard_normal((T, F))
    if kind == "normal":
        x = 1.5 * x - 0.7 + 0.05 * np.arange(T)[:, None]       # rows differ, so a wrong frame index shows
    elif kind == "offset":
        x = 1000.0 + 1e-3 * x
    elif kind == "small":
        x = 1e-3 * x
    elif kind == "constant":
        x = np.full((T, F), 0.5)
    return _f32(x)


# ---- augment: hand-written plans; name -> (T, F, t_masks, f_masks, subs, out_rows)
def _augment_cases():
    c = {}
    c["t1-f1-identity"] = (1, 1, [], [], [], 1)
    c["t1-f7-all16-empty"] = (1, 7, [(0, 0)] * 16, [(3, 3)] * 16, [(0, 0, 0)] * 16, 1)        # 16 of each, all empty
    c["t1-f7-masked"] = (1, 7, [(0, 0)], [(2, 4)], [(0, 1, 0)], 1)
    c["t1-f1-time-stripe"] = (1, 1, [(0, 1)], [], [], 1)
    c["t2-f1-sub"] = (2, 1, [], [], [(1, 2, 1)], 2)                                            # pos = start: row 0 -> row 1
    c["t2-f80-trim1"] = (2, 80, [(1, 2)], [(79, 80)], [(1, 2, 1)], 1)                          # stripe and sub past out_rows
    # T = 300, F = 80: 16 stripes of each kind; substitutions 5 and 6 overlap (6 wins on [120, 130)); sub 0 reads rows
    # [10, 20), inside time stripe 0, into [40, 50), outside every stripe: zeros arrive; sub 1 reads clean rows [60, 70)
    # into [100, 110), inside time stripe 1: the rows arrive intact; pos = 0 (sub 2) and pos = start (sub 3)
    t16 = [(10, 20), (100, 110), (299, 300), (0, 1), (150, 150), (200, 203)] + [(250 + k, 251 + k) for k in range(10)]
    f16 = [(0, 1), (79, 80), (30, 30), (40, 47)] + [(50 + 2 * k, 51 + 2 * k) for k in range(12)]
    s16 = [(40, 50, 30), (100, 110, 40), (70, 75, 0), (5, 9, 5), (180, 190, 7), (115, 130, 3), (120, 135, 60),
           (290, 300, 289), (220, 220, 4)] + [(230 + k, 231 + k, 1 + k) for k in range(7)]
    c["t300-f80-all16"] = (300, 80, t16, f16, s16, 300)
    c["t300-f80-all16-trim299"] = (300, 80, t16, f16, s16, 299)
    c["t300-f80-overlap-a"] = (300, 80, [], [], [(115, 130, 3), (120, 135, 60)], 300)          # the later one wins
    c["t300-f80-overlap-b"] = (300, 80, [], [], [(120, 135, 60), (115, 130, 3)], 300)          # the other order
    c["t300-f80-src-striped"] = (300, 80, [(10, 20)], [], [(40, 50, 30)], 300)
    c["t300-f80-dst-striped"] = (300, 80, [(100, 110)], [], [(100, 110, 40)], 300)
    c["t300-f7-past-out-rows"] = (300, 7, [(200, 260)], [(6, 7)], [(150, 300, 1)], 128)        # 128 * 7 = 896: not 256 k
    c["t300-f1-trim256"] = (300, 1, [(255, 257)], [], [(250, 260, 250)], 256)                  # out_rows * F = 256
    c["t300-f80-trim16"] = (300, 80, [(15, 17)], [(0, 80)], [], 16)                            # 1280 = 5 * 256; F all masked
    c["t300-f7-trim1"] = (300, 7, [], [(0, 3)], [(0, 300, 0)], 1)
    return c


AUGMENT_CASES = _augment_cases()
AUGMENT_REFUSALS = {      # name -> (T, F, t_masks, f_masks, subs, out_rows): the entry point answers -22
    "sub-end-past-T": (8, 4, [], [], [(6, 9, 1)], 8),
    "pos-beyond-start": (8, 4, [], [], [(2, 4, 3)], 8),
    "17-time-stripes": (8, 4, [(0, 1)] * 17, [], [], 8),
    "17-frequency-stripes": (8, 4, [], [(0, 1)] * 17, [], 8),
    "17-substitutions": (8, 4, [], [], [(1, 2, 1)] * 17, 8),
    "out-rows-beyond-T": (8, 4, [], [], [], 9),
}


@functools.lru_cache(maxsize=None)
def augment_input(T, F):
    """Every element distinct and nonzero: a wrong source row or a missed zero cannot hide."""
    return _f32(1.0 + np.arange(T * F).reshape(T, F) / 8.0)


# ---- BEST-RQ: name -> dict(E, V, F, T, seed, plant)
def _bestrq_cases():
    c = {}
    for name, E, V, F, T, seed in [
            ("e8-v64-f24-t97", 8, 64, 24, 97, 1),          # V below one workgroup's 256 threads; 4 frame groups
            ("e8-v1-f1-t1", 8, 1, 1, 1, 1),
            ("e8-v257-f63-t31", 8, 257, 63, 31, 1),
            ("e16-v63-f64-t32", 16, 63, 64, 32, 1),        # V below one wave; F exactly one staging chunk
            ("e16-v300-f65-t33", 16, 300, 65, 33, 1),      # one column into the second chunk; one frame into the second group
            ("e16-v256-f560-t33", 16, 256, 560, 33, 1),
            ("e16-v8192-f24-t64", 16, 8192, 24, 64, 1),
            ("e32-v257-f560-t33", 32, 257, 560, 33, 1),
            ("e32-v1024-f64-t97", 32, 1024, 64, 97, 1),
            ("e32-v300-f1-t31", 32, 300, 1, 31, 1)]:
        c[name] = dict(E=E, V=V, F=F, T=T, seed=seed, plant=None)
    # ties: the frame-0 winner duplicated bit for bit at two places; the lower index must come back
    for tag, a, b in [("same-thread", 5, 261), ("next-lane", 71, 72), ("next-wave", 10, 74), ("last-row", 37, 299)]:
        for order, (orig, copy) in (("up", (a, b)), ("down", (b, a))):
            c[f"tie-{tag}-{order}-e{16 if order == 'up' else 32}"] = dict(
                E=16 if order == "up" else 32, V=300, F=24, T=33, seed=2, plant=("tie", orig, copy))
    c["tie-same-thread-e8"] = dict(E=8, V=300, F=24, T=33, seed=2, plant=("tie", 5, 261))
    c["tiny-norm-e16"] = dict(E=16, V=300, F=24, T=33, seed=3, plant=("tiny",))     # frame 3 zero, frame 7 all 1e-30
    c["nan-e16"] = dict(E=16, V=300, F=65, T=33, seed=4, plant=("poison", float("nan")))
    c["inf-e32"] = dict(E=32, V=257, F=24, T=33, seed=4, plant=("poison", float("inf")))
    return c


BESTRQ_CASES = _bestrq_cases()
POISON_FRAME = 17


@functools.lru_cache(maxsize=None)
def bestrq_input(name):
    """dict(feat, quantizer, codebook fp32; clean = the feature matrix before a NaN / inf was planted, or None).
    Tables as BestRQTokenizer draws them (tokenizer.py:258-265): Xavier-uniform projection, unit-norm Gaussian rows."""
    k = BESTRQ_CASES[name]
    E, V, F, T = k["E"], k["V"], k["F"], k["T"]
    g = _rng(3, k["seed"], E, V, F, T)
    a = math.sqrt(6.0 / (F + E))
    q = _f32(g.uniform(-a, a, (F, E)))
    book = g.standard_normal((V, E))
    feat = _f32(g.standard_normal((T, F)))
    clean = None
    plant = k["plant"]
    if plant and plant[0] == "tiny":
        book = _f32(book / np.linalg.norm(book, axis=1, keepdims=True) * (0.5 + g.uniform(0.0, 1.0, (V, 1))))
        feat[3] = 0.0
        feat[7] = 1e-30
    else:
        book = _f32(book / np.linalg.norm(book, axis=1, keepdims=True))
    if plant and plant[0] == "tie":
        orig, copy = plant[1], plant[2]
        win = int(bestrq(feat[:1], q, book)[0][0])
        book[[win, orig]] = book[[orig, win]]          # the winner of frame 0 moves to `orig` ...
        book[copy] = book[orig]                        # ... and is copied, bit for bit, to `copy`
    if plant and plant[0] == "poison":
        clean = feat.copy()
        feat[POISON_FRAME, F // 2] = plant[1]
    return dict(feat=feat, quantizer=q, codebook=book, clean=clean)


CASES = {"log_mel": LOG_MEL_CASES, "stack": STACK_CASES, "augment": AUGMENT_CASES, "bestrq": BESTRQ_CASES}
