"""float64 numpy restatement of the energy VAD rule of csrc/vad.hip (Kaldi's compute-vad-energy) — log-energy, threshold,
vote, runs — and nothing else.  Written from the rule's text, not from the kernel:

  framing    win, shift in samples; T = 1 + (N - win) // shift for N >= win, else 0; frame t = samples [t shift, t shift + win)
  loge[t]    samples on the int16 scale, minus the frame's mean; E = sum d^2; log(max(E, FLT_EPSILON))
  thr        energy_threshold + energy_mean_scale * mean(loge)
  vote       den = the frames of [t - ctx, t + ctx] inside [0, T), num = those with loge > thr,
             voiced[t] = (num >= den * proportion_threshold)
  runs       the maximal intervals of voiced frames as ordered (start, end) pairs, end exclusive
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)


def num_frames(n, win, shift):
    return 0 if n < win else 1 + (n - win) // shift


def log_energy(x, win, shift):
    """x: samples on the int16 scale (any real dtype) -> float64 [T]"""
    x = np.asarray(x, dtype=np.float64)
    T = num_frames(x.size, win, shift)
    out = np.empty(T, dtype=np.float64)
    for t in range(T):
        f = x[t * shift:t * shift + win]
        d = f - f.mean()
        out[t] = np.log(max(float(np.dot(d, d)), FLT_EPSILON))
    return out


def threshold(loge, energy_threshold, energy_mean_scale):
    return float(energy_threshold) + float(energy_mean_scale) * float(np.mean(np.asarray(loge, dtype=np.float64)))


def vote(above, ctx, proportion):
    """above: bool [T] (loge > thr) -> voiced bool [T]"""
    above = np.asarray(above, dtype=bool)
    T = above.size
    c = np.concatenate([[0], np.cumsum(above.astype(np.int64))])
    t = np.arange(T)
    lo, hi = np.maximum(t - ctx, 0), np.minimum(t + ctx, T - 1)
    num, den = c[hi + 1] - c[lo], hi - lo + 1
    return num.astype(np.float64) >= den.astype(np.float64) * float(proportion)


def runs(voiced):
    """bool [T] -> int64 [R, 2]"""
    v = np.concatenate([[0], np.asarray(voiced, dtype=np.int8), [0]])
    d = np.diff(v)
    return np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1)], axis=1).astype(np.int64)


def vad(x, win, shift, energy_threshold=5.0, energy_mean_scale=0.5, ctx=0, proportion=0.6):
    loge = log_energy(x, win, shift)
    if loge.size == 0:
        return loge, 0.0, np.zeros(0, dtype=bool), np.zeros((0, 2), dtype=np.int64)
    thr = threshold(loge, energy_threshold, energy_mean_scale)
    voiced = vote(loge > thr, ctx, proportion)
    return loge, thr, voiced, runs(voiced)
