"""Float64 restatement of `torchaudio.transforms.Resample(orig, new)` at torchaudio's defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99) — the resampler of touchnet/data/functions.py:83-96 — written from its published
formula, independently of touchnet_amd/functional.py: the full kernel table, the strided dot products over the padded
waveform, the cut.  torchaudio itself is not available to compare with; tests/test_resample_cpu.py holds this restatement
to scipy's polyphase engine fed the same window.

Pure numpy.  Also here: the float64 evaluation of the compact polyphase sum the HIP kernel computes (`polyphase_dot`), which
the GPU tests compare the kernel with."""
import math

import numpy as np

PAIRS = [(8000, 16000), (48000, 16000), (44100, 16000), (22050, 16000), (11025, 16000), (16000, 8000), (32000, 16000)]
WIDTH, ROLLOFF = 6, 0.99


def geometry(orig, new):
    """(o, n, base, width) of a pair of rates"""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * ROLLOFF
    return o, n, base, int(math.ceil(WIDTH * o / base))


def kernel_table(orig, new):
    """(o, n, width, K): K[j][k], j < n, k < 2 width + o, in float64 — not yet rounded to float32"""
    o, n, base, width = geometry(orig, new)
    K = np.empty((n, 2 * width + o), dtype=np.float64)
    k = np.arange(2 * width + o, dtype=np.float64)
    for j in range(n):
        t = (-j / n + (k - width) / o) * base
        t = np.clip(t, -float(WIDTH), float(WIDTH))
        w = np.cos(t * math.pi / WIDTH / 2) ** 2
        t = t * math.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            K[j] = np.where(t == 0, 1.0, np.sin(t) / t) * w * (base / o)
    return o, n, width, K


def resample(x, orig, new, round_table=True):
    """x [N] -> float64 [ceil(N n / o)]: the waveform padded by (width, width + o), frame f / phase j = K[j] . padded[f o:],
    read in the order f n + j and cut.  round_table: K rounded to float32 first, as torchaudio holds it."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    o, n, width, K = kernel_table(orig, new)
    if round_table:
        K = K.astype(np.float32).astype(np.float64)
    N = x.shape[0]
    padded = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
    frames = (padded.shape[0] - K.shape[1]) // o + 1
    win = np.lib.stride_tricks.as_strided(padded, shape=(frames, K.shape[1]), strides=(o * padded.strides[0], padded.strides[0]),
                                          writeable=False)
    out = np.empty((frames, n), dtype=np.float64)
    for j in range(n):                                       # (one phase at a time keeps the products in float64 order)
        out[:, j] = (win * K[j][None, :]).sum(axis=1)
    return out.reshape(-1)[:-((-N * n) // o)]


def polyphase_dot(x, tab, o, n, m):
    """(y, mag) at the output indices m of y[m] = sum_j tab[r][j] x[i - ntap / 2 + 1 + j], i = floor(m o / n),
    r = (m o) mod n, x = 0 outside [0, N), summed in float64; mag = sum_j |tab[r][j] x[.]|."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    tab = np.asarray(tab, dtype=np.float64)
    m = np.asarray(m, dtype=np.int64)
    ntap = tab.shape[1]
    pos = m * o
    i, r = pos // n, pos % n
    idx = (i - ntap // 2 + 1)[:, None] + np.arange(ntap, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < x.shape[0])
    prod = tab[r] * np.where(inside, x[np.clip(idx, 0, x.shape[0] - 1)], 0.0)
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)
