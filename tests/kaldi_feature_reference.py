"""Float64 restatement of `torchaudio.compliance.kaldi.fbank` / `.mfcc` at any sample rate and frame geometry — the
feature stages of touchnet/data/functions.py:117-156 (snip_edges, dither 0, remove_dc_offset, pre-emphasis 0.97, Povey
window, round_to_power_of_two, use_power, use_log_fbank, use_energy false, cepstral_lifter 22) — written from torchaudio's
published algorithm, independently of touchnet_amd/functional.py: DENSE mel banks `max(0, min(up, down))` over the
padded / 2 FFT bins, torchaudio's DCT matrix (`create_dct(N, N, "ortho")` with column 0 overwritten by sqrt(1 / N)) and
lifter.  torchaudio itself is not available to compare with; tests/test_kaldi_feats_cpu.py holds this restatement to
  1. Kaldi's pipeline written from its specification (tests/golden/kaldi_from_spec.py, with Kaldi's ComputeDctMatrix and
     ComputeLifterCoeffs restated here as scalar loops: `kaldi_spec_fbank` / `kaldi_spec_mfcc`), and
  2. transformers.audio_utils' Kaldi-compatible fbank with scipy's orthonormal DCT-II (tests/golden/kaldi_mfcc_hf.npz).
Pure numpy; nothing in the product imports it."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import kaldi_from_spec as K  # noqa: E402

FLT_EPSILON = 1.1920928955078125e-07
LIFTER = 22.0
FBANK_ATOL = 3e-3       # the gate tests/test_kernels_gpu.py::test_frontend_kaldi_fbank holds this arithmetic to

# name -> sample rate, frame length / shift in ms, mel bins, cepstra, low / high cutoff (high <= 0: offset from Nyquist)
GEOMETRIES = {
    "16k_25_10": dict(sr=16000, length=25, shift=10, bins=23, ceps=13, low=20.0, high=0.0),
    "8k_25_10": dict(sr=8000, length=25, shift=10, bins=23, ceps=13, low=20.0, high=-200.0),
    "16k_20_10": dict(sr=16000, length=20, shift=10, bins=40, ceps=40, low=60.0, high=7600.0),
    "48k_25_10": dict(sr=48000, length=25, shift=10, bins=80, ceps=20, low=20.0, high=0.0),
    "22k_32_8": dict(sr=22050, length=32, shift=8, bins=40, ceps=13, low=0.0, high=0.0),
    "44k_25_10": dict(sr=44100, length=25, shift=10, bins=64, ceps=20, low=20.0, high=0.0),
    # 80 bins at 8 kHz: the narrowest triangle (33 Hz at 20 Hz) is still wider than an FFT bin (31.25 Hz), so every mel
    # bin holds one and Kaldi accepts it; 128 bins (21 Hz) leave mel bins that no FFT bin falls into
    "8k_80bins": dict(sr=8000, length=25, shift=10, bins=80, ceps=13, low=20.0, high=0.0),
    "8k_128bins": dict(sr=8000, length=25, shift=10, bins=128, ceps=13, low=20.0, high=0.0),
}
EMPTY_BINS = ("8k_128bins",)         # Kaldi itself raises on these; torchaudio's dense banks give log(FLT_EPSILON)
KALDI_ACCEPTS = tuple(k for k in GEOMETRIES if k not in EMPTY_BINS)
SECONDS = 0.35
SEED = 20251


def frame_geometry(g):
    """(win, shift, padded) in samples"""
    win, shift = int(g["sr"] * g["length"] * 0.001), int(g["sr"] * g["shift"] * 0.001)
    return win, shift, 1 << (win - 1).bit_length()


def num_frames(n, g):
    win, shift, _ = frame_geometry(g)
    return 0 if n < win else 1 + (n - win) // shift


def synthetic_pcm(g, seconds=SECONDS, seed=SEED):
    """int16: two tones (sr / 37 and sr / 5.3 Hz) plus a uniform noise floor in every band, so that no mel bin an FFT bin
    falls into is near-empty"""
    n = int(g["sr"] * seconds)
    rng = np.random.default_rng(seed + g["sr"])
    t = np.arange(n, dtype=np.float64) / g["sr"]
    x = 0.3 * np.sin(2 * math.pi * (g["sr"] / 37.0) * t) + 0.1 * np.sin(2 * math.pi * (g["sr"] / 5.3) * t) \
        + 0.05 * rng.uniform(-1.0, 1.0, n)
    return np.round(x * 32767.0).astype(np.int16)


def tables(g):
    """float64 (window [win], dense banks [bins, padded / 2], lifter . DCT [ceps, bins])"""
    win, _, padded = frame_geometry(g)
    n = np.arange(win, dtype=np.float64)
    window = (0.5 - 0.5 * np.cos(2.0 * math.pi * n / (win - 1))) ** 0.85
    nyquist = 0.5 * g["sr"]
    high = g["high"] if g["high"] > 0.0 else nyquist + g["high"]
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    mel_lo, mel_hi = mel(g["low"]), mel(high)
    delta = (mel_hi - mel_lo) / (g["bins"] + 1)
    b = np.arange(g["bins"], dtype=np.float64)[:, None]
    left, center, right = mel_lo + b * delta, mel_lo + (b + 1.0) * delta, mel_lo + (b + 2.0) * delta
    m = mel((g["sr"] / padded) * np.arange(padded // 2, dtype=np.float64))[None, :]
    banks = np.maximum(0.0, np.minimum((m - left) / (center - left), (right - m) / (right - center)))
    N = g["bins"]
    k = np.arange(g["ceps"], dtype=np.float64)[:, None]
    dct = np.cos(math.pi / N * (np.arange(N, dtype=np.float64)[None, :] + 0.5) * k) * math.sqrt(2.0 / N)
    dct[0] = math.sqrt(1.0 / N)
    lifter = 1.0 + 0.5 * LIFTER * np.sin(math.pi * k / LIFTER)
    return window, banks, lifter * dct


def fbank(wav, g, window=None, banks=None):
    """wav in [-1, 1) [N] -> float64 [frames, bins] (`[0, bins]` for less than one window).  window / banks: tables to use
    instead of the float64 ones (the float32 tables the kernel reads, widened)."""
    win, shift, padded = frame_geometry(g)
    w64, b64, _ = tables(g)
    window = w64 if window is None else np.asarray(window, dtype=np.float64)
    banks = b64 if banks is None else np.asarray(banks, dtype=np.float64)
    x = np.asarray(wav, dtype=np.float64).reshape(-1) * 32768.0
    m = num_frames(x.size, g)
    if m == 0:
        return np.zeros((0, g["bins"]))
    fr = x[np.arange(win)[None, :] + shift * np.arange(m)[:, None]]
    fr = fr - fr.mean(axis=1, keepdims=True)
    fr = fr - 0.97 * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = np.pad(fr * window[None, :], ((0, 0), (0, padded - win)))
    spec = np.fft.rfft(fr, axis=-1)[:, :padded // 2]                    # (the Nyquist column carries zero weight)
    return np.log(np.maximum((spec.real ** 2 + spec.imag ** 2) @ banks.T, FLT_EPSILON))


def mfcc(wav, g):
    """-> float64 [frames, ceps]"""
    return fbank(wav, g) @ tables(g)[2].T


def mfcc_bound(g, atol=FBANK_ATOL):
    """per cepstrum: the fbank gate pushed through the matrix, lifter_k sum_n |D[k, n]| atol"""
    return np.abs(tables(g)[2]).sum(axis=1) * atol


# ---- Kaldi from its specification (second pin)
def _kaldi_opts(g):
    return K.FbankOptions(K.FrameExtractionOptions(samp_freq=float(g["sr"]), dither=0.0, frame_length_ms=float(g["length"]),
                                                   frame_shift_ms=float(g["shift"])),
                          K.MelBanksOptions(num_bins=g["bins"], low_freq=g["low"], high_freq=g["high"]), energy_floor=0.0)


def kaldi_spec_fbank(pcm_int16, g):
    return K.compute_fbank_feats(pcm_int16, _kaldi_opts(g))


def kaldi_spec_mfcc(pcm_int16, g):
    """feature-mfcc.cc: ComputeDctMatrix (row 0 sqrt(1 / N), row k sqrt(2 / N) cos(pi / N (n + 0.5) k)), its first num_ceps
    rows applied to the log mel energies, then ComputeLifterCoeffs 1 + 0.5 Q sin(pi i / Q)"""
    fb = kaldi_spec_fbank(pcm_int16, g)
    N, C = g["bins"], g["ceps"]
    out = np.zeros((fb.shape[0], C))
    for k in range(C):
        row = [math.sqrt(1.0 / N) if k == 0 else math.sqrt(2.0 / N) * math.cos(math.pi / N * (n + 0.5) * k)
               for n in range(N)]
        lift = 1.0 + 0.5 * LIFTER * math.sin(math.pi * k / LIFTER)
        for t in range(fb.shape[0]):
            out[t, k] = lift * sum(row[n] * fb[t, n] for n in range(N))
    return out
