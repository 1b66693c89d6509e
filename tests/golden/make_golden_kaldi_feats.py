"""Writes tests/golden/kaldi_mfcc_hf.npz: an independent third-party pin for Kaldi fbank / MFCC at several sample rates and
frame geometries (touchnet/data/functions.py:117-156).  torchaudio is not installed; `transformers.audio_utils` ships a
NumPy implementation written to match torchaudio.compliance.kaldi.fbank (see make_golden.py::fbank_cases), and the
cepstra are scipy's orthonormal DCT-II of its log-fbank rows times Kaldi's lifter 1 + 11 sin(pi k / 22).

Per geometry of tests/kaldi_feature_reference.py::GEOMETRIES the file holds `<name>/pcm` (int16 input), `<name>/fbank`
[frames, bins] and `<name>/mfcc` [frames, ceps] in float32, plus `seed`.  The 16 kHz inputs are the first 0.35 s of
`wav0/pcm` of logmel.npz (the reference's first test wav); the other rates are kaldi_feature_reference.synthetic_pcm.

    python tests/golden/make_golden_kaldi_feats.py
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kaldi_feature_reference as R  # noqa: E402


def hf_features(pcm, g):
    from scipy.fft import dct
    from transformers.audio_utils import mel_filter_bank, spectrogram, window_function
    win, shift, padded = R.frame_geometry(g)
    nyquist = 0.5 * g["sr"]
    high = g["high"] if g["high"] > 0.0 else nyquist + g["high"]
    mel = mel_filter_bank(num_frequency_bins=padded // 2 + 1, num_mel_filters=g["bins"], min_frequency=g["low"],
                          max_frequency=high, sampling_rate=g["sr"], norm=None, mel_scale="kaldi",
                          triangularize_in_mel_space=True)
    fb = spectrogram(pcm.astype(np.float32), window_function(win, "povey", periodic=False), frame_length=win,
                     hop_length=shift, fft_length=padded, power=2.0, center=False, preemphasis=0.97, mel_filters=mel,
                     log_mel="log", mel_floor=1.192092955078125e-07, remove_dc_offset=True).T
    k = np.arange(g["ceps"], dtype=np.float64)
    cep = dct(fb.astype(np.float64), type=2, norm="ortho", axis=1)[:, :g["ceps"]] * (1.0 + 11.0 * np.sin(math.pi * k / 22.0))
    return fb.astype(np.float32), cep.astype(np.float32)


def main():
    wav0 = np.load(os.path.join(HERE, "logmel.npz"))["wav0/pcm"]
    out = {"seed": np.int64(R.SEED)}
    for name, g in R.GEOMETRIES.items():
        pcm = wav0[:int(16000 * R.SECONDS)] if g["sr"] == 16000 else R.synthetic_pcm(g)
        fb, cep = hf_features(pcm, g)
        assert fb.shape == (R.num_frames(pcm.size, g), g["bins"]) and cep.shape == (fb.shape[0], g["ceps"])
        out[f"{name}/pcm"], out[f"{name}/fbank"], out[f"{name}/mfcc"] = pcm, fb, cep
    path = os.path.join(HERE, "kaldi_mfcc_hf.npz")
    np.savez_compressed(path, **out)
    print(f"wrote kaldi_mfcc_hf.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
