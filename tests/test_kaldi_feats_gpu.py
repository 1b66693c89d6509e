"""csrc/kaldi_feats.hip (tn_kaldi_feats) on the device: Kaldi log-fbank and MFCC at any sample rate and frame geometry
against the float64 restatement of torchaudio's algorithm (tests/kaldi_feature_reference.py; tests/test_kaldi_feats_cpu.py
holds that restatement to from-spec Kaldi and to transformers.audio_utils + scipy's DCT, and the float32 tables the kernel
reads to the restatement's, bit for bit).

Gates:
  fbank    atol 3e-3 on the log energies, the gate of tests/test_kernels_gpu.py::test_frontend_kaldi_fbank for this
           arithmetic (every input has a noise floor: the tolerance is absolute on a log and cannot hold for a mel bin of
           pure cancellation; a bin no FFT bin falls into is exactly log(FLT_EPSILON) on both sides)
  MFCC     per cepstrum k, lifter_k sum_n |D[k, n]| 3e-3: the fbank gate pushed through the matrix
  DCT      the kernel's own fbank rows through the float64 product with the float32 table: N fused multiply-adds leave at
           most (N + 1) 2^-24 sum_n |tab[k, n] logmel[n]|
Each comparison prints its worst error (as a fraction of the bound where the bound is derived).  Measured on an MI355X:
fbank worst 9.1e-5 (44.1 kHz), MFCC worst 0.0030 of the bound, DCT stage worst 0.14 of the bound."""
import ctypes as C
import types
import wave

import numpy as np
import pytest
import torch

import kaldi_feature_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRID_CAP = 2048                  # workgroups of one launch: more frames than this go round the grid-stride loop
LOG_EPS = float(np.log(np.float32(R.FLT_EPSILON)))


def _F():
    import touchnet_amd.functional as F
    return F


def _L():
    import touchnet_amd.library as L
    return L


def _geo(sr, length, shift, bins=23, ceps=13, low=20.0, high=0.0):
    return dict(sr=sr, length=length, shift=shift, bins=bins, ceps=ceps, low=low, high=high)


def _signal(g, n, seed=0):
    """float32 in [-1, 1): a tone at sr / 29 Hz over a uniform noise floor"""
    rng = np.random.default_rng(seed + n)
    t = np.arange(n, dtype=np.float64)
    return (0.25 * np.sin(2 * np.pi * t / 29.0) + 0.05 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


def _fbank(x, g):
    return _F().kaldi_fbank(torch.from_numpy(x).to(DEV), g["bins"], sample_rate=g["sr"], frame_length=g["length"],
                            frame_shift=g["shift"], low_freq=g["low"], high_freq=g["high"])


def _mfcc(x, g):
    return _F().kaldi_mfcc(torch.from_numpy(x).to(DEV), g["sr"], g["bins"], g["ceps"], g["length"], g["shift"], g["low"],
                           g["high"])


def _check_fbank(x, g, what):
    got, want = _fbank(x, g).cpu().numpy(), R.fbank(x, g)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"{what}: {got.shape[0]} frames, fbank worst error {err:.2e} (gate {R.FBANK_ATOL})")
    assert np.isfinite(got).all() and err <= R.FBANK_ATOL, (what, err)
    return got


def _device_tables(g, mfcc=True):
    t = _F().kaldi_feature_tables(g["sr"], g["length"], g["shift"], g["bins"], g["low"], g["high"], g["ceps"] if mfcc else None)
    dev = lambda a, dt: torch.from_numpy(a).to(dt).to(DEV).contiguous()
    return t, dev(t["window"], torch.float32), dev(t["bank_idx"], torch.int32), dev(t["bank_w"], torch.float32), \
        (dev(t["dct"], torch.float32) if mfcc else None)


@pytest.fixture(scope="module")
def hf(golden):
    return golden("kaldi_mfcc_hf.npz")


# ------------------------------------------------------------------------------------------------------ fbank mode
@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_fbank_at_every_fixture_geometry(hf, name):
    g = R.GEOMETRIES[name]
    x = hf[f"{name}/pcm"].astype(np.float32) / 32768.0
    got = _check_fbank(x, g, name)
    err = float(np.abs(got - hf[f"{name}/fbank"]).max())
    print(f"{name}: against transformers.audio_utils {err:.2e}")
    assert err <= R.FBANK_ATOL
    empty = R.tables(g)[1].sum(axis=1) == 0
    assert bool(empty.any()) == (name in R.EMPTY_BINS)
    if empty.any():                                                   # no FFT bin inside the triangle: log(FLT_EPSILON)
        assert (got[:, empty] == np.float32(LOG_EPS)).all()


def test_fbank_at_the_recipes_geometry_against_the_80_bin_fixture(golden):
    """16 kHz 25 / 10, 80 bins, the reference's two test wavs against the third-party fixture
    (tests/golden/kaldi_fbank_hf.npz), at the same gate; `kaldi_fbank`'s defaults are that geometry, bit for bit"""
    g, wavs, F = _geo(16000, 25, 10, bins=80), golden("logmel.npz"), _F()
    fix = golden("kaldi_fbank_hf.npz")
    for i in (0, 1):
        x = wavs[f"wav{i}/pcm"].astype(np.float32) / 32768.0
        got = _fbank(x, g).cpu().numpy()
        err = float(np.abs(got - fix[f"wav{i}/fbank80"]).max())
        print(f"wav{i}: {got.shape[0]} frames, against kaldi_fbank_hf.npz {err:.2e}")
        assert got.shape == fix[f"wav{i}/fbank80"].shape and err <= R.FBANK_ATOL
        x = torch.from_numpy(x).to(DEV)
        assert torch.equal(F.kaldi_fbank(x, 80), F.kaldi_fbank(x, 80, sample_rate=16000, frame_length=25, frame_shift=10))


@pytest.mark.parametrize("g", [_geo(8000, 25, 10), _geo(22050, 32, 8, bins=40, low=0.0)], ids=["8k", "22k"])
def test_frame_counts_around_one_window_and_one_shift(g):
    win, shift, _ = R.frame_geometry(g)
    for n, frames in ((win - 1, 0), (win, 1), (win + shift - 1, 1), (win + shift, 2)):
        got = _check_fbank(_signal(g, n), g, f"{n} samples")
        assert got.shape == (frames, g["bins"])
        assert tuple(_mfcc(_signal(g, n), g).shape) == (frames, g["ceps"])


def test_more_frames_than_workgroups_go_round_the_grid_stride_loop():
    g = _geo(8000, 25, 10)
    n = 165000
    assert R.num_frames(n, g) > GRID_CAP
    _check_fbank(_signal(g, n), g, "8 kHz, 165000 samples")


def test_window_that_fills_the_fft_and_odd_window():
    g = _geo(16000, 32, 10, bins=40)
    assert R.frame_geometry(g)[0] == R.frame_geometry(g)[2] == 512
    _check_fbank(_signal(g, 512 + 7 * 160 + 3), g, "win == padded")
    g = _geo(22050, 25, 10, bins=40)
    assert R.frame_geometry(g)[0] == 551
    _check_fbank(_signal(g, 551 + 9 * 220 + 100), g, "odd window")
    g = _geo(16000, 128, 10, bins=40)                                   # the largest FFT with a full window
    assert R.frame_geometry(g)[0] == R.frame_geometry(g)[2] == 2048
    _check_fbank(_signal(g, 2048 + 5 * 160), g, "win == padded == 2048")
    g = _geo(8000, 4, 2, bins=4, ceps=4, low=0.0)                       # the smallest: 32 samples, fewer butterflies than threads
    assert R.frame_geometry(g) == (32, 16, 32)
    _check_fbank(_signal(g, 32 + 40 * 16), g, "padded 32")


# ------------------------------------------------------------------------------------------------------ MFCC mode
@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_mfcc_end_to_end(hf, name):
    g = R.GEOMETRIES[name]
    x = hf[f"{name}/pcm"].astype(np.float32) / 32768.0
    got, want, bound = _mfcc(x, g).cpu().numpy(), R.mfcc(x, g), R.mfcc_bound(g)
    assert got.shape == want.shape
    frac = float((np.abs(got - want) / bound[None, :]).max())
    print(f"{name}: MFCC worst error {float(np.abs(got - want).max()):.2e}, {frac:.4f} of the bound")
    assert np.isfinite(got).all() and frac <= 1.0, (name, frac)


@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_dct_stage_on_the_kernels_own_fbank_rows(hf, name):
    """MFCC mode with the identity for `dct` returns its log-fbank rows untouched (fma(1, v, 0) and fma(0, v, acc) are
    exact): they equal fbank mode's bit for bit.  Then the real table: within the dot product's own bound of the float64
    product of the float32 table with those rows."""
    L, g = _L(), R.GEOMETRIES[name]
    x = torch.from_numpy(hf[f"{name}/pcm"].astype(np.float32) / 32768.0).to(DEV)
    t, window, idx, w, dct = _device_tables(g)
    args = (g["sr"], t["shift"], g["low"], g["high"])
    fb = L.kaldi_feats(x, window, idx, w, *args)
    through = L.kaldi_mfcc(x, window, idx, w, torch.eye(g["bins"], device=DEV), *args)
    assert torch.equal(fb, through), name
    got = L.kaldi_mfcc(x, window, idx, w, dct, *args).cpu().numpy().astype(np.float64)
    tab, rows = dct.cpu().numpy().astype(np.float64), fb.cpu().numpy().astype(np.float64)
    want = rows @ tab.T
    bound = (g["bins"] + 1) * 2.0 ** -24 * (np.abs(rows)[:, None, :] * np.abs(tab)[None, :, :]).sum(axis=2) + 1e-30
    frac = float((np.abs(got - want) / bound).max())
    print(f"{name}: DCT stage worst error {frac:.3f} of the bound")
    assert frac <= 1.0, (name, frac)


# ------------------------------------------------------------------------------------------------------ the raw entry
def _raw(lib, wav_t, out_t, g, t, window_t, idx_t, w_t, dct_t, **over):
    """tn_kaldi_feats with the geometry of `g` and its tables, single arguments replaced by `over`"""
    a = dict(wav=wav_t.data_ptr(), out=out_t.data_ptr(), n=wav_t.numel(), sr=g["sr"], win=t["win"], shift=t["shift"],
             padded=t["padded"], bins=g["bins"], ceps=0 if dct_t is None else g["ceps"], low=g["low"], high=g["high"],
             window=window_t.data_ptr(), idx=idx_t.data_ptr(), w=w_t.data_ptr(), n_w=w_t.numel(),
             dct=None if dct_t is None else dct_t.data_ptr())
    a.update(over)
    return lib.tn_kaldi_feats(a["wav"], a["out"], a["n"], a["sr"], a["win"], a["shift"], a["padded"], a["bins"], a["ceps"],
                              a["low"], a["high"], a["window"], a["idx"], a["w"], a["n_w"], a["dct"],
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("mode", ["fbank", "mfcc"])
def test_repeated_calls_are_bit_identical_and_stay_inside_the_output(mode):
    from touchnet_amd import _C
    g = R.GEOMETRIES["44k_25_10"]
    t, window, idx, w, dct = _device_tables(g, mfcc=mode == "mfcc")
    x = torch.from_numpy(_signal(g, 44100 // 2)).to(DEV)
    cols = g["ceps"] if mode == "mfcc" else g["bins"]
    n = R.num_frames(x.numel(), g) * cols
    outs = []
    for _ in range(3):
        out = torch.full((n + 4096,), -12345.0, device=DEV)
        _C.check(_raw(_C.lib(), x, out, g, t, window, idx, w, dct), "tn_kaldi_feats")
        assert (out[n:] == -12345.0).all() and not (out[:n] == -12345.0).any()
        outs.append(out[:n].clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    want = (_mfcc if mode == "mfcc" else _fbank)(x.cpu().numpy(), g)
    assert torch.equal(outs[0].view(-1, cols), want)


def test_refused_arguments_raise_before_any_launch():
    from touchnet_amd import _C
    g = R.GEOMETRIES["16k_25_10"]
    t, window, idx, w, dct = _device_tables(g)
    x = torch.from_numpy(_signal(g, 4000)).to(DEV)
    out = torch.full((R.num_frames(4000, g) * g["bins"],), 7.0, device=DEV)
    big = torch.zeros(4096, device=DEV)
    refused = dict(
        padded_4096=dict(win=2100, padded=4096, window=big.data_ptr()), padded_16=dict(win=16, padded=16),
        padded_not_of_win=dict(padded=1024), padded_no_power_of_two=dict(padded=500), win_above_padded=dict(win=513),
        shift_0=dict(shift=0), bins_3=dict(bins=3), bins_257=dict(bins=257), ceps_above_bins=dict(ceps=g["bins"] + 1),
        ceps_negative=dict(ceps=-1), low_not_below_high=dict(low=4000.0, high=4000.0), low_negative=dict(low=-1.0),
        high_above_nyquist=dict(high=8000.5), high_offset_below_low=dict(high=-7990.0), mfcc_without_dct=dict(dct=None),
        weights_past_the_fft=dict(n_w=513), null_window=dict(window=None), null_banks=dict(idx=None),
        null_output=dict(out=None), output_is_input=dict(out=x.data_ptr()), negative_length=dict(n=-1),
        rate_0=dict(sr=0))
    for what, over in refused.items():
        with pytest.raises(_C.KernelError, match="-22"):
            _C.check(_raw(_C.lib(), x, out, g, t, window, idx, w, dct, **over), f"tn_kaldi_feats[{what}]")
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    _C.check(_raw(_C.lib(), x, out, g, t, window, idx, w, dct), "tn_kaldi_feats")          # (and the untouched call runs)
    assert not (out[:R.num_frames(4000, g) * g["ceps"]] == 7.0).any()
    F = _F()
    for kw, field in ((dict(num_ceps=24), "audiofeat_num_ceps"), (dict(num_mel_bins=3, num_ceps=2), "audiofeat_num_mel_bins"),
                      (dict(frame_length=200), "audiofeat_frame_length"), (dict(low_freq=9000.0), "audiofeat_low_freq")):
        a = dict(sample_rate=16000, num_mel_bins=23, num_ceps=13, frame_length=25, frame_shift=10, low_freq=20.0,
                 high_freq=0.0)
        a.update(kw)
        with pytest.raises(ValueError, match=field):
            F.kaldi_mfcc(x, **a)


def test_opcheck():
    g = R.GEOMETRIES["8k_25_10"]
    t, window, idx, w, dct = _device_tables(g)
    args = (g["sr"], t["shift"], g["low"], g["high"])
    for n in (199, 200, 1000):
        x = torch.from_numpy(_signal(g, n)).to(DEV)
        torch.library.opcheck(torch.ops.mi355_touch.kaldi_feats.default, (x, window, idx, w, *args))
        torch.library.opcheck(torch.ops.mi355_touch.kaldi_mfcc.default, (x, window, idx, w, dct, *args))


# ------------------------------------------------------------------------------------------------------ stages
def _cfg(**kw):
    d = dict(audio_feat_type="mfcc", audio_resample_rate=8000, audiofeat_dither=0.0, audiofeat_frame_length=25,
             audiofeat_frame_shift=10, audiofeat_num_mel_bins=23, audiofeat_num_ceps=13, audiofeat_low_freq=20.0,
             audiofeat_high_freq=0.0, audiofeat_stack_length=7, audiofeat_stride_length=6, audiofeat_normalize=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _check_mfcc(got, x, g, what):
    want, bound = R.mfcc(x, g), R.mfcc_bound(g)
    assert tuple(got.shape) == want.shape, (what, got.shape, want.shape)
    frac = float((np.abs(got.cpu().numpy() - want) / bound[None, :]).max())
    print(f"{what}: {frac:.4f} of the MFCC bound")
    assert frac <= 1.0, (what, frac)


def test_stage_audio_compute_mfcc_on_int16_and_float_samples(hf):
    from touchnet_amd.data import functions as stages
    g = dict(R.GEOMETRIES["8k_25_10"], high=0.0)
    pcm = hf["8k_25_10/pcm"]
    x = pcm.astype(np.float32) / 32768.0
    samples = [{"sample_rate": 8000, "waveform": torch.from_numpy(pcm.copy())[None]},
               {"sample_rate": 8000, "waveform": torch.from_numpy(x)[None]}]
    a, b = list(stages.audio_compute_mfcc(iter(samples), _cfg()))
    _check_mfcc(a["audiofeat"], x, g, "audio_compute_mfcc")
    assert a["audiofeat"].is_cuda and torch.equal(a["audiofeat"], b["audiofeat"])
    with pytest.raises(ValueError, match="audiofeat_dither"):
        next(stages.audio_compute_mfcc(iter(samples), _cfg(audiofeat_dither=0.1)))
    with pytest.raises(ValueError, match="audiofeat_dither"):
        next(stages.audio_compute_fbank(iter(samples), _cfg(audiofeat_dither=0.1)))


def test_stage_fbank_behind_a_resample_to_8_khz(golden):
    """A 16 kHz sample through audio_resample to 8000 and audio_compute_fbank: the fbank of the waveform the resample stage
    produced, at 8 kHz"""
    from touchnet_amd.data import functions as stages
    pcm = golden("logmel.npz")["wav0/pcm"][:16000]
    cfg = _cfg(audio_feat_type="fbank", audiofeat_num_mel_bins=40)
    s = next(stages.audio_compute_fbank(stages.audio_resample(iter([{"sample_rate": 16000,
                                                                      "waveform": torch.from_numpy(pcm.copy())[None]}]), cfg), cfg))
    assert s["sample_rate"] == 8000 and s["waveform"].shape == (1, 8000)
    g = _geo(8000, 25, 10, bins=40)
    want = R.fbank(s["waveform"].cpu().numpy().reshape(-1), g)
    err = float(np.abs(s["audiofeat"].cpu().numpy() - want).max())
    print(f"resample + fbank at 8 kHz: worst error {err:.2e}")
    assert s["audiofeat"].shape == (98, 40) and err <= R.FBANK_ATOL


def test_stage_fbank_at_the_recipes_geometry_takes_the_one_kernel(golden):
    from touchnet_amd.data import functions as stages
    F = _F()
    pcm = torch.from_numpy(golden("logmel.npz")["wav0/pcm"][:16000].copy())
    cfg = _cfg(audio_feat_type="fbank", audio_resample_rate=16000, audiofeat_num_mel_bins=80)
    s = next(stages.audio_compute_fbank(iter([{"sample_rate": 16000, "waveform": pcm[None]}]), cfg))
    assert torch.equal(s["audiofeat"], F.kaldi_fbank(F.pcm16_to_float(pcm.to(DEV)), 80))
    s = next(stages.audio_compute_fbank(iter([{"sample_rate": 16000, "waveform": pcm[None]}]),
                                        _cfg(audio_feat_type="fbank", audiofeat_num_mel_bins=80, audiofeat_frame_length=20)))
    _ = s["audiofeat"].cpu().numpy()
    err = float(np.abs(_ - R.fbank(pcm.numpy().astype(np.float32) / 32768.0, _geo(16000, 20, 10, bins=80))).max())
    assert _.shape == (99, 80) and err <= R.FBANK_ATOL, err


def test_infer_asr_features_take_mfcc(tmp_path, hf):
    from touchnet_amd.bin import infer_asr
    pcm = hf["8k_25_10/pcm"]
    with wave.open(str(tmp_path / "a.wav"), "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(8000), f.writeframes(pcm.tobytes())
    cfg = _cfg(audiofeat_stack_length=1, audiofeat_stride_length=1)
    w = infer_asr.read_wav(str(tmp_path / "a.wav"), cfg.audio_resample_rate)
    assert w.dtype == torch.int16 and w.shape == (1, pcm.size)                         # at the config's rate: untouched
    feats = infer_asr.features([w], cfg)
    _check_mfcc(feats[0], pcm.astype(np.float32) / 32768.0, dict(R.GEOMETRIES["8k_25_10"], high=0.0), "infer_asr.features")
    for k in ("audiofeat_num_ceps", "audiofeat_low_freq", "audiofeat_high_freq"):
        assert k in infer_asr._DATA_DEFAULTS


def test_stacking_mfcc_rows(hf):
    """audiofeat_stack at F = num_ceps.  Without normalisation the stage only gathers rows, so the MFCC bound holds
    element for element against the oracle's stack of the restatement; with it, the stack kernel against the oracle's stack
    of the same device rows at the stack kernel's own gate (tests/test_kernels_gpu.py::test_frontend_stack, 5e-5)."""
    from oracle import frontend as ofe
    from touchnet_amd.data import functions as stages
    g = dict(R.GEOMETRIES["8k_25_10"], high=0.0)
    pcm = hf["8k_25_10/pcm"]
    x = pcm.astype(np.float32) / 32768.0
    sample = lambda: iter([{"sample_rate": 8000, "waveform": torch.from_numpy(pcm.copy())[None]}])
    cfg = _cfg()
    got = next(stages.audiofeat_stack(stages.audio_compute_mfcc(sample(), cfg), cfg))["audiofeat"].cpu().numpy()
    want = ofe.audiofeat_stack(R.mfcc(x, g), 7, 6, False)
    bound = np.tile(R.mfcc_bound(g), 7)
    assert got.shape == want.shape == (6, 7 * 13)
    frac = float((np.abs(got - want) / bound[None, :]).max())
    print(f"stacked MFCC: {frac:.4f} of the bound")
    assert frac <= 1.0
    cfg = _cfg(audiofeat_normalize=True)
    rows = next(stages.audio_compute_mfcc(sample(), cfg))["audiofeat"]
    got = _F().audiofeat_stack(rows, 7, 6, True).cpu().numpy()
    np.testing.assert_allclose(got, ofe.audiofeat_stack(rows.cpu().numpy(), 7, 6, True), atol=5e-5)
