"""Kaldi fbank / MFCC at any sample rate and frame geometry, the parts that need no GPU:
  - the float64 restatement of torchaudio's algorithm (tests/kaldi_feature_reference.py) against Kaldi's pipeline written
    from its specification and against transformers.audio_utils + scipy's orthonormal DCT-II (tests/golden/
    kaldi_mfcc_hf.npz).  Gates 1e-5 (log-fbank) and 2e-4 (MFCC, values in [-120, 185]): ten times the 1.0e-6 / 1.8e-5 the
    two third-party float32 pipelines were measured at, so that another input lands inside their rounding too.  Measured
    here: from-spec 3.3e-13 / 9.7e-13, fixture 1.01e-6 / 2.2e-5;
  - the host tables the kernel reads (functional.kaldi_feature_tables) against the restatement's, bit for bit as float32;
  - the refusals, by field name, of the functional layer, the stages, build_datapipe and the C entry point (which refuses
    on the host before it touches a pointer);
  - the `mfcc` branch of build_datapipe and the ops' fake kernels."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import kaldi_feature_reference as R

FBANK_GATE, MFCC_GATE = 1e-5, 2e-4


@pytest.fixture(scope="module")
def hf(golden):
    return golden("kaldi_mfcc_hf.npz")


def _wave(hf, name):
    return hf[f"{name}/pcm"].astype(np.float32) / 32768.0


def _F():
    import touchnet_amd.functional as F
    return F


# ------------------------------------------------------------------------------------------------------ the restatement
def test_fixture_inputs_are_what_the_maker_says(hf, golden):
    assert int(hf["seed"]) == R.SEED
    wav0 = golden("logmel.npz")["wav0/pcm"]
    for name, g in R.GEOMETRIES.items():
        want = wav0[:int(16000 * R.SECONDS)] if g["sr"] == 16000 else R.synthetic_pcm(g)
        assert np.array_equal(hf[f"{name}/pcm"], want), name
        assert hf[f"{name}/fbank"].shape == (R.num_frames(want.size, g), g["bins"])
        assert hf[f"{name}/mfcc"].shape == (R.num_frames(want.size, g), g["ceps"])


@pytest.mark.parametrize("name", R.KALDI_ACCEPTS)
def test_restatement_against_kaldi_from_its_specification(hf, name):
    g, pcm = R.GEOMETRIES[name], hf[f"{name}/pcm"]
    fb = float(np.abs(R.fbank(_wave(hf, name), g) - R.kaldi_spec_fbank(pcm, g)).max())
    mf = float(np.abs(R.mfcc(_wave(hf, name), g) - R.kaldi_spec_mfcc(pcm, g)).max())
    print(f"{name}: from-spec Kaldi fbank {fb:.2e}, MFCC {mf:.2e}")
    assert fb <= FBANK_GATE and mf <= MFCC_GATE, (name, fb, mf)


@pytest.mark.parametrize("name", R.KALDI_ACCEPTS)
def test_restatement_against_the_third_party_fixture(hf, name):
    g = R.GEOMETRIES[name]
    fb = float(np.abs(R.fbank(_wave(hf, name), g) - hf[f"{name}/fbank"]).max())
    mf = float(np.abs(R.mfcc(_wave(hf, name), g) - hf[f"{name}/mfcc"]).max())
    print(f"{name}: transformers.audio_utils fbank {fb:.2e}, scipy DCT MFCC {mf:.2e}")
    assert fb <= FBANK_GATE and mf <= MFCC_GATE, (name, fb, mf)


@pytest.mark.parametrize("name", R.EMPTY_BINS)
def test_a_mel_bin_without_an_fft_bin_is_log_epsilon(hf, name):
    """torchaudio's dense banks leave an all-zero row, so the energy is floored; Kaldi itself refuses the configuration"""
    g = R.GEOMETRIES[name]
    empty = R.tables(g)[1].sum(axis=1) == 0
    assert empty.any() and not empty.all()
    fb = R.fbank(_wave(hf, name), g)
    assert (fb[:, empty] == np.log(R.FLT_EPSILON)).all() and (fb[:, ~empty] > 0.0).all()
    with pytest.raises(ValueError, match="empty mel bin"):
        R.kaldi_spec_fbank(hf[f"{name}/pcm"], g)
    t = _F().kaldi_feature_tables(g["sr"], g["length"], g["shift"], g["bins"], g["low"], g["high"])
    assert np.array_equal(t["bank_idx"][:, 1] == 0, empty)


def test_restatement_of_a_short_waveform_is_empty():
    g = R.GEOMETRIES["8k_25_10"]
    assert R.fbank(np.zeros(199, dtype=np.float32), g).shape == (0, 23)
    assert R.mfcc(np.zeros(199, dtype=np.float32), g).shape == (0, 13)
    assert R.fbank(np.ones(200, dtype=np.float32), g).shape == (1, 23)


# ------------------------------------------------------------------------------------------------------ host tables
def _dense32(t, padded):
    dense = np.zeros((t["bank_idx"].shape[0], padded // 2), dtype=np.float32)
    for r, (first, count, off) in enumerate(t["bank_idx"]):
        dense[r, first:first + count] = t["bank_w"][off:off + count].astype(np.float32)
    return dense


@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_host_tables_equal_the_restatements_as_float32(name):
    g = R.GEOMETRIES[name]
    t = _F().kaldi_feature_tables(g["sr"], g["length"], g["shift"], g["bins"], g["low"], g["high"], g["ceps"])
    window, banks, dct = R.tables(g)
    win, shift, padded = R.frame_geometry(g)
    assert (t["win"], t["shift"], t["padded"]) == (win, shift, padded)
    assert t["window"].dtype == np.float64 and np.array_equal(t["window"].astype(np.float32), window.astype(np.float32))
    assert np.array_equal(t["dct"].astype(np.float32), dct.astype(np.float32)) and t["dct"].shape == (g["ceps"], g["bins"])
    banks32 = banks.astype(np.float32)
    assert np.array_equal(_dense32(t, padded), banks32)              # (so every weight the sparse form leaves out is 0.0f)
    idx = t["bank_idx"]
    assert idx.dtype == np.int32 and idx.shape == (g["bins"], 3)
    assert int(idx[:, 1].sum()) == t["bank_w"].size <= padded and (idx[:, 0] + idx[:, 1] <= padded // 2).all()
    assert np.array_equal(idx[:, 2], np.concatenate([[0], np.cumsum(idx[:, 1])[:-1]]))
    for r in range(g["bins"]):                                         # the kept span starts and ends on a non-zero weight
        if idx[r, 1]:
            assert banks32[r, idx[r, 0]] != 0 and banks32[r, idx[r, 0] + idx[r, 1] - 1] != 0
    assert _F().kaldi_feature_tables(g["sr"], g["length"], g["shift"], g["bins"], g["low"], g["high"])["dct"] is None


@pytest.mark.parametrize("sr,length,padded", [(8000, 25, 256), (16000, 25, 512), (22050, 32, 1024), (48000, 25, 2048),
                                              (16000, 128, 2048), (16000, 2, 32)])
def test_table_sizes(sr, length, padded):
    t = _F().kaldi_feature_tables(sr, length, 10, 40, 20.0, 0.0, 13)
    win = int(sr * length * 0.001)
    assert t["padded"] == padded and t["window"].shape == (win,) and padded // 2 < win <= padded
    assert t["bank_idx"].shape == (40, 3) and t["dct"].shape == (13, 40)
    assert 0 < t["bank_w"].size <= padded                              # an FFT bin lies in at most two triangles
    assert t["window"][0] == 0.0 and 0.99 < t["window"][win // 2] <= t["window"].max() <= 1.0


# ------------------------------------------------------------------------------------------------------ refusals
_OK = dict(sample_rate=16000, frame_length=25, frame_shift=10, num_mel_bins=23, low_freq=20.0, high_freq=0.0, num_ceps=13)


@pytest.mark.parametrize("over,field", [
    (dict(num_ceps=24), "audiofeat_num_ceps"), (dict(num_ceps=0), "audiofeat_num_ceps"),
    (dict(num_mel_bins=3, num_ceps=2), "audiofeat_num_mel_bins"), (dict(num_mel_bins=257), "audiofeat_num_mel_bins"),
    (dict(frame_length=129), "audiofeat_frame_length"), (dict(sample_rate=96000), "audiofeat_frame_length"),
    (dict(frame_length=1), "audiofeat_frame_length"), (dict(frame_shift=0), "audiofeat_frame_shift"),
    (dict(low_freq=8000.0), "audiofeat_low_freq"), (dict(low_freq=300.0, high_freq=300.0), "audiofeat_low_freq"),
    (dict(high_freq=8001.0), "audiofeat_high_freq"), (dict(high_freq=-7990.0), "audiofeat_high_freq"),
    (dict(low_freq=-1.0), "audiofeat_low_freq"), (dict(sample_rate=0), "sample_rate")])
def test_tables_refuse_by_field_name(over, field):
    with pytest.raises(ValueError, match=field):
        _F().kaldi_feature_tables(**dict(_OK, **over))
    _F().kaldi_feature_tables(**_OK)


def test_stages_refuse_dither_and_say_why():
    from touchnet_amd.data import functions as stages
    cfg = types.SimpleNamespace(audiofeat_dither=0.1, audiofeat_frame_length=25, audiofeat_frame_shift=10,
                                audiofeat_num_mel_bins=23, audiofeat_num_ceps=13, audiofeat_low_freq=20.0,
                                audiofeat_high_freq=0.0)
    sample = {"sample_rate": 16000, "waveform": torch.zeros(1, 1600)}
    for stage in (stages.audio_compute_fbank, stages.audio_compute_mfcc):
        with pytest.raises(ValueError, match="audiofeat_dither = 0.1.*random"):
            next(stage(iter([dict(sample)]), cfg))


def test_entry_point_refuses_on_the_host():
    """tn_kaldi_feats checks its arguments before it touches a pointer or launches: -22 with host addresses that are never
    dereferenced (the GPU tests repeat this with device buffers and check that the output stays untouched)"""
    from touchnet_amd import _C
    lib = _C.lib()
    raw = (C.c_char * 4096)()
    p = (C.addressof(raw) + 255) // 256 * 256
    ok = dict(wav=p, out=p + 1024, n=4000, sr=16000, win=400, shift=160, padded=512, bins=23, ceps=13, low=20.0, high=0.0,
              window=p, idx=p, w=p, n_w=480, dct=p)
    call = lambda **kw: lib.tn_kaldi_feats(*[dict(ok, **kw)[k] for k in ok], None)
    for what, kw in dict(
            padded_4096=dict(win=2100, padded=4096), padded_16=dict(win=16, padded=16), padded_not_of_win=dict(padded=1024),
            no_power_of_two=dict(padded=500), win_above_padded=dict(win=513), shift_0=dict(shift=0), bins_3=dict(bins=3),
            bins_257=dict(bins=257), ceps_above_bins=dict(ceps=24), ceps_negative=dict(ceps=-1),
            low_at_high=dict(low=4000.0, high=4000.0), low_negative=dict(low=-1.0), high_above_nyquist=dict(high=8000.5),
            offset_below_low=dict(high=-7990.0), mfcc_without_dct=dict(dct=None), weights_past_the_fft=dict(n_w=513),
            weights_negative=dict(n_w=-1), null_window=dict(window=None), null_banks=dict(idx=None), null_output=dict(out=None),
            null_input=dict(wav=None), output_is_input=dict(out=p), negative_length=dict(n=-1), rate_0=dict(sr=0),
            too_many_frames=dict(n=2 ** 31 + 400, shift=1)).items():
        assert call(**kw) == -22, what
    assert call(n=399) == 0 and call(n=399, out=None, wav=None) == 0      # no frame: nothing to launch, nothing to check


# ------------------------------------------------------------------------------------------------------ build_datapipe
def _pipe_cfg(tmp_path, **over):
    lst = tmp_path / "data.list"
    lst.write_text("/nonexistent audio+metainfo\n")
    d = dict(datapipe_type="touch_audio", datalist_path=str(lst), dataset_enable_pack=True, audio_feat_type="mfcc",
             audio_resample_rate=16000, audiofeat_num_mel_bins=23, audiofeat_num_ceps=13, audiofeat_low_freq=20.0,
             audiofeat_high_freq=0.0, audiofeat_frame_length=25, audiofeat_frame_shift=10, audiofeat_dither=0.0,
             audio_speed_perturb=False, audiofeat_spec_aug=False, audiofeat_spec_sub=False, audiofeat_spec_trim=False)
    d.update(over)
    return types.SimpleNamespace(**d)


def _stage_functions(pipe):
    out = []
    while hasattr(pipe, "f"):
        out.append(pipe.f)
        pipe = pipe.source
    return out[::-1]


class _Tok:
    bos, eos, pad = 1, 2, 0

    def tokenize(self, text, add_special_tokens=False):
        return [3]


def test_build_datapipe_takes_mfcc(tmp_path):
    from touchnet_amd.data import functions as stages
    from touchnet_amd.data.dataloader import build_datapipe
    chain = _stage_functions(build_datapipe(_pipe_cfg(tmp_path), _Tok(), 0, 1))
    assert stages.audio_compute_mfcc in chain and stages.audio_compute_fbank not in chain
    assert chain.index(stages.audio_resample) < chain.index(stages.audio_compute_mfcc) < chain.index(stages.audiofeat_stack)
    chain = _stage_functions(build_datapipe(_pipe_cfg(tmp_path, audio_feat_type="fbank", audio_resample_rate=8000), _Tok(), 0, 1))
    assert stages.audio_compute_fbank in chain and stages.audio_compute_mfcc not in chain


@pytest.mark.parametrize("over,field", [
    (dict(audiofeat_num_ceps=40), "audiofeat_num_ceps"),                   # the reference's own defaults: 40 cepstra, 23 bins
    (dict(audio_resample_rate=96000), "audiofeat_frame_length"), (dict(audiofeat_num_mel_bins=3, audiofeat_num_ceps=2),
                                                                   "audiofeat_num_mel_bins"),
    (dict(audiofeat_low_freq=9000.0), "audiofeat_low_freq"), (dict(audiofeat_dither=0.1), "audiofeat_dither"),
    (dict(audio_feat_type="fbank", audiofeat_frame_length=200), "audiofeat_frame_length")])
def test_build_datapipe_refuses_what_the_kernel_cannot_run(tmp_path, over, field):
    from touchnet_amd.data.dataloader import build_datapipe
    with pytest.raises(ValueError, match=field):
        build_datapipe(_pipe_cfg(tmp_path, **over), _Tok(), 0, 1)


# ------------------------------------------------------------------------------------------------------ ops
def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import touchnet_amd.library as L
    from touchnet_amd import _C
    assert "kaldi_feats" in L.OPS and "kaldi_mfcc" in L.OPS and "tn_kaldi_feats" in _C.PROTOTYPES
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "touchnet_amd.h")).read()
    assert "int tn_kaldi_feats(" in text and "touchnet/data/functions.py:117-156" in text
    for name in ("kaldi_feats", "kaldi_mfcc"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"mi355_touch::{name}", "Meta")
    with FakeTensorMode():
        f32 = lambda *s: torch.empty(*s, device="cuda")
        idx = torch.empty(40, 3, dtype=torch.int32, device="cuda")
        for n, frames in ((199, 0), (200, 1), (279, 1), (280, 2), (165000, 2061)):
            fb = torch.ops.mi355_touch.kaldi_feats(f32(n), f32(200), idx, f32(230), 8000, 80, 20.0, 0.0)
            mf = torch.ops.mi355_touch.kaldi_mfcc(f32(n), f32(200), idx, f32(230), f32(13, 40), 8000, 80, 20.0, 0.0)
            assert tuple(fb.shape) == (frames, 40) and tuple(mf.shape) == (frames, 13)
            assert fb.dtype == mf.dtype == torch.float32 and fb.device.type == "cuda"


def test_backend_exposes_the_new_functions():
    from touchnet_amd.models.backend import ops
    for name in ("kaldi_fbank", "kaldi_mfcc", "kaldi_feature_tables"):
        assert callable(getattr(ops(), name))
