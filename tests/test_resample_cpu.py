"""Sample-rate conversion (touchnet/data/functions.py:83-96, `torchaudio.transforms.Resample`) without the device: the
pin and the host side.

torchaudio is not installed, so its resampler is pinned in two steps: tests/resample_reference.py restates its published
formula in float64 (full kernel table, strided dot products over the padded waveform, cut), and scipy's polyphase engine
`resample_poly`, an independent implementation of rational-rate FIR filtering, is fed the same window and must give the
same samples.  The compact per-phase table the HIP kernel reads (functional.sinc_resample_table) is then held to that
table bit for bit, column by column, and the stage and the refusals of the entry point are exercised on the host."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import resample_reference as R

EINVAL = -22


def _noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_restatement_equals_scipy_polyphase_engine(orig, new):
    """resample_poly(x, n, o, window=g / n) upsamples by n, filters with n * window and keeps every o-th sample:
    y[m] = sum_k x[k] g[m o - k n], with g[u] the kernel's expression at t = u base / (o n) — the same sum as torchaudio's
    strided convolution, by another engine.  Bound 1e-12: float64 sums of at most 40 products of magnitude <= 1
    (observed: at most 7e-14)."""
    signal = pytest.importorskip("scipy.signal")
    o, n, base, width = R.geometry(orig, new)
    U = (width + o + 1) * n                                   # past every column of the kernel table
    u = np.arange(-U, U + 1, dtype=np.float64)
    t = np.clip(u * base / (o * n), -6.0, 6.0)
    g = np.sinc(t) * np.cos(t * math.pi / 12) ** 2 * base / o
    for N in (1, 2, 7, 2003):
        x = _noise(N, 100 + N)
        got = R.resample(x, orig, new, round_table=False)
        want = signal.resample_poly(x, n, o, window=g / n)
        assert got.shape == want.shape == (-((-N * n) // o),)
        err = float(np.abs(got - want).max())
        print(f"{orig}->{new} N={N}: restatement vs scipy {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_compact_table_is_the_kernel_table_without_its_zero_columns(orig, new):
    """float32(compact table) == the columns of float32(K) around each phase's centre, bit for bit; every other column of
    float32(K) is 0.0f.  And the compact sum equals the strided form in float64."""
    from touchnet_amd import functional as F
    o, n, width, K = R.kernel_table(orig, new)
    o2, n2, ntap, tab = F.sinc_resample_table(orig, new)
    assert (o2, n2) == (o, n) and tab.shape == (n, ntap) and tab.dtype == np.float64
    assert ntap == 2 * int(math.floor(6 * o / (min(o, n) * 0.99))) + 2
    K32, tab32 = K.astype(np.float32), tab.astype(np.float32)
    for j in range(n):
        r, k0 = (j * o) % n, width + (j * o) // n - ntap // 2 + 1
        assert k0 >= 0
        kept = K32[j, k0:k0 + ntap]
        assert np.array_equal(kept.view(np.int32), tab32[r, :kept.shape[0]].view(np.int32)), (j, r)
        assert not tab32[r, kept.shape[0]:].any()                 # (a column past K's last one is the padding's zero)
        assert not K32[j, :k0].any() and not K32[j, k0 + ntap:].any(), (j, "a dropped column is not 0.0f")
    x = _noise(1999, 7)
    want = R.resample(x, orig, new, round_table=True)
    got, _ = R.polyphase_dot(x, tab32, o, n, np.arange(want.shape[0]))
    assert float(np.abs(got - want).max()) <= 1e-12


def test_ntap_of_the_recipes_pairs():
    from touchnet_amd import functional as F
    assert [F.sinc_resample_table(a, b)[2] for a, b in R.PAIRS] == [14, 38, 34, 18, 14, 26, 26]


def test_restatement_is_a_resampler():
    """A tone in the pass band comes out as the same tone at the new rate, a tone above the new Nyquist frequency is
    removed (interior: 200 samples cut from each end).  The restatement alone gives 4.0e-4 and 1.9e-4."""
    N = 9600
    y = R.resample(np.sin(2 * np.pi * 1000.0 * np.arange(N) / 48000.0), 48000, 16000)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(y.shape[0]) / 16000.0)
    e_pass = float(np.abs(y - want)[200:-200].max())
    N = 8820
    z = R.resample(np.sin(2 * np.pi * 15000.0 * np.arange(N) / 44100.0), 44100, 16000)
    e_stop = float(np.abs(z)[200:-200].max())
    print(f"1 kHz 48k->16k: {e_pass:.2e}; 15 kHz 44.1k->16k: {e_stop:.2e}")
    assert y.shape[0] == 3200 and z.shape[0] == 3200
    assert e_pass < 1e-3 and e_stop < 1e-3


def test_entry_point_refuses_what_it_cannot_serve():
    """tn_resample_sinc returns -22 before any launch (only refused calls are made; the addresses are host memory,
    never dereferenced by a refused call)."""
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    raw = (C.c_char * 8192)()
    p = (C.addressof(raw) + 255) // 256 * 256
    x, y, tab = p, p + 2048, p + 4096
    ok = dict(x=x, pcm=0, y=y, tab=tab, n_in=1000, n_out=334, orig=48000, new=16000, ntap=38)

    def call(**kw):
        a = {**ok, **kw}
        return lib.tn_resample_sinc(a["x"], a["pcm"], a["y"], a["tab"], a["n_in"], a["n_out"], a["orig"], a["new"],
                                    a["ntap"], None)
    for pcm in (0, 1):
        assert call(pcm=pcm, x=None) == EINVAL and call(pcm=pcm, y=None) == EINVAL and call(pcm=pcm, tab=None) == EINVAL
        assert call(pcm=pcm, n_in=0) == EINVAL and call(pcm=pcm, n_in=-5) == EINVAL
        assert call(pcm=pcm, n_out=0) == EINVAL and call(pcm=pcm, n_out=-1) == EINVAL
        assert call(pcm=pcm, n_out=335) == EINVAL                       # ceil(1000 / 3) = 334
        assert call(pcm=pcm, n_in=2 ** 40, n_out=2 ** 40) == EINVAL
        assert call(pcm=pcm, orig=8000, new=16000, n_out=2001) == EINVAL
        assert call(pcm=pcm, orig=0) == EINVAL and call(pcm=pcm, orig=-48000) == EINVAL
        assert call(pcm=pcm, new=0) == EINVAL and call(pcm=pcm, new=-1) == EINVAL
        assert call(pcm=pcm, ntap=0) == EINVAL and call(pcm=pcm, ntap=1) == EINVAL and call(pcm=pcm, ntap=37) == EINVAL
        assert call(pcm=pcm, ntap=-2) == EINVAL and call(pcm=pcm, ntap=12288) == EINVAL    # one output's taps: 48 KiB of LDS
        assert call(pcm=pcm, y=x) == EINVAL


def test_resample_refuses_rates_and_tensors_it_cannot_serve():
    from touchnet_amd import functional as F
    w = torch.zeros(100)
    with pytest.raises(ValueError, match="1000 -> 192000"):
        F.resample(w, 1000, 192000)                                    # ratio 1 / 192
    with pytest.raises(ValueError, match="192000 -> 1000"):
        F.resample(w, 192000, 1000)
    with pytest.raises(ValueError, match="400001 -> 400000"):
        F.resample(w, 400001, 400000)                                  # 400000 phases x 14 taps > 2^22 table entries
    assert F.sinc_resample_table(16001, 16000)[2] * 16000 <= 2 ** 22   # (16001 -> 16000 passes the cap: 16000 x 14)
    with pytest.raises(ValueError):
        F.resample(w, 0, 16000)
    assert F.resample(w, 16000, 16000) is w and F.resample(w, 32000, 32000) is w
    with pytest.raises(RuntimeError):
        F.resample(w, 8000, 16000)                                     # a CPU tensor: no host fallback
    with pytest.raises(RuntimeError):
        F.resample(w, 16001, 16000)


def test_stage_resamples_other_rates_and_passes_the_target_rate_through():
    """audio_resample with an op namespace whose `resample` is the restatement: an 8 kHz sample leaves at 16 kHz with
    2 N samples, a 16 kHz sample is yielded as the same object with its waveform untouched on the host."""
    from touchnet_amd.data import functions as stages
    from touchnet_amd.models.backend import use_ops
    calls = []

    def resample(wave, orig, new):
        calls.append((orig, new))
        assert wave.dim() == 1
        x = wave.cpu().numpy() / (32768.0 if wave.dtype == torch.int16 else 1.0)
        return torch.from_numpy(R.resample(x, orig, new)).float().to(wave.device)
    cfg = types.SimpleNamespace(audio_resample_rate=16000)
    x8 = torch.from_numpy(_noise(801, 3)).float()[None]
    keep = torch.from_numpy(_noise(500, 4)).float()[None]
    pcm = (torch.from_numpy(_noise(333, 5)) * 30000).to(torch.int16)[None]
    s8, s16 = {"key": "a", "sample_rate": 8000, "waveform": x8}, {"key": "b", "sample_rate": 16000, "waveform": keep}
    s44, bare = {"key": "c", "sample_rate": 44100, "waveform": pcm}, {"key": "d", "waveform": keep}
    with use_ops(types.SimpleNamespace(resample=resample)):
        out = list(stages.audio_resample(iter([s8, s16, s44, bare]), cfg))
    assert calls == [(8000, 16000), (44100, 16000)]
    assert out[0] is s8 and out[0]["sample_rate"] == 16000 and out[0]["waveform"].shape == (1, 1602)
    assert out[0]["waveform"].dtype == torch.float32
    assert torch.equal(out[0]["waveform"][0].cpu(), torch.from_numpy(R.resample(x8[0].numpy(), 8000, 16000)).float())
    assert out[1] is s16 and out[1]["waveform"] is keep and not keep.is_cuda and out[1]["sample_rate"] == 16000
    assert out[2]["sample_rate"] == 16000 and out[2]["waveform"].shape == (1, -((-333 * 160) // 441))
    assert out[3] is bare and out[3]["waveform"] is keep and "sample_rate" not in bare
