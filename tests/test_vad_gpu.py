"""csrc/vad.hip (tn_vad_log_energy, tn_vad_runs) on the device against the float64 restatement of the rule
(tests/vad_reference.py), and long-form transcription (touchnet_amd/longform.py) end to end on tiny random models.

Gates:
  loge       |d| <= (win + 8) 2^-24 + 4 ulp32(|loge|): the fp32 sum of win non-negative terms, and the log's rounding.
             Frames of digital silence equal log(FLT_EPSILON) exactly; int16 and fp32 sources give the same bits.
  decisions  equal to the restatement's outside a guard band: a frame with |loge64 - thr64| <= 1.5 tol may fall either
             way, so the device's votes must lie between the restatement's with every such frame below and with every
             such frame above the threshold; at most 0.5 % of a case's frames may be in the band (asserted).  The runs
             must be exactly the runs of the device's own votes.
  hand-made  loge of +-20 around a threshold of 0: exact.
Each comparison prints its worst figure before it asserts."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import vad_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GEOMETRIES = [(16000, 400, 160), (8000, 200, 80), (48000, 1200, 480), (44100, 1102, 441), (16000, 400, 400),
              (16000, 400, 37)]
LOG_EPS = np.float32(np.log(np.float64(R.FLT_EPSILON)))
RUN_FRAMES = 1024                         # frames of one workgroup of tn_vad_runs


def _F():
    import touchnet_amd.functional as F
    return F


def _L():
    import touchnet_amd.library as L
    return L


def clip(sr, n, seed, dc=0, sigma=30.0):
    """int16: a noise floor (sigma) with sine bursts of amplitude 500 - 8000 lasting 20 ms - 2 s, plus a DC offset"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, sigma, n)
    for _ in range(6):
        dur = int(sr * rng.uniform(0.02, max(0.02, min(2.0, 0.4 * n / sr))))
        if dur < 1 or dur >= n:
            continue
        a = int(rng.integers(0, n - dur))
        t = np.arange(dur)
        x[a:a + dur] += rng.uniform(500, 8000) * np.sin(2 * np.pi * rng.uniform(100.0, sr / 4.0) * t / sr)
    return np.clip(np.rint(x + dc), -32768, 32767).astype(np.int16)


def tol(loge64, win):
    return (win + 8) * 2.0 ** -24 + 4.0 * np.spacing(np.abs(loge64).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(geo, dc, seed=0, seconds=6.0):
    sr, win, shift = geo
    x = clip(sr, int(sr * seconds), seed, dc)
    return x, R.log_energy(x, win, shift)


def device_loge(x, win, shift):
    loge, partials = _L().vad_log_energy(x if torch.is_tensor(x) else torch.from_numpy(x).to(DEV), win, shift)
    return loge, partials


def check_loge(x, win, shift, want, what):
    got, partials = device_loge(x, win, shift)
    got_f, _ = device_loge(torch.from_numpy(x.astype(np.float32) / 32768.0).to(DEV), win, shift)
    assert got.dtype == torch.float32 and got.shape == (want.size,), (what, got.shape)
    assert torch.equal(got, got_f), f"{what}: int16 and fp32 sources differ"
    assert partials.numel() == -(-want.size // _L().vad_frames_per_block(win, shift))
    if want.size == 0:
        return got
    g = got.cpu().numpy().astype(np.float64)
    ratio = float((np.abs(g - want) / tol(want, win)).max())
    psum = float(partials.sum().cpu())
    print(f"{what}: {want.size} frames, loge worst error {ratio:.3f} of the bound; partials sum {psum:.6f} vs {g.sum():.6f}")
    assert np.isfinite(g).all() and ratio <= 1.0, (what, ratio)
    assert abs(psum - g.sum()) <= 1e-9 * max(1.0, abs(g.sum()))
    return got


# ---------------------------------------------------------------------------------------------------------- loge
@pytest.mark.parametrize("dc", [0, 12000, -9000])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_loge_against_the_restatement(geo, dc):
    x, want = case(geo, dc)
    check_loge(x, geo[1], geo[2], want, f"{geo} dc {dc}")


def test_digital_silence_is_log_epsilon_exactly():
    sr, win, shift = 16000, 400, 160
    x = clip(sr, 3 * sr, 5)
    x[sr:2 * sr] = 0                               # digital silence
    x[2 * sr:2 * sr + 4000] = 12000                # a constant: its deviations are exactly zero too
    got = check_loge(x, win, shift, R.log_energy(x, win, shift), "silence").cpu().numpy()
    inside = lambda t, a, b: a <= t * shift and t * shift + win <= b
    silent = [t for t in range(got.size) if inside(t, sr, 2 * sr) or inside(t, 2 * sr, 2 * sr + 4000)]
    assert len(silent) > 100 and (got[silent] == LOG_EPS).all()
    assert (got[:50] != LOG_EPS).all()


@pytest.mark.parametrize("geo", [(16000, 400, 160), (48000, 1200, 480), (16000, 400, 400), (16000, 400, 1000), (8000, 4096, 1)],
                         ids=lambda g: "-".join(map(str, g)))
def test_frame_counts_around_one_window_and_one_workgroup(geo):
    sr, win, shift = geo
    fpb = _L().vad_frames_per_block(win, shift)
    assert 1 <= fpb <= 64
    x = clip(sr, win - 1, 1)
    loge, partials = device_loge(x, win, shift)
    assert loge.numel() == 0 and partials.numel() == 0
    if geo == (16000, 400, 160):
        runs, voiced, loge = _F().vad_energy(torch.from_numpy(x).to(DEV), sr)
        assert runs.shape == (0, 2) and voiced.numel() == 0 and loge.numel() == 0
    for T in (1, fpb - 1, fpb, fpb + 1, 2 * fpb + 1):
        if T < 1:
            continue
        n = win + (T - 1) * shift
        for extra in (0, shift - 1):
            x = clip(sr, n + extra, T)
            want = R.log_energy(x, win, shift)
            assert want.size == T
            check_loge(x, win, shift, want, f"{geo} T {T} (+{extra})")


def test_a_waveform_at_any_element_offset():
    """the staged span starts at the 16-byte boundary below the workgroup's first sample, wherever the waveform starts"""
    sr, win, shift = 16000, 400, 160
    x = clip(sr, 2 * sr, 9)
    dev16, dev32 = torch.from_numpy(x).to(DEV), torch.from_numpy(x.astype(np.float32) / 32768.0).to(DEV)
    for off in (1, 3, 7, 8, 13):
        want = R.log_energy(x[off:], win, shift)
        a, _ = device_loge(dev16[off:], win, shift)
        b, _ = device_loge(dev32[off:], win, shift)
        assert torch.equal(a, b)
        ratio = float((np.abs(a.cpu().numpy().astype(np.float64) - want) / tol(want, win)).max())
        print(f"offset {off}: worst {ratio:.3f} of the bound")
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ decisions and runs
def device_runs(loge, partials, et, ms, ctx, prop):
    voiced, buf = _L().vad_runs(loge, partials, et, ms, ctx, prop)
    host = buf.cpu().numpy()
    n = int(host[0])
    return voiced.cpu().numpy().astype(bool), host[1:1 + 2 * n].reshape(n, 2).astype(np.int64), (voiced, buf[:1 + 2 * n])


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_decisions_and_runs_against_the_restatement(geo):
    sr, win, shift = geo
    x, want = case(geo, 0)
    loge, partials = device_loge(x, win, shift)
    T = want.size
    for et, ms in ((5.0, 0.5), (0.0, 1.0), (1.5, 1.0)):
        thr = R.threshold(want, et, ms)
        band = np.abs(want - thr) <= 1.5 * tol(want, win)
        share = band.mean()
        print(f"{geo} thr {thr:.4f} ({et}, {ms}): {int(band.sum())} of {T} frames in the guard band ({100 * share:.3f} %); "
              f"{int((want > thr).sum())} above")
        assert share <= 0.005
        for ctx in (0, 2, 64):
            for prop in (0.12, 0.6, 1.0):
                lo, hi = R.vote((want > thr) & ~band, ctx, prop), R.vote((want > thr) | band, ctx, prop)
                voiced, runs, _ = device_runs(loge, partials, et, ms, ctx, prop)
                free = lo != hi
                assert (voiced[~free] == lo[~free]).all() and (voiced >= lo).all() and (voiced <= hi).all(), (ctx, prop)
                assert np.array_equal(runs, R.runs(voiced)), (ctx, prop)
                if not band.any():
                    assert np.array_equal(runs, R.vad(x, win, shift, et, ms, ctx, prop)[3])


def _pattern(name, T):
    v = np.zeros(T, dtype=bool)
    if name == "from_frame_0":
        v[:5] = True
        v[9:12] = True
    elif name == "to_the_last_frame":
        v[3:7] = True
        v[T - 4:] = True
    elif name == "single_frames":
        v[[2, 5, 11, T - 1]] = True
    elif name == "alternating_from_0":
        v[0::2] = True
    elif name == "alternating_from_1":
        v[1::2] = True
    elif name == "across_every_boundary":
        for b in range(RUN_FRAMES, T, RUN_FRAMES):
            v[b - 3:b + 4] = True
        v[RUN_FRAMES + 500:2 * RUN_FRAMES - 100] = True
    elif name == "ending_and_starting_at_a_boundary":
        v[RUN_FRAMES - 9:RUN_FRAMES] = True
        v[2 * RUN_FRAMES:2 * RUN_FRAMES + 6] = True
        v[3 * RUN_FRAMES - 1] = True
        v[3 * RUN_FRAMES] = False
        v[3 * RUN_FRAMES + 1] = True
    elif name == "all":
        v[:] = True
    elif name != "none":
        raise KeyError(name)
    return v


SMALL, EDGES = (16, 17), (RUN_FRAMES, RUN_FRAMES + 1, 3 * RUN_FRAMES + 5, 4 * RUN_FRAMES)
HAND_MADE = [(name, T) for name in ("from_frame_0", "to_the_last_frame", "single_frames", "alternating_from_0",
                                    "alternating_from_1", "all", "none") for T in SMALL + EDGES] + \
            [(name, T) for name in ("across_every_boundary", "ending_and_starting_at_a_boundary") for T in EDGES[2:]] + \
            [(name, T) for name in ("alternating_from_0", "alternating_from_1", "all", "none") for T in (1, 2, 3)]


@pytest.mark.parametrize("name,T", HAND_MADE)
def test_runs_of_hand_made_loge_are_exact(name, T):
    above = _pattern(name, T)
    loge = torch.from_numpy(np.where(above, 20.0, -20.0).astype(np.float32)).to(DEV)
    partials = loge.double().sum()[None]
    for ctx, prop in ((0, 0.6), (2, 0.6), (64, 0.12), (1, 1.0)):
        want = R.vote(above, ctx, prop)
        voiced, runs, raw = device_runs(loge, partials, 0.0, 0.0, ctx, prop)
        assert np.array_equal(voiced, want), (name, T, ctx, prop)
        assert np.array_equal(runs, R.runs(want)), (name, T, ctx, prop)
        again = device_runs(loge, partials, 0.0, 0.0, ctx, prop)[2]
        assert torch.equal(raw[0], again[0]) and torch.equal(raw[1], again[1])
    if name == "alternating_from_0":
        assert device_runs(loge, partials, 0.0, 0.0, 0, 0.6)[1].shape[0] == (T + 1) // 2      # T odd: the capacity itself


def test_one_frame_with_the_widest_context_and_split_partials():
    loge = torch.tensor([20.0], device=DEV)
    for prop in (0.12, 1.0):
        voiced, runs, _ = device_runs(loge, loge.double(), 0.0, 0.0, 64, prop)
        assert voiced.tolist() == [True] and runs.tolist() == [[0, 1]]
    voiced, runs, _ = device_runs(-loge, -loge.double(), 0.0, 0.0, 64, 0.12)
    assert voiced.tolist() == [False] and runs.shape == (0, 2)
    # the threshold is the same whatever the split of the sum: thr = 1 + 0.5 * mean; mean = 2 puts it at 2
    vals = torch.tensor([1.0, 3.0, 2.5, 1.5] * 300, device=DEV)
    for parts in (vals.double().sum()[None], vals.double().view(-1, 4).sum(1), vals.double()):
        voiced, runs, _ = device_runs(vals, parts.contiguous(), 1.0, 0.5, 0, 0.6)
        assert np.array_equal(voiced, (vals.cpu().numpy() > 2.0))


def test_vad_energy_is_the_restatement_end_to_end():
    F = _F()
    sr, win, shift = 16000, 400, 160
    x, want = case((sr, win, shift), 0)
    cfg = F.VadConfig(energy_threshold=0.0, energy_mean_scale=1.0, frames_context=2)
    assert F.vad_geometry(sr, cfg) == (win, shift)
    runs, voiced, loge = F.vad_energy(torch.from_numpy(x).to(DEV)[None], sr, cfg)
    ref = R.vad(x, win, shift, 0.0, 1.0, 2, 0.6)
    band = np.abs(want - ref[1]) <= 1.5 * tol(want, win)
    got = voiced.cpu().numpy().astype(bool)
    lo, hi = R.vote((want > ref[1]) & ~band, 2, 0.6), R.vote((want > ref[1]) | band, 2, 0.6)
    assert band.mean() <= 0.005 and (got >= lo).all() and (got <= hi).all() and loge.shape == (want.size,)
    assert runs.dtype == torch.int64 and not runs.is_cuda and np.array_equal(runs.numpy(), R.runs(got))
    if not band.any():
        assert np.array_equal(runs.numpy(), ref[3])


# ------------------------------------------------------------------------------------------------------ refusals
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_refused_arguments_return_22_before_any_launch():
    from touchnet_amd import _C
    lib = _C.lib()
    win, shift, n = 400, 160, 4000
    T = R.num_frames(n, win, shift)
    x = torch.from_numpy(clip(16000, n + 8, 2)).to(DEV)
    loge = torch.full((T,), 7.0, device=DEV)
    partials = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)

    def energy(**over):
        a = dict(x=x.data_ptr(), pcm=1, loge=loge.data_ptr(), partials=partials.data_ptr(), n=n, win=win, shift=shift)
        a.update(over)
        return lib.tn_vad_log_energy(a["x"], a["pcm"], a["loge"], a["partials"], a["n"], a["win"], a["shift"], _stream())

    refused = dict(win_0=dict(win=0), win_4097=dict(win=4097, n=10000), shift_0=dict(shift=0), negative_length=dict(n=-1),
                   frames_2_31=dict(n=2 ** 31 + 5, win=1, shift=1), null_wave=dict(x=None), null_loge=dict(loge=None),
                   null_partials=dict(partials=None), output_is_input=dict(loge=x.data_ptr()),
                   odd_int16_address=dict(x=x.data_ptr() + 1), int16_address_as_fp32=dict(x=x.data_ptr() + 2, pcm=0),
                   partials_off_8=dict(partials=partials.data_ptr() + 4), loge_off_4=dict(loge=loge.data_ptr() + 2))
    for what, over in refused.items():
        with pytest.raises(_C.KernelError, match="-22"):
            _C.check(energy(**over), f"tn_vad_log_energy[{what}]")
    torch.cuda.synchronize()
    assert (loge == 7.0).all() and (partials == 7.0).all()
    _C.check(energy(), "tn_vad_log_energy")                    # (and the untouched call runs; shift > win is legal)
    _C.check(energy(shift=win + 1), "tn_vad_log_energy")
    assert not (loge[:R.num_frames(n, win, win + 1)] == 7.0).any() and (partials[1:] == 7.0).all()

    _C.check(energy(), "tn_vad_log_energy")
    cap = T // 2 + 1
    voiced = torch.full((T,), 9, dtype=torch.uint8, device=DEV)
    buf = torch.full((1 + 2 * cap,), -5, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(lib.tn_vad_runs_workspace_bytes(T)) // 8 + 1, dtype=torch.float64, device=DEV)
    assert lib.tn_vad_runs_workspace_bytes(-1) == -1 and lib.tn_vad_runs_workspace_bytes(2 ** 31) == -1

    def runs(**over):
        a = dict(loge=loge.data_ptr(), T=T, partials=partials.data_ptr(), n_partials=1, et=5.0, ms=0.5, ctx=0, prop=0.6,
                 voiced=voiced.data_ptr(), runs=buf.data_ptr() + 4, count=buf.data_ptr(), cap=cap, ws=ws.data_ptr())
        a.update(over)
        return lib.tn_vad_runs(a["loge"], a["T"], a["partials"], a["n_partials"], a["et"], a["ms"], a["ctx"], a["prop"],
                               a["voiced"], a["runs"], a["count"], a["cap"], a["ws"], _stream())

    refused = dict(negative_frames=dict(T=-1), frames_2_31=dict(T=2 ** 31, cap=2 ** 30 + 1), ctx_negative=dict(ctx=-1),
                   ctx_65=dict(ctx=65), proportion_0=dict(prop=0.0), proportion_above_1=dict(prop=1.0001),
                   proportion_nan=dict(prop=float("nan")), threshold_nan=dict(et=float("nan")),
                   capacity_short_by_one=dict(cap=cap - 1), null_count=dict(count=None), null_loge=dict(loge=None),
                   null_partials=dict(partials=None), no_partials=dict(n_partials=0), null_voiced=dict(voiced=None),
                   null_runs=dict(runs=None), null_workspace=dict(ws=None), workspace_off_8=dict(ws=ws.data_ptr() + 4),
                   runs_off_4=dict(runs=buf.data_ptr() + 2))
    for what, over in refused.items():
        with pytest.raises(_C.KernelError, match="-22"):
            _C.check(runs(**over), f"tn_vad_runs[{what}]")
    torch.cuda.synchronize()
    assert (voiced == 9).all() and (buf == -5).all()
    _C.check(runs(), "tn_vad_runs")
    assert int(buf[0]) >= 0 and (voiced <= 1).all()
    F = _F()
    for kw, field in ((dict(frame_length=300.0), "frame_length"), (dict(frame_shift=0.01), "frame_shift"),
                      (dict(frames_context=65), "frames_context"), (dict(proportion_threshold=0.0), "proportion_threshold")):
        with pytest.raises(ValueError, match=field):
            F.vad_energy(x, 16000, F.VadConfig(**kw))


def test_opcheck():
    from torch.library import opcheck
    x = torch.from_numpy(clip(8000, 3000, 4)).to(DEV)
    tests = ("test_schema", "test_faketensor")
    for wave in (x, x[:150], x.float() / 32768.0):
        opcheck(torch.ops.mi355_touch.vad_log_energy.default, (wave, 200, 80), test_utils=tests)
    loge, partials = _L().vad_log_energy(x, 200, 80)
    opcheck(torch.ops.mi355_touch.vad_runs.default, (loge, partials, 5.0, 0.5, 2, 0.6), test_utils=("test_schema",))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        v, buf = torch.ops.mi355_touch.vad_runs(torch.empty(35, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda"),
                                                5.0, 0.5, 0, 0.6)
        assert v.shape == (35,) and v.dtype == torch.uint8 and buf.shape == (1 + 2 * 18,) and buf.dtype == torch.int32


# ------------------------------------------------------------------------------------------------------ end to end
def _recording(seconds=7.0, bursts=((0.5, 1.8), (2.8, 4.0), (5.2, 6.4)), seed=0, sr=16000):
    """int16 [1, N]: three tone bursts separated by near-silence (a noise floor of sigma 3)"""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    x = rng.normal(0.0, 3.0, n)
    for i, (a, b) in enumerate(bursts):
        t = np.arange(int(a * sr), int(b * sr))
        x[t] += 5000.0 * np.sin(2 * np.pi * (300.0 + 170.0 * i) * t / sr) * (1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * t / sr))
    return torch.from_numpy(np.clip(np.rint(x), -32768, 32767).astype(np.int16))[None]


def _tiny_touch_audio(seed, F_in=320):
    """the tiny TouchAudio Llama of tests/test_generation_gpu.py"""
    from touchnet_amd.models.llama import DecoderConfig
    from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
    text = dict(model_type="llama", hidden_size=256, intermediate_size=512, num_attention_heads=8, num_key_value_heads=2,
                head_dim=64, num_hidden_layers=2, vocab_size=512, rope_theta=500000.0, tie_word_embeddings=True,
                rms_norm_eps=1e-5, initializer_range=0.08, pad_token_id=1, bos_token_id=2, eos_token_id=3)
    cfg = TouchAudioConfig(text_config=DecoderConfig.from_dict(text), input_size=F_in, pad_token_id=1)
    torch.manual_seed(seed)
    m = TouchAudioForCausalLM(cfg)
    m.post_init()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_(0, 0.1)
    return m.to(DEV).to(torch.bfloat16).eval()


def _segments_as_planned(wav, sr, lcfg):
    from touchnet_amd import longform as LF
    spans = LF.segment_recording(wav, sr, lcfg, torch.device(DEV))
    assert len(spans) == 3, spans
    for (a, b), (s, e) in zip(spans, ((0.5, 1.8), (2.8, 4.0), (5.2, 6.4))):
        assert b - a <= lcfg.max_segment_s * sr and abs(a / sr - (s - 0.1)) <= 0.03 and abs(b / sr - (e + 0.1)) <= 0.04, spans
    return spans


def test_llama_asr_long_recording_is_its_segments_transcribed():
    from touchnet_amd import longform as LF
    from touchnet_amd.bin import infer_asr
    from touchnet_amd.generation import GenerationConfig
    from touchnet_amd.models.touch_audio.inference_touch_audio import transcribe
    model = _tiny_touch_audio(11)
    dcfg = types.SimpleNamespace(**dict(infer_asr._DATA_DEFAULTS, audiofeat_stack_length=4, audiofeat_stride_length=4))
    feats = lambda ws: infer_asr.features(ws, dcfg)
    gen = GenerationConfig(max_new_tokens=12, output_scores=True)
    lcfg = LF.LongFormConfig(max_segment_s=2.0)
    sr, wav, short = 16000, _recording(), _recording(1.5, ((0.3, 1.2),), seed=3)
    spans = _segments_as_planned(wav, sr, lcfg)
    decode = LF.touch_audio_decoder(model, gen, feats)
    to_text = lambda ids: " ".join(map(str, ids))
    out = LF.transcribe_long(decode, [short, wav], sr, lcfg, batch_size=2, to_text=to_text, output_scores=True,
                             device=torch.device(DEV))
    # the driver's own order and batches: the pool is [short, seg 0, seg 1, seg 2], heaviest first, two at a time
    pool = [short] + [wav[:, a:b] for a, b in spans]
    order = LF.pool_order([p.numel() for p in pool])
    want = {}
    for o in range(0, 4, 2):
        chunk = order[o:o + 2]
        ids, extras = transcribe(model, feats([pool[i] for i in chunk]), gen, details=True)
        want.update({i: (ids[n], extras[n]) for n, i in enumerate(chunk)})
    rec = out[1]
    assert rec["segments"] == spans and [s["predict_ids"] for s in rec["extra"]["segments"]] == [want[i][0] for i in (1, 2, 3)]
    assert rec["predict_ids"] == want[1][0] + want[2][0] + want[3][0] and rec["predict"] == to_text(rec["predict_ids"])
    assert sum(len(want[i][0]) for i in (1, 2, 3)) > 0
    logps = []
    for seg, (a, b), i in zip(rec["extra"]["segments"], spans, (1, 2, 3)):
        assert seg["start"] == a / sr and seg["end"] == b / sr and seg["predict"] == to_text(seg["predict_ids"])
        assert seg["token_logprobs"] == want[i][1]["token_logprobs"] and seg["confidence"] == want[i][1]["confidence"]
        logps += seg["token_logprobs"]
    assert abs(rec["extra"]["confidence"] - float(np.exp(np.mean(logps)))) <= 1e-12
    assert list(rec["extra"]) == ["confidence", "segments"]
    assert out[0]["segments"] is None and out[0]["predict_ids"] == want[0][0] and out[0]["extra"] == want[0][1]
    # a recording within max_segment_s alone: exactly what transcribe returns
    ids, extras = transcribe(model, feats([short]), gen, details=True)
    alone = LF.transcribe_long(decode, [short], sr, lcfg, batch_size=2, to_text=to_text, output_scores=True)
    assert alone[0]["predict_ids"] == ids[0] and alone[0]["extra"] == extras[0] and alone[0]["segments"] is None
    # no voiced frame: no segment, an empty transcript
    quiet = torch.zeros(1, 3 * sr, dtype=torch.int16)
    quiet[0, ::2] = 1
    empty = LF.transcribe_long(decode, [quiet], sr, LF.LongFormConfig(max_segment_s=2.0, vad=_F().VadConfig(
        energy_threshold=8.0, energy_mean_scale=0.5)), batch_size=2, to_text=to_text, device=torch.device(DEV))
    assert empty[0]["predict_ids"] == [] and empty[0]["predict"] == "" and empty[0]["extra"] == {"segments": []}
    with pytest.raises(ValueError, match="nbest"):
        LF.transcribe_long(decode, [wav], sr, lcfg, batch_size=2, nbest=2)


@pytest.fixture(scope="module")
def qwen2_audio(tmp_path_factory):
    from test_sampling_gpu import _tiny_qwen2_audio, _tiny_tokenizer
    from touchnet_amd import longform as LF
    from touchnet_amd.generation import GenerationConfig
    tok, _ = _tiny_tokenizer(tmp_path_factory.mktemp("qwen2_audio"))
    _, m, _, eos = _tiny_qwen2_audio(tok, seed=3)
    cfg = GenerationConfig.from_hf({"do_sample": True, "top_k": 20, "temperature": 1.0, "repetition_penalty": 1.1,
                                    "eos_token_id": eos, "max_new_tokens": 10, "seed": 7})
    lcfg = LF.LongFormConfig(max_segment_s=2.0)
    wav, short = _recording(), _recording(1.5, ((0.3, 1.2),), seed=3)
    to_text = lambda r: tok.decode(r, skip_special_tokens=True, clean_up_tokenization_spaces=False)
    run = lambda bs: LF.transcribe_long(LF.qwen2_audio_decoder(m, tok, "w1 w2", cfg), [wav, short], 16000, lcfg, batch_size=bs,
                                        row_keys=[41, 5], to_text=to_text, sampled=True, device=torch.device(DEV))
    return types.SimpleNamespace(tok=tok, model=m, cfg=cfg, lcfg=lcfg, wav=wav, short=short, to_text=to_text, run=run)


def test_qwen2_audio_sampled_segments_draw_with_their_own_keys(qwen2_audio):
    """Sampling on: the driver's result is `transcribe` on every pooled slice in a call of its own (what `sampled` makes
    of any batch_size), with the key rule: segment i of the recording with key k draws with k + (i + 1) 2^40, the
    unsegmented recording keeps k."""
    from touchnet_amd.models.qwen2_audio import inference_qwen2_audio as Q
    q = qwen2_audio
    spans = _segments_as_planned(q.wav, 16000, q.lcfg)
    out = q.run(4)
    pool = [q.wav[:, a:b] for a, b in spans] + [q.short]
    pool_keys = [41 + (i + 1) * 2 ** 40 for i in range(3)] + [5]
    alone = lambda shift: [Q.transcribe(q.model, [w], q.tok, "w1 w2", q.cfg, row_keys=torch.tensor([k + shift]))
                           for w, k in zip(pool, pool_keys)]
    got = [(ids[0], texts[0]) for ids, texts in alone(0)]
    rec = out[0]
    assert [s["predict_ids"] for s in rec["extra"]["segments"]] == [got[0][0], got[1][0], got[2][0]]
    assert rec["predict_ids"] == got[0][0] + got[1][0] + got[2][0] and rec["predict"] == q.to_text(rec["predict_ids"])
    assert out[1]["predict_ids"] == got[3][0] and out[1]["predict"] == got[3][1] and out[1]["segments"] is None
    assert sum(len(g[0]) for g in got) > 0
    # other keys, other draws: the keys do reach the sampler
    assert [ids[0] for ids, _ in alone(1)] != [g[0] for g in got]


def test_qwen2_audio_sampled_segments_do_not_depend_on_the_batching(qwen2_audio):
    """Sampling on: the same recordings decoded with batch_size 1 and 4 give the same ids and text.

    The keys alone do not achieve that.  The decoders' forward depends on the place an utterance has in a batch; measured
    on this test's pool with the tiny model, alone against inside the batch of four: the first utterance is bit-equal,
    log-probabilities of all ten steps included; prefill embeddings of the third and fourth differ by 7.8e-3 and 1.6e-2
    (one bf16 step of the audio tower's rows); greedy token log-probabilities differ by 2.9e-2 for the second and third and
    by 1.4 for the fourth.  With top_k 20 on a random model's flat distribution that moved a draw when the driver still
    batched sampled segments: segment 1's third token came out 73 at batch_size 1 and 72 at 4.  So a sampled run decodes
    every segment in a call of its own (`sampled`), and this test holds the driver to it."""
    q = qwen2_audio
    strip = lambda out: [(r["predict_ids"], r["predict"], [s["predict_ids"] for s in (r["extra"].get("segments") or [])])
                         for r in out]
    one, four = strip(q.run(1)), strip(q.run(4))
    for a, b in zip(one, four):
        print("batch_size 1:", a[0], "\nbatch_size 4:", b[0])
    assert one == four
