"""Long-form transcription without the device: the segment planner of touchnet_amd/longform.py on hand-worked run lists and
on seeded random ones, the refusals of the two VAD entry points with host addresses (they refuse before they touch a
pointer), the registrations, the command lines' new flags, and the driver's refusal of nbest > 1.

Frames below are the default VAD frames, 25 ms every 10 ms: min_silence 300 ms = 30 frames, min_speech 100 ms = 10,
pad 100 ms = 10, and max_segment_s = 30 is 2998 frames ((2998 - 1) 10 + 25 = 29995 ms <= 30000 < 30005)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _LF():
    from touchnet_amd import longform
    return longform


def _cfg(**kw):
    return _LF().LongFormConfig(**kw)


def _bare(**kw):
    """only the rule under test: the others switched off"""
    return _cfg(**dict(dict(min_silence_ms=0.0, min_speech_ms=0.0, pad_ms=0.0), **kw))


# ------------------------------------------------------------------------------------------------ the planner's rules
def test_frames_of_the_defaults():
    assert _cfg().frames() == (30, 10, 10, 2998)
    assert _cfg(max_segment_s=2.0).frames()[3] == 198                      # 197 * 10 + 25 = 1995 ms
    assert _cfg(max_segment_s=0.025).frames()[3] == 1
    with pytest.raises(ValueError, match="max_segment_s"):
        _cfg(max_segment_s=0.01)
    with pytest.raises(ValueError, match="pad_ms"):
        _cfg(pad_ms=-1.0)


def test_rule_1_gaps_shorter_than_min_silence_are_closed():
    """max_segment is 38 frames here, so that rule 5 cannot close what rule 1 left open; a closed gap makes a run of 50
    frames, which rule 4 then cuts at the planted minimum"""
    loge = np.full(10000, 9.0)
    loge[125] = 1.0
    plan = lambda runs: _LF().plan_segments(runs, 10000, loge, _bare(min_silence_ms=300.0, max_segment_s=0.4))
    assert plan([(100, 110), (139, 150)]) == [(100, 125), (125, 150)]       # a gap of 29 frames: closed
    assert plan([(100, 110), (140, 150)]) == [(100, 110), (140, 150)]       # exactly min_silence: it stays open


def test_rule_2_runs_shorter_than_min_speech_are_dropped():
    plan = lambda runs: _LF().plan_segments(runs, 10000, None, _bare(min_speech_ms=100.0, max_segment_s=1.0))
    assert plan([(100, 109), (300, 310), (500, 511)]) == [(300, 310), (500, 511)]      # 9 dropped, exactly 10 kept
    # rule 1 runs first: two short runs across a short gap make one that is long enough
    both = _LF().plan_segments([(100, 105), (110, 116)], 10000, None,
                               _bare(min_silence_ms=300.0, min_speech_ms=100.0, max_segment_s=1.0))
    assert both == [(100, 116)]


def test_rule_3_padding_is_clamped_and_merges_what_touches():
    plan = lambda runs, T: _LF().plan_segments(runs, T, None, _bare(pad_ms=100.0, max_segment_s=1.0))
    assert plan([(3, 20)], 1000) == [(0, 30)]                               # clamped at 0
    assert plan([(980, 995)], 1000) == [(970, 1000)]                        # clamped at T
    # runs that touch after padding become one run (50 frames > max_segment = 48: rule 4 cuts it at the planted minimum);
    # one frame apart they stay two (and rule 5 cannot merge them: 50 frames)
    loge = np.full(1000, 9.0)
    loge[120] = 1.0
    tight = lambda runs: _LF().plan_segments(runs, 1000, loge, _bare(pad_ms=100.0, max_segment_s=0.5))
    assert tight([(100, 105), (125, 130)]) == [(90, 120), (120, 140)]
    assert tight([(100, 105), (126, 130)]) == [(90, 115), (116, 140)]


def test_rule_4_cuts_at_the_lowest_energy_of_the_second_half():
    LF = _LF()
    cfg = _bare(max_segment_s=1.0)                                          # 98 frames
    most = cfg.frames()[3]
    assert most == 98
    loge = np.full(1000, 9.0)
    assert LF.plan_segments([(100, 100 + most)], 1000, None, cfg) == [(100, 100 + most)]     # exactly max: no cut, no loge
    with pytest.raises(ValueError, match="loge"):
        LF.plan_segments([(100, 101 + most)], 1000, None, cfg)
    # one frame more: the window is [100 + 49, 100 + 98); all equal, so the lowest index
    assert LF.plan_segments([(100, 101 + most)], 1000, loge, cfg) == [(100, 149), (149, 199)]
    loge[170], loge[180] = 2.0, 2.0                                         # a tie: the lower index
    assert LF.plan_segments([(100, 101 + most)], 1000, loge, cfg) == [(100, 170), (170, 199)]
    loge[197] = 1.0                                                         # the last frame of the window
    assert LF.plan_segments([(100, 101 + most)], 1000, loge, cfg) == [(100, 197), (197, 199)]
    loge[198], loge[148] = 0.0, 0.0                                         # just outside the window on both sides
    assert LF.plan_segments([(100, 101 + most)], 1000, loge, cfg) == [(100, 197), (197, 199)]
    # the remainder is cut again, and loge may be a function that is only called when a cut is needed
    calls = []
    lazy = lambda: calls.append(1) or np.full(1000, 9.0)
    assert LF.plan_segments([(0, 98), (200, 298)], 1000, lazy, cfg) == [(0, 98), (200, 298)] and not calls
    # flat energy: cuts at 49, 98, 147, 196, 245 (each the first frame of its window); rule 5 then rejoins the pairs that fit
    assert LF.plan_segments([(0, 300)], 1000, lazy, cfg) == [(0, 98), (98, 196), (196, 245), (245, 300)] and len(calls) == 1


def test_rule_5_merges_greedily_while_the_span_fits():
    LF = _LF()
    cfg = _bare(max_segment_s=1.0)                                          # 98 frames
    assert LF.plan_segments([(0, 10), (50, 98), (99, 120)], 1000, None, cfg) == [(0, 98), (99, 120)]
    assert LF.plan_segments([(0, 10), (50, 99)], 1000, None, cfg) == [(0, 10), (50, 99)]        # 99 frames would not fit
    assert LF.plan_segments([(0, 10), (20, 30), (40, 50), (100, 110), (150, 190)], 1000, None, cfg) == \
        [(0, 50), (100, 190)]


def test_the_empty_list_and_sample_ranges():
    LF = _LF()
    assert LF.plan_segments([], 1000, None, _cfg()) == []
    assert LF.plan_segments(torch.empty(0, 2, dtype=torch.int64), 0, None, _cfg()) == []
    assert LF.segment_samples([(0, 1), (10, 30)], 400, 160) == [(0, 400), (1600, 29 * 160 + 400)]
    with pytest.raises(ValueError, match="ordered"):
        LF.plan_segments([(10, 20), (15, 30)], 1000, None, _cfg())
    with pytest.raises(ValueError, match="ordered"):
        LF.plan_segments([(10, 1001)], 1000, None, _cfg())


def test_all_rules_in_order_on_a_worked_example():
    # runs: A (5, 9) too short alone but 12 frames from B; B (21, 60); C (95, 130) 35 frames behind B; D (400, 404) dropped
    got = _LF().plan_segments([(5, 9), (21, 60), (95, 130), (400, 404)], 1000, None, _cfg(max_segment_s=1.0))
    # 1: (5, 60), (95, 130), (400, 404).  2: D goes.  3: (0, 70), (85, 140).  5: 140 - 0 > 98: two segments
    assert got == [(0, 70), (85, 140)]


@pytest.mark.parametrize("seed", range(8))
def test_properties_over_random_run_lists(seed):
    LF = _LF()
    rng = np.random.default_rng(seed)
    T = int(rng.integers(500, 6000))
    cfg = _cfg(max_segment_s=float(rng.choice([0.5, 1.0, 3.0, 30.0])), min_silence_ms=float(rng.choice([0, 50, 300])),
               min_speech_ms=float(rng.choice([0, 30, 100])), pad_ms=float(rng.choice([0, 40, 100])))
    min_sil, min_speech, pad, most = cfg.frames()
    voiced = np.zeros(T, dtype=bool)
    t = int(rng.integers(0, 40))
    while t < T:
        n = int(rng.choice([1, 3, 12, 80, 700])) + int(rng.integers(0, 9))
        voiced[t:t + n] = True
        t += n + int(rng.choice([1, 5, 31, 200])) + int(rng.integers(0, 5))
    d = np.diff(np.concatenate([[0], voiced.astype(np.int8), [0]]))
    runs = list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))
    loge = rng.normal(10.0, 3.0, T)
    segs = LF.plan_segments(runs, T, loge, cfg)
    assert all(0 <= s < e <= T for s, e in segs)
    assert all(a[1] <= b[0] for a, b in zip(segs, segs[1:]))                # ordered and disjoint
    assert all(e - s <= most for s, e in segs)                              # none longer than max_segment_s
    win, shift = 400, 160
    assert all(b - a <= cfg.max_segment_s * 16000 for a, b in LF.segment_samples(segs, win, shift))
    # the kept runs: rules 1 and 2 restated; every frame of them is covered
    kept = []
    for s, e in runs:
        if kept and s - kept[-1][1] < min_sil:
            kept[-1][1] = e
        else:
            kept.append([s, e])
    covered = np.zeros(T, dtype=bool)
    for s, e in segs:
        covered[s:e] = True
    for s, e in kept:
        if e - s >= min_speech:
            assert covered[s:e].all()
    assert LF.plan_segments(np.asarray(runs, dtype=np.int64).reshape(-1, 2), T, lambda: loge, cfg) == segs


def test_pool_order_and_segment_keys():
    LF = _LF()
    assert LF.pool_order([5, 9, 9, 1, 7]) == [1, 2, 4, 0, 3]
    assert LF.segment_key(7, 0) == 7 + 2 ** 40 and LF.segment_key(7, 2) == 7 + 3 * 2 ** 40


# ----------------------------------------------------------------------------------------------------- the driver
def _fake_decode(log):
    def decode(wavs, keys):
        log.append(([int(w.numel()) for w in wavs], keys.tolist()))
        ids = [[int(w.numel()) % 97, int(k) % 89] for w, k in zip(wavs, keys.tolist())]
        return ids, None, [{"token_logprobs": [-0.5, None, -1.5], "confidence": 0.4} for _ in wavs]
    return decode


def test_driver_pools_keys_and_scatters(monkeypatch):
    LF = _LF()
    sr = 16000
    spans = {100000: [(0, 30000), (40000, 60000), (70000, 99000)], 50000: []}
    monkeypatch.setattr(LF, "segment_recording", lambda w, rate, cfg, device=None: spans[w.numel()])
    wavs = [torch.zeros(1, 20000, dtype=torch.int16), torch.zeros(1, 100000, dtype=torch.int16),
            torch.zeros(50000, dtype=torch.int16), torch.zeros(1, 32000, dtype=torch.int16)]
    log = []
    out = LF.transcribe_long(_fake_decode(log), wavs, sr, _cfg(max_segment_s=2.0), batch_size=2, row_keys=[10, 11, 12, 13],
                             to_text=lambda ids: "-".join(map(str, ids)), output_scores=True)
    K = 2 ** 40
    # the pool: rec 0 whole (20000), rec 1's three segments (30000, 20000, 29000), rec 3 whole (32000: exactly 2 s)
    assert log == [([32000, 30000], [13, 11 + K]), ([29000, 20000], [11 + 3 * K, 10]), ([20000], [11 + 2 * K])]
    assert [r["segments"] for r in out] == [None, spans[100000], [], None]
    assert out[0]["predict_ids"] == [20000 % 97, 10] and out[0]["extra"] == {"token_logprobs": [-0.5, None, -1.5],
                                                                             "confidence": 0.4}
    segs = out[1]["extra"]["segments"]
    assert [s["start"] for s in segs] == [0.0, 2.5, 4.375] and [s["end"] for s in segs] == [1.875, 3.75, 6.1875]
    assert [s["predict_ids"] for s in segs] == [[30000 % 97, (11 + K) % 89], [20000 % 97, (11 + 2 * K) % 89],
                                                [29000 % 97, (11 + 3 * K) % 89]]
    assert out[1]["predict_ids"] == sum((s["predict_ids"] for s in segs), [])
    assert out[1]["predict"] == "-".join(map(str, out[1]["predict_ids"])) and segs[0]["predict"] == "-".join(
        map(str, segs[0]["predict_ids"]))
    assert abs(out[1]["extra"]["confidence"] - float(np.exp(-1.0))) < 1e-15 and segs[2]["confidence"] == 0.4
    assert list(out[1]["extra"]) == ["confidence", "segments"]
    assert out[2]["predict_ids"] == [] and out[2]["predict"] == "" and out[2]["extra"] == {"confidence": None, "segments": []}


def test_a_sampled_run_decodes_one_segment_per_call(monkeypatch):
    LF = _LF()
    monkeypatch.setattr(LF, "segment_recording", lambda w, rate, cfg, device=None: [(0, 30000), (40000, 60000)])
    wavs = [torch.zeros(1, 20000, dtype=torch.int16), torch.zeros(1, 100000, dtype=torch.int16)]
    logs = []
    for bs in (1, 3):
        log = []
        LF.transcribe_long(_fake_decode(log), wavs, 16000, _cfg(max_segment_s=2.0), batch_size=bs, row_keys=[10, 11],
                           sampled=True)
        logs.append(log)
    K = 2 ** 40
    assert logs[0] == logs[1] == [([30000], [11 + K]), ([20000], [10]), ([20000], [11 + 2 * K])]


def test_nbest_with_a_segmented_recording_is_refused_by_name():
    LF = _LF()
    long_wav, short_wav = torch.zeros(1, 16000 * 3, dtype=torch.int16), torch.zeros(1, 16000, dtype=torch.int16)
    with pytest.raises(ValueError, match="nbest = 2"):
        LF.transcribe_long(_fake_decode([]), [short_wav, long_wav], 16000, _cfg(max_segment_s=2.0), batch_size=4, nbest=2)
    out = LF.transcribe_long(_fake_decode([]), [short_wav], 16000, _cfg(max_segment_s=2.0), batch_size=4, nbest=2)
    assert out[0]["segments"] is None                    # nothing is cut: N-best lists stay available


# ----------------------------------------------------------------------------------------- entry points and registrations
def test_entry_points_refuse_on_the_host():
    """-22 with host addresses that are never dereferenced (tests/test_vad_gpu.py repeats this with device buffers and
    checks that the outputs stay untouched)"""
    from touchnet_amd import _C
    lib = _C.lib()
    x = np.zeros(8192, dtype=np.int16)
    loge, partials = np.zeros(64, dtype=np.float32), np.zeros(8, dtype=np.float64)
    voiced, buf, ws = np.zeros(64, dtype=np.uint8), np.zeros(80, dtype=np.int32), np.zeros(8, dtype=np.float64)
    p = lambda a: a.ctypes.data

    def energy(**over):
        a = dict(x=p(x), pcm=1, loge=p(loge), partials=p(partials), n=4000, win=400, shift=160)
        a.update(over)
        return lib.tn_vad_log_energy(a["x"], a["pcm"], a["loge"], a["partials"], a["n"], a["win"], a["shift"], None)

    for what, over in dict(win_0=dict(win=0), win_4097=dict(win=4097, n=8000), shift_0=dict(shift=0), n_negative=dict(n=-1),
                           frames_2_31=dict(n=2 ** 31 + 5, win=1, shift=1), null_wave=dict(x=None),
                           null_loge=dict(loge=None), null_partials=dict(partials=None), loge_is_wave=dict(loge=p(x)),
                           odd_address=dict(x=p(x) + 1), fp32_at_2=dict(x=p(x) + 2, pcm=0),
                           partials_at_4=dict(partials=p(partials) + 4)).items():
        assert energy(**over) == -22, what
    assert energy(n=399) == 0 and energy(n=399, x=None, loge=None, partials=None) == 0       # no frame: nothing to launch
    assert lib.tn_vad_frames_per_block(400, 160) == 64 and lib.tn_vad_frames_per_block(4096, 4096) == 3
    assert lib.tn_vad_frames_per_block(0, 1) == -1 and lib.tn_vad_frames_per_block(4097, 1) == -1
    assert lib.tn_vad_frames_per_block(400, 0) == -1 and 1 <= lib.tn_vad_frames_per_block(1, 10 ** 9) <= 64
    T = 23

    def runs(**over):
        a = dict(loge=p(loge), T=T, partials=p(partials), n_partials=1, et=5.0, ms=0.5, ctx=0, prop=0.6, voiced=p(voiced),
                 runs=p(buf) + 4, count=p(buf), cap=T // 2 + 1, ws=p(ws))
        a.update(over)
        return lib.tn_vad_runs(a["loge"], a["T"], a["partials"], a["n_partials"], a["et"], a["ms"], a["ctx"], a["prop"],
                               a["voiced"], a["runs"], a["count"], a["cap"], a["ws"], None)

    for what, over in dict(T_negative=dict(T=-1), T_2_31=dict(T=2 ** 31, cap=2 ** 30 + 1), ctx_negative=dict(ctx=-1),
                           ctx_65=dict(ctx=65), proportion_0=dict(prop=0.0), proportion_above_1=dict(prop=1.5),
                           proportion_nan=dict(prop=float("nan")), scale_nan=dict(ms=float("nan")),
                           capacity_short=dict(cap=T // 2), null_count=dict(count=None), null_loge=dict(loge=None),
                           null_partials=dict(partials=None), n_partials_0=dict(n_partials=0), null_voiced=dict(voiced=None),
                           null_runs=dict(runs=None), null_workspace=dict(ws=None), workspace_at_4=dict(ws=p(ws) + 4)).items():
        assert runs(**over) == -22, what
    assert lib.tn_vad_runs_workspace_bytes(0) == 16 and lib.tn_vad_runs_workspace_bytes(1025) == 8 + 16
    assert lib.tn_vad_runs_workspace_bytes(-1) == -1 and lib.tn_vad_runs_workspace_bytes(2 ** 31) == -1


def test_ops_prototypes_and_header_entries():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import touchnet_amd.library as L
    from touchnet_amd import _C
    for name in ("vad_log_energy", "vad_runs"):
        assert name in L.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"mi355_touch::{name}", "Meta"), name
    text = open(os.path.join(ROOT, "include", "touchnet_amd.h")).read()
    for name, nargs in (("tn_vad_log_energy", 8), ("tn_vad_runs", 14), ("tn_vad_frames_per_block", 2),
                        ("tn_vad_runs_workspace_bytes", 1)):
        assert name in _C.PROTOTYPES and len(_C.PROTOTYPES[name]) == nargs and f"{name}(" in text
    assert "inference_qwen2_audio.py:101" in text and "processing_kimi_audio.py:73" in text
    with FakeTensorMode():
        for dt in (torch.int16, torch.float32):
            loge, partials = torch.ops.mi355_touch.vad_log_energy(torch.empty(16000, dtype=dt, device="cuda"), 400, 160)
            assert loge.shape == (98,) and loge.dtype == torch.float32 and partials.shape == (2,)
            assert partials.dtype == torch.float64
        loge, partials = torch.ops.mi355_touch.vad_log_energy(torch.empty(399, dtype=torch.int16, device="cuda"), 400, 160)
        assert loge.shape == (0,) and partials.shape == (0,)
        voiced, buf = torch.ops.mi355_touch.vad_runs(torch.empty(98, device="cuda"),
                                                     torch.empty(2, dtype=torch.float64, device="cuda"), 5.0, 0.5, 0, 0.6)
        assert voiced.shape == (98,) and voiced.dtype == torch.uint8 and buf.shape == (1 + 2 * 50,) and buf.dtype == torch.int32


def test_vad_config_and_geometry():
    import touchnet_amd.functional as F
    from touchnet_amd.models.backend import ops
    c = F.VadConfig()
    assert (c.frame_length, c.frame_shift, c.energy_threshold, c.energy_mean_scale, c.frames_context,
            c.proportion_threshold) == (25.0, 10.0, 5.0, 0.5, 0, 0.6)
    assert "tuned" in F.VadConfig.__doc__
    assert F.vad_geometry(16000, c) == (400, 160) and F.vad_geometry(44100, c) == (1102, 441)
    assert F.vad_geometry(8000, c) == (200, 80) and F.vad_geometry(48000, c) == (1200, 480)
    for kw, field in ((dict(frame_length=100.0), "frame_length"), (dict(frame_length=0.0), "frame_length"),
                      (dict(frame_shift=0.001), "frame_shift"), (dict(frames_context=65), "frames_context"),
                      (dict(frames_context=1.5), "frames_context"), (dict(proportion_threshold=0.0), "proportion_threshold"),
                      (dict(proportion_threshold=1.01), "proportion_threshold"), (dict(energy_threshold=float("inf")),
                                                                                  "energy_threshold")):
        with pytest.raises(ValueError, match=field):
            F.vad_geometry(48000, F.VadConfig(**kw))
    with pytest.raises(ValueError, match="sample_rate"):
        F.vad_geometry(0, c)
    with pytest.raises(RuntimeError, match="device waveform"):
        F.vad_energy(torch.zeros(16000), 16000)
    assert callable(ops().vad_energy) and callable(ops().vad_geometry)


# ------------------------------------------------------------------------------------------------- the command lines
_LONG = ["--long_form", "--max_segment_s", "20", "--vad_energy_threshold", "4.5", "--vad_energy_mean_scale", "0.6",
         "--vad_frames_context", "2", "--vad_proportion_threshold", "0.5", "--vad_min_silence_ms", "250",
         "--vad_min_speech_ms", "80", "--vad_pad_ms", "60"]


@pytest.mark.parametrize("name", ["infer_asr", "infer_qwen2_audio", "infer_kimi_audio"])
def test_parsers_take_the_flags_and_leave_the_generation_config_alone(name, tmp_path):
    import importlib
    LF = _LF()
    mod = importlib.import_module(f"touchnet_amd.bin.{name}")
    base = ["--model_path", str(tmp_path), "--data_list", "l", "--output_dir", "o"]
    plain, long_ = mod.build_parser().parse_args(base), mod.build_parser().parse_args(base + _LONG)
    assert LF.longform_from_args(plain) is None and plain.long_form is False
    cfg = LF.longform_from_args(long_)
    assert (cfg.max_segment_s, cfg.min_silence_ms, cfg.min_speech_ms, cfg.pad_ms) == (20.0, 250.0, 80.0, 60.0)
    assert (cfg.vad.energy_threshold, cfg.vad.energy_mean_scale, cfg.vad.frames_context, cfg.vad.proportion_threshold) == \
        (4.5, 0.6, 2, 0.5)
    default = LF.longform_from_args(mod.build_parser().parse_args(base + ["--long_form"]))
    assert default == LF.LongFormConfig()
    assert mod.generation_config(plain) == mod.generation_config(long_)
    was = {k: v for k, v in vars(long_).items() if k != "long_form" and not k.startswith("vad_") and k != "max_segment_s"}
    assert was == {k: v for k, v in vars(plain).items() if k in was} and set(vars(plain)) == set(vars(long_))


def test_segment_audio_parser():
    from touchnet_amd.bin import segment_audio
    a = segment_audio.build_parser().parse_args(["--data_list", "l", "--output", "o", "--vad_pad_ms", "50"])
    assert a.sample_rate == 16000 and a.vad_pad_ms == 50.0 and not hasattr(a, "long_form")
