"""Hotword biasing, forbidden sequences and min_new_tokens on the MI355X: tn_logits_constrain exactly against the torch
restatement of transformers' processors (tests/logits_constraints_reference.py, pinned to transformers by
test_logits_constraints_cpu.py), tn_beam_step_edits against tn_beam_step and against the composed beam reference, generate()
with a plan against host-driven loops built from existing parts, opcheck, and the command line."""
import ctypes
import json
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_search_reference as bsr  # noqa: E402
import logits_constraints_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
INF = math.inf
S_HIST, GUARD = 24, 4096


# ---------------------------------------------------------------------------------------------------- (1) the kernel
def _kernel_case(V, n_table, seed=0):
    """Three history rows of 1, 5 and S_HIST ids and a table of n_table sequences.  With t the newest id of all three rows:
    (t, b) matches rows 1 and 2 but is longer than row 0's context (whose one id is t: only the length rule excludes
    it); (p, t, b) and the length-1 (b,) share b, so row 2 sums three biases whose order matters (1e8, -1e8, 0.1); a
    16-id sequence ends row 2; e carries a length-1 bias and a matching -inf."""
    g = torch.Generator().manual_seed(seed + n_table)
    ids = (torch.randperm(V - 20, generator=g)[:64] + 20).tolist()          # distinct ids >= 20
    t, b, c, d, e, p = ids[:6]
    rows = [[t], ids[6:9] + [p, t], ids[10:10 + S_HIST - 2] + [p, t]]
    long16 = tuple(rows[2][-15:]) + (c,)
    if n_table == 1:
        sb = {(t, b): 1.25}
    else:
        sb = {(p, t, b): 1.0e8, (b,): 0.1, (t, b): -1.0e8, long16: 4.0, (ids[40], d): 3.0, (e,): 2.0, (t, e): -INF}
        while len(sb) < n_table:                                             # fillers: lengths 1 .. 16, ids anywhere
            n = 1 + len(sb) % 16
            sb.setdefault(tuple(torch.randint(4, V, (n,), generator=g).tolist()), float(len(sb) % 7) - 3.0)
        assert len(sb) == n_table
    hist = torch.zeros(3, S_HIST, dtype=torch.int32)
    for r, h in enumerate(rows):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    return sb, rows, hist, (t, b, c, d, e)


def _expected(logits, rows, prompt_lens, sb, m, eos):
    """The logits after the in-place edit: only the reference's targets change, to T(fp32(logit) + total)."""
    want = logits.clone()
    V = logits.shape[1]
    for r, h in enumerate(rows):
        for i, total in ref.targets(h, prompt_lens[r], sb, m, eos, V).items():
            want[r, i] = (logits[r, i].float() + torch.tensor(total, dtype=torch.float32)).to(logits.dtype)
    assert torch.equal(want, ref.constrain(logits, rows, prompt_lens, sb, m, eos))       # the HF-pinned dense form
    return want


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,n_table", [(1000, 1), (1000, 7), (1000, 8192), (156032, 7)])
def test_constrain_kernel_equals_the_reference(V, n_table, dtype):
    """Apply and emit mode, with and without min_new_tokens (two eos ids, one of them a biased id; row 1 has generated
    m - 1 ids, row 2 m).  Apply: the targets equal the reference exactly, every other logit and the guard behind the
    buffer keep their bytes.  Emit: the same ids with the same totals, the logits untouched.  Repeats are bit-identical."""
    import touchnet_amd.functional as F
    from touchnet_amd.generation import ConstraintPlan
    sb, rows, hist, (t, b, c, d, e) = _kernel_case(V, n_table)
    g = torch.Generator().manual_seed(V + n_table)
    buf = (torch.randn(3 * V + GUARD, generator=g) * 3).to(dtype)
    logits = buf[:3 * V].view(3, V)
    hist_d = hist.to(DEV)
    hist_len = torch.tensor([len(h) for h in rows], dtype=torch.int32, device=DEV)
    m, eos = 3, [3, b]
    prompt_lens = [1, len(rows[1]) - (m - 1), len(rows[2]) - m]
    prompt_len = torch.tensor(prompt_lens, dtype=torch.int32, device=DEV)
    for min_new in (0, m):
        plan = ConstraintPlan.build(sb, min_new, eos, V, DEV)
        want = _expected(logits, rows, prompt_lens, sb, min_new, eos)
        runs = []
        for _ in range(2):
            dev = buf.to(DEV)
            F.constrain_logits_(dev[:3 * V].view(3, V), hist_d, hist_len, plan, prompt_len if min_new else None)
            torch.cuda.synchronize()
            runs.append(dev.cpu())
        assert torch.equal(_bits(runs[0][:3 * V].view(3, V)), _bits(want)), (V, n_table, min_new)
        assert torch.equal(_bits(runs[0][3 * V:]), _bits(buf[3 * V:]))                  # the guard
        assert torch.equal(_bits(runs[0]), _bits(runs[1]))
        changed = (_bits(want) != _bits(logits)).sum().item()
        assert changed >= (1 if n_table == 1 else 4)
        # emit
        dev = buf.to(DEV)
        outs = []
        for _ in range(2):
            edits = plan.edit_buffers(3)
            F.constrain_logits_(dev[:3 * V].view(3, V), hist_d, hist_len, plan, prompt_len if min_new else None,
                                edits=edits)
            torch.cuda.synchronize()
            outs.append([x.cpu() for x in edits])
        assert torch.equal(_bits(dev.cpu()), _bits(buf))
        ids, val, cnt = outs[0]
        for r, h in enumerate(rows):
            got = {int(i): float(v) for i, v in zip(ids[r].tolist(), val[r].tolist()) if i >= 0}
            assert got == ref.targets(h, prompt_lens[r], sb, min_new, eos, V), (r, min_new)
            assert int(cnt[r]) == len(got)
        key = torch.where(ids >= 0, ids, -1 - ids)
        assert torch.equal(key, plan.grp_tok.cpu()[None].expand(3, -1)) and bool((key[:, 1:] > key[:, :-1]).all())
        assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    if n_table == 7:
        # the cases were reached: row 0 ignores (t, b) by the length rule; row 2's b sums in HF's order; -inf wins
        t0 = ref.targets(rows[0], 1, sb, 0, (), V)
        t2 = ref.targets(rows[2], 1, sb, 0, (), V)
        assert t0[b] == pytest.approx(0.1) and t2[b] == 0.0 and t2[e] == -INF and t2[c] == 4.0 and d not in t2


def test_constrain_kernel_follows_the_beam_row_map():
    """B 2 x K 3 history rows; right after the prefill the B logits rows belong to rows 0 and 3 (K_in = 1), afterwards
    row for row (K_in = K).  Apply and emit."""
    import touchnet_amd.functional as F
    from touchnet_amd.generation import ConstraintPlan
    V, K, B = 1000, 3, 2
    g = torch.Generator().manual_seed(9)
    rows = [torch.randint(20, V, (n,), generator=g).tolist() for n in (4, 6, 6, 7, 5, 5)]
    sb = {(rows[r][-1], 100 + r): 1.0 + r for r in range(6)}
    sb[(rows[3][-2], rows[3][-1], 7)] = -INF
    sb[(50,)] = 0.5
    hist = torch.zeros(6, 16, dtype=torch.int32)
    for r, h in enumerate(rows):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    hist_len = torch.tensor([len(h) for h in rows], dtype=torch.int32, device=DEV)
    plan = ConstraintPlan.build(sb, 2, [3], V, DEV)
    for K_in in (1, K):
        live = [b * K + k for b in range(B) for k in range(K_in)]
        P = [len(rows[r]) - (r % 2) * 2 for r in range(6)]                  # odd rows have generated 2 ids: eos is free
        logits = torch.randn(B * K_in, V, generator=g)
        want = _expected(logits, [rows[r] for r in live], [P[r] for r in live], sb, 2, [3])
        dev = logits.to(DEV)
        prompt_len = torch.tensor(P, dtype=torch.int32, device=DEV)
        edits = plan.edit_buffers(B * K)
        F.constrain_logits_(dev, hist.to(DEV), hist_len, plan, prompt_len, num_beams=K, edits=edits)
        assert torch.equal(dev.cpu(), logits)
        for n, r in enumerate(live):
            got = {int(i): float(v) for i, v in zip(edits[0][n].tolist(), edits[1][n].tolist()) if i >= 0}
            assert got == ref.targets(rows[r], P[r], sb, 2, [3], V), (K_in, r)
            assert 100 + r in got
        F.constrain_logits_(dev, hist.to(DEV), hist_len, plan, prompt_len, num_beams=K)
        assert torch.equal(_bits(dev.cpu()), _bits(want))


def test_constrain_refuses_before_any_launch():
    import touchnet_amd.functional as F
    from touchnet_amd import _C
    from touchnet_amd.generation import ConstraintPlan
    plan = ConstraintPlan.build({(5, 6): 1.0}, 0, [], 1000, DEV)
    hist = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    n = torch.ones(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="vocabulary"):
        ConstraintPlan.build({(5, 1000): 1.0}, 0, [], 1000, DEV)
    with pytest.raises(ValueError, match="vocabulary"):
        F.constrain_logits_(torch.zeros(2, 900, device=DEV), hist, n, plan)
    with pytest.raises(_C.KernelError, match="contiguous"):
        F.constrain_logits_(torch.zeros(2, 2000, device=DEV)[:, :1000], hist, n, plan)
    with pytest.raises(_C.KernelError):
        F.constrain_logits_(torch.zeros(3, 1000, device=DEV), hist, n, plan)


# ---------------------------------------------------------------------------------------------------- (2) the beam step
def _state_to(st, device, float_dtype):
    return {k: v.to(device=device, dtype=float_dtype if v.is_floating_point() else v.dtype).contiguous()
            for k, v in st.items()}


class _S:                                               # the attribute view functional.beam_step takes
    def __init__(self, d, K):
        self.__dict__.update(d)
        self.num_beams = K


STATE = ("hist", "hist_len", "cache_len", "src", "run_score", "fin_ids", "fin_len", "fin_score", "fin_flag", "gen", "unsat",
         "done", "n_unfinished", "out_ids", "out_parent")


def _spiked(rows, V, g, forced):
    """[rows, V] fp32: a background in [-4, -2] and twelve spikes per row, 8 down in steps of 0.61 plus a jitter below 0.3, the first ones on
    `forced` ids in that order."""
    x = torch.rand(rows, V, generator=g) * 2 - 4
    for r in range(rows):
        ids = list(forced)
        for i in torch.randperm(V, generator=g).tolist():
            if len(ids) == 12:
                break
            if i not in ids:
                ids.append(i)
        x[r, ids] = 8.0 - 0.61 * torch.arange(12, dtype=torch.float32) + 0.3 * torch.rand(12, generator=g)
    return x


def _call_entry(name, logits, dev, B, K, kw, edits=None, null_list=False):
    """tn_beam_step / tn_beam_step_edits through ctypes, so that a NULL list reaches the entry itself."""
    from touchnet_amd import _C
    lib = _C.lib()
    R, S = dev["hist"].shape
    ws = torch.empty(int(lib.tn_beam_step_workspace_bytes(B, K)) // 4, dtype=torch.float32, device=DEV)
    eos = kw["eos"]
    eos_arr = (ctypes.c_int * max(1, len(eos)))(*eos)
    args = [_C.ptr(logits)] + [_C.ptr(dev[k]) for k in STATE] + [
        _C.ptr(ws), B, K, logits.shape[0] // B, logits.shape[1], S, kw["penalty"], kw["ngram"], eos_arr, len(eos),
        kw["n_new"], kw["length_penalty"], 0, 0]
    if name == "tn_beam_step":
        rc = lib.tn_beam_step(*args, _C.stream())
    elif null_list:
        rc = lib.tn_beam_step_edits(*args, None, None, None, 0, _C.stream())
    else:
        rc = lib.tn_beam_step_edits(*args, *[_C.ptr(x) for x in edits], edits[0].shape[1], _C.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc


BEAM_SB = {(11,): -INF, (12,): -3.0, (13,): 2.0, (12, 14): 5.0, (13, 14): 1.0, (15, 16, 14): 0.75, (17,): 0.5}
BEAM_FORCED = [11, 12, 13, 5, 14]                       # the top spike is forbidden; 5 is the eos id


def test_beam_step_edits_null_or_idle_list_equals_beam_step():
    """Two steps (K_in = 1, then K) from the same state through three paths: tn_beam_step, tn_beam_step_edits with a NULL
    list, and with a list in which no slot is active.  Every state tensor is byte-identical."""
    import touchnet_amd.functional as F
    from touchnet_amd.generation import ConstraintPlan
    B, K, V, S = 2, 3, 1000, 16
    g = torch.Generator().manual_seed(4)
    kw = dict(penalty=1.5, ngram=2, eos=[5], n_new=8, length_penalty=1.0)
    prompts = [[21, 22, 23], [31, 32, 33, 34, 32]]
    states = [_state_to(bsr.new_state(prompts, K, S), DEV, torch.float32) for _ in range(3)]
    idle = ConstraintPlan.build({(900, 901): 3.0, (902, 903, 904): -INF}, 0, [], V, DEV)      # never matches
    for K_in in (1, K):
        logits = _spiked(B * K_in, V, g, BEAM_FORCED).to(DEV)
        _call_entry("tn_beam_step", logits, states[0], B, K, kw)
        _call_entry("tn_beam_step_edits", logits, states[1], B, K, kw, null_list=True)
        edits = idle.edit_buffers(B * K)
        F.constrain_logits_(logits, states[2]["hist"], states[2]["hist_len"], idle, num_beams=K, edits=edits)
        assert int(edits[2][:B * K_in].sum()) == 0
        _call_entry("tn_beam_step_edits", logits, states[2], B, K, kw, edits=edits)
        for k in STATE:
            a = states[0][k].view(torch.int32)
            assert torch.equal(a, states[1][k].view(torch.int32)), (K_in, k, "NULL list")
            assert torch.equal(a, states[2][k].view(torch.int32)), (K_in, k, "idle list")
    assert int(states[0]["gen"][0]) == 2


def _fp32_path_error(logits, st, K, K_in, P, sb, m, eos, penalty):
    """max |acc of torch's fp32 path on the device - the fp64 restatement| over every finite candidate (the measure the
    beam step's own test uses: tests/test_beam_search_gpu.py)."""
    B = st["hist"].shape[0] // K
    worst = 0.0
    for b in range(B):
        if int(st["done"][b]):
            continue
        for k in range(K_in):
            r = b * K + k
            h = st["hist"][r, :int(st["hist_len"][r])].tolist()
            row = logits[b * K_in + k]
            lp32 = torch.log_softmax(row.to(DEV).float(), -1) + ref.bias_row(h, sb, row.shape[0]).to(DEV)
            idx = torch.tensor(sorted(set(h)), device=DEV)
            lp32[idx] = torch.where(lp32[idx] < 0, lp32[idx] * penalty, lp32[idx] / penalty)
            base = float(st["run_score"][r].float())
            acc32 = (lp32 + base).cpu().double()
            acc64 = ref.processed_log_probs(row, h, P[b], sb, 0, eos, penalty, 0, torch.float64) + base
            ok = torch.isfinite(acc64)
            worst = max(worst, float((acc32[ok] - acc64[ok]).abs().max()))
    return worst


def test_beam_step_edits_matches_the_composed_reference_over_six_steps():
    """B 2, K 3, V 1000, fp32 logits, penalty 1.5, min_new_tokens 3; the table forbids the top spike of every row, demotes
    the second, boosts the third and, after either of them, a fourth (whose log-probability a bias of 5 turns positive, so
    the penalty divides once it was seen).  Ids, parents, histories, tables and counters are exact at every step; scores
    within the accumulated bound: per step 4 x the error of torch's own fp32 path against the fp64 restatement (the
    existing beam test's measure; on the MI355X 1e-6 to 4e-6 here).  Every decision of the restatement has a margin above
    twice that, which is asserted (near-ties are no decision of the arithmetic: beam_search_reference._gaps)."""
    picked, want = _beam_steps_against_reference(1000, BEAM_SB, 6, seed=1)   # (seeds 0 .. 11: margins 2e-4 .. 2e-2)
    assert 11 not in picked and 14 in picked and int(want["fin_flag"].sum()) > 0


def test_beam_step_edits_with_a_large_table_at_a_large_vocabulary():
    """The same, two steps at V 156 032 (4 877 bitmap words: five per thread in the slot index) with 3 000 further
    length-1 biases in [-1, 1) spread over the vocabulary, so that every thread of the top-k kernel looks slots up."""
    V = 156032
    g = torch.Generator().manual_seed(3)
    sb = dict(BEAM_SB)
    ids, biases = torch.randperm(V - 20, generator=g)[:3000] + 20, torch.rand(3000, generator=g) * 2 - 1
    sb.update({(i,): v for i, v in zip(ids.tolist(), biases.tolist())})
    picked, want = _beam_steps_against_reference(V, sb, 2, seed=1)
    assert 11 not in picked


def _beam_steps_against_reference(V, sb, n_steps, seed):
    import touchnet_amd.functional as F
    from touchnet_amd.generation import ConstraintPlan
    B, K, S, m, eos = 2, 3, 16, 3, [5]
    g = torch.Generator().manual_seed(seed)
    prompts = [[21, 13, 12], [31, 32, 15, 16]]
    P = [len(p) for p in prompts]
    kw = dict(penalty=1.5, ngram=0, eos=eos, n_new=10, length_penalty=1.0, early_stopping=False)
    want = bsr.new_state(prompts, K, S)
    dev = _state_to(want, DEV, torch.float32)
    plan = ConstraintPlan.build(sb, m, eos, V, DEV)
    prompt_len = torch.tensor(P, dtype=torch.int32, device=DEV).repeat_interleave(K)
    edits = plan.edit_buffers(B * K)
    tol, picked = 0.0, set()
    for step in range(n_steps):
        K_in = 1 if step == 0 else K
        logits = _spiked(B * K_in, V, g, BEAM_FORCED)
        tol += 4 * _fp32_path_error(logits, want, K, K_in, P, sb, m, eos, kw["penalty"])
        margin = ref.beam_step(bsr, want, logits, K, P, sb, m, dtype=torch.float64, **kw)
        print(f"step {step}: margin {margin:.3g}, accumulated bound {tol:.3g}")
        assert margin > 2 * tol, (step, margin, tol)
        F.constrain_logits_(logits.to(DEV), dev["hist"], dev["hist_len"], plan, prompt_len, num_beams=K, edits=edits)
        F.beam_step(logits.to(DEV), _S(dev, K), edits=edits, **kw)
        torch.cuda.synchronize()
        got = {k: v.cpu() for k, v in dev.items()}
        for k in ("hist_len", "cache_len", "out_ids", "out_parent", "fin_flag", "fin_len", "gen", "unsat", "done",
                  "n_unfinished"):
            assert torch.equal(got[k], want[k]), (step, k, got[k], want[k])
        for r in range(B * K):
            n = int(want["hist_len"][r])
            assert torch.equal(got["hist"][r, :n], want["hist"][r, :n]), (step, r)
            assert torch.equal(got["src"][r, :n - 1], want["src"][r, :n - 1]), (step, r)
            if int(want["fin_flag"][r]):
                f = int(want["fin_len"][r])
                assert torch.equal(got["fin_ids"][r, :f], want["fin_ids"][r, :f]), (step, r)
        for k in ("run_score", "fin_score"):
            assert float((got[k].double() - want[k]).abs().max()) <= tol, (step, k)
        picked |= set(want["out_ids"].tolist())
        if step < m:
            assert eos[0] not in want["out_ids"].tolist()
    return picked, want


# ---------------------------------------------------------------------------------------------------- (3) end to end
def _tiny_touch_audio(seed, vocab=512, F_in=80):
    """The tiny TouchAudio Llama of tests/test_generation_gpu.py (rebuilt here), on the device in bf16."""
    from touchnet_amd.models.llama import DecoderConfig
    from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
    text = dict(model_type="llama", hidden_size=256, intermediate_size=512, num_attention_heads=8, num_key_value_heads=2,
                head_dim=64, num_hidden_layers=2, vocab_size=vocab, rope_theta=500000.0, tie_word_embeddings=True,
                rms_norm_eps=1e-5, initializer_range=0.08, pad_token_id=1, bos_token_id=2, eos_token_id=3)
    cfg = TouchAudioConfig(text_config=DecoderConfig.from_dict(text), input_size=F_in, pad_token_id=1)
    torch.manual_seed(seed)
    m = TouchAudioForCausalLM(cfg)
    m.post_init()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_(0, 0.1)
            p.copy_(p.to(torch.bfloat16).float())
    return m, text


@pytest.fixture(scope="module")
def tiny():
    m, _ = _tiny_touch_audio(seed=5)
    return m.to(DEV).to(torch.bfloat16).eval()


def _prompts(seed, lens=(9, 4, 14)):
    from touchnet_amd import generation as G
    g = torch.Generator().manual_seed(seed)
    return G.Prompts([torch.randint(4, 512, (n,), generator=g) for n in lens])


def _bias_from(free):
    """A sequence_bias that changes the run it is derived from (row 0 of `free`): a pair of it is forbidden, its first id
    demoted, a few sequences boosted."""
    r = free[0].tolist()
    return {(r[1], r[2]): -INF, (r[0],): -1.5, (40,): 1.0, (r[0], r[1], 41): 2.0, (r[3],): 0.25, (r[2], r[3]): -0.5}


def _host_loop(model, prompts, cfg, sb, m, eos, row_keys=None):
    """generate() from existing parts: decode_logits, the reference edit in torch on the host, the existing step ops."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    lm, proj = G._parts(model)
    P = [int(t.numel()) for t in prompts.input_ids]
    B, n_new = len(P), cfg.new_tokens(max(P))
    c = lm.config
    cache = G.KVCache.allocate(len(lm.model.layers), B, max(P) + n_new, c.num_key_value_heads, c.head_dim, DEV)
    logits = G._prefill(lm, proj, prompts, cache, DEV)
    for step in range(n_new):
        hists = [cache.hist[b, :int(cache.hist_len[b])].tolist() for b in range(B)]
        edited = ref.constrain(logits.cpu(), hists, P, sb, m, eos).to(DEV)
        if cfg.do_sample:
            F.sample_step(edited, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                          cfg.repetition_penalty, True, cfg.temperature, cfg.top_k, cfg.top_p, cfg.seed, eos, 1,
                          row_key=row_keys)
        else:
            F.greedy_step(edited, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                          cfg.repetition_penalty, cfg.no_repeat_ngram_size, eos[0], 1)
        if int(cache.n_unfinished.item()) == 0 or step + 1 == n_new:
            break
        logits = G.decode_logits(lm, cache)
    idx = torch.tensor(P, device=DEV)[:, None] + torch.arange(step + 1, device=DEV)[None]
    return cache.hist.gather(1, idx).to(torch.int64)


@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_generate_with_a_plan_equals_the_host_driven_loop(tiny, mode):
    """Token-exact: both sides see the same bf16 logits, and the reference edit (logits.float() + bias).to(bfloat16) is the
    kernel's arithmetic."""
    from touchnet_amd import generation as G
    prompts, eos, m = _prompts(1), [3], 5
    if mode == "greedy":
        base = dict(max_new_tokens=14, repetition_penalty=1.5, no_repeat_ngram_size=2, eos_token_id=3, pad_token_id=1)
    else:
        base = dict(max_new_tokens=14, repetition_penalty=1.2, no_repeat_ngram_size=0, eos_token_id=3, pad_token_id=1,
                    do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=7)
    with torch.no_grad():
        free = G.generate(tiny, prompts, G.GenerationConfig(**base))
        sb = _bias_from(free)
        cfg = G.GenerationConfig(sequence_bias=sb, min_new_tokens=m, **base)
        out = G.generate(tiny, prompts, cfg)
        keys = torch.arange(3, dtype=torch.int64, device=DEV)
        want = _host_loop(tiny, prompts, cfg, sb, m, eos, keys)
    n = min(out.shape[1], want.shape[1])
    assert torch.equal(out[:, :n], want[:, :n]) and (out[:, n:] == 1).all() and (want[:, n:] == 1).all()
    assert out[0].tolist() != free[0].tolist()
    assert not (out[:, :m] == 3).any()
    r = free[0].tolist()
    assert (r[1], r[2]) not in list(zip(out[0].tolist(), out[0].tolist()[1:]))


def test_a_hotword_appears_with_the_plan_and_not_without(tiny):
    """A three-token phrase none of whose ids the free run emits.  bias 30 towers over this model's logits (|l| < 12), and
    a repetition penalty of 3 cuts an emitted hotword token back to a third, so the next token of the phrase wins."""
    from touchnet_amd import generation as G
    prompts = _prompts(2)
    base = dict(max_new_tokens=10, repetition_penalty=3.0, no_repeat_ngram_size=0, eos_token_id=3, pad_token_id=1)
    with torch.no_grad():
        free = G.generate(tiny, prompts, G.GenerationConfig(**base))
        used = set(free.flatten().tolist()) | {int(t) for p in prompts.input_ids for t in p}
        phrase = [t for t in range(100, 512) if t not in used][:3]
        out = G.generate(tiny, prompts, G.GenerationConfig(sequence_bias=G.hotword_bias([phrase], 30.0), **base))
    inside = lambda row: any(row[i:i + 3] == phrase for i in range(len(row) - 2))
    assert all(inside(r) for r in out.tolist()) and not any(inside(r) for r in free.tolist())
    assert out[:, :3].tolist() == [phrase] * 3


def test_a_forbidden_sequence_never_appears(tiny):
    from touchnet_amd import generation as G
    prompts = _prompts(3)
    base = dict(max_new_tokens=16, repetition_penalty=1.0, no_repeat_ngram_size=0, eos_token_id=3, pad_token_id=1)
    with torch.no_grad():
        free = G.generate(tiny, prompts, G.GenerationConfig(**base))
        pairs = {(r[i], r[i + 1]) for r in free.tolist() for i in range(2, 6)}
        out = G.generate(tiny, prompts, G.GenerationConfig(sequence_bias={p: -INF for p in pairs}, **base))
    for row in out.tolist():
        assert not pairs & set(zip(row, row[1:]))
    assert out.tolist() != free.tolist()


BEAM_E2E_SEED = 0            # prompt seed whose composed reference run has every decision margin above 1e-3 on the MI355X


def test_generate_with_beams_and_a_plan_equals_the_composed_reference(tiny):
    """B 3, K 3, 12 new tokens: the composed reference (fp64, host) on log-probabilities computed from the device's logits,
    dense caches reordered like HF's; the product follows its table and adds the totals inside the step.  Both see
    bit-identical logits as long as they take the same decisions; the reference's margins are all above 1e-3."""
    from touchnet_amd import generation as G
    K, eos, m = 3, [3], 4
    prompts = _prompts(100 + BEAM_E2E_SEED)
    P = [int(t.numel()) for t in prompts.input_ids]
    base = dict(max_new_tokens=12, repetition_penalty=1.5, no_repeat_ngram_size=2, num_beams=K, eos_token_id=3,
                pad_token_id=1)
    lm, proj = G._parts(tiny)
    c = lm.config
    with torch.no_grad():
        free = G.generate(tiny, prompts, G.GenerationConfig(**base))
        sb = _bias_from(free)
        cfg = G.GenerationConfig(sequence_bias=sb, min_new_tokens=m, **base)
        out, state = G.generate(tiny, prompts, cfg, return_cache=True)
        # the reference loop (tests/test_beam_search_gpu.py's, with the composed step)
        B, n_new = 3, 12
        R, S = B * K, max(P) + n_new
        small = G.KVCache.allocate(len(lm.model.layers), B, S, c.num_key_value_heads, c.head_dim, DEV)
        logits = G._prefill(lm, proj, prompts, small, DEV)
        rep = torch.arange(R, device=DEV) // K
        dense = G.KVCache.allocate(len(lm.model.layers), R, S, c.num_key_value_heads, c.head_dim, DEV)
        dense.k = [t.index_select(0, rep) for t in small.k]
        dense.v = [t.index_select(0, rep) for t in small.v]
        st = bsr.new_state([t.tolist() for t in prompts.input_ids], K, S)
        kw = dict(penalty=1.5, ngram=2, eos=eos, n_new=n_new, length_penalty=1.0, early_stopping=False,
                  dtype=torch.float64)
        margin, steps = math.inf, 0
        for step in range(n_new):
            live = [b for b in range(B) if not int(st["done"][b])]
            if not live:
                break
            steps += 1
            margin = min(margin, ref.beam_step(bsr, st, logits.float().cpu().contiguous(), K, P, sb, m, **kw))
            parent = torch.arange(R)
            for b in live:
                parent[b * K:b * K + K] = st["out_parent"][b * K:b * K + K].long()
            parent = parent.to(DEV)
            dense.k = [t.index_select(0, parent) for t in dense.k]
            dense.v = [t.index_select(0, parent) for t in dense.v]
            dense.hist, dense.hist_len = st["hist"].to(DEV), st["hist_len"].to(DEV)
            dense.cache_len = st["cache_len"].to(DEV)
            if step + 1 < n_new:
                logits = G.decode_logits(lm, dense)
    print(f"smallest decision margin {margin:.3g} over {steps} steps")
    assert margin > 1e-3, margin
    ids, scores = state.best(P, pad=1)
    assert torch.equal(ids, out)
    for b, (w_ids, w_score) in enumerate(bsr.best_hypotheses(st, K, P)):
        assert out[b, :len(w_ids)].tolist() == w_ids and (out[b, len(w_ids):] == 1).all(), (b, out[b].tolist(), w_ids)
        assert abs(float(scores[b]) - w_score) <= 8.6e-6 * steps, (b, float(scores[b]), w_score)
        assert 3 not in w_ids[:m]
    assert out.tolist() != free.tolist()


# ---------------------------------------------------------------------------------------------------- (4) wiring
def test_opcheck_of_the_constrain_op():
    from torch.library import opcheck
    from touchnet_amd.generation import ConstraintPlan
    sb, rows, hist, _ = _kernel_case(1000, 7)
    plan = ConstraintPlan.build(sb, 2, [3], 1000, DEV)
    hist_len = torch.tensor([len(h) for h in rows], dtype=torch.int32, device=DEV)
    prompt_len = torch.ones(3, dtype=torch.int32, device=DEV)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    table = (plan.seq_off, plan.seq_ids, plan.seq_bias, plan.grp_off, plan.grp_tok, plan.grp_eos)
    for dtype in (torch.float32, torch.bfloat16):
        logits = torch.randn(3, 1000, device=DEV).to(dtype)
        opcheck(torch.ops.mi355_touch.constrain_logits_.default,
                (logits, hist.to(DEV), hist_len, prompt_len, *table, None, None, None, 1, 2), test_utils=tests)
        opcheck(torch.ops.mi355_touch.constrain_logits_.default,
                (logits, hist.to(DEV), hist_len, prompt_len, *table, *plan.edit_buffers(3), 1, 2), test_utils=tests)


def test_infer_asr_command_line_with_hotwords(tmp_path):
    """--hotwords / --forbid_words / --min_new_tokens on a temporary checkpoint directory with a word-level tokenizer: the
    command's output equals transcribe() with the config the flags describe; without a tokenizer the flag is refused."""
    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from touchnet_amd.bin import infer_asr
    from touchnet_amd.generation import GenerationConfig, hotword_bias
    from touchnet_amd.models.touch_audio.inference_touch_audio import transcribe
    m, text = _tiny_touch_audio(seed=21, vocab=512, F_in=320)
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    save_file({k: v.contiguous() for k, v in m.state_dict().items() if k != "language_model.lm_head.weight"},
              str(ckpt / "model.safetensors"))                               # (tied to the embedding)
    (ckpt / "config.json").write_text(json.dumps({"text_config": text, "audio_config": {"input_size": 320},
                                                  "pad_token_id": 1}))
    (tmp_path / "data_config.json").write_text(json.dumps({"audio_feat_type": "fbank", "audiofeat_num_mel_bins": 80,
                                                           "audiofeat_stack_length": 4, "audiofeat_stride_length": 4}))
    rng = np.random.RandomState(0)
    lines = []
    for i, sec in enumerate([1.3, 0.4]):
        p = tmp_path / f"u{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes((rng.randn(int(sec * 16000)) * 3000).clip(-32768, 32767).astype(np.int16).tobytes())
        lines.append({"key": f"u{i}", "wav": str(p), "txt": "x"})
    (tmp_path / "data.list").write_text("".join(json.dumps(x) + "\n" for x in lines))
    (tmp_path / "hot.txt").write_text("w200 w201 w202\n\n")
    (tmp_path / "forbid.txt").write_text("w7 w8\n")
    args = ["--model_path", str(ckpt), "--data_list", str(tmp_path / "data.list"), "--data_config",
            str(tmp_path / "data_config.json"), "--batch_size", "2", "--max_new_tokens", "8", "--hotwords",
            str(tmp_path / "hot.txt"), "--hotword_bias", "30", "--forbid_words", str(tmp_path / "forbid.txt"),
            "--min_new_tokens", "3", "--repetition_penalty", "3.0"]
    with pytest.raises(ValueError, match="tokenizer"):
        infer_asr.main(args + ["--output_dir", str(tmp_path / "none")])
    vocab = {"[UNK]": 0, **{f"w{i}": i for i in range(1, 512)}}
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="[UNK]").save_pretrained(str(ckpt))
    out = infer_asr.main(args + ["--output_dir", str(tmp_path / "out")])
    recs = [json.loads(x) for x in open(out)]
    model = infer_asr.load_model(str(ckpt), DEV)
    dcfg = infer_asr.data_config(type("A", (), {"data_config": str(tmp_path / "data_config.json"),
                                                "model_path": str(ckpt)})(), model)
    feats = infer_asr.features([infer_asr.read_wav(x["wav"]) for x in lines], dcfg)
    sb = hotword_bias([[200, 201, 202]], 30.0)
    sb[(7, 8)] = -INF
    cfg = GenerationConfig(max_new_tokens=8, repetition_penalty=3.0, sequence_bias=sb, min_new_tokens=3)
    assert [r["predict_ids"] for r in recs] == transcribe(model, feats, cfg)
    assert all(r["predict_ids"][:3] == [200, 201, 202] for r in recs), recs


def test_infer_qwen2_audio_command_line_merges_hotwords_with_the_generation_config(tmp_path):
    """generation_config.json carries a sequence_bias and min_new_tokens of its own; --hotwords and --forbid_words are merged
    over it (the file's entries, then the hotwords, then the forbidden phrases)."""
    from safetensors.torch import save_file
    from test_sampling_gpu import _tiny_qwen2_audio, _tiny_tokenizer, _wavs
    from touchnet_amd.bin import infer_qwen2_audio as cli
    from touchnet_amd.generation import GenerationConfig, hotword_bias
    from touchnet_amd.models.qwen2_audio import inference_qwen2_audio as Q
    tok, _ = _tiny_tokenizer(tmp_path)
    hf, _, d, eos = _tiny_qwen2_audio(tok, seed=6)
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    save_file({k: v.contiguous() for k, v in hf.state_dict().items()}, str(ckpt / "model.safetensors"))
    (ckpt / "config.json").write_text(json.dumps(d))
    gen = {"repetition_penalty": 1.1, "eos_token_id": eos, "pad_token_id": eos[0], "min_new_tokens": 2,
           "sequence_bias": [[[5, 6], 1.5], [[40, 41], 4.0]]}
    (ckpt / "generation_config.json").write_text(json.dumps(gen))
    tok.save_pretrained(str(ckpt))
    wavs = _wavs([1.3, 0.4], seed=3)
    lines = []
    for i, w in enumerate(wavs):
        p = tmp_path / f"u{i}.wav"
        with wave.open(str(p), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(w.numpy().tobytes())
        lines.append({"key": f"u{i}", "wav": str(p), "txt": "x"})
    (tmp_path / "data.list").write_text("".join(json.dumps(x) + "\n" for x in lines))
    (tmp_path / "hot.txt").write_text("w40 w41 w42\n")
    (tmp_path / "forbid.txt").write_text("w5 w6\n")
    out = cli.main(["--model_path", str(ckpt), "--data_list", str(tmp_path / "data.list"), "--instruct", "w3",
                    "--batch_size", "2", "--max_length", "400", "--max_new_tokens", "8", "--hotwords",
                    str(tmp_path / "hot.txt"), "--hotword_bias", "3.5", "--forbid_words", str(tmp_path / "forbid.txt"),
                    "--output_dir", str(tmp_path / "out")])
    recs = [json.loads(x) for x in open(out)]
    model = cli.load_model(str(ckpt), DEV)
    sb = {(5, 6): -INF, (40, 41): 3.5, (40,): 3.5, (40, 41, 42): 3.5}
    cfg = GenerationConfig.from_hf(str(ckpt), max_length=400)
    assert cfg.sequence_bias == {(5, 6): 1.5, (40, 41): 4.0} and cfg.min_new_tokens == 2
    cfg.max_new_tokens = 8
    cfg.sequence_bias = sb
    assert hotword_bias([[40, 41, 42]], 3.5) == {k: v for k, v in sb.items() if k != (5, 6)}
    assert [r["predict"] for r in recs] == Q.transcribe(model, wavs, tok, "w3", cfg)[1]
