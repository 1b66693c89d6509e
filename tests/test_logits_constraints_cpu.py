"""Hotword biasing / forbidden sequences / min_new_tokens (touchnet_amd.generation, csrc/constrain.hip, csrc/beam.hip):
everything that must hold without a GPU — the oracle of the GPU tests (tests/logits_constraints_reference.py) against
transformers' processors and generate(), the generation config, the host-side plan, the op registrations and the argument
checks of the two C entry points."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_search_reference as bsr  # noqa: E402
import logits_constraints_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


# ------------------------------------------------------------------------------------------------ (1) the oracle is HF's
LONG = tuple(range(20, 36))                      # a sequence of 16 ids
CASES = {    # name -> (sequence_bias in dict order, contexts [R][n])
    "length 1, 2, 3 and 16": ({(7,): 1.5, (3, 7): -2.25, (2, 3, 9): 0.5, LONG: 4.0},
                              [[1] * 4 + list(LONG[:-1]), [5] * 16 + [2, 3, 7], [7] * 17 + [3, 3]]),
    "a sequence longer than the context": ({(4, 5, 6): 3.0, (5, 8): 1.0}, [[4, 5], [9, 5]]),
    "a context of one id": ({(4, 6): 3.0, (6,): 1.0, (4, 4, 6): 2.0}, [[4], [6]]),
    "same last id, both match, the order of the sum matters": (
        {(2, 3, 7): 1.0e8, (7,): 0.1, (3, 7): -1.0e8, (9, 3, 7): 5.0, (1, 2, 3, 7): 0.3}, [[1, 2, 3], [9, 9, 3], [9, 2, 3]]),
    "-inf and a finite bias on one id": ({(3, 7): -INF, (7,): 2.0, (2, 3, 7): 1.0, (8,): -INF}, [[1, 2, 3], [3, 3, 4]]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_transformers_sequence_bias(name):
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    sb, contexts = CASES[name]
    V = 40
    g = torch.Generator().manual_seed(len(name))
    scores = torch.randn(len(contexts), V, generator=g) * 3
    hf = SequenceBiasLogitsProcessor([[list(ids), float(b)] for ids, b in sb.items()])
    want = hf(torch.tensor(contexts, dtype=torch.int64), scores.clone())
    got = ref.constrain(scores, contexts, [1] * len(contexts), sb)
    assert torch.equal(got, want)
    assert not torch.equal(got, scores)
    # the sparse form the kernel writes holds exactly the ids that changed, with the same totals
    for r, h in enumerate(contexts):
        t = ref.targets(h, 1, sb, 0, (), V)
        dense = torch.zeros(V)
        for i, v in t.items():
            dense[i] = v
        assert torch.equal(scores[r] + dense, want[r])
        assert set(torch.nonzero(want[r] != scores[r]).flatten().tolist()) <= set(t)


def test_reference_equals_transformers_min_new_tokens_across_the_prompt_boundary():
    """min_new_tokens at generated = m - 1 and m, two eos ids, and a biased sequence whose ids lie on both sides of the
    prompt / generated boundary (the processors see one context: the prompt is part of it)."""
    from transformers.generation.logits_process import MinNewTokensLengthLogitsProcessor, SequenceBiasLogitsProcessor
    V, P, m, eos = 40, 3, 4, [2, 11]
    sb = {(5, 6, 7, 9): 2.5, (11,): 1.0}
    g = torch.Generator().manual_seed(1)
    for gen, held in ((m - 1, True), (m, False)):
        ctx = [[1, 5, 6] + [7] * gen, [4, 5, 6] + [7] + [8] * (gen - 1)]  # row 1 at gen = 3 ... 7 8 8: no match any more
        scores = torch.randn(2, V, generator=g)
        ids = torch.tensor(ctx, dtype=torch.int64)
        want = SequenceBiasLogitsProcessor([[list(k), v] for k, v in sb.items()])(ids, scores.clone())
        want = MinNewTokensLengthLogitsProcessor(P, m, eos)(ids, want)
        got = ref.constrain(scores, ctx, [P, P], sb, m, eos)
        assert torch.equal(got, want)
        assert bool(torch.isinf(got[:, eos]).all()) == held
    # the boundary case on its own: prompt [1, 5, 6], one generated id 7 -> (5, 6, 7, 9) matches
    t = ref.targets([1, 5, 6, 7], 3, sb, 0, (), V)
    assert t == {9: 2.5, 11: 1.0}
    scores = torch.randn(1, V, generator=g)
    want = SequenceBiasLogitsProcessor([[list(k), v] for k, v in sb.items()])(torch.tensor([[1, 5, 6, 7]]), scores.clone())
    assert torch.equal(ref.constrain(scores, [[1, 5, 6, 7]], [3], sb), want) and want[0, 9] == scores[0, 9] + 2.5


def test_composed_log_probs_equal_transformers_processor_list():
    """Beam search hands the processors log-probabilities.  A bias that turns a negative log-probability positive makes the
    repetition penalty divide where it would have multiplied: the order of the two matters, and is HF's."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SequenceBiasLogitsProcessor)
    V, P, m, eos, penalty, ngram = 40, 2, 3, [2], 1.5, 2
    hist = [6, 3, 7, 3]                                  # 7 was seen: penalised; the bigram (3, 7) bans 7 ... and biases it
    sb = {(3,): 30.0, (7, 3, 9): 25.0, (3, 7): 1.0, (6,): -INF}
    row = torch.randn(V, generator=torch.Generator().manual_seed(5))
    procs = LogitsProcessorList([SequenceBiasLogitsProcessor([[list(k), v] for k, v in sb.items()]),
                                 RepetitionPenaltyLogitsProcessor(penalty), NoRepeatNGramLogitsProcessor(ngram),
                                 MinNewTokensLengthLogitsProcessor(P, m, eos)])
    want = procs(torch.tensor([hist]), torch.log_softmax(row[None], -1))[0]
    got = ref.processed_log_probs(row, hist, P, sb, m, eos, penalty, ngram, torch.float32)
    assert torch.equal(got, want)
    lp = torch.log_softmax(row, -1)
    assert lp[3] < 0 and got[3] == (lp[3] + 30.0) / penalty > 0          # positive after the bias: divided
    assert got[7] == -INF and got[2] == -INF and got[6] == -INF


def _tiny_llama(seed):
    import transformers
    cfg = transformers.LlamaConfig(vocab_size=48, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                   num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=64,
                                   eos_token_id=2, pad_token_id=0, bos_token_id=1)
    torch.manual_seed(seed)
    m = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0, 0.25)
    return m


def _bias_for(free_run):
    """A sequence_bias that changes the run it is derived from: its second and third generated ids are forbidden as a
    pair, its first id and a few fixed sequences are boosted."""
    g = [int(t) for t in free_run]
    sb = {(g[1], g[2]): -INF, (g[0],): 0.75, (5,): 3.0, (5, 6): 6.0, (4, 5, 6, 8): 5.0, (g[0], g[1], 9): 2.0}
    return {k: v for k, v in sb.items() if all(t > 0 for t in k)}          # (HF's list form takes positive ids only)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_loop_equals_transformers_greedy_generate(seed):
    model = _tiny_llama(seed)
    n_new, eos, m, penalty, P = 12, 2, 4, 1.5, 6
    prompt = torch.randint(3, 48, (1, P), generator=torch.Generator().manual_seed(100 + seed))
    kw = dict(attention_mask=torch.ones_like(prompt), do_sample=False, repetition_penalty=penalty, max_new_tokens=n_new,
              eos_token_id=eos, pad_token_id=0)
    with torch.no_grad():
        free = model.generate(prompt, **kw)[0, P:].tolist()
        sb = _bias_for(free)
        out = model.generate(prompt, sequence_bias=[[list(k), v] for k, v in sb.items()], min_new_tokens=m, **kw)
    want = out[0, P:].tolist()
    assert want != free[:len(want)]
    hist = prompt[0].tolist()
    for _ in range(n_new):
        with torch.no_grad():
            logits = model(torch.tensor([hist])).logits[:, -1].float()
        s = ref.constrain(logits, [hist], [P], sb, m, [eos])[0]
        idx = torch.tensor(sorted(set(hist)))
        s[idx] = torch.where(s[idx] < 0, s[idx] * penalty, s[idx] / penalty)
        hist.append(int(s.argmax()))
        if hist[-1] == eos:
            break
    assert hist[P:] == want
    assert eos not in want[:m]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_composed_beam_reference_equals_transformers_beam_generate(seed):
    model = _tiny_llama(seed)
    K, n_new, eos, m, penalty, P = 3, 12, [2], 4, 1.5, 6
    prompts = torch.randint(3, 48, (2, P), generator=torch.Generator().manual_seed(200 + seed))
    kw = dict(attention_mask=torch.ones_like(prompts), num_beams=K, do_sample=False, repetition_penalty=penalty,
              max_new_tokens=n_new, eos_token_id=eos[0], pad_token_id=0, return_dict_in_generate=True, output_scores=True)
    with torch.no_grad():
        free = model.generate(prompts, **kw).sequences[:, P:]
        sb = _bias_for(free[0].tolist())
        out = model.generate(prompts, sequence_bias=[[list(k), v] for k, v in sb.items()], min_new_tokens=m, **kw)
    assert not torch.equal(out.sequences[:, P:], free)
    st = bsr.new_state(prompts.tolist(), K, P + n_new)
    skw = dict(penalty=penalty, ngram=0, eos=eos, n_new=n_new, length_penalty=1.0, early_stopping=False,
               dtype=torch.float32)
    for step in range(n_new):
        if int(st["n_unfinished"][0]) == 0:
            break
        rows = [r for r in range(2 * K) if step > 0 or r % K == 0]
        with torch.no_grad():
            logits = model(st["hist"][rows, :P + step].to(torch.int64)).logits[:, -1].float().detach().contiguous()
        ref.beam_step(bsr, st, logits, K, [P, P], sb, m, **skw)
    assert int(st["n_unfinished"][0]) == 0
    assert bsr.processed_log_probs.__module__ == "beam_search_reference"       # the composition put the module back
    for b, (ids, score) in enumerate(bsr.best_hypotheses(st, K, [P, P])):
        want = out.sequences[b, P:].tolist()
        assert want[:len(ids)] == ids and all(t in (0, eos[0]) for t in want[len(ids):]), (seed, b, ids, want)
        assert abs(score - float(out.sequences_scores[b])) < 1e-4, (seed, b)
        assert eos[0] not in ids[:m]


# ------------------------------------------------------------------------------------------------ (2) config and plan
def test_from_hf_accepts_sequence_bias_and_min_new_tokens():
    from touchnet_amd.generation import GenerationConfig
    c = GenerationConfig.from_hf({"sequence_bias": [[[5, 6], 2.0], [[6], -INF], [[5, 6], 3.0]], "min_new_tokens": 3})
    assert c.sequence_bias == {(5, 6): 3.0, (6,): -INF} and list(c.sequence_bias) == [(5, 6), (6,)]   # a dict's rule
    assert c.min_new_tokens == 3
    d = GenerationConfig.from_hf({"min_new_tokens": None, "sequence_bias": None})
    assert d.sequence_bias is None and d.min_new_tokens == 0
    assert GenerationConfig().sequence_bias is None and GenerationConfig().min_new_tokens == 0
    assert GenerationConfig.from_hf({}, sequence_bias={(1, 2): 1.0}, min_new_tokens=2).sequence_bias == {(1, 2): 1.0}
    for key, value in (("bad_words_ids", [[5]]), ("suppress_tokens", [1, 2])):
        with pytest.raises(ValueError, match=key) as e:
            GenerationConfig.from_hf({key: value})
        assert "sequence_bias" in str(e.value) and "-inf" in str(e.value)
    for key, value in (("min_length", 3), ("begin_suppress_tokens", [1]), ("forced_eos_token_id", 2),
                       ("forced_bos_token_id", 1)):
        with pytest.raises(ValueError, match=key):
            GenerationConfig.from_hf({key: value})
    for bad in ([[[5], INF]], [[[5], math.nan]], [[[], 1.0]], [[[5, -1], 1.0]], [[[5.5], 1.0]], [[5, 1.0, 2]], "x",
                [[[5], "a"]]):
        with pytest.raises(ValueError, match="sequence_bias"):
            GenerationConfig.from_hf({"sequence_bias": bad})
    with pytest.raises(ValueError, match="min_new_tokens"):
        GenerationConfig.from_hf({"min_new_tokens": -1})


def test_kimi_generation_config_keeps_refusing():
    from touchnet_amd.generation import KimiGenerationConfig
    with pytest.raises(TypeError):
        KimiGenerationConfig(sequence_bias={(1,): 1.0})


def test_hotword_bias_expands_prefixes_once():
    from touchnet_amd.generation import hotword_bias
    sb = hotword_bias([[1, 2, 3], [1, 2, 4], [7], [1, 2, 3]], 1.5)
    assert sb == {(1,): 1.5, (1, 2): 1.5, (1, 2, 3): 1.5, (1, 2, 4): 1.5, (7,): 1.5}
    assert list(sb) == [(1,), (1, 2), (1, 2, 3), (1, 2, 4), (7,)]
    assert hotword_bias([], 2.0) == {}
    with pytest.raises(ValueError):
        hotword_bias([[1, 2]], INF)


def test_plan_groups_by_last_id_in_hf_order():
    from touchnet_amd.generation import constraint_tables
    sb = {(2, 3, 7): 1.0, (9,): 4.0, (7,): 0.1, (3, 7): -1.0, (5, 9): 2.0, (4,): -INF}
    t = constraint_tables(sb, 3, [11, 7, 11], 50)
    assert t["grp_tok"] == [4, 7, 9, 11] and t["grp_eos"] == [0, 1, 0, 1] and t["min_new"] == 3 and t["vocab"] == 50
    seqs = [tuple(t["seq_ids"][a:b]) for a, b in zip(t["seq_off"], t["seq_off"][1:])]
    # within a group: the length-1 sequence first, then dict order; the last group (an eos id) holds no sequence
    assert seqs == [(4,), (7,), (2, 3, 7), (3, 7), (9,), (5, 9)]
    assert t["seq_bias"] == [-INF, 0.1, 1.0, -1.0, 4.0, 2.0] and t["grp_off"] == [0, 1, 4, 6, 6]
    # nothing to do: no plan; min_new_tokens alone: eos groups only; without an eos id it is inert
    assert constraint_tables(None, 0, [2], 50) is None and constraint_tables({}, 3, [], 50) is None
    only = constraint_tables(None, 2, [2], 50)
    assert only["grp_tok"] == [2] and only["seq_off"] == [0] and only["grp_off"] == [0, 0] and only["min_new"] == 2
    assert constraint_tables(sb, 0, [7], 50)["grp_eos"] == [0, 0, 0]
    # the totals the table yields equal the reference's, whatever the history
    for hist in ([2, 3], [5], [1, 2, 3, 3]):
        want = ref.targets(hist, 1, sb, 0, (), 50)
        got = {}
        for g, tok in enumerate(t["grp_tok"]):
            total, hit = torch.zeros((), dtype=torch.float32), False
            for s in range(t["grp_off"][g], t["grp_off"][g + 1]):
                ids = seqs[s]
                if len(ids) == 1 or (len(ids) <= len(hist) and hist[len(hist) - len(ids) + 1:] == list(ids[:-1])):
                    total, hit = total + torch.tensor(t["seq_bias"][s], dtype=torch.float32), True
            if hit:
                got[tok] = float(total)
        assert got == want, hist


def test_plan_limits():
    from touchnet_amd import generation as G
    assert G.MAX_BIAS_SEQS >= 8192 and G.MAX_BIAS_LEN >= 16
    ok = {(i % 100, i // 100 + 1, 3): 1.0 for i in range(G.MAX_BIAS_SEQS)}
    assert len(G.constraint_tables(ok, 0, [], 1000)["seq_bias"]) == G.MAX_BIAS_SEQS
    ok[(999,)] = 1.0
    with pytest.raises(ValueError, match="exceed"):
        G.constraint_tables(ok, 0, [], 1000)
    G.constraint_tables({tuple(range(1, G.MAX_BIAS_LEN + 1)): 1.0}, 0, [], 1000)
    with pytest.raises(ValueError, match="exceeds"):
        G.constraint_tables({tuple(range(1, G.MAX_BIAS_LEN + 2)): 1.0}, 0, [], 1000)
    with pytest.raises(ValueError, match="vocabulary"):
        G.constraint_tables({(5, 1000): 1.0}, 0, [], 1000)
    with pytest.raises(ValueError, match="empty"):
        G.constraint_tables({(): 1.0}, 0, [], 1000)
    with pytest.raises(ValueError, match="min_new_tokens"):
        G.constraint_tables(None, -2, [2], 1000)


# ------------------------------------------------------------------------------------------------ (3) ops and C ABI
def test_constraint_ops_are_registered_with_meta_kernels():
    from touchnet_amd import library as L
    for name in ("constrain_logits_", "beam_step_edits_"):
        assert name in L.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"mi355_touch::{name}", "Meta")
    s = str(torch.ops.mi355_touch.constrain_logits_.default._schema)
    assert "!) logits" in s and "!)? edit_ids" in s and "!)? edit_val" in s and "!)? edit_cnt" in s and "Tensor hist," in s
    s = str(torch.ops.mi355_touch.beam_step_edits_.default._schema)
    for name in ("hist", "src", "run_score", "fin_ids", "done", "n_unfinished"):
        assert f"!) {name}" in s, (name, s)
    assert "Tensor edit_ids" in s and "Tensor edit_val" in s
    m = lambda *shape, dt=torch.int32: torch.empty(*shape, dtype=dt, device="meta")
    out = torch.ops.mi355_touch.constrain_logits_(m(3, 100, dt=torch.bfloat16), m(3, 16), m(3), m(3), m(5), m(9),
                                                  m(4, dt=torch.float32), m(3), m(2), m(2), None, None, None, 1, 2)
    assert out is None


def test_header_and_stub_declare_the_constraint_entries():
    from touchnet_amd import _C
    text = open(os.path.join(ROOT, "include", "touchnet_amd.h")).read()
    assert "int tn_logits_constrain(" in text and "int tn_beam_step_edits(" in text
    assert "SequenceBiasLogitsProcessor" in text and "16384" in text
    assert "tn_logits_constrain" in _C.PROTOTYPES and "tn_beam_step_edits" in _C.PROTOTYPES


def test_c_entries_return_einval_before_any_launch():
    """Host addresses only: a launch would fault, -22 must come first."""
    from touchnet_amd import _C
    lib = _C.lib()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)
    odd = ctypes.c_void_p(a.value + 2)

    def con(ptrs=None, R_in=3, K=1, K_in=1, V=1000, S=16, n_seq=4, n_ids=9, n_grp=3, min_new=0, mode=0, dtype=0):
        p = [a] * 13
        for i, v in (ptrs or {}).items():
            p[i] = v
        return lib.tn_logits_constrain(*p, R_in, K, K_in, V, S, n_seq, n_ids, n_grp, min_new, mode, dtype, None)
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9):                     # logits, hist, hist_len, the six tables
        assert con({i: None}) == -22, i
        assert con({i: odd}) == -22, i
    assert con({3: None}, min_new=2) == -22                   # prompt_len is needed for min_new_tokens
    for i in (10, 11, 12):
        assert con({i: None}, mode=1) == -22 and con({i: odd}, mode=1) == -22, i
    assert con(n_seq=16385, n_ids=16385, n_grp=5) == -22 and con(n_grp=0) == -22 and con(n_grp=13) == -22
    assert con(n_ids=3) == -22 and con(n_ids=16384 * 64 + 1) == -22 and con(n_seq=-1) == -22
    assert con(V=0) == -22 and con(V=262145) == -22 and con(S=0) == -22 and con(R_in=0) == -22
    assert con(K=3, K_in=2) == -22 and con(R_in=4, K=3, K_in=3) == -22 and con(K=0) == -22
    assert con(min_new=-1) == -22 and con(mode=2) == -22 and con(dtype=2) == -22

    eos = (ctypes.c_int * 4)(1, 2, 3, 4)

    def step(ptrs=None, edits=(a, a, a), n_edit=5, K_in=3, V=128):
        p = [a] * 17
        for i, v in (ptrs or {}).items():
            p[i] = v
        return lib.tn_beam_step_edits(*p, 2, 3, K_in, V, 32, 1.5, 2, eos, 1, 8, 1.0, 0, 0, *edits, n_edit, None)
    for i in range(17):
        assert step({i: None}) == -22, i
    assert step(K_in=2) == -22 and step(V=63) == -22
    assert step(edits=(a, None, a)) == -22 and step(edits=(None, a, a)) == -22 and step(edits=(a, a, None)) == -22
    assert step(edits=(odd, a, a)) == -22 and step(edits=(a, a, odd)) == -22 and step(n_edit=0) == -22
    assert step({0: None}, edits=(None, None, None)) == -22   # a null list: tn_beam_step's own checks
