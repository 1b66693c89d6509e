"""Token confidences and N-best lists: everything that must hold without a GPU — the float64 restatement of
tn_token_scores against torch, its budget against a plain fp32 evaluation, op registration, header and prototype, the
refusals of the C entry point before any launch, the config knobs, BeamState.nbest against the beam-search restatement
and against transformers' num_return_sequences, and the command-line side (records, --jsonl, --oracle)."""
import ctypes as C
import json
import math
import os

import pytest
import torch

import beam_search_reference as beam_ref
import edit_align_reference as align_ref
import token_scores_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_equals_torch_on_tie_free_rows(dtype):
    g = torch.Generator().manual_seed(0)
    V, k = 200, 8
    logits = ((torch.randperm(V, generator=g).float() - 100.0) / 8.0).to(dtype)[None].repeat(3, 1)   # distinct in bf16 too
    logits[1] = logits[1].flip(0)
    logits[2] = logits[2].roll(17)
    assert all(logits[r].unique().numel() == V for r in range(3))
    tok = torch.tensor([0, V - 1, V // 2])
    ref = R.scores(logits, tok, k)
    lsm = torch.log_softmax(logits.double(), -1)
    assert torch.allclose(ref["logp"], lsm[torch.arange(3), tok], rtol=0, atol=1e-12)
    assert torch.allclose(ref["entropy"], -(lsm.exp() * lsm).sum(-1), rtol=0, atol=1e-12)
    top = torch.topk(logits.double(), k, dim=-1)
    assert torch.equal(ref["alt_id"], top.indices)
    assert torch.allclose(ref["alt_logp"], lsm.gather(1, top.indices), rtol=0, atol=1e-12)


def test_reference_tie_rule_tail_and_sick_rows():
    row = torch.tensor([1.0, 3.0, 3.0, -math.inf, 3.0, 1.0])
    r = R.row_scores(row, 3, 8)
    assert r["alt_id"] == [1, 2, 4, 0, 5, 3, -1, -1] and r["logp"] == -math.inf
    assert r["alt_logp"][5] == -math.inf and r["alt_logp"][6] == -math.inf and not math.isnan(r["entropy"])
    assert math.isnan(R.row_scores(row, 6, 0)["logp"]) and math.isnan(R.row_scores(row, -1, 0)["logp"])
    for bad in (torch.tensor([0.0, math.nan]), torch.tensor([math.inf, 0.0]), torch.tensor([-math.inf, -math.inf])):
        r = R.row_scores(bad, 0, 2)
        assert math.isnan(r["logp"]) and math.isnan(r["entropy"]) and r["alt_id"] == [-1, -1]
    assert abs(R.row_scores(torch.zeros(16), 3, 0)["entropy"] - math.log(16)) < 1e-12


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [65, 4097, 152064, 262144])
def test_budget_covers_a_plain_fp32_evaluation_and_stays_under_its_ceilings(dtype, V):
    """the kernel's arithmetic and partition restated in fp32 on the CPU (torch's exp / log in place of the device's)"""
    for seed, kind in enumerate(("random", "equal", "dominant")):
        row = R.make_rows(kind, 1, V, dtype, seed)[0]
        tok = V // 3
        ref = R.row_scores(row, tok, 0)
        assert ref["budget_logp"] < R.LOGP_CEILING and ref["budget_entropy"] < R.ENTROPY_CEILING, (kind, ref)
        lp, ent = R.fp32_partial_sum_evaluation(row, tok)
        assert abs(lp - ref["logp"]) <= ref["budget_logp"], (kind, lp - ref["logp"], ref["budget_logp"])
        assert abs(ent - ref["entropy"]) <= ref["budget_entropy"], (kind, ent - ref["entropy"], ref["budget_entropy"])


# ------------------------------------------------------------------------------------------------ ops, header, prototype
def test_ops_are_registered_with_meta_shapes_in_both_modes():
    import touchnet_amd.library as L
    for name in ("token_scores", "token_scores_"):
        assert name in L.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"mi355_touch::{name}", "Meta")
    s = str(torch.ops.mi355_touch.token_scores_.default._schema)
    for name in ("logp", "entropy", "alt_id", "alt_logp"):
        assert f"!) {name}" in s or f"!)? {name}" in s, s                # (the alternatives are optional: k == 0)
    assert "!" not in str(torch.ops.mi355_touch.token_scores.default._schema)
    m = lambda *shape, dt=torch.bfloat16: torch.empty(*shape, dtype=dt, device="meta")
    for k in (0, 5):
        logp, ent, ids, alp = torch.ops.mi355_touch.token_scores(m(7, 1000), m(7, dt=torch.int32), k)
        assert logp.shape == ent.shape == (7,) and logp.dtype == ent.dtype == alp.dtype == torch.float32
        assert ids.shape == alp.shape == (7, k) and ids.dtype == torch.int32
    f = lambda *shape: m(*shape, dt=torch.float32)
    assert torch.ops.mi355_touch.token_scores_(m(7, 1000), m(7, 9, dt=torch.int32), m(7, dt=torch.int32), f(7, 9), f(7, 9),
                                               m(7, 9, 5, dt=torch.int32), f(7, 9, 5), 5) is None
    assert torch.ops.mi355_touch.token_scores_(m(7, 1000), m(7, 9, dt=torch.int32), m(7, dt=torch.int32), f(7, 9), f(7, 9),
                                               None, None, 0) is None


def test_functional_layer_and_backend_expose_the_scores():
    import touchnet_amd.functional as F
    from touchnet_amd.models.backend import ops
    assert callable(F.token_scores) and callable(F.token_scores_) and callable(getattr(ops(), "token_scores"))


def test_header_and_stub_declare_the_entry():
    from touchnet_amd import _C
    text = open(os.path.join(ROOT, "include", "touchnet_amd.h")).read()
    assert "int tn_token_scores(" in text and "compute_transition_scores" in text and "ties to the lower id" in text
    assert len(_C.PROTOTYPES["tn_token_scores"]) == 14


def test_entry_point_refuses_every_rule_before_any_launch():
    """Host addresses only: a launch would fault, -22 must come first."""
    from touchnet_amd import _C
    lib = _C.lib()
    buf = (C.c_char * 4096)()
    a = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)
    odd2, odd1 = C.c_void_p(a.value + 2), C.c_void_p(a.value + 1)

    def call(logits=a, tok=a, hist=None, hist_len=None, logp=a, entropy=a, alt_id=a, alt_logp=a, R_=3, V=100, S=0, k=2,
             dtype=1):
        return lib.tn_token_scores(logits, tok, hist, hist_len, logp, entropy, alt_id, alt_logp, R_, V, S, k, dtype, None)
    hist = dict(tok=None, hist=a, hist_len=a, S=8)
    cases = dict(
        null_logits=dict(logits=None), null_logp=dict(logp=None), null_entropy=dict(entropy=None),
        null_alt_id=dict(alt_id=None), null_alt_logp=dict(alt_logp=None),
        bf16_logits_on_an_odd_byte=dict(logits=odd1), fp32_logits_on_a_half_word=dict(logits=odd2, dtype=0),
        tok_misaligned=dict(tok=odd2), logp_misaligned=dict(logp=odd2), entropy_misaligned=dict(entropy=odd2),
        alt_id_misaligned=dict(alt_id=odd2), alt_logp_misaligned=dict(alt_logp=odd2),
        hist_misaligned=dict(hist, hist=odd2), hist_len_misaligned=dict(hist, hist_len=odd2),
        vocab_zero=dict(V=0), vocab_negative=dict(V=-1), vocab_too_large=dict(V=262145),
        k_negative=dict(k=-1), k_nine=dict(k=9), rows_negative=dict(R_=-1),
        both_ways=dict(hist, tok=a), both_ways_half=dict(hist_len=a), neither_way=dict(tok=None),
        hist_without_len=dict(hist, hist_len=None), len_without_hist=dict(hist, hist=None),
        s_hist_zero=dict(hist, S=0), s_hist_negative=dict(hist, S=-4),
        dtype_unknown=dict(dtype=2), dtype_negative=dict(dtype=-1))
    for what, kw in cases.items():
        assert call(**kw) == -22, what
    # nothing to do is no error and launches nothing; k == 0 needs no alternative buffers (the check, then R == 0)
    assert call(R_=0) == 0 and call(R_=0, k=0, alt_id=None, alt_logp=None) == 0 and call(R_=0, **hist) == 0
    assert call(R_=0, V=262144, k=8) == 0 and call(R_=0, logits=odd2) == 0


# ------------------------------------------------------------------------------------------------ the knobs
def test_config_knobs_default_off_and_are_validated():
    from touchnet_amd.generation import GenerationConfig, KimiGenerationConfig
    d = GenerationConfig()
    assert (d.output_scores, d.top_alternatives, d.nbest, d.wants_scores) == (False, 0, 1, False)
    k = KimiGenerationConfig()
    assert (k.output_scores, k.top_alternatives, k.wants_scores) == (False, 0, False) and not hasattr(k, "nbest")
    assert GenerationConfig(top_alternatives=3).wants_scores and KimiGenerationConfig(top_alternatives=8).wants_scores
    assert GenerationConfig(output_scores=True).wants_scores
    with pytest.raises(ValueError, match="nbest"):
        GenerationConfig(nbest=2)                                   # no beams
    with pytest.raises(ValueError, match="nbest"):
        GenerationConfig(nbest=5, num_beams=4)
    with pytest.raises(ValueError, match="nbest"):
        GenerationConfig(nbest=0)
    assert GenerationConfig(nbest=4, num_beams=4).nbest == 4
    for bad in (9, -1, True, 2.0):
        with pytest.raises(ValueError, match="top_alternatives"):
            GenerationConfig(top_alternatives=bad)
        with pytest.raises(ValueError, match="top_alternatives"):
            KimiGenerationConfig(top_alternatives=bad)
    cfg = GenerationConfig(num_beams=4, nbest=2)
    cfg.num_beams = 1
    with pytest.raises(ValueError, match="nbest"):
        cfg.check_scores()


def test_from_hf_takes_the_knobs_as_overrides_and_still_refuses_num_return_sequences():
    from touchnet_amd.generation import GenerationConfig
    cfg = GenerationConfig.from_hf({"num_beams": 4}, nbest=3, output_scores=True, top_alternatives=2)
    assert (cfg.nbest, cfg.output_scores, cfg.top_alternatives) == (3, True, 2)
    assert GenerationConfig.from_hf({"output_scores": True}).output_scores is False      # (HF's key means something else)
    with pytest.raises(ValueError, match="nbest"):
        GenerationConfig.from_hf({}, nbest=2)
    with pytest.raises(ValueError, match="top_alternatives"):
        GenerationConfig.from_hf({}, top_alternatives=9)
    with pytest.raises(ValueError, match="num_return_sequences.*nbest = N"):
        GenerationConfig.from_hf({"num_beams": 4, "num_return_sequences": 2})
    with pytest.raises(ValueError, match="num_return_sequences"):
        GenerationConfig.from_hf({"num_beams": 4, "num_return_sequences": 3}, nbest=2)
    for key, value in (("num_beam_groups", 2), ("penalty_alpha", 0.6), ("bad_words_ids", [[1]])):
        with pytest.raises(ValueError, match=key):
            GenerationConfig.from_hf({key: value})


# ------------------------------------------------------------------------------------------------ BeamState.nbest
def _beam_state(st, K):
    from touchnet_amd.generation import BeamState
    return BeamState(num_beams=K, k=[], v=[], **{name: st[name] for name in (
        "cache_len", "hist", "hist_len", "src", "run_score", "fin_ids", "fin_len", "fin_score", "fin_flag", "gen", "unsat",
        "done", "n_unfinished", "out_ids", "out_parent")})


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


def _drive(model, prompts, K, n_new, eos, **kw):
    P = prompts.shape[1]
    st = beam_ref.new_state(prompts.tolist(), K, P + n_new)
    B = prompts.shape[0]
    for step in range(n_new):
        if int(st["n_unfinished"][0]) == 0:
            break
        rows = [r for r in range(B * K) if step > 0 or r % K == 0]
        with torch.no_grad():
            logits = model(st["hist"][rows, :P + step].to(torch.int64)).logits[:, -1].float().detach()
        beam_ref.beam_step(st, logits, K=K, eos=eos, n_new=n_new, dtype=torch.float32, **kw)
    return st


def test_nbest_reads_the_finished_set_and_reports_short_lists():
    K, P, S = 4, 3, 12
    st = beam_ref.new_state([[5, 6, 7], [8, 9, 10]], K, S)
    # utterance 0: three finished hypotheses of lengths 2, 4, 1; utterance 1: one
    for r, (ids, score) in {0: ([11, 2], -0.5), 1: ([12, 13, 14, 2], -0.75), 2: ([2], -1.5), 4: ([21, 22, 2], -0.25)}.items():
        st["fin_ids"][r, :P] = st["hist"][r // K * K, :P]
        st["fin_ids"][r, P:P + len(ids)] = torch.tensor(ids, dtype=torch.int32)
        st["fin_ids"][r, P + len(ids):] = 99                        # junk behind the end must not leak
        st["fin_len"][r] = P + len(ids)
        st["fin_score"][r] = score
    bs = _beam_state(st, K)
    ids, score, count = bs.nbest([P, P], pad=0, n=3)
    assert ids.shape == (2, 3, 4) and ids.dtype == torch.int64 and count.tolist() == [3, 1]
    assert ids[0].tolist() == [[11, 2, 0, 0], [12, 13, 14, 2], [2, 0, 0, 0]]
    assert ids[1].tolist() == [[21, 22, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert score[0].tolist() == [-0.5, -0.75, -1.5] and score[1].tolist() == [-0.25, -math.inf, -math.inf]
    best_ids, best_score = bs.best([P, P], pad=0)
    one, s1, c1 = bs.nbest([P, P], pad=0, n=1)
    assert torch.equal(one[:, 0], best_ids) and torch.equal(s1[:, 0], best_score) and c1.tolist() == [1, 1]
    for bad in (0, 5):
        with pytest.raises(ValueError, match="nbest"):
            bs.nbest([P, P], 0, bad)


@pytest.mark.parametrize("K,n", [(4, 3), (4, 4), (2, 2)])
def test_nbest_equals_transformers_num_return_sequences(K, n):
    """sequences and sequences_scores of generate(num_beams=K, num_return_sequences=n) for every utterance whose finished
    set holds at least n entries (HF fills the others with rows this decoder does not return); seeds chosen so that most do"""
    n_new, eos, compared = 12, [2], 0
    for seed in range(4):
        model = _tiny_llama(seed)
        g = torch.Generator().manual_seed(100 + seed)
        P = 5 + seed
        prompts = torch.randint(3, 48, (2, P), generator=g)
        with torch.no_grad():
            out = model.generate(prompts, attention_mask=torch.ones_like(prompts), num_beams=K, num_return_sequences=n,
                                 do_sample=False, max_new_tokens=n_new, eos_token_id=eos[0], pad_token_id=0,
                                 return_dict_in_generate=True, output_scores=True)
        st = _drive(model, prompts, K, n_new, eos)
        ids, score, count = _beam_state(st, K).nbest([P, P], pad=0, n=n)
        for b in range(2):
            if int(count[b]) < n:
                continue
            compared += 1
            for j in range(n):
                want = out.sequences[b * n + j, P:].tolist()
                got = ids[b, j].tolist()
                m = int(st["fin_len"][b * K + j]) - P
                assert got[:m] == want[:m] and all(t == 0 for t in got[m:]), (seed, b, j)
                assert all(t in (0, eos[0]) for t in want[m:]), (seed, b, j)
                assert abs(float(score[b, j]) - float(out.sequences_scores[b * n + j])) < 1e-4, (seed, b, j)
    assert compared >= 4, compared


# ------------------------------------------------------------------------------------------------ records, --jsonl, --oracle
def _scores(B=2, N=4, k=2):
    from touchnet_amd.generation import TokenScores
    g = torch.Generator().manual_seed(3)
    ts = TokenScores.buffers(B, N, k, "cpu")
    ts.logp = -torch.rand(B, N, generator=g)
    ts.entropy = torch.rand(B, N, generator=g)
    ts.alt_id = torch.randint(0, 50, (B, N, k), generator=g, dtype=torch.int32)
    ts.alt_logp = -torch.rand(B, N, k, generator=g)
    return ts


def test_token_scores_close_blanks_the_tail_and_sets_the_confidence():
    from touchnet_amd.generation import _generated_lengths
    ts = _scores()
    logp = ts.logp.clone()
    ids = torch.tensor([[7, 2, 0, 0], [7, 8, 9, 10]])
    n = _generated_lengths(ids, [2])
    assert n.tolist() == [2, 4]
    ts.close(n)
    assert ts.logp[0, 2:].tolist() == [0, 0] and ts.entropy[0, 2:].tolist() == [0, 0]
    assert (ts.alt_id[0, 2:] == -1).all() and (ts.alt_logp[0, 2:] == 0).all() and torch.equal(ts.logp[1], logp[1])
    assert torch.allclose(ts.confidence, torch.stack([logp[0, :2].mean().exp(), logp[1].mean().exp()]))


def test_record_fields_and_lines():
    from touchnet_amd.bin.infer_asr import record_line
    from touchnet_amd.generation import GenerationConfig, record_fields, score_fields
    item = {"key": "utt1", "wav": "a.wav", "txt": "你 好"}
    # no knob: the line this command has always written, byte for byte
    plain = json.dumps({"label": json.dumps(item, ensure_ascii=False), "predict_ids": [7, 8]}, ensure_ascii=False) + "\n"
    out = torch.tensor([[7, 8, 2, 0]])
    ids, extras = record_fields(out, GenerationConfig(), [2])
    assert ids == [[7, 8]] and extras == [{}] and record_line(item, ids[0], extras[0]) == plain
    # scores of a greedy run
    ts = _scores(1, 4, 2).close(torch.tensor([3]))
    ts.alt_id[0, 1, 1] = -1
    cfg = GenerationConfig(top_alternatives=2)
    ids, extras = record_fields((out, ts), cfg, [2])
    e = extras[0]
    assert ids == [[7, 8]] and list(e) == ["confidence", "token_logprobs", "token_entropy", "alternatives"]
    assert len(e["token_logprobs"]) == len(e["token_entropy"]) == len(e["alternatives"]) == 3      # 7, 8 and the eos
    assert len(e["alternatives"][0]) == 2 and len(e["alternatives"][1]) == 1
    assert abs(e["confidence"] - math.exp(sum(e["token_logprobs"]) / 3)) < 1e-6
    assert score_fields(ts, 0, keep=[0, 2])["token_logprobs"] == [e["token_logprobs"][0], e["token_logprobs"][2]]
    json.loads(record_line(item, ids[0], e))
    # an N-best list of a beam search, the second utterance one hypothesis short
    cfg = GenerationConfig(num_beams=4, nbest=2, output_scores=True)
    ids3 = torch.tensor([[[7, 8, 2], [7, 2, 0]], [[9, 2, 0], [0, 0, 0]]])
    hyp_score = torch.tensor([[-0.5, -0.75], [-0.25, -math.inf]])
    ts = _scores(4, 3, 0).close(torch.tensor([3, 2, 2, 0]))
    ids, extras = record_fields((ids3, hyp_score, torch.tensor([2, 1]), ts), cfg, [2])
    assert ids == [[7, 8], [9]]
    assert [h["predict_ids"] for h in extras[0]["nbest"]] == [[7, 8], [7]] and len(extras[1]["nbest"]) == 1
    assert extras[0]["nbest"][0]["predict_ids"] == ids[0] and extras[0]["nbest"][0]["score"] == -0.5
    assert extras[0]["nbest"][0]["confidence"] == extras[0]["confidence"]
    assert extras[1]["nbest"][0]["confidence"] == pytest.approx(float(ts.confidence[2]))

    class Tok:
        def decode(self, row, **kw):
            return " ".join(f"w{t}" for t in row)
    rec = json.loads(record_line(item, ids[0], extras[0], Tok()))
    assert rec["predict"] == "w7 w8" and [h["predict"] for h in rec["nbest"]] == ["w7 w8", "w7"]
    assert list(rec["nbest"][0]) == ["predict_ids", "predict", "score", "confidence"]


def _write_jsonl(path, with_nbest):
    recs = []
    for key, txt, hyps in (("u1", "a b c", ["a b c", "a b", "a c"]), ("u2", "d e", ["d f", "d e"]), ("u3", "g", ["g"])):
        rec = {"label": json.dumps({"key": key, "txt": txt}), "predict": hyps[0]}
        if with_nbest:
            rec["nbest"] = [{"predict_ids": [1], "predict": h, "score": -1.0 * j} for j, h in enumerate(hyps)]
        recs.append(json.dumps(rec, ensure_ascii=False))
    path.write_text("\n".join(recs) + "\n", encoding="utf-8")


def test_jsonl_extraction_writes_one_file_per_rank_and_leaves_the_usual_two_alone(tmp_path):
    from touchnet_amd.metrics import error_rate as E
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _write_jsonl(a / "final.jsonl", False)
    _write_jsonl(b / "final.jsonl", True)
    E.extract_trans_and_pred(str(a / "final.jsonl"))
    E.extract_trans_and_pred(str(b / "final.jsonl"))
    assert sorted(os.listdir(a)) == ["final.jsonl", "raw_rec.txt", "trans.txt"]
    assert sorted(os.listdir(b)) == ["final.jsonl", "raw_rec.2.txt", "raw_rec.3.txt", "raw_rec.txt", "trans.txt"]
    for name in ("raw_rec.txt", "trans.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes()
    assert (b / "raw_rec.txt").read_text() == "u1 a b c\nu2 d f\nu3 g\n"
    assert (b / "raw_rec.2.txt").read_text() == "u1 a b\nu2 d e\n"
    assert (b / "raw_rec.3.txt").read_text() == "u1 a c\n"
    assert E.nbest_rec_path(str(b / "final.jsonl"), 2) == str(b / "raw_rec.2.txt")


def test_oracle_picks_the_fewest_errors_per_utterance_with_ties_to_the_earlier_file(tmp_path, capsys):
    from touchnet_amd.metrics import error_rate as E
    _write_jsonl(tmp_path / "final.jsonl", True)
    E.extract_trans_and_pred(str(tmp_path / "final.jsonl"))
    ref = E.load_utterances(str(tmp_path / "trans.txt"))
    sets = [E.load_utterances(str(tmp_path / n)) for n in ("raw_rec.txt", "raw_rec.2.txt", "raw_rec.3.txt")]
    plain = E.evaluate(ref, sets[0], "whitespace", align_fn=align_ref.align_fn)
    best = E.evaluate_oracle(ref, sets, "whitespace", align_fn=align_ref.align_fn)
    assert (plain.S, plain.I, plain.D, plain.num_utts_with_error) == (1, 0, 0, 1)
    assert (best.C, best.S, best.I, best.D, best.num_utts_with_error, best.num_eval_utts) == (6, 0, 0, 0, 0, 3)
    # ties go to the earlier file: two hypotheses with one error each, the first one's alignment is the one printed
    tie = E.evaluate_oracle({"u": E.Utterance("u", "a b")}, [{"u": E.Utterance("u", "a")}, {"u": E.Utterance("u", "b")},
                                                             {"v": E.Utterance("v", "a b")}], "whitespace", align_ref.align_fn)
    assert (tie.C, tie.D) == (1, 1) and "  HYP  : a * " in tie.details
    # plain-Python scorer of the restatement, per utterance
    for uid, want in (("u1", 0), ("u2", 0), ("u3", 0)):
        errs = [-align_ref.align(ref[uid].text.split(), s[uid].text.split())[2] for s in sets if uid in s]
        assert min(errs) == want
    # the command line: the unchanged normal output first, then the two prefixed blocks
    real, E.device_align = E.device_align, align_ref.align_fn
    try:
        argv = ["--ref", str(tmp_path / "trans.txt"), "--hyp", str(tmp_path / "raw_rec.txt")]
        assert E.main(argv + [str(tmp_path / "D1.txt")]) == 0
        usual = capsys.readouterr().out
        assert E.main(argv + ["--oracle", str(tmp_path / "raw_rec.2.txt"), str(tmp_path / "raw_rec.3.txt"), "--",
                              str(tmp_path / "D2.txt")]) == 0
        both = capsys.readouterr().out
    finally:
        E.device_align = real
    assert both.startswith(usual) and (tmp_path / "D1.txt").read_bytes() == (tmp_path / "D2.txt").read_bytes()
    tail = both[len(usual):].splitlines()
    assert tail[0] == "oracle: " + best.to_json() and tail[1].startswith("oracle: %WER 0.00 [ 0 / 6")
    assert tail[2].startswith("oracle: %SER 0.00 [ 0 / 3 ]")
