"""tn_token_scores on the device against the float64 restatement of tests/token_scores_reference.py, within that module's
derived budget (asserted to stay under 1e-4 for logp and 1e-3 for entropy on these inputs), alternative ids exactly; both
modes, bf16 and fp32, every row type; then the wiring of the scores into the decoders on tiny models."""
import json
import math

import pytest
import torch

import token_scores_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL_V = (1, 2, 63, 64, 65, 127, 1000, 1025, 4097)
LARGE_V = (128256, 152064, 262144)
KS = (0, 1, 5, 8)
KINDS = ("random", "equal", "dominant", "ties", "neg_inf")
DTYPES = (torch.bfloat16, torch.float32)
WORST = {}                                    # output -> worst fraction of its budget seen in this session (printed)


def _tok(Rn, V, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (Rn,), generator=g, dtype=torch.int32)
    t[0] = 0 if seed % 2 else V - 1
    t[-1] = V - 1 if seed % 2 else 0
    return t


def _check(got, ref, k, what):
    logp, ent, alt_id, alt_logp = got
    assert R.budget_ok(ref), (what, float(ref["budget_logp"].max()), float(ref["budget_entropy"].max()))
    for name, g, want, b in (("logp", logp, ref["logp"], ref["budget_logp"]),
                             ("entropy", ent, ref["entropy"], ref["budget_entropy"]),
                             ("alt_logp", alt_logp, ref["alt_logp"][:, :k], ref["budget_alt"][:, :k])):
        ok, frac = R.close(g, want, b)
        WORST[name] = max(WORST.get(name, 0.0), frac)
        assert ok, (what, name, frac)
    assert alt_id.dtype == torch.int32 and torch.equal(alt_id.cpu().to(torch.int64), ref["alt_id"][:, :k]), (what, "alt_id")


def _run_shapes(F, dtype, V, Rs, ks):
    for seed, kind in enumerate(KINDS):
        for Rn in Rs:
            logits = R.make_rows(kind, Rn, V, dtype, seed)
            tok = _tok(Rn, V, seed + Rn)
            ref = R.scores(logits, tok, R.MAX_ALT)
            if kind == "equal":
                assert ref["alt_id"][0].tolist() == list(range(min(V, 8))) + [-1] * (8 - min(V, 8))
            ld, td = logits.to(DEV), tok.to(DEV)
            for k in ks:
                _check(F.token_scores(ld, td, k), ref, k, (kind, Rn, V, k, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", SMALL_V)
def test_token_mode_equals_the_reference_at_small_vocabularies(dtype, V):
    import touchnet_amd.functional as F
    _run_shapes(F, dtype, V, (1, 3, 13), KS)                      # (k > V at V = 1, 2)
    print("worst fraction of the budget so far:", WORST)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", LARGE_V)
def test_token_mode_equals_the_reference_at_real_vocabularies(dtype, V):
    import touchnet_amd.functional as F
    _run_shapes(F, dtype, V, (3,), KS)
    print("worst fraction of the budget so far:", WORST)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_token_out_of_range_scores_nan_and_the_rest_of_the_row_stands(dtype):
    import touchnet_amd.functional as F
    V = 1025
    logits = R.make_rows("random", 6, V, dtype, 3)
    tok = torch.tensor([0, V - 1, -1, V, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    ref = R.scores(logits, tok, 5)
    assert torch.isnan(ref["logp"][2:]).all() and not torch.isnan(ref["logp"][:2]).any()
    assert not torch.isnan(ref["entropy"]).any()
    _check(F.token_scores(logits.to(DEV), tok.to(DEV), 5), ref, 5, "out of range")


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", (65, 4097))
def test_sick_rows_are_nan_and_their_neighbours_stay_correct(dtype, V):
    import touchnet_amd.functional as F
    logits = R.make_rows("random", 7, V, dtype, 5)
    logits[1] = -math.inf
    logits[3, V - 1] = math.nan
    logits[5, 0] = math.inf
    tok = _tok(7, V, 11)
    ref = R.scores(logits, tok, 8)
    for r in (1, 3, 5):
        assert math.isnan(ref["logp"][r]) and math.isnan(ref["entropy"][r]) and ref["alt_id"][r].tolist() == [-1] * 8
    for k in (0, 8):
        got = F.token_scores(logits.to(DEV), tok.to(DEV), k)
        _check(got, ref, k, ("sick", V, k))
        assert torch.isnan(got[3][[1, 3, 5]]).all()


def _buffers(Rn, S, k, poison=-7.0):
    from touchnet_amd.generation import TokenScores
    b = TokenScores.buffers(Rn, S, k, DEV)
    b.logp.fill_(poison)
    b.entropy.fill_(poison)
    if k:
        b.alt_id.fill_(-77)
        b.alt_logp.fill_(poison)
    return b


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("k", (0, 5))
def test_history_mode_writes_the_newest_tokens_column_and_nothing_else(dtype, k):
    import touchnet_amd.functional as F
    V, S = 1025, 6
    lens = torch.tensor([0, 1, S, S + 1, 3, -2, 2], dtype=torch.int32)
    Rn = lens.numel()
    logits = R.make_rows("random", Rn, V, dtype, 9)
    hist = torch.randint(0, V, (Rn, S), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    hist[6, 1] = V + 5                                            # an id outside the vocabulary in the newest slot
    tok = torch.tensor([int(hist[r, n - 1]) if 1 <= n <= S else 0 for r, n in enumerate(lens.tolist())], dtype=torch.int32)
    ref = R.scores(logits, tok, 8)
    out = _buffers(Rn, S, k)
    F.token_scores_(logits.to(DEV), hist.to(DEV), lens.to(DEV), out, k)
    written = torch.zeros(Rn, S, dtype=torch.bool)
    rows = [r for r, n in enumerate(lens.tolist()) if 1 <= n <= S]
    assert rows == [1, 2, 4, 6]
    cols = [int(lens[r]) - 1 for r in rows]
    written[rows, cols] = True
    assert (out.logp.cpu()[~written] == -7.0).all() and (out.entropy.cpu()[~written] == -7.0).all()
    if k:
        assert (out.alt_id.cpu()[~written] == -77).all() and (out.alt_logp.cpu()[~written] == -7.0).all()
    sub = {key: v[rows] for key, v in ref.items()}
    got = (out.logp[rows, cols], out.entropy[rows, cols],
           out.alt_id[rows, cols] if k else torch.empty(len(rows), 0, dtype=torch.int32),
           out.alt_logp[rows, cols] if k else torch.empty(len(rows), 0))
    _check(got, sub, k, ("history", k))
    assert math.isnan(float(out.logp[6, 1]))


def _bits(ts):
    return [t.cpu().contiguous().view(torch.int32) for t in ts]


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("V", (1025, 4097, 128256))
def test_repeats_are_bit_identical_and_a_row_scores_the_same_alone_and_in_a_batch(dtype, V):
    """odd V: the rows of a batch sit at every 2-byte (bf16) / 4-byte (fp32) phase of a 16-byte line, the lone copy at 0"""
    import touchnet_amd.functional as F
    Rn = 13 if V < 10000 else 3
    logits = R.make_rows("random", Rn, V, dtype, 21).to(DEV)
    tok = _tok(Rn, V, 4).to(DEV)
    first = _bits(F.token_scores(logits, tok, 8))
    again = _bits(F.token_scores(logits, tok, 8))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for r in range(Rn):
        alone = _bits(F.token_scores(logits[r:r + 1].clone(), tok[r:r + 1].clone(), 8))
        assert all(torch.equal(a[r:r + 1], b) for a, b in zip(first, alone)), r


def test_opcheck_on_both_ops():
    from torch.library import opcheck
    logits = R.make_rows("random", 5, 257, torch.bfloat16, 2).to(DEV)
    tok = _tok(5, 257, 1).to(DEV)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic")
    opcheck(torch.ops.mi355_touch.token_scores.default, (logits, tok, 3), test_utils=tests)
    opcheck(torch.ops.mi355_touch.token_scores.default, (logits.float(), tok, 0), test_utils=tests)
    hist = torch.randint(0, 257, (5, 4), dtype=torch.int32, device=DEV)
    lens = torch.tensor([1, 2, 3, 4, 0], dtype=torch.int32, device=DEV)
    b = _buffers(5, 4, 3)
    opcheck(torch.ops.mi355_touch.token_scores_.default, (logits, hist, lens, b.logp, b.entropy, b.alt_id, b.alt_logp, 3),
            test_utils=tests)
    opcheck(torch.ops.mi355_touch.token_scores_.default, (logits, hist, lens, b.logp, b.entropy, None, None, 0),
            test_utils=tests)


# ======================================================================================================= the decoders
def _tiny_touch_audio(kind, seed, F_in=80):
    """the tiny TouchAudio Llama / Qwen2 of tests/test_generation_gpu.py"""
    from touchnet_amd.models.llama import DecoderConfig
    from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
    if kind == "llama":
        text = dict(model_type="llama", hidden_size=256, intermediate_size=512, num_attention_heads=8, num_key_value_heads=2,
                    head_dim=64, num_hidden_layers=2, vocab_size=512, rope_theta=500000.0, tie_word_embeddings=True,
                    rms_norm_eps=1e-5)
    else:
        text = dict(model_type="qwen2", hidden_size=512, intermediate_size=768, num_attention_heads=4, num_key_value_heads=1,
                    head_dim=128, num_hidden_layers=2, vocab_size=640, rope_theta=1000000.0, tie_word_embeddings=False,
                    rms_norm_eps=1e-6)
    text.update(initializer_range=0.08, pad_token_id=1, bos_token_id=2, eos_token_id=3)
    cfg = TouchAudioConfig(text_config=DecoderConfig.from_dict(text), input_size=F_in, pad_token_id=1)
    torch.manual_seed(seed)
    m = TouchAudioForCausalLM(cfg)
    m.post_init()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_(0, 0.1)
    return m.to(DEV).to(torch.bfloat16).eval()


def _touch_prompts(seed=5, lens=(23, 1, 57, 8)):
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts
    g = torch.Generator().manual_seed(seed)
    return build_prompts([torch.randn(n, 80, generator=g).bfloat16() for n in lens], 1, 2)


@pytest.fixture(scope="module")
def llama():
    return _tiny_touch_audio("llama", 11)


@pytest.fixture(scope="module")
def qwen2():
    return _tiny_touch_audio("qwen2", 12)


DL_CAP = 0.25                                 # sanity ceiling of max |logits cached - logits packed| on the tiny models


class _Spy:
    """records what functional.token_scores_ / token_scores were handed (copies taken at the call) and what the decoder's
    two logits producers returned (the tensors themselves and copies taken when they were produced)"""

    def __init__(self, monkeypatch, producers=True):
        import touchnet_amd.functional as F
        from touchnet_amd import generation as G
        self.hist_calls, self.tok_calls, self.produced = [], [], []
        real_hist, real_tok, real_prefill, real_decode = F.token_scores_, F.token_scores, G._prefill, G.decode_logits

        def hist_mode(logits, hist, hist_len, out, k=0):
            self.hist_calls.append(dict(logits=logits, copy=logits.clone(), hist=hist.clone(), hist_len=hist_len.clone(), k=k,
                                        before=out.logp.clone()))
            real_hist(logits, hist, hist_len, out, k)
            self.hist_calls[-1]["after"] = out.logp.clone()

        def tok_mode(logits, tok, k=0):
            self.tok_calls.append(dict(copy=logits.clone(), tok=tok.clone(), k=k))
            return real_tok(logits, tok, k)

        def prefill(*a, **kw):
            x = real_prefill(*a, **kw)
            self.produced.append((x, x.clone()))
            return x

        def decode(*a, **kw):
            x = real_decode(*a, **kw)
            self.produced.append((x, x.clone()))
            return x
        monkeypatch.setattr(F, "token_scores_", hist_mode)
        monkeypatch.setattr(F, "token_scores", tok_mode)
        if producers:
            monkeypatch.setattr(G, "_prefill", prefill)
            monkeypatch.setattr(G, "decode_logits", decode)

    def reset(self):
        del self.hist_calls[:], self.tok_calls[:], self.produced[:]


def _check_in_loop(spy, ids, scores, prompt_lens, eos, k):
    """every step's launch saw lm_head's own rows and wrote the appended token's column; the result equals the reference"""
    ids = ids.cpu()
    B, N = ids.shape
    assert len(spy.hist_calls) >= N and len(spy.produced) == len(spy.hist_calls)
    done = [False] * B
    for s in range(N):
        call, (made, made_copy) = spy.hist_calls[s], spy.produced[s]
        assert call["logits"] is made and torch.equal(call["copy"], made_copy), s      # raw: the tensor and its values
        assert call["k"] == k
        hl = call["hist_len"].cpu()
        assert hl.tolist() == [p + s + 1 for p in prompt_lens], s                    # the step kernel ran first
        newest = call["hist"].cpu().gather(1, (hl.to(torch.int64) - 1)[:, None])[:, 0]
        changed = (call["before"] != call["after"]).cpu()
        for b in range(B):
            if not done[b]:
                assert int(newest[b]) == int(ids[b, s]), (s, b)
            cols = changed[b].nonzero().reshape(-1).tolist()
            assert cols in ([], [int(hl[b]) - 1]), (s, b, cols)                        # (an unchanged value: the poison 0)
        ref = R.scores(call["copy"].cpu(), newest, k)
        assert R.budget_ok(ref)
        for b in range(B):
            if done[b]:
                assert float(scores.logp[b, s]) == 0.0 and float(scores.entropy[b, s]) == 0.0
                assert k == 0 or (scores.alt_id[b, s] == -1).all()
                continue
            for name, got, want, bud in (("logp", scores.logp[b, s], ref["logp"][b], ref["budget_logp"][b]),
                                         ("entropy", scores.entropy[b, s], ref["entropy"][b], ref["budget_entropy"][b])):
                assert abs(float(got) - float(want)) <= float(bud), (name, s, b)
            if k:
                assert scores.alt_id[b, s].cpu().tolist() == ref["alt_id"][b].tolist(), (s, b)
                ok, _ = R.close(scores.alt_logp[b, s], ref["alt_logp"][b], ref["budget_alt"][b])
                assert ok, (s, b)
            done[b] = int(ids[b, s]) in eos
    n_tok = torch.tensor([next((i + 1 for i, t in enumerate(r) if t in eos), N) for r in ids.tolist()])
    want = torch.stack([scores.logp[b, :n_tok[b]].double().mean().exp() for b in range(B)]).cpu()
    assert torch.allclose(scores.confidence.cpu().double(), want, rtol=1e-5, atol=0)


def test_greedy_scores_come_from_the_raw_logits_also_under_a_hotword_plan(llama, monkeypatch):
    from touchnet_amd.generation import GenerationConfig, TokenScores, generate
    prompts = _touch_prompts()
    lens = [int(t.numel()) for t in prompts.input_ids]
    base = dict(max_new_tokens=12, eos_token_id=3, pad_token_id=1, check_every=4, cache_chunk=4)   # (the buffers grow twice)
    plain = generate(llama, prompts, GenerationConfig(**base))
    spy = _Spy(monkeypatch)
    ids, scores = generate(llama, prompts, GenerationConfig(top_alternatives=3, **base))
    assert isinstance(scores, TokenScores) and torch.equal(ids, plain) and scores.logp.shape == ids.shape
    assert scores.alt_id.shape == (*ids.shape, 3)
    _check_in_loop(spy, ids, scores, lens, [3], 3)
    # a bias large enough to change what row 0 says first: the scores are still those of lm_head's logits
    first = int(plain[0, 0])
    other = int(scores.alt_id[0, 0, 1]) if int(scores.alt_id[0, 0, 0]) == first else int(scores.alt_id[0, 0, 0])
    spy = _Spy(monkeypatch)
    ids_b, scores_b = generate(llama, prompts, GenerationConfig(sequence_bias={(other,): 30.0}, **base), return_scores=True)
    assert int(ids_b[0, 0]) == other != first
    _check_in_loop(spy, ids_b, scores_b, lens, [3], 0)
    assert abs(float(scores_b.logp[0, 0]) - float(scores.alt_logp[0, 0].cpu()[scores.alt_id[0, 0].cpu() == other][0])) < 1e-6


def test_sampling_scores_come_from_the_raw_logits(qwen2, monkeypatch):
    from touchnet_amd.generation import GenerationConfig, generate
    prompts = _touch_prompts(7, (9, 30, 2))
    lens = [int(t.numel()) for t in prompts.input_ids]
    kw = dict(max_new_tokens=10, eos_token_id=[3, 4], pad_token_id=1, do_sample=True, temperature=0.7, top_k=20, top_p=0.9,
              seed=5, repetition_penalty=1.1, no_repeat_ngram_size=0, check_every=3)
    plain = generate(qwen2, prompts, GenerationConfig(**kw))
    spy = _Spy(monkeypatch)
    ids, scores = generate(qwen2, prompts, GenerationConfig(output_scores=True, top_alternatives=8, **kw))
    assert torch.equal(ids, plain)
    _check_in_loop(spy, ids, scores, lens, [3, 4], 8)


def _tiny_kimi(seed=0):
    """the tiny Kimi-Audio of tests/test_kimi_generation_gpu.py (the audio-input side unused here)"""
    from touchnet_amd.models.kimi_audio import KimiAudioConfig, KimiAudioPackedForCausalLM
    kw = dict(vocab_size=1024, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
              num_key_value_heads=1, head_dim=64, kimia_mimo_layers=1, kimia_mimo_transformer_from_layer_index=0,
              kimia_token_offset=512, kimia_media_begin=5, kimia_media_end=6, initializer_range=0.1)
    torch.manual_seed(seed)
    m = KimiAudioPackedForCausalLM(KimiAudioConfig(**kw))
    m.post_init()
    return m.to(DEV).to(torch.bfloat16).eval()


def _kimi_prompts():
    from touchnet_amd.models.kimi_audio.inference_kimi_audio import KimiPrompts
    g = torch.Generator().manual_seed(2)
    text, audio = [], []
    for n in (20, 9, 14):
        a = [7, 7, 7, 5] + [7] * n + [6, 9, 10, 11]
        audio.append(torch.tensor(a))
        text.append(torch.cat([torch.randint(12, 500, (3,), generator=g), torch.full((len(a) - 3,), 7)]))
    return KimiPrompts(text_ids=text, audio_ids=audio)


def test_kimi_scores_come_from_the_raw_logits(monkeypatch):
    from touchnet_amd.generation import KimiGenerationConfig
    from touchnet_amd.models.kimi_audio import inference_kimi_audio as KI
    m, prompts = _tiny_kimi(), _kimi_prompts()
    lens = [int(t.numel()) for t in prompts.text_ids]
    kw = dict(text_repetition_window_size=4, max_new_tokens=10, kimia_text_blank=7, kimia_text_eos=8, check_every=4,
              cache_chunk=4)
    spy = _Spy(monkeypatch)
    plain = KI.generate_kimi(m, prompts, KimiGenerationConfig(**kw), return_raw=True)
    assert len(plain) == 3 and spy.hist_calls == [] and spy.tok_calls == [] and len(spy.produced) == plain[1].shape[1]
    spy.reset()
    out, raw, _, scores = KI.generate_kimi(m, prompts, KimiGenerationConfig(top_alternatives=2, **kw), return_raw=True)
    assert out == plain[0] and torch.equal(raw, plain[1])
    _check_in_loop(spy, raw, scores, lens, [8], 2)
    out2, scores2 = KI.generate_kimi(m, prompts, KimiGenerationConfig(output_scores=True, **kw))
    assert out2 == out and torch.equal(scores2.logp, scores.logp) and scores2.alt_id.shape[-1] == 0


def test_no_knob_no_launch_no_copy_same_return_values(llama, monkeypatch):
    from touchnet_amd.generation import GenerationConfig, generate
    prompts = _touch_prompts()
    spy = _Spy(monkeypatch, producers=False)                  # (its producer hooks copy the logits themselves)
    clones = []
    real_clone = torch.Tensor.clone
    base = dict(max_new_tokens=6, eos_token_id=3, pad_token_id=1)
    for cfg in (GenerationConfig(**base), GenerationConfig(sequence_bias={(9,): 4.0}, **base),
                GenerationConfig(do_sample=True, no_repeat_ngram_size=0, **base), GenerationConfig(num_beams=4, **base)):
        del clones[:]
        monkeypatch.setattr(torch.Tensor, "clone", lambda t, *a, **kw: (clones.append(tuple(t.shape)), real_clone(t, *a, **kw))[1])
        out = generate(llama, prompts, cfg)
        monkeypatch.setattr(torch.Tensor, "clone", real_clone)
        assert isinstance(out, torch.Tensor) and out.dtype == torch.int64 and out.dim() == 2
        V = 512
        assert not any(shape[-1:] == (V,) for shape in clones if len(shape) == 2), clones    # no logits copy
    assert spy.hist_calls == [] and spy.tok_calls == []
    # (the hook sees such a copy when there is one: a plan with scores makes one per step, and the spy another)
    del clones[:]
    monkeypatch.setattr(torch.Tensor, "clone", lambda t, *a, **kw: (clones.append(tuple(t.shape)), real_clone(t, *a, **kw))[1])
    generate(llama, prompts, GenerationConfig(sequence_bias={(9,): 4.0}, output_scores=True, **base))
    monkeypatch.setattr(torch.Tensor, "clone", real_clone)
    assert sum(shape == (len(prompts), V) for shape in clones) == 2 * len(spy.hist_calls) > 0


def _plain_docs(seed, P=(6, 11, 3, 9), C=(5, 1, 0, 7), V=512):
    g = torch.Generator().manual_seed(seed)
    prompts = [torch.randint(4, V, (p,), generator=g) for p in P]
    conts = [torch.randint(4, V, (c,), generator=g) for c in C]
    return prompts, conts


@pytest.mark.parametrize("rows_per_chunk", [4096, 5, 1])
def test_score_continuations_equals_the_reference_on_a_packed_forward(llama, monkeypatch, rows_per_chunk):
    from touchnet_amd.generation import Prompts, score_continuations
    lm = llama.language_model
    prompts, conts = _plain_docs(3)
    spy = _Spy(monkeypatch)
    k = 4
    ts = score_continuations(lm, Prompts(input_ids=prompts), conts, k=k, rows_per_chunk=rows_per_chunk)
    n_rows = sum(c.numel() for c in conts)
    assert [c["copy"].shape[0] for c in spy.tok_calls] == [min(rows_per_chunk, n_rows - a) for a in
                                                           range(0, n_rows, rows_per_chunk)]
    logits = torch.cat([c["copy"] for c in spy.tok_calls]).cpu()
    toks = torch.cat([c["tok"] for c in spy.tok_calls]).cpu()
    assert toks.tolist() == torch.cat(conts).tolist()
    # the packed forward of the test: every document prompt + continuation, all rows through lm_head
    lens = [p.numel() + c.numel() for p, c in zip(prompts, conts)]
    T = sum(lens)
    Tp = (T + 255) // 256 * 256
    ids, pos, doc = (torch.zeros(Tp, dtype=torch.int64) for _ in range(3))
    rows, o = [], 0
    for b, (p, c) in enumerate(zip(prompts, conts)):
        ids[o:o + lens[b]] = torch.cat([p, c])
        pos[o:o + lens[b]] = torch.arange(lens[b])
        doc[o:o + lens[b]] = b + 1
        rows += [o + p.numel() - 1 + j for j in range(c.numel())]
        o += lens[b]
    with torch.no_grad():
        full = lm(input_ids=ids[None].to(DEV), position_ids=pos[None].to(DEV),
                  attention_mask=doc[None].to(torch.int32).to(DEV)).logits[0].float().cpu()[rows]
    assert float((logits.float() - full).abs().max()) <= 3e-2 * float(full.abs().max())       # the same forward, in bf16
    ref = R.scores(logits, toks, k)
    assert R.budget_ok(ref)
    N = max(c.numel() for c in conts)
    assert ts.logp.shape == (4, N) and ts.alt_id.shape == (4, N, k)
    o = 0
    for b, c in enumerate(conts):
        n = c.numel()
        sub = {key: v[o:o + n] for key, v in ref.items()}
        for name, got, want, bud in (("logp", ts.logp[b, :n], sub["logp"], sub["budget_logp"]),
                                     ("entropy", ts.entropy[b, :n], sub["entropy"], sub["budget_entropy"]),
                                     ("alt_logp", ts.alt_logp[b, :n], sub["alt_logp"], sub["budget_alt"])):
            assert R.close(got, want, bud)[0], (name, b)
        assert torch.equal(ts.alt_id[b, :n].cpu().to(torch.int64), sub["alt_id"])
        assert (ts.logp[b, n:] == 0).all() and (ts.alt_id[b, n:] == -1).all() and (ts.entropy[b, n:] == 0).all()
        want = math.exp(float(sub["logp"].mean())) if n else 1.0
        assert abs(float(ts.confidence[b]) - want) <= 1e-4 * want
        o += n
    empty = score_continuations(lm, Prompts(input_ids=prompts[:2]), [[], []], k=1)
    assert empty.logp.shape == (2, 0) and empty.confidence.tolist() == [1.0, 1.0]


@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_in_loop_scores_agree_with_rescoring_the_same_ids(kind, llama, qwen2, monkeypatch):
    """|logp_loop - logp_rescored| <= 2 max|logits_loop - logits_rescored| + both budgets: a log_softmax moves by at most
    twice the largest logit change (once through l_t, once through the normaliser)"""
    from touchnet_amd.generation import GenerationConfig, score_continuations, trim_at_eos
    model = llama if kind == "llama" else qwen2
    prompts = _touch_prompts()
    spy = _Spy(monkeypatch)
    from touchnet_amd.generation import generate
    ids, loop = generate(model, prompts, GenerationConfig(max_new_tokens=12, eos_token_id=3, pad_token_id=1, output_scores=True))
    n_tok = [len(r) + 1 if len(r) < ids.shape[1] else len(r) for r in trim_at_eos(ids, 3)]
    conts = [ids[b, :n].cpu() for b, n in enumerate(n_tok)]
    again = score_continuations(model, prompts, conts)
    rescored = torch.cat([c["copy"] for c in spy.tok_calls]).cpu()
    worst_dl, o = 0.0, 0
    for b, n in enumerate(n_tok):
        for s in range(n):
            in_loop = spy.hist_calls[s]["copy"][b].cpu()
            dl = float((in_loop.float() - rescored[o + s].float()).abs().max())
            worst_dl = max(worst_dl, dl)
            bud = (R.row_scores(in_loop, int(ids[b, s]), 0)["budget_logp"]
                   + R.row_scores(rescored[o + s], int(ids[b, s]), 0)["budget_logp"])
            assert abs(float(loop.logp[b, s]) - float(again.logp[b, s])) <= 2 * dl + bud, (b, s, dl)
        o += n
    print(f"{kind}: max |logits in the loop - logits of the packed rescoring forward| = {worst_dl:.4g}")
    assert worst_dl < DL_CAP                     # (sanity: the same model on the same tokens, bf16 both ways)


def test_beam_search_nbest_reads_the_finished_set_and_rank_one_is_todays_output(llama, monkeypatch):
    from touchnet_amd.generation import GenerationConfig, generate, score_continuations
    prompts = _touch_prompts()
    lens = [int(t.numel()) for t in prompts.input_ids]
    base = dict(max_new_tokens=10, eos_token_id=3, pad_token_id=1, num_beams=4, repetition_penalty=1.0,
                no_repeat_ngram_size=0)
    today, st0 = generate(llama, prompts, GenerationConfig(**base), return_cache=True)
    ids, score, count, st = generate(llama, prompts, GenerationConfig(nbest=3, **base), return_cache=True)
    B, K = len(lens), 4
    assert ids.shape[:2] == (B, 3) and score.shape == (B, 3) and count.shape == (B,)
    assert torch.equal(st.fin_score, st0.fin_score) and torch.equal(st.fin_ids, st0.fin_ids)     # the search is the same
    assert torch.equal(ids[:, 0, :today.shape[1]], today) and (ids[:, 0, today.shape[1]:] == 1).all()
    fin_score, fin_len, fin_ids = st.fin_score.view(B, K).cpu(), st.fin_len.view(B, K).cpu(), st.fin_ids.view(B, K, -1).cpu()
    assert int(count.min()) >= 1
    for b in range(B):
        assert int(count[b]) == int((fin_score[b, :3] > -1e9).sum())
        for j in range(3):
            if j < int(count[b]):
                n = int(fin_len[b, j]) - lens[b]
                assert float(score[b, j]) == float(fin_score[b, j])
                assert ids[b, j, :n].tolist() == fin_ids[b, j, lens[b]:lens[b] + n].tolist() and (ids[b, j, n:] == 1).all()
            else:
                assert float(score[b, j]) == -math.inf and (ids[b, j] == 1).all()
    # with scores: one teacher-forced forward behind the search, a row per returned hypothesis
    spy = _Spy(monkeypatch)
    ids2, score2, count2, ts = generate(llama, prompts, GenerationConfig(nbest=3, top_alternatives=2, **base))
    assert torch.equal(ids2, ids) and torch.equal(score2, score) and spy.hist_calls == [] and len(spy.tok_calls) == 1
    assert ts.logp.shape[0] == B * 3 and ts.alt_id.shape[-1] == 2
    # ... which is score_continuations over the returned hypotheses, row b * nbest + j, bit for bit
    from touchnet_amd.generation import Prompts
    rep3 = Prompts(input_ids=[t for t in prompts.input_ids for _ in range(3)],
                   input_features=[f for f in prompts.input_features for _ in range(3)])
    conts = [ids[b, j, :int(fin_len[b, j]) - lens[b]].cpu() if j < int(count[b]) else [] for b in range(B) for j in range(3)]
    direct = score_continuations(llama, rep3, conts, k=2)
    for name in ("logp", "entropy", "alt_id", "alt_logp", "confidence"):
        assert torch.equal(getattr(ts, name), getattr(direct, name)), name
    for b in range(B):
        for j in range(int(count[b])):
            n = int(fin_len[b, j]) - lens[b]
            # the hypothesis' score is the sum of PROCESSED log-probabilities over length ** length_penalty; with penalty and
            # n-gram ban off the processing is the identity, so the raw per-token scores add up to it, each within twice the
            # logits' difference between the cached decode and the packed forward (DL_CAP, the rescoring test's ceiling)
            total = float(ts.logp[b * 3 + j, :n].sum()) / n
            assert abs(total - float(score[b, j])) <= 2 * DL_CAP, (b, j, total, float(score[b, j]))


def test_oracle_on_the_device_selects_what_the_plain_python_scorer_selects(tmp_path, capsys):
    import edit_align_reference as A
    from touchnet_amd.metrics import error_rate as E
    g = torch.Generator().manual_seed(0)
    words = [f"w{i}" for i in range(12)]
    ref, h1, h2 = {}, {}, {}
    for u in range(40):
        r = [words[int(i)] for i in torch.randint(0, 12, (int(torch.randint(1, 9, (1,), generator=g)),), generator=g)]
        noisy = lambda: [w for w in r if float(torch.rand(1, generator=g)) > 0.25] + \
            ([words[int(torch.randint(0, 12, (1,), generator=g))]] if float(torch.rand(1, generator=g)) > 0.6 else [])
        ref[f"u{u:02d}"], h1[f"u{u:02d}"] = " ".join(r), " ".join(noisy())
        if u % 5:
            h2[f"u{u:02d}"] = " ".join(noisy())                  # (every fifth key is missing from the second file)
    for name, d in (("ref.txt", ref), ("h1.txt", h1), ("h2.txt", h2)):
        (tmp_path / name).write_text("".join(f"{k} {v}\n" for k, v in d.items()), encoding="utf8")
    want = dict(C=0, S=0, I=0, D=0)
    for u, r in ref.items():
        best = None
        for hyp in (h1, h2):
            if u in hyp:
                _, counts, score = A.align(r.split(), hyp[u].split())
                if best is None or -score < best[0]:
                    best = (-score, counts)
        for key, n in zip("CSID", best[1]):
            want[key] += n
    assert E.main(["--ref", str(tmp_path / "ref.txt"), "--hyp", str(tmp_path / "h1.txt"), "--oracle", str(tmp_path / "h2.txt"),
                   "--", str(tmp_path / "D.txt")]) == 0
    lines = capsys.readouterr().out.splitlines()
    plain = json.loads(lines[0])
    oracle = json.loads(next(l for l in lines if l.startswith("oracle: {"))[len("oracle: "):])
    assert {k: oracle[k] for k in "CSID"} == want and oracle["num_eval_utts"] == 40
    assert oracle["S"] + oracle["I"] + oracle["D"] <= plain["S"] + plain["I"] + plain["D"]
    assert any(l.startswith("oracle: %WER") for l in lines) and any(l.startswith("oracle: %SER") for l in lines)
