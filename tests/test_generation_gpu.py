"""KV-cache greedy decoding on the MI355X: tn_attn_decode against an fp32 reference, tn_greedy_step against transformers'
logits processors, end-to-end transcripts against transformers' Llama / Qwen2 teacher-forced on the CPU, cached decoding
against the packed forward recomputing the prefix at LlamaForASR-1B width, and the infer_asr command line."""
import json
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------- (1) decode attention
def _attn_ref(q, k_cache, v_cache, k_new, v_new, cache_len, scale):
    """fp32 attention of q [B, Nh, D] over cache[b, :len_b] + the new key / value."""
    B, Nh, D = q.shape
    Nkv = k_cache.shape[2]
    out = torch.empty(B, Nh, D, dtype=torch.float32, device=q.device)
    for b in range(B):
        n = int(cache_len[b])
        k = torch.cat([k_cache[b, :n], k_new[b:b + 1]]).float()          # [n + 1, Nkv, D]
        v = torch.cat([v_cache[b, :n], v_new[b:b + 1]]).float()
        k = k.repeat_interleave(Nh // Nkv, dim=1)
        v = v.repeat_interleave(Nh // Nkv, dim=1)
        s = torch.einsum("hd,nhd->hn", q[b].float(), k) * scale
        out[b] = torch.einsum("hn,nhd->hd", torch.softmax(s, dim=-1), v)
    return out


CASES = [  # B, cache lengths, Nh, Nkv, D
    (1, [8191], 32, 8, 64),
    (1, [1], 28, 4, 128),
    (12, [1, 63, 64, 65, 1000, 0, 127, 128, 129, 600, 2, 8191], 28, 4, 128),
    (12, [1, 63, 64, 65, 1000, 0, 127, 128, 129, 600, 2, 8191], 32, 8, 64),
    (12, [63, 64, 65, 1000, 5, 300, 301, 17, 600, 600, 599, 4095], 7, 1, 128),
    (64, None, 8, 8, 64),
    (64, None, 16, 16, 128),
    (3, [64, 1000, 8191], 16, 1, 64),
]


@pytest.mark.parametrize("B,lens,Nh,Nkv,D", CASES)
def test_attn_decode_matches_fp32_reference(B, lens, Nh, Nkv, D):
    import touchnet_amd.functional as F
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + Nh + D)
    if lens is None:
        lens = torch.randint(1, 1200, (B,), generator=g).tolist()
        lens[:6] = [1, 63, 64, 65, 1000, 8191]
    S_max = max(lens) + 3
    guard = 4096
    # the caches are views of a longer buffer: the guard region behind them must stay untouched
    gd = torch.Generator(device=DEV).manual_seed(B + Nh + D)
    kbuf = torch.randn(B * S_max * Nkv * D + guard, generator=gd, device=DEV).to(torch.bfloat16)
    vbuf = torch.randn(B * S_max * Nkv * D + guard, generator=gd, device=DEV).to(torch.bfloat16)
    kc = kbuf[:B * S_max * Nkv * D].view(B, S_max, Nkv, D)
    vc = vbuf[:B * S_max * Nkv * D].view(B, S_max, Nkv, D)
    q = torch.randn(B, Nh, D, generator=g).to(torch.bfloat16).to(DEV)
    kn = torch.randn(B, Nkv, D, generator=g).to(torch.bfloat16).to(DEV)
    vn = torch.randn(B, Nkv, D, generator=g).to(torch.bfloat16).to(DEV)
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    k0, v0 = kbuf.clone(), vbuf.clone()
    scale = D ** -0.5
    with torch.no_grad():
        o = F.attn_decode(q, kn, vn, kc, vc, cl, scale)
        torch.cuda.synchronize()
        ref = _attn_ref(q, kc, vc, kn, vn, lens, scale)
    err = (o.float() - ref).abs()
    bound = 4e-3 + 8e-3 * ref.abs()
    print(f"B={B} Nh={Nh} Nkv={Nkv} D={D}: max |err| {float(err.max()):.2e}, max |ref| {float(ref.abs().max()):.2e}, "
          f"max err / bound {float((err / bound).max()):.2f}")
    assert bool((err <= bound).all())
    assert torch.equal(cl.cpu(), torch.tensor(lens, dtype=torch.int32))                  # not advanced
    # the new slot holds k_new / v_new, every other byte (and the guard) is untouched
    k_exp, v_exp = k0.clone(), v0.clone()
    ke = k_exp[:B * S_max * Nkv * D].view(B, S_max, Nkv, D)
    ve = v_exp[:B * S_max * Nkv * D].view(B, S_max, Nkv, D)
    for b, n in enumerate(lens):
        ke[b, n] = kn[b]
        ve[b, n] = vn[b]
    assert torch.equal(kbuf.view(torch.int16), k_exp.view(torch.int16))
    assert torch.equal(vbuf.view(torch.int16), v_exp.view(torch.int16))
    # a repeated call (same cache state) is bit-identical
    with torch.no_grad():
        o2 = F.attn_decode(q, kn, vn, kc, vc, cl, scale)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16))


def test_attn_decode_poisons_an_overflowed_row_and_leaves_its_cache_alone():
    import touchnet_amd.functional as F
    for B, Nh, Nkv, D in ((2, 32, 8, 64), (1, 16, 1, 128)):       # (one launch; split launch + combine)
        S_max = 700
        g = torch.Generator(device="cpu").manual_seed(7)
        kc = torch.randn(B, S_max, Nkv, D, generator=g).to(torch.bfloat16).to(DEV)
        vc = torch.randn(B, S_max, Nkv, D, generator=g).to(torch.bfloat16).to(DEV)
        q = torch.randn(B, Nh, D, generator=g).to(torch.bfloat16).to(DEV)
        kn = torch.randn(B, Nkv, D, generator=g).to(torch.bfloat16).to(DEV)
        lens = [S_max] + [100] * (B - 1)
        cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        k0 = kc.clone()
        with torch.no_grad():
            o = F.attn_decode(q, kn, kn, kc, vc, cl)
        torch.cuda.synchronize()
        assert torch.isnan(o[0].float()).all()
        assert torch.equal(kc[0].view(torch.int16), k0[0].view(torch.int16))
        if B > 1:
            assert torch.isfinite(o[1:].float()).all()


# ---------------------------------------------------------------------------------------------------- (2) greedy step
def _hf_step(scores_f32, hist_row, penalty, ngram):
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    ids = torch.tensor([hist_row], dtype=torch.int64)
    s = scores_f32[None].clone()
    s = RepetitionPenaltyLogitsProcessor(penalty)(ids, s)
    s = NoRepeatNGramLogitsProcessor(ngram)(ids, s)
    return int(torch.argmax(s, dim=-1))


def test_greedy_step_matches_transformers_processors():
    import touchnet_amd.functional as F
    V, S_hist, pen, ngram, eos, pad = 128256, 64, 1.5, 2, 128001, 128004
    g = torch.Generator(device="cpu").manual_seed(3)
    hists = [
        [pad] * 9 + [128000],                       # prompt only
        [pad] * 3 + [128000, 17, 17, 17],           # repeats
        [pad] * 2 + [128000, 5, 9, 5],              # bigram (5, 9) exists: 9 banned after 5
        [pad] * 4 + [128000, 300, 301, 302, 300],   # ban 301
        [1, 2, 3, 1],                               # ban 2
        [pad, 128000, 42],                          # ties
        [pad, 128000, 77, 78],                      # negative logits on seen ids
        [pad] * 5 + [128000, 11],                   # finished row: emits pad
        [7],                                        # too short for any bigram
        [pad] * 20 + [128000] + list(range(1000, 1030)) + [1000],   # ban 1001
    ]
    B = len(hists)
    for dtype in (torch.bfloat16, torch.float32):
        logits = torch.randn(B, V, generator=g).to(dtype)
        # craft: the banned continuation is the raw maximum; equal maxima (lowest id wins); negative seen logits
        logits[2, 9] = 30.0
        logits[3, 301] = 30.0
        logits[4, 2] = 30.0
        logits[9, 1001] = 30.0
        logits[5, 500] = 25.0
        logits[5, 200] = 25.0
        logits[5, 42] = 36.0                        # seen: 36 / 1.5 = 24 < 25
        logits[6] = -torch.rand(V, generator=g).to(dtype) - 1.0
        logits[6, 77] = -0.6                        # seen: * 1.5 -> -0.9 ...
        logits[6, 100] = -0.7                       # ... loses against this unseen one
        logits[1, 17] = 40.0                        # the raw maximum, but banned
        hist = torch.zeros(B, S_hist, dtype=torch.int32)
        for b, h in enumerate(hists):
            hist[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
        hl = torch.tensor([len(h) for h in hists], dtype=torch.int32)
        fin = torch.zeros(B, dtype=torch.int32)
        fin[7] = 1
        cl = hl - 1
        expect = []
        for b, h in enumerate(hists):
            expect.append(pad if fin[b] else _hf_step(logits[b].float(), h, pen, ngram))
        assert expect[2] != 9 and expect[3] != 301 and expect[4] != 2 and expect[5] == 200 and expect[6] == 100
        assert expect[1] != 17                      # (17, 17) occurred: 17 is banned after 17
        logits[0, eos] = 60.0                       # row 0 emits eos
        expect[0] = _hf_step(logits[0].float(), hists[0], pen, ngram)
        assert expect[0] == eos
        d = {k: v.to(DEV) for k, v in dict(hist=hist, hl=hl, cl=cl, fin=fin).items()}
        nu = torch.tensor([B - 1], dtype=torch.int32, device=DEV)
        F.greedy_step(logits.to(DEV), d["hist"], d["hl"], d["cl"], d["fin"], nu, pen, ngram, eos, pad)
        torch.cuda.synchronize()
        got = [int(d["hist"][b, len(h)]) for b, h in enumerate(hists)]
        print(dtype, "tokens", got)
        assert got == expect
        assert torch.equal(d["hl"].cpu(), hl + 1) and torch.equal(d["cl"].cpu(), cl + 1)
        want = hist.clone()
        for b, h in enumerate(hists):
            want[b, len(h)] = expect[b]
        assert torch.equal(d["hist"].cpu(), want)
        f = d["fin"].cpu()
        assert f[0] == 1 and f[7] == 1 and int(f.sum()) == 2 and int(nu) == B - 2


# ------------------------------------------------------------------------------------- (2b) the argmax rule at its edges
def _planted_rows(V, dtype):
    """Six rows of seeded normal logits with the argmax decided by a tie, a NaN or an infinity.  A thread of the
    1024-thread workgroup owns ids tid, tid + 1024, ...; wave w owns the ids with (id % 1024) // 64 == w."""
    g = torch.Generator(device="cpu").manual_seed(V)
    x = torch.randn(6, V, generator=g)
    big = V > 1024
    a, b = (100, 700) if big else (5, 37)               # equal maxima in waves 1 and 10 (V = 50: one wave, two lanes)
    x[0, a] = x[0, b] = 9.0
    x[1, 3] = float("inf")                              # one NaN at the highest id (a later stride where V > 1024) beats +inf
    x[1, V - 1] = float("nan")
    a, b = (200, 1224) if big else (11, 30)             # two NaNs in one thread's stride (V = 50: in one wave)
    x[2, a] = x[2, b] = float("nan")
    a, b = (70, 1031) if big else (7, 40)               # two NaNs, the lower id in the higher wave (70: wave 1, 1031: wave 0)
    x[3, a] = x[3, b] = float("nan")
    x[4] = float("-inf")                                # nothing to choose: token 0
    a, b = (300, 1100) if big else (20, 45)
    x[5, a] = x[5, b] = float("inf")
    x = x.to(dtype)
    return x, torch.argmax(x.float(), dim=-1).tolist()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [50, 1500, 2051])
def test_step_kernels_share_torch_argmax_at_ties_nan_and_inf(V, dtype):
    """tn_greedy_step, tn_sample_step (do_sample = 0) and tn_kimi_text_step (temperature = 0) on the same planted rows:
    the token is torch.argmax of the fp32 row (the lowest NaN id beats +inf, ties go to the lower id, an all -inf row
    gives 0), and the books advance by exactly that token."""
    import touchnet_amd.functional as F
    logits, expect = _planted_rows(V, dtype)
    big = V > 1024
    assert expect == [100 if big else 5, V - 1, 200 if big else 11, 70 if big else 7, 0, 300 if big else 20]
    B, S_hist, H = 6, 8, 16
    eos = next(i for i in range(V) if i not in expect)              # no row emits it
    g = torch.Generator(device="cpu").manual_seed(V + 1)
    hl = torch.tensor([1, 2, 3, 1, 2, 3], dtype=torch.int32)
    hist = torch.randint(0, V, (B, S_hist), generator=g, dtype=torch.int32)
    embed = torch.randn(V, H, generator=g).to(torch.bfloat16)
    audio_token = 1
    want = hist.clone()
    for b in range(B):
        want[b, hl[b]] = expect[b]
    dl = logits.to(DEV)
    for entry in ("greedy", "sample", "kimi"):
        d = {k: v.to(DEV) for k, v in dict(hist=hist, hl=hl, cl=hl - 1, fin=torch.zeros(B, dtype=torch.int32)).items()}
        nu = torch.tensor([B], dtype=torch.int32, device=DEV)
        state = (dl, d["hist"], d["hl"], d["cl"], d["fin"], nu)
        if entry == "greedy":
            F.greedy_step(*state, penalty=1.0, ngram=0, eos=eos, pad=0)
        elif entry == "sample":
            F.sample_step(*state, penalty=1.0, do_sample=False, eos=[eos], pad=0)
        else:
            x_next = torch.zeros(B, H, dtype=torch.bfloat16, device=DEV)
            F.kimi_text_step(*state, torch.ones(B, dtype=torch.int32, device=DEV), embed.to(DEV), x_next, penalty=1.0,
                             temperature=0.0, eos=eos, blank=0, audio_token=audio_token)
        torch.cuda.synchronize()
        got = [int(d["hist"][b, hl[b]]) for b in range(B)]
        assert got == expect, (entry, got, expect)
        assert torch.equal(d["hist"].cpu(), want), entry
        assert torch.equal(d["hl"].cpu(), hl + 1) and torch.equal(d["cl"].cpu(), hl), entry
        assert int(d["fin"].sum()) == 0 and int(nu) == B, entry
        if entry == "kimi":
            x_want = embed[torch.tensor(expect)] + embed[audio_token]          # one bf16 add
            assert torch.equal(x_next.cpu().view(torch.int16), x_want.view(torch.int16))


# ---------------------------------------------------------------------------------------------------- helpers: tiny models
def _tiny_touch_audio(kind, seed, F_in=80):
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
            p.copy_(p.to(torch.bfloat16).float())          # bf16-representable weights: the CPU oracle sees the same
    return m, text


def _hf_model(m, text):
    import transformers
    kind = text["model_type"]
    keys = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
            "num_key_value_heads", "head_dim", "rope_theta", "rms_norm_eps", "tie_word_embeddings")
    kw = {k: text[k] for k in keys}
    if kind == "llama":
        hf = transformers.LlamaForCausalLM(transformers.LlamaConfig(**kw, attention_bias=False))
    else:
        hf = transformers.Qwen2ForCausalLM(transformers.Qwen2Config(**kw))
    sd = {k: v.float() for k, v in m.language_model.state_dict().items()}
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    hf.config._attn_implementation = "eager"
    return hf.eval()


# ---------------------------------------------------------------------------------------------------- (3) end to end vs HF
@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_transcribe_matches_transformers_teacher_forced(kind):
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    from touchnet_amd.generation import GenerationConfig
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts, transcribe
    m, text = _tiny_touch_audio(kind, seed=11 if kind == "llama" else 12)
    hf = _hf_model(m, text)
    g = torch.Generator().manual_seed(5)
    lens = [23, 1, 57, 8, 40]
    feats = [torch.randn(n, 80, generator=g).bfloat16().float() for n in lens]
    cfg = GenerationConfig(max_new_tokens=40)
    gpu_model = m.to(DEV).to(torch.bfloat16)
    out = transcribe(gpu_model, feats, cfg)
    prompts = build_prompts(feats, 1, 2)
    rep, ngr = RepetitionPenaltyLogitsProcessor(1.5), NoRepeatNGramLogitsProcessor(2)
    proj = m.projector.weight.detach().float().cpu()
    compared = equal = 0
    worst = 0.0
    for b, toks in enumerate(out):
        full = toks + ([3] if len(toks) < cfg.max_new_tokens else [])          # the eos the GPU emitted
        ids = torch.cat([prompts.input_ids[b], torch.tensor(full, dtype=torch.int64)])
        P = prompts.input_ids[b].numel()
        feat = torch.cat([prompts.input_features[b], torch.zeros(len(full), 80)])
        with torch.no_grad():
            emb = hf.model.embed_tokens(ids[None]) + (feat @ proj.t())[None]
            logits = hf(inputs_embeds=emb, position_ids=torch.arange(ids.numel())[None]).logits[0].float()
        for s, tok in enumerate(full):
            sc = logits[P - 1 + s][None].clone()
            hist = ids[None, :P + s]
            sc = ngr(hist, rep(hist, sc))[0]
            best = int(torch.argmax(sc))
            top2 = torch.topk(sc, 2).values
            tol = 0.02 * float(top2[0].abs()) + 0.05
            compared += 1
            if tok == best:
                equal += 1
            else:
                gap = float(sc[best] - sc[tok])
                worst = max(worst, gap)
                assert gap <= tol, (kind, b, s, tok, best, gap, tol)
    print(f"{kind}: {equal}/{compared} steps equal to the CPU argmax; worst near-tie gap {worst:.3g}; "
          f"lengths {[len(t) for t in out]}")
    assert compared >= 20 and equal >= 0.9 * compared


# ---------------------------------------------------------------------------------------------------- (4) cached vs recompute
def test_cached_decoding_matches_the_packed_forward_at_llama_asr_1b_width():
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.llama import DecoderConfig
    from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts
    text = DecoderConfig.from_dict(dict(
        model_type="llama", hidden_size=2048, intermediate_size=8192, num_attention_heads=32, num_key_value_heads=8,
        head_dim=64, num_hidden_layers=2, vocab_size=128256, rope_theta=500000.0, tie_word_embeddings=True,
        rope_scaling={"factor": 32.0, "high_freq_factor": 4.0, "low_freq_factor": 1.0,
                      "original_max_position_embeddings": 8192, "rope_type": "llama3"},
        pad_token_id=128004, bos_token_id=128000, eos_token_id=128001, initializer_range=0.02))
    torch.manual_seed(0)
    with torch.device(DEV):
        m = TouchAudioForCausalLM(TouchAudioConfig(text_config=text, input_size=400))
    m.post_init()
    m = m.to(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(60, 180, (12,), generator=g).tolist()                 # AISHELL: 2-7 s at 4 stacked frames
    feats = [torch.randn(n, 400, generator=g) for n in lens]
    pr = build_prompts(feats, 128004, 128000)
    lm, proj = m.language_model, m.projector.weight
    steps, B = 64, len(lens)
    P = [int(t.numel()) for t in pr.input_ids]
    cache = G.KVCache.allocate(2, B, max(P) + steps, 8, 64, DEV)
    worst_rel, tok_cmp, tok_eq = 0.0, 0, 0
    with torch.no_grad():
        logits = G._prefill(lm, proj, pr, cache, DEV)
        for s in range(steps):
            # recompute: the packed forward over every prefix (prompt + the tokens emitted so far)
            hist = cache.hist.cpu()
            ids = [hist[b, :P[b] + s].to(torch.int64) for b in range(B)]
            fs = [torch.cat([pr.input_features[b], torch.zeros(s, 400)]) for b in range(B)]
            ref_cache = G.KVCache.allocate(2, B, max(P) + s + 1, 8, 64, DEV)
            ref = G._prefill(lm, proj, G.Prompts(ids, fs), ref_cache, DEV).float()
            got = logits.float()
            rel = float((got - ref).abs().max() / ref.abs().max())
            worst_rel = max(worst_rel, rel)
            assert rel < 3e-2, (s, rel)
            top2 = torch.topk(ref, 2, dim=1).values
            sure = (top2[:, 0] - top2[:, 1]) > 2 * (got - ref).abs().max(1).values      # margin above the observed error
            tok_cmp += int(sure.sum())
            tok_eq += int((sure & (got.argmax(1) == ref.argmax(1))).sum())
            F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                          1.5, 2, -1, 128004)
            logits = G.decode_logits(lm, cache)
    print(f"cached vs recompute: worst max|diff| / max|logit| {worst_rel:.2e}; tokens {tok_eq}/{tok_cmp} where the "
          f"margin is clear")
    assert tok_eq == tok_cmp and tok_cmp > 0


# ---------------------------------------------------------------------------------------------------- (5) command line
def test_infer_asr_command_line(tmp_path):
    from safetensors.torch import save_file
    from touchnet_amd.bin import infer_asr
    from touchnet_amd.generation import GenerationConfig
    from touchnet_amd.models.touch_audio.inference_touch_audio import transcribe
    m, text = _tiny_touch_audio("qwen2", seed=21, F_in=320)
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    save_file({k: v.contiguous() for k, v in m.state_dict().items()}, str(ckpt / "model.safetensors"))
    (ckpt / "config.json").write_text(json.dumps({"text_config": text, "audio_config": {"input_size": 320},
                                                  "pad_token_id": 1}))
    (tmp_path / "data_config.json").write_text(json.dumps({"audio_feat_type": "fbank", "audiofeat_num_mel_bins": 80,
                                                           "audiofeat_stack_length": 4, "audiofeat_stride_length": 4}))
    rng = np.random.RandomState(0)
    lines = []
    for i, sec in enumerate([1.3, 0.4, 2.1]):
        p = tmp_path / f"u{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes((rng.randn(int(sec * 16000)) * 3000).clip(-32768, 32767).astype(np.int16).tobytes())
        lines.append({"key": f"u{i}", "wav": str(p), "txt": "x"})
    (tmp_path / "data.list").write_text("".join(json.dumps(x) + "\n" for x in lines))
    out = infer_asr.main(["--model_path", str(ckpt), "--data_list", str(tmp_path / "data.list"), "--output_dir",
                          str(tmp_path / "out"), "--data_config", str(tmp_path / "data_config.json"), "--batch_size", "2",
                          "--max_new_tokens", "24"])
    recs = [json.loads(x) for x in open(out)]
    assert len(recs) == 3 and [json.loads(r["label"])["key"] for r in recs] == ["u0", "u1", "u2"]
    assert all("predict" not in r for r in recs)                                # no tokenizer in the directory
    model = infer_asr.load_model(str(ckpt), DEV)
    dcfg = infer_asr.data_config(type("A", (), {"data_config": str(tmp_path / "data_config.json"),
                                                "model_path": str(ckpt)})(), model)
    feats = infer_asr.features([infer_asr.read_wav(x["wav"]) for x in lines], dcfg)
    assert [f.shape[1] for f in feats] == [320] * 3
    cfg = GenerationConfig(max_new_tokens=24)
    ids = transcribe(model, feats[:2], cfg) + transcribe(model, feats[2:], cfg)          # the command's batches
    assert [r["predict_ids"] for r in recs] == ids
