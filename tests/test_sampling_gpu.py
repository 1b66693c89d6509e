"""Sampled decoding and Qwen2-Audio inference on the MI355X: tn_sample_step against transformers' logits processors and
warpers (fp64), the seeded draws' distribution and keying, greedy mode against tn_greedy_step, a tiny Qwen2-Audio against
transformers' decoder teacher-forced, the growing KV cache, the device features against WhisperFeatureExtractor and the
infer_qwen2_audio command line."""
import json
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _state(hists, S_hist=96):
    B = len(hists)
    hist = torch.zeros(B, S_hist, dtype=torch.int32)
    for b, h in enumerate(hists):
        hist[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
    hl = torch.tensor([len(h) for h in hists], dtype=torch.int32)
    return {k: v.to(DEV) for k, v in dict(hist=hist, hl=hl, cl=hl - 1, fin=torch.zeros(B, dtype=torch.int32),
                                          nu=torch.tensor([B], dtype=torch.int32)).items()}


def _threshold_top_p(s, p):
    """TopPLogitsWarper's rule as a threshold (the kernel's): keep a token iff the mass strictly above its VALUE is < p —
    HF's sort breaks ties at the boundary in an arbitrary order, this keeps the whole tied group."""
    probs = torch.softmax(s, dim=-1)
    vals, inv = torch.unique(s, sorted=True, return_inverse=True)            # ascending distinct values
    mass = torch.zeros(vals.numel(), dtype=torch.float64).index_add_(0, inv, probs)
    above = mass.flip(0).cumsum(0).flip(0) - mass                            # mass strictly above each value
    return torch.where(above[inv] < p, s, torch.full_like(s, -float("inf")))


def _hf_probs(logits_row, hist_row, penalty, T, k, p, hf_top_p=False):
    """HF's pipeline in fp64: RepetitionPenalty, Temperature, TopK, TopP, softmax -> probabilities [V]."""
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    ids = torch.tensor([hist_row], dtype=torch.int64)
    s = logits_row.double()[None].clone()
    s = RepetitionPenaltyLogitsProcessor(penalty)(ids, s)
    s = TemperatureLogitsWarper(T)(ids, s)
    if k > 0:
        s = TopKLogitsWarper(k)(ids, s)
    if p < 1.0:
        s = TopPLogitsWarper(p)(ids, s) if hf_top_p else _threshold_top_p(s[0], p)[None]
    return torch.softmax(s[0], dim=-1)


# ---------------------------------------------------------------------------------------------------- (1) vs transformers
@pytest.mark.parametrize("B,V,dtype", [(1, 156032, torch.bfloat16), (12, 156032, torch.float32),
                                       (12, 128256, torch.bfloat16), (64, 128256, torch.float32),
                                       (64, 156032, torch.bfloat16)])
def test_sample_step_matches_transformers_warpers(B, V, dtype):
    import touchnet_amd.functional as F
    g = torch.Generator().manual_seed(B + V)
    T, pen = 0.8, 1.3
    hists = [torch.randint(0, V, (int(torch.randint(1, 80, (1,), generator=g)),), generator=g).tolist() for _ in range(B)]
    scale = torch.rand(B, 1, generator=g) * 4 + 0.5
    logits = (torch.randn(B, V, generator=g) * scale).to(dtype)
    for b in range(B):                                # seen ids among the largest logits, some negative
        logits[b, hists[b][0]] = float(logits[b].float().max()) + 0.5
    uni = torch.rand(B, generator=g)
    checked = near = 0
    for k in (0, 1, 20, 2000):
        for p in (1.0, 0.9, 0.5):
            st = _state(hists)
            kept = torch.zeros(B, dtype=torch.int32, device=DEV)
            F.sample_step(logits.to(DEV), st["hist"], st["hl"], st["cl"], st["fin"], st["nu"], pen, True, T, k, p, 0,
                          [V - 1], 0, uniforms=uni.to(DEV), n_kept=kept)
            torch.cuda.synchronize()
            got = [int(st["hist"][b, len(h)]) for b, h in enumerate(hists)]
            kept = kept.cpu().tolist()
            for b in range(B):
                probs = _hf_probs(logits[b].float(), hists[b], pen, T, k, p)
                n_ref = int((probs > 0).sum())
                cdf = torch.cumsum(probs, 0)
                want = int(torch.searchsorted(cdf, torch.tensor([float(uni[b])], dtype=torch.float64), right=True))
                checked += 1
                if p < 1.0:
                    # transformers' own TopPLogitsWarper keeps the same set up to the tied group at its boundary
                    hf = _hf_probs(logits[b].float(), hists[b], pen, T, k, p, hf_top_p=True) > 0
                    mine = probs > 0
                    assert bool((hf <= mine).all()) or kept[b] != n_ref
                    extra = torch.nonzero(mine & ~hf).reshape(-1)
                    if extra.numel():
                        lv = logits[b].float()
                        assert torch.unique(lv[extra]).numel() <= 2, (k, p, b, extra.numel())   # one tied value
                if kept[b] != n_ref:
                    # only a token whose mass above lies within 1e-5 of top_p may fall on the other side
                    pre = _hf_probs(logits[b].float(), hists[b], pen, T, k, 1.0)
                    sp, _ = torch.sort(pre, descending=True)
                    above = torch.cumsum(sp, 0) - sp
                    lo, hi = min(kept[b], n_ref), max(kept[b], n_ref)
                    assert p < 1.0 and bool(((above[lo:hi] - p).abs() < 1e-5).all()), (k, p, b, kept[b], n_ref)
                    near += 1
                    continue
                if got[b] != want:
                    assert abs(float(cdf[min(got[b], want)]) - float(uni[b])) < 1e-6, (k, p, b, got[b], want)
                    near += 1
            assert torch.equal(st["hl"].cpu(), torch.tensor([len(h) + 1 for h in hists], dtype=torch.int32))
    print(f"B={B} V={V} {dtype}: {checked} rows, {near} boundary cases")
    assert near <= checked // 50


# ---------------------------------------------------------------------------------------------------- (2) seeded draws
def test_seeded_draws_follow_the_warped_distribution_and_are_keyed():
    from scipy.stats import chi2
    import touchnet_amd.functional as F
    V, N = 4096, 20000
    g = torch.Generator().manual_seed(1)
    row = torch.randn(V, generator=g) * 2.0
    hist0 = [3, 17, 3]
    for k, p in ((20, 1.0), (0, 0.9), (50, 0.8)):
        probs = _hf_probs(row, hist0, 1.2, 0.9, k, p)
        st = _state([hist0] * N, S_hist=8)
        keys = torch.arange(N, dtype=torch.int64, device=DEV) * 7919 + 11
        F.sample_step(row.to(DEV)[None].expand(N, V).contiguous(), st["hist"], st["hl"], st["cl"], st["fin"], st["nu"],
                      1.2, True, 0.9, k, p, 1234, [], 0, row_key=keys)
        tok = st["hist"][:, len(hist0)].cpu().to(torch.int64)
        counts = torch.bincount(tok, minlength=V).double()
        support = probs > 0
        assert bool((counts[~support] == 0).all())
        exp = probs[support] * N
        obs = counts[support]
        # pool the rare categories (expected < 5) into one
        rare = exp < 5
        e = torch.cat([exp[~rare], exp[rare].sum()[None]]) if rare.any() else exp
        o = torch.cat([obs[~rare], obs[rare].sum()[None]]) if rare.any() else obs
        stat = float(((o - e) ** 2 / e.clamp_min(1e-12)).sum())
        pval = float(chi2.sf(stat, max(1, e.numel() - 1)))
        print(f"top_k {k} top_p {p}: {int(support.sum())} tokens, chi2 {stat:.1f}, p {pval:.3g}")
        assert pval > 1e-3
    # keying: the same (seed, row_key, step) draws the same token under any permutation; another seed changes the draws
    B = 64
    logits = torch.randn(B, 8192, generator=g).to(DEV)
    keys = torch.randint(0, 2 ** 40, (B,), generator=g).to(DEV)
    hists = [[int(x) for x in torch.randint(0, 8192, (int(n),), generator=g)] for n in torch.randint(1, 40, (B,), generator=g)]

    def draw(perm, seed):
        st = _state([hists[i] for i in perm.tolist()], S_hist=64)
        F.sample_step(logits[perm.to(DEV)], st["hist"], st["hl"], st["cl"], st["fin"], st["nu"], 1.1, True, 1.0, 0, 0.95,
                      seed, [], 0, row_key=keys[perm.to(DEV)])
        return torch.tensor([int(st["hist"][i, len(hists[j])]) for i, j in enumerate(perm.tolist())])
    ident = torch.arange(B)
    a = draw(ident, 99)
    perm = torch.randperm(B, generator=g)
    b = draw(perm, 99)
    assert torch.equal(a[perm], b)
    c = draw(ident, 100)
    assert int((a != c).sum()) > B // 4


# ---------------------------------------------------------------------------------------------------- (3) greedy mode
def test_greedy_mode_equals_tn_greedy_step_and_keeps_the_books():
    import touchnet_amd.functional as F
    V, pen, pad = 128256, 1.5, 128004
    g = torch.Generator().manual_seed(4)
    B = 24
    hists = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(1, 60, (B,), generator=g)]
    for dtype in (torch.bfloat16, torch.float32):
        logits = torch.randn(B, V, generator=g).to(dtype)
        for b in range(B):
            logits[b, hists[b][-1]] = 9.0                           # seen: 9 / 1.5 = 6 competes with the rest
        logits[3, 500] = logits[3, 300] = 20.0                      # tie: lowest id
        a, s = _state(hists), _state(hists)
        a["fin"][5] = s["fin"][5] = 1
        F.greedy_step(logits.to(DEV), a["hist"], a["hl"], a["cl"], a["fin"], a["nu"], pen, 0, 128001, pad)
        F.sample_step(logits.to(DEV), s["hist"], s["hl"], s["cl"], s["fin"], s["nu"], pen, False, eos=[128001], pad=pad)
        for k in a:
            assert torch.equal(a[k].cpu(), s[k].cpu()), k
        assert int(s["hist"][3, len(hists[3])]) == 300 and int(s["hist"][5, len(hists[5])]) == pad
    # several eos ids: either finishes a row, once; a finished row then emits pad and is not counted again
    logits = torch.full((4, 1000), -5.0)
    logits[0, 7] = logits[1, 9] = logits[2, 7] = logits[3, 100] = 5.0
    s = _state([[1], [1], [1], [1]], S_hist=8)
    s["fin"][2] = 1
    s["nu"].fill_(3)
    for _ in range(2):
        F.sample_step(logits.to(DEV), s["hist"], s["hl"], s["cl"], s["fin"], s["nu"], 1.0, False, eos=[7, 9], pad=0)
    assert s["hist"][:, 1:3].cpu().tolist() == [[7, 0], [9, 0], [0, 0], [100, 100]]
    assert s["fin"].cpu().tolist() == [1, 1, 1, 0] and int(s["nu"]) == 1
    assert s["hl"].cpu().tolist() == [3] * 4 and s["cl"].cpu().tolist() == [2] * 4


def test_sample_op_refuses_malformed_arguments():
    from touchnet_amd import _C
    import touchnet_amd.functional as F
    i32 = lambda *sh: torch.zeros(*sh, dtype=torch.int32, device=DEV)
    lg = torch.zeros(2, 100, device=DEV)
    good = [i32(2, 8), i32(2), i32(2), i32(2), i32(1)]
    with pytest.raises(_C.KernelError, match="at most 8"):
        F.sample_step(lg, *good, eos=list(range(9)))
    with pytest.raises(_C.KernelError, match="temperature"):
        F.sample_step(lg, *good, temperature=0.0)
    with pytest.raises(_C.KernelError, match="row_key"):
        F.sample_step(lg, *good, row_key=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(_C.KernelError, match="hist_len"):
        F.sample_step(lg, good[0], i32(3), *good[2:])


# ---------------------------------------------------------------------------------------------------- tiny Qwen2-Audio
def _tiny_tokenizer(tmp_path):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import AutoTokenizer, PreTrainedTokenizerFast
    vocab = {"[UNK]": 0}
    for i in range(1, 290):
        vocab[f"w{i}"] = i
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="[UNK]", eos_token="<|endoftext|>",
                                   pad_token="<|endoftext|>",
                                   additional_special_tokens=["<|audio_bos|>", "<|AUDIO|>", "<|audio_eos|>", "<|im_end|>"])
    d = tmp_path / "tok"
    fast.save_pretrained(str(d))
    t = AutoTokenizer.from_pretrained(str(d))
    return t, d


def _tiny_qwen2_audio(tok, seed=0):
    """A random transformers Qwen2AudioForConditionalGeneration with bf16-representable weights and the packed model
    holding the same weights (on the device, bf16)."""
    import transformers
    from touchnet_amd.bin.infer_qwen2_audio import hf_names
    from touchnet_amd.models.qwen2_audio import Qwen2AudioConfig, Qwen2AudioPackedForConditionalGeneration
    V = len(tok)
    audio = tok.convert_tokens_to_ids("<|AUDIO|>")
    eos = [tok.convert_tokens_to_ids("<|endoftext|>"), tok.convert_tokens_to_ids("<|im_end|>")]
    d = dict(audio_config=dict(num_mel_bins=128, d_model=128, encoder_layers=2, encoder_attention_heads=2,
                               encoder_ffn_dim=256, max_source_positions=1500),
             text_config=dict(model_type="qwen2", hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                              num_attention_heads=2, num_key_value_heads=2, head_dim=128, vocab_size=V,
                              rope_theta=1000000.0, rms_norm_eps=1e-6, tie_word_embeddings=False,
                              eos_token_id=eos[0], pad_token_id=eos[0], bos_token_id=eos[0]),
             audio_token_index=audio)
    torch.manual_seed(seed)
    hf = transformers.Qwen2AudioForConditionalGeneration(transformers.Qwen2AudioConfig(**d)).eval()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            p.normal_(0, 0.08 if p.dim() > 1 else 0.1)
            if "norm" in n and n.endswith("weight"):
                p.add_(1.0)
            p.copy_(p.to(torch.bfloat16).float())
    sd = hf_names({k: v.clone() for k, v in hf.state_dict().items()})
    m = Qwen2AudioPackedForConditionalGeneration(Qwen2AudioConfig.from_dict(d))
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if "rotary" not in k], (missing, unexpected)
    return hf, m.to(DEV).to(torch.bfloat16).eval(), d, eos


def _wavs(secs, seed=0):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy((rng.randn(int(s * 16000)) * 3000).clip(-32768, 32767).astype(np.int16)) for s in secs]


def test_qwen2_audio_greedy_matches_transformers_teacher_forced(tmp_path):
    """With do_sample off the transcripts follow transformers' Qwen2 decoder teacher-forced in fp32 (the audio rows as
    the packed model computed them: its tower is the reference's causal one); top_k 1 with sampling on is greedy."""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from touchnet_amd.generation import GenerationConfig
    from touchnet_amd.models.qwen2_audio import inference_qwen2_audio as Q
    tok, _ = _tiny_tokenizer(tmp_path)
    hf, m, d, eos = _tiny_qwen2_audio(tok, seed=3)
    wavs = _wavs([1.2, 0.3, 2.5, 0.8])
    cfg = GenerationConfig.from_hf({"repetition_penalty": 1.1, "eos_token_id": eos, "max_new_tokens": 24})
    ids, texts = Q.transcribe(m, wavs, tok, "w1 w2", cfg)
    assert len(ids) == 4 and all(isinstance(t, str) for t in texts)
    # the prefill embeddings (prompt rows) as the packed model builds them, in fp32 on the CPU
    mel, valid = Q.features(wavs, DEV)
    prompts = Q.build_prompts(tok, valid, "w1 w2")
    embed = Q.audio_embedder(m, mel, valid, prompts)
    lens = [int(t.numel()) for t in prompts.input_ids]
    flat = torch.cat(prompts.input_ids).to(DEV)
    with torch.no_grad():
        pe = embed(flat, lens, flat.numel()).float().cpu()
    lm = hf.model.language_model if hasattr(hf.model, "language_model") else hf.language_model.model
    head = hf.lm_head if hasattr(hf, "lm_head") else hf.language_model.lm_head
    rep = RepetitionPenaltyLogitsProcessor(1.1)
    compared = equal = 0
    o = 0
    for b, toks in enumerate(ids):
        P = lens[b]
        full = toks + ([eos[0]] if len(toks) < 24 else [])
        seq = torch.cat([prompts.input_ids[b], torch.tensor(full, dtype=torch.int64)])
        with torch.no_grad():
            emb = torch.cat([pe[o:o + P], lm.embed_tokens(torch.tensor(full, dtype=torch.int64))])[None]
            h = lm(inputs_embeds=emb, position_ids=torch.arange(seq.numel())[None]).last_hidden_state
            logits = head(h)[0].float()
        o += P
        for s_, t in enumerate(full):
            sc = rep(seq[None, :P + s_], logits[P - 1 + s_][None].clone())[0]
            best = int(torch.argmax(sc))
            compared += 1
            if t == best or int(sc.argmax()) in eos and t in eos:
                equal += 1
            else:
                top = torch.topk(sc, 2).values
                assert float(sc[best] - sc[t]) <= 0.02 * float(top[0].abs()) + 0.05, (b, s_, t, best)
    print(f"qwen2-audio: {equal}/{compared} steps equal to transformers' argmax; lengths {[len(t) for t in ids]}")
    assert compared >= 20 and equal >= 0.9 * compared
    # top_k 1 with sampling on is greedy
    cfg_k1 = GenerationConfig.from_hf({"repetition_penalty": 1.1, "eos_token_id": eos, "max_new_tokens": 24,
                                       "do_sample": True, "top_k": 1, "temperature": 0.7}, seed=5)
    ids_k1, _ = Q.transcribe(m, wavs, tok, "w1 w2", cfg_k1)
    # (TopKLogitsWarper keeps every token tied with the maximum and the draw may pick any of them, greedy the lowest id:
    # a row may part from greedy only where its bf16 logits tie)
    from touchnet_amd import generation as G
    for b, (x, y) in enumerate(zip(ids_k1, ids)):
        if x == y:
            continue
        s_ = next(i for i in range(min(len(x), len(y))) if x[i] != y[i])
        one = G.Prompts([torch.cat([prompts.input_ids[b], torch.tensor(y[:s_], dtype=torch.int64)])])
        emb1 = Q.audio_embedder(m, mel[b:b + 1], valid[b:b + 1], G.Prompts([prompts.input_ids[b]]))
        cache = G.KVCache.allocate(2, 1, one.input_ids[0].numel() + 1, 2, 128, DEV)
        with torch.no_grad():
            lg = G._prefill(m.language_model, None, one, cache, DEV,
                            lambda ids_, lens_, Tp: torch.cat([emb1(ids_[:lens[b]], [lens[b]], lens[b]),
                                                               m.language_model.model.embed_tokens(ids_[lens[b]:])]))
        lg = rep(one.input_ids[0][None], lg.float().cpu())[0]
        assert abs(float(lg[x[s_]] - lg[y[s_]])) <= 0.05, (b, s_, x[s_], y[s_])
        print(f"row {b}: top_k 1 parts from greedy at step {s_} on a tie ({x[s_]} / {y[s_]})")


def test_growing_cache_gives_the_tokens_of_full_preallocation(tmp_path):
    from touchnet_amd.generation import GenerationConfig
    from touchnet_amd.models.qwen2_audio import inference_qwen2_audio as Q
    tok, _ = _tiny_tokenizer(tmp_path)
    _, m, _, eos = _tiny_qwen2_audio(tok, seed=4)
    wavs = _wavs([0.9, 2.0, 0.4], seed=1)
    for smp in ({"do_sample": False}, {"do_sample": True, "top_k": 30, "top_p": 0.9, "temperature": 1.3}):
        base = dict(repetition_penalty=1.05, eos_token_id=[-7], max_new_tokens=40, **smp)  # (an eos never drawn)
        full = Q.transcribe(m, wavs, tok, "w1", GenerationConfig.from_hf(base, seed=9, cache_chunk=4096))[0]
        grown = Q.transcribe(m, wavs, tok, "w1", GenerationConfig.from_hf(base, seed=9, cache_chunk=8))[0]
        assert [len(r) for r in full] == [40] * 3
        assert grown == full


# ---------------------------------------------------------------------------------------------------- (6) features
def test_device_features_match_whisper_feature_extractor():
    from transformers import WhisperFeatureExtractor
    from touchnet_amd.models.qwen2_audio import inference_qwen2_audio as Q
    fe = WhisperFeatureExtractor(feature_size=128)
    wavs = _wavs([3.0, 30.0, 35.0], seed=2)
    mel, valid = Q.features(wavs, DEV)
    for w, m_, L in zip(wavs, mel.cpu(), valid):
        x = w.numpy().astype(np.float32) / 32768.0
        out = fe(x, sampling_rate=16000, truncation=True, return_attention_mask=True, padding="max_length",
                 return_tensors="np")
        ref = torch.from_numpy(out["input_features"][0])
        assert int(out["attention_mask"].sum()) == L
        assert m_.shape == ref.shape == (128, 3000)
        err = float((m_[:, :L] - ref[:, :L]).abs().max())
        print(f"{w.numel() / 16000:.0f} s: {L} valid frames, max |diff| {err:.2e}")
        assert err < 2e-3


# ---------------------------------------------------------------------------------------------------- (7) command line
def test_infer_qwen2_audio_command_line(tmp_path):
    from safetensors.torch import save_file
    from touchnet_amd.bin import infer_qwen2_audio as cli
    from touchnet_amd.generation import GenerationConfig
    from touchnet_amd.models.qwen2_audio import inference_qwen2_audio as Q
    tok, tdir = _tiny_tokenizer(tmp_path)
    hf, _, d, eos = _tiny_qwen2_audio(tok, seed=6)
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    save_file({k: v.contiguous() for k, v in hf.state_dict().items()}, str(ckpt / "model.safetensors"))
    (ckpt / "config.json").write_text(json.dumps(d))
    gen = {"do_sample": True, "temperature": 0.9, "top_k": 40, "top_p": 0.8, "repetition_penalty": 1.1,
           "eos_token_id": eos, "pad_token_id": eos[0]}
    (ckpt / "generation_config.json").write_text(json.dumps(gen))
    tok.save_pretrained(str(ckpt))
    wavs = _wavs([1.3, 0.4, 2.1], seed=3)
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
    args = ["--model_path", str(ckpt), "--data_list", str(tmp_path / "data.list"), "--instruct", "w3",
            "--batch_size", "2", "--max_length", "400", "--seed", "17"]
    out = cli.main(args + ["--output_dir", str(tmp_path / "out")])
    recs = [json.loads(x) for x in open(out)]
    assert [json.loads(r["label"])["key"] for r in recs] == ["u0", "u1", "u2"]
    model = cli.load_model(str(ckpt), DEV)
    cfg = GenerationConfig.from_hf(str(ckpt), max_length=400, seed=17)
    texts = (Q.transcribe(model, wavs[:2], tok, "w3", cfg, row_keys=torch.tensor([0, 1]))[1]
             + Q.transcribe(model, wavs[2:], tok, "w3", cfg, row_keys=torch.tensor([2]))[1])
    assert [r["predict"] for r in recs] == texts
    # sharding: the utterance keeps its line number as its row key
    out2 = cli.main(args + ["--output_dir", str(tmp_path / "out2"), "--batch_size", "1", "--num_shards", "2",
                            "--shard_index", "1"])
    assert [json.loads(x)["predict"] for x in open(out2)] == \
        Q.transcribe(model, wavs[1:2], tok, "w3", cfg, row_keys=torch.tensor([1]))[1]
    # a batch whose longest prompt exceeds max_length is skipped
    out3 = cli.main(args[:-4] + ["--max_length", "20", "--output_dir", str(tmp_path / "out3")])
    assert open(out3).read() == ""
