"""KV-cache decoding on one MI355X: tn_attn_decode per call (µs, achieved TB/s) and greedy ASR decoding end to end on
LlamaForASR-1B (random weights, eos unreachable: every run decodes max_new_tokens), against transformers' own bf16
generate() (sdpa, same knobs, same weights).  Prints one JSON object per measurement.

    python scripts/decode_bench.py [--skip-hf] [--layers 16] [--batch 12] [--new 256]
    python scripts/decode_bench.py --qwen2-audio-7b [--batch 12]
    python scripts/decode_bench.py --num-beams 4 [--batch 12]
    python scripts/decode_bench.py --kimi-audio-7b [--batch 12]
    python scripts/decode_bench.py --hotwords 1024 [--batch 12]
    python scripts/decode_bench.py --token-scores [K] [--batch 12]
    python scripts/decode_bench.py --attn-extend [--layers 16]

--qwen2-audio-7b: the decoder of Qwen2-Audio-7B (32 layers, 32 / 32 heads, D 128, V 156 032, random weights): tn_sample_step
per call (µs) for top-k + top-p, top-p alone and greedy on bf16 logits [B, 156 032], and ms per decode step end to end
(decode_logits + tn_sample_step, top_k 50 / top_p 0.9, caches of ~300 tokens per row).

--num-beams K: beam search at LlamaForASR-1B and Qwen2-Audio-7B widths (B utterances, K beams, prompts of 300 ids, random
weights, eos unreachable): tn_beam_step per call (µs) and its share of the decode step (decode_logits through the table +
tn_beam_step), and per layer tn_attn_decode_beam against the path it replaces — index_select of both caches by the beams'
parents (HF's reorder_cache) followed by tn_attn_decode on the dense result.

--kimi-audio-7b: the decoder of Kimi-Audio-7B (28 layers, 28 / 4 heads, D 128, H 3584, V 168 448, random bf16 weights, prompts
of 300 rows, eos unreachable): tn_kimi_text_step per call (µs) in greedy and top-k 5 mode on bf16 logits [B, 168 448] with
tn_sample_step's greedy mode beside it at the same shape, prefill ms, and ms per decode step (decode_logits on the row the
step kernel wrote + tn_kimi_text_step) against the same step with the row built by torch (history gather, two embedding
lookups, add) — the launches the fused write removes.

--hotwords N: tn_logits_constrain with a table of N phrases x 4 prefixes on bf16 logits [B, 156 032]: per call (µs, apply
and emit mode), its share of the Qwen2-Audio-7B sampled decode step timed in the same run (with an A/B of the whole step
with and without the plan), and tn_beam_step with and without the edit list (K 4).

--token-scores [K]: tn_token_scores per call (µs) in history mode on bf16 logits [B, V] at V = 128 256 and 152 064 with k = 0
and k = K (default 8), rows/s in token mode on [4096, V] (the rescoring shape), and its share of the Qwen2-Audio-7B sampled
decode step timed in the same run (with an A/B of the whole step with and without the launch).

--kv-fp8: the FP8 (e4m3) KV cache beside the bf16 kernels of the same build, alternated in one process (medians of 5 rounds):
tn_attn_decode_fp8 against tn_attn_decode at B rows behind 750 and 8 192 positions (32 / 8 heads at D 64, 28 / 4 at D 128),
tn_attn_extend_fp8 against tn_attn_extend at --attn-extend's two shapes (with and without the two tn_kv_quantize launches
of the new rows), tn_kv_quantize at a 12 x 750-row prefill, the largest logit difference between an fp8 and a bf16 cache
over one teacher-forced generation of a random-weight model (a recorded number, not a gate), and ms per decode step at
Qwen2-Audio-7B's widths behind 750 and 8 192 cached positions (profiles/kv_fp8_bench.log).

--decode-gemm-mxfp4 [DECODER]: the MXFP4 arms of the weight-streaming kernels beside the FP8 arms of the same build, alternated
in one process: the decode step's product families and lm_head at M = 1, 12, 48, 96 (small-M kernel) and 256 (mid-M kernel),
weights cycled through copies that outgrow L2 / MALL, then the whole step at B rows with lib, own, fp8 and mxfp4 alternated
(profiles/decode_gemm_mxfp4_bench.log).

--prefill-codes [DECODER]: one decoder layer's seven products (q/k/v + RoPE, o_proj, gate/up + SwiGLU, down_proj) on FP8 and
MXFP4 weights at M = 257 .. 8192 rows, through `linear_group` / `swiglu_mlp` with the router's row bound at 256 (dequantise per
call, then the bf16 path) and unbounded (the prefill kernel for codes, csrc/gemm_codes.hip), alternated in one process on weight
sets cycled past L2 / MALL; achieved TF/s and weight TB/s of the new route beside it (profiles/prefill_codes_bench.log).

bytes per attention call = sum_b (len_b + 1) * Nkv * D * 2 (K and V) * 2 bytes — the cache read; q / o and the appended
row are noise beside it.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = torch.device("cuda", 0)


def _events_time(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # µs


def bench_kernel(B, L, Nh, Nkv, D, iters=200):
    import touchnet_amd.functional as F
    S_max = L + 1
    kc = torch.randn(B, S_max, Nkv, D, device=DEV, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    q = torch.randn(B, Nh, D, device=DEV, dtype=torch.bfloat16)
    kn = torch.randn(B, Nkv, D, device=DEV, dtype=torch.bfloat16)
    cl = torch.full((B,), L - 1, dtype=torch.int32, device=DEV)           # L keys attended
    flush = torch.empty(512 * 2 ** 20, dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        for _ in range(10):
            F.attn_decode(q, kn, kn, kc, vc, cl)
        torch.cuda.synchronize()
        hot = _events_time(lambda: F.attn_decode(q, kn, kn, kc, vc, cl), iters)
        # cold: a 512 MiB write between calls evicts the caches from L2 / MALL; the flush is timed alone and subtracted
        cold_total = _events_time(lambda: (flush.zero_(), F.attn_decode(q, kn, kn, kc, vc, cl)), 50)
        flush_only = _events_time(lambda: flush.zero_(), 50)
    nbytes = B * L * Nkv * D * 2 * 2
    return dict(what="attn_decode", B=B, L=L, Nh=Nh, Nkv=Nkv, D=D, bytes=nbytes, us_back_to_back=round(hot, 2),
                tbps_back_to_back=round(nbytes / hot / 1e6, 3), us_cold=round(cold_total - flush_only, 2),
                tbps_cold=round(nbytes / (cold_total - flush_only) / 1e6, 3))


def _model(layers):
    from touchnet_amd.models.llama import DecoderConfig
    from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
    text = dict(model_type="llama", hidden_size=2048, intermediate_size=8192, num_attention_heads=32, num_key_value_heads=8,
                head_dim=64, num_hidden_layers=layers, vocab_size=128256, rope_theta=500000.0, tie_word_embeddings=True,
                rope_scaling={"factor": 32.0, "high_freq_factor": 4.0, "low_freq_factor": 1.0,
                              "original_max_position_embeddings": 8192, "rope_type": "llama3"},
                pad_token_id=128004, bos_token_id=128000, eos_token_id=128001, initializer_range=0.02, rms_norm_eps=1e-5)
    torch.manual_seed(0)
    with torch.device(DEV):
        m = TouchAudioForCausalLM(TouchAudioConfig(text_config=DecoderConfig.from_dict(text), input_size=400))
    m.post_init()
    return m.to(torch.bfloat16).eval(), text


def bench_e2e(layers, B, new, skip_hf):
    from touchnet_amd import generation as G
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts
    m, text = _model(layers)
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(60, 180, (B,), generator=g).tolist()      # AISHELL utterances: 2.4-7 s at 4 stacked 10 ms frames
    feats = [torch.randn(n, 400, generator=g) * 0.5 for n in lens]
    pr = build_prompts(feats, 128004, 128000)
    cfg = G.GenerationConfig(max_new_tokens=new, eos_token_id=-1, pad_token_id=128004)      # eos unreachable
    lm, proj = m.language_model, m.projector.weight
    res = []
    with torch.no_grad():
        for _ in range(2):                                           # warm-up (GEMM algorithm selection, code objects)
            G.generate(m, pr, G.GenerationConfig(max_new_tokens=8, eos_token_id=-1, pad_token_id=128004))
        torch.cuda.synchronize()
        P = [int(t.numel()) for t in pr.input_ids]
        runs = []
        for _ in range(3):
            cache = G.KVCache.allocate(layers, B, max(P) + new, 8, 64, DEV)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logits = G._prefill(lm, proj, pr, cache, DEV)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            import touchnet_amd.functional as F
            F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, 1.5, 2,
                          -1, 128004)
            for _ in range(new - 1):
                logits = G.decode_logits(lm, cache)
                F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                              1.5, 2, -1, 128004)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            runs.append((t1 - t0, (t2 - t1) / (new - 1)))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            G.generate(m, pr, cfg)
            torch.cuda.synchronize()
            runs[-1] = runs[-1] + (time.perf_counter() - t3,)
        pre = min(r[0] for r in runs)
        step = min(r[1] for r in runs)
        total = min(r[2] for r in runs)
        res.append(dict(what="touchnet_amd.generate", layers=layers, B=B, new_tokens=new, prompt_rows=lens,
                        prefill_ms=round(pre * 1e3, 2), ms_per_decode_step=round(step * 1e3, 3),
                        generate_total_ms=round(total * 1e3, 1)))
    if not skip_hf:
        import transformers
        hf_cfg = transformers.LlamaConfig(vocab_size=128256, hidden_size=2048, intermediate_size=8192,
                                          num_hidden_layers=layers, num_attention_heads=32, num_key_value_heads=8, head_dim=64,
                                          rope_theta=500000.0, rope_scaling=text["rope_scaling"], tie_word_embeddings=True,
                                          rms_norm_eps=1e-5, pad_token_id=128004, bos_token_id=128000,
                                          max_position_embeddings=131072)
        hf_cfg._attn_implementation = "sdpa"
        with torch.device(DEV):
            hf = transformers.LlamaForCausalLM(hf_cfg).to(torch.bfloat16).eval()
        hf.load_state_dict({k: v for k, v in lm.state_dict().items()}, strict=False)
        # the reference's batch: left-padded prompts, embed(ids) + projector(features)
        T = max(P)
        ids = torch.full((B, T), 128004, dtype=torch.int64)
        fs = torch.zeros(B, T, 400)
        mask = torch.zeros(B, T, dtype=torch.int64)
        pos = torch.zeros(B, T, dtype=torch.int64)
        for b in range(B):
            n = P[b]
            ids[b, T - n:] = pr.input_ids[b]
            fs[b, T - n:] = pr.input_features[b]
            mask[b, T - n:] = 1
            pos[b, T - n:] = torch.arange(n)
        ids, fs, mask, pos = ids.to(DEV), fs.to(DEV, torch.bfloat16), mask.to(DEV), pos.to(DEV)
        with torch.no_grad():
            emb = hf.model.embed_tokens(ids) + fs @ proj.t()
            kw = dict(inputs_embeds=emb, attention_mask=mask, use_cache=True, do_sample=False, num_beams=1,
                      repetition_penalty=1.5, no_repeat_ngram_size=2, pad_token_id=128004, eos_token_id=None,
                      bos_token_id=128000)
            hf.generate(**kw, max_new_tokens=8)
            torch.cuda.synchronize()
            times = []
            for _ in range(2):
                t0 = time.perf_counter()
                out = hf.generate(**kw, max_new_tokens=new, min_new_tokens=new)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
        res.append(dict(what="transformers.generate (bf16, sdpa)", layers=layers, B=B, new_tokens=int(out.shape[1]),
                        generate_total_ms=round(min(times) * 1e3, 1),
                        ms_per_token_incl_prefill=round(min(times) * 1e3 / new, 3)))
    return res


def bench_qwen2_audio_7b(B, steps=32, iters=200):
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    V = 156032
    g = torch.Generator(device=DEV).manual_seed(0)
    logits = (torch.randn(B, V, device=DEV, generator=g) * 3).to(torch.bfloat16)
    hist = torch.randint(0, V, (B, 512), device=DEV, generator=g, dtype=torch.int32)
    z = lambda: torch.zeros(B, dtype=torch.int32, device=DEV)
    fin, nu, keys = z(), torch.ones(1, dtype=torch.int32, device=DEV), torch.arange(B, device=DEV)
    rows = []
    for name, smp, k, p in (("top_k 20 + top_p 0.8", True, 20, 0.8), ("top_k 50 + top_p 0.9", True, 50, 0.9),
                            ("top_p 0.9", True, 0, 0.9), ("greedy", False, 0, 1.0)):
        hl, cl = torch.full((B,), 300, dtype=torch.int32, device=DEV), z()

        def call():
            hl.fill_(300)
            F.sample_step(logits, hist, hl, cl, fin, nu, 1.1, smp, 0.7, k, p, 1, [151643, 151645], 151643, row_key=keys)
        call()
        us = _events_time(call, iters)
        rows.append(dict(kernel="tn_sample_step", mode=name, B=B, V=V, us=round(us, 2)))
    text = DecoderConfig.from_dict(dict(model_type="qwen2", hidden_size=4096, intermediate_size=11008, num_attention_heads=32,
                                        num_key_value_heads=32, head_dim=128, num_hidden_layers=32, vocab_size=V,
                                        rope_theta=10000.0, rms_norm_eps=1e-5, tie_word_embeddings=False,
                                        initializer_range=0.02, eos_token_id=151643, pad_token_id=151643))
    torch.manual_seed(0)
    with torch.device(DEV):
        lm = PackedCausalLM(text)
    lm.post_init()
    lm = lm.to(torch.bfloat16).eval()
    lens = [300] * B
    prompts = G.Prompts([torch.randint(0, 150000, (n,)) for n in lens])
    cache = G.KVCache.allocate(32, B, max(lens) + steps + 8, 32, 128, DEV)
    with torch.no_grad():
        logits = G._prefill(lm, None, prompts, cache, DEV)

        def step():
            F.sample_step(G.decode_logits(lm, cache), cache.hist, cache.hist_len, cache.cache_len, cache.finished,
                          cache.n_unfinished, 1.1, True, 0.7, 50, 0.9, 1, [151643, 151645], 151643, row_key=keys)
        F.sample_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, 1.1,
                      True, 0.7, 50, 0.9, 1, [151643, 151645], 151643, row_key=keys)
        step()
        ms = _events_time(step, steps - 2) / 1e3
    k50 = next(r["us"] for r in rows if r["mode"] == "top_k 50 + top_p 0.9")
    rows.append(dict(e2e="qwen2_audio_7b_decode_step", B=B, ms_per_step=round(ms, 3),
                     sample_share_top_k50_top_p=round(k50 / (ms * 1e3), 4),
                     sample_share_top_p_only=round(next(r["us"] for r in rows if r.get("mode") == "top_p 0.9") /
                                                   (ms * 1e3), 4)))
    return rows


def bench_kimi_audio_7b(B, steps=32, iters=200):
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.kimi_audio import KimiAudioConfig, KimiAudioPackedForCausalLM
    from touchnet_amd.models.kimi_audio.inference_kimi_audio import _TextDecoder
    V, H, P, W = 168448, 3584, 300, 16
    blank, eos = 151666, -1                                              # eos unreachable
    g = torch.Generator(device=DEV).manual_seed(0)
    cfg = KimiAudioConfig(vocab_size=V, hidden_size=H, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28,
                          num_key_value_heads=4, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6, initializer_range=0.02)
    torch.manual_seed(0)
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(DEV):
            m = KimiAudioPackedForCausalLM(cfg)
        m.post_init()
    finally:
        torch.set_default_dtype(torch.float32)
    m = m.eval()
    lm = _TextDecoder(m)
    E = m.model.embed_tokens.weight.detach()
    logits = (torch.randn(B, V, device=DEV, generator=g) * 3).to(torch.bfloat16)
    hist = torch.randint(0, V, (B, 512), device=DEV, generator=g, dtype=torch.int32)
    z = lambda: torch.zeros(B, dtype=torch.int32, device=DEV)
    fin, nu, keys = z(), torch.ones(1, dtype=torch.int32, device=DEV), torch.arange(B, device=DEV)
    pl = torch.full((B,), 200, dtype=torch.int32, device=DEV)            # 100 generated: the penalty window is in force
    x = torch.empty(B, H, dtype=torch.bfloat16, device=DEV)
    rows = []
    with torch.no_grad():
        for name, T, k in (("greedy", 0.0, 5), ("top_k 5", 0.8, 5), ("top_k 64", 0.8, 64)):
            hl, cl = torch.full((B,), 300, dtype=torch.int32, device=DEV), z()

            def call():
                hl.fill_(300)
                F.kimi_text_step(logits, hist, hl, cl, fin, nu, pl, E, x, 1.1, W, T, k, 1, eos, blank, row_key=keys)
            call()
            rows.append(dict(kernel="tn_kimi_text_step", mode=name, B=B, V=V, H=H, us=round(_events_time(call, iters), 2)))
        hl, cl = torch.full((B,), 300, dtype=torch.int32, device=DEV), z()

        def call_sample():
            hl.fill_(300)
            F.sample_step(logits, hist, hl, cl, fin, nu, 1.1, False, 1.0, 0, 1.0, 1, [], blank, row_key=keys)
        call_sample()
        rows.append(dict(kernel="tn_sample_step", mode="greedy", B=B, V=V, us=round(_events_time(call_sample, iters), 2)))
        rows.append(dict(kernel="fill_ of hist_len alone (inside every figure above)", B=B,
                         us=round(_events_time(lambda: hl.fill_(300), iters), 2)))
        prompts = G.Prompts([torch.randint(0, 150000, (P,)) for _ in range(B)])
        pre = []
        for _ in range(3):
            cache = G.KVCache.allocate(28, B, P + 6 * steps + 8, 4, 128, DEV)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            first = G._prefill(lm, None, prompts, cache, DEV, lambda ids, lens, Tp: E[ids] + E[blank][None])
            torch.cuda.synchronize()
            pre.append(time.perf_counter() - t0)
        pl = torch.full((B,), P, dtype=torch.int32, device=DEV)
        kstep = lambda lg: F.kimi_text_step(lg, cache.hist, cache.hist_len, cache.cache_len, cache.finished,
                                            cache.n_unfinished, pl, E, x, 1.1, W, 0.0, 5, 1, eos, blank, row_key=keys)
        kstep(first)

        def fused():
            kstep(G.decode_logits(lm, cache, inputs_embeds=x))

        def by_torch():
            tok = cache.hist.gather(1, (cache.hist_len.to(torch.int64) - 1)[:, None])[:, 0].to(torch.int64)
            kstep(G.decode_logits(lm, cache, inputs_embeds=E[tok] + E[blank][None]))
        fused()
        by_torch()
        ab = [(_events_time(fused, steps - 2) / 1e3, _events_time(by_torch, steps - 2) / 1e3) for _ in range(3)]   # A B A B A B
        ms_fused, ms_torch = min(a for a, _ in ab), min(b for _, b in ab)
    greedy = next(r["us"] for r in rows if r.get("kernel") == "tn_kimi_text_step" and r["mode"] == "greedy")
    k5 = next(r["us"] for r in rows if r.get("mode") == "top_k 5")
    rows.append(dict(e2e="kimi_audio_7b_decode", B=B, prompt_rows=P, prefill_ms=round(min(pre) * 1e3, 2),
                     ms_per_step_x_next=round(ms_fused, 3), ms_per_step_gather_add_by_torch=round(ms_torch, 3),
                     ab_runs_ms=[[round(a, 3), round(b, 3)] for a, b in ab],
                     step_share_greedy=round(greedy / (ms_fused * 1e3), 4), step_share_top_k5=round(k5 / (ms_fused * 1e3), 4)))
    return rows


def bench_beams(K, B, steps=24, iters=100):
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    widths = (("llama_asr_1b", dict(model_type="llama", hidden_size=2048, intermediate_size=8192, num_attention_heads=32,
                                    num_key_value_heads=8, head_dim=64, num_hidden_layers=16, vocab_size=128256,
                                    rope_theta=500000.0, tie_word_embeddings=True, rms_norm_eps=1e-5), [-1], 1.5, 2),
              ("qwen2_audio_7b", dict(model_type="qwen2", hidden_size=4096, intermediate_size=11008,
                                      num_attention_heads=32, num_key_value_heads=32, head_dim=128, num_hidden_layers=32,
                                      vocab_size=156032, rope_theta=10000.0, rms_norm_eps=1e-5,
                                      tie_word_embeddings=False), [-1, -2], 1.1, 0))
    rows = []
    for name, text, eos, penalty, ngram in widths:
        text.update(initializer_range=0.02, eos_token_id=1, pad_token_id=0)
        cfg = DecoderConfig.from_dict(text)
        torch.manual_seed(0)
        with torch.device(DEV):
            lm = PackedCausalLM(cfg)
        lm.post_init()
        lm = lm.to(torch.bfloat16).eval()
        P, L, Nh, Nkv, D = 300, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        prompts = G.Prompts([torch.randint(2, 100000, (P,)) for _ in range(B)])
        n_new = steps + iters + 8
        st = G.BeamState.allocate(L, B, K, P + n_new, Nkv, D, DEV)
        kw = dict(penalty=penalty, ngram=ngram, eos=eos, n_new=n_new, length_penalty=1.0, early_stopping=False)
        with torch.no_grad():
            F.beam_step(G._prefill(lm, None, prompts, st, DEV, row_stride=K), st, **kw)

            def step():
                F.beam_step(G.decode_logits(lm, st, table=st.src), st, **kw)
            step()
            ms = _events_time(step, steps - 2) / 1e3
            # attention of one layer at this state: through the table, against reorder-copy + dense attention
            R = B * K
            q = torch.randn(R, Nh, D, device=DEV, dtype=torch.bfloat16)
            kn = torch.randn(R, Nkv, D, device=DEV, dtype=torch.bfloat16)
            kc, vc, cl, src = st.k[0], st.v[0], st.cache_len, st.src
            parent = st.out_parent.to(torch.int64)
            F.attn_decode_beam(q, kn, kn, kc, vc, cl, src)
            us_table = _events_time(lambda: F.attn_decode_beam(q, kn, kn, kc, vc, cl, src), iters)

            # HF's reorder_cache copies the cache at its current length: the live rows plus the slot of the new token
            live = int(cl.max()) + 1

            def reorder_then_dense():
                F.attn_decode(q, kn, kn, kc[:, :live].index_select(0, parent), vc[:, :live].index_select(0, parent), cl)
            reorder_then_dense()
            us_copy = _events_time(reorder_then_dense, iters)
            kd, vd = kc[:, :live].contiguous(), vc[:, :live].contiguous()
            us_dense = _events_time(lambda: F.attn_decode(q, kn, kn, kd, vd, cl), iters)
            logits = G.decode_logits(lm, st, table=st.src)
            us_step = _events_time(lambda: F.beam_step(logits, st, **kw), iters)
        rows.append(dict(width=name, B=B, K=K, V=cfg.vocab_size, cache_rows=int(st.cache_len[0]), S_max=st.capacity,
                         ms_per_decode_step=round(ms, 3), beam_step_us=round(us_step, 2),
                         beam_step_share=round(us_step / (ms * 1e3), 4), attn_decode_beam_us_per_layer=round(us_table, 2),
                         reorder_copy_plus_attn_decode_us_per_layer=round(us_copy, 2), reorder_copied_rows=live,
                         attn_decode_dense_alone_us_per_layer=round(us_dense, 2),
                         utterances_still_running=int(st.n_unfinished.item())))
        del lm, st, kc, vc, kd, vd
        torch.cuda.empty_cache()
    return rows


def bench_hotwords(N, B, K=4, steps=32, iters=200):
    """tn_logits_constrain with a table of N phrases x 4 prefixes (generation.hotword_bias) at Qwen2-Audio-7B's width:
    alone on bf16 logits [B, 156 032] (apply and emit mode), inside the sampled decode step (decode_logits + constrain +
    tn_sample_step against the same step without a plan, A/B twice in one process), and the beam step with and without
    the edit list.  B phrases continue a row's history, so every row has one sequence of each length that matches."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    V, P = 156032, 300
    g = torch.Generator().manual_seed(0)
    prompts = G.Prompts([torch.randint(0, 150000, (P,), generator=g) for _ in range(B)])
    phrases = [p[-3:].tolist() + [int(torch.randint(0, V, (1,), generator=g))] for p in prompts.input_ids]
    while len(phrases) < N:
        phrases.append(torch.randint(0, V, (4,), generator=g).tolist())
    sb = G.hotword_bias(phrases[:N], 2.0)
    plan = G.ConstraintPlan.build(sb, 0, [], V, DEV)
    rows = [dict(table="hotwords", phrases=N, sequences=len(sb), groups=int(plan.grp_tok.shape[0]))]
    text = DecoderConfig.from_dict(dict(model_type="qwen2", hidden_size=4096, intermediate_size=11008, num_attention_heads=32,
                                        num_key_value_heads=32, head_dim=128, num_hidden_layers=32, vocab_size=V,
                                        rope_theta=10000.0, rms_norm_eps=1e-5, tie_word_embeddings=False,
                                        initializer_range=0.02, eos_token_id=151643, pad_token_id=151643))
    torch.manual_seed(0)
    with torch.device(DEV):
        lm = PackedCausalLM(text)
    lm.post_init()
    lm = lm.to(torch.bfloat16).eval()
    keys = torch.arange(B, device=DEV)
    cache = G.KVCache.allocate(32, B, P + 4 * steps + 8, 32, 128, DEV)
    sample = lambda lg: F.sample_step(lg, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                                      1.1, True, 0.7, 50, 0.9, 1, [151643, 151645], 151643, row_key=keys)
    with torch.no_grad():
        logits = G._prefill(lm, None, prompts, cache, DEV)
        # the kernel alone, at the state right after the prefill (the matching phrases match); the logits drift by the
        # bias per call, which the kernel's time does not depend on
        edits = plan.edit_buffers(B)
        F.constrain_logits_(logits, cache.hist, cache.hist_len, plan)
        us_apply = _events_time(lambda: F.constrain_logits_(logits, cache.hist, cache.hist_len, plan), iters)
        us_emit = _events_time(lambda: F.constrain_logits_(logits, cache.hist, cache.hist_len, plan, edits=edits), iters)
        matched = int(edits[2].sum())
        sample(logits)

        def step_plain():
            sample(G.decode_logits(lm, cache))

        def step_plan():
            lg = G.decode_logits(lm, cache)
            F.constrain_logits_(lg, cache.hist, cache.hist_len, plan)
            sample(lg)
        step_plain(), step_plan()
        ab = [[_events_time(step_plain, steps - 2) / 1e3, _events_time(step_plan, steps - 2) / 1e3] for _ in range(2)]
    ms = min(a for a, _ in ab)
    rows.append(dict(kernel="tn_logits_constrain", B=B, V=V, sequences=len(sb), apply_us=round(us_apply, 2),
                     emit_us=round(us_emit, 2), ids_edited_per_call=matched))
    rows.append(dict(e2e="qwen2_audio_7b_decode_step", B=B, ms_per_step_without_plan=round(ms, 3),
                     ms_per_step_with_plan=round(min(b for _, b in ab), 3),
                     ab_runs_ms=[[round(a, 3), round(b, 3)] for a, b in ab],
                     constrain_share_of_step=round(us_apply / (ms * 1e3), 4)))
    del cache
    torch.cuda.empty_cache()
    # beam search: the step with and without the edit list, on fixed logits at the state after the prefill
    n_new = 4 * iters + 16
    st = G.BeamState.allocate(32, B, K, P + n_new, 32, 128, DEV)
    kw = dict(penalty=1.1, ngram=0, eos=[-1, -2], n_new=n_new, length_penalty=1.0, early_stopping=False)
    edits = plan.edit_buffers(B * K)
    with torch.no_grad():
        F.beam_step(G._prefill(lm, None, prompts, st, DEV, row_stride=K), st, **kw)
        logits = G.decode_logits(lm, st, table=st.src)

        def with_list():
            F.constrain_logits_(logits, st.hist, st.hist_len, plan, num_beams=K, edits=edits)
            F.beam_step(logits, st, edits=edits, **kw)
        F.beam_step(logits, st, **kw), with_list()
        ab = [[_events_time(lambda: F.beam_step(logits, st, **kw), iters), _events_time(with_list, iters)]
              for _ in range(2)]
        us_emit = _events_time(lambda: F.constrain_logits_(logits, st.hist, st.hist_len, plan, num_beams=K, edits=edits),
                               iters)
    rows.append(dict(kernel="tn_beam_step", B=B, K=K, V=V, beam_step_us=round(min(a for a, _ in ab), 2),
                     emit_plus_beam_step_edits_us=round(min(b for _, b in ab), 2), emit_alone_us=round(us_emit, 2),
                     ab_runs_us=[[round(a, 2), round(b, 2)] for a, b in ab]))
    return rows


def bench_token_scores(K, B, steps=32, iters=200):
    """tn_token_scores alone (history mode at the decode batch, token mode at 4096 rows) and inside the sampled decode
    step of Qwen2-Audio-7B's decoder (decode_logits + tn_sample_step + the scores, against the step without them, A/B
    twice in one process)."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    rows = []
    g = torch.Generator(device=DEV).manual_seed(0)
    for V in (128256, 152064):
        logits = (torch.randn(B, V, generator=g, device=DEV) * 4).to(torch.bfloat16)
        S = 64
        hist = torch.randint(0, V, (B, S), generator=g, device=DEV, dtype=torch.int32)
        hist_len = torch.full((B,), 40, dtype=torch.int32, device=DEV)
        r = dict(kernel="tn_token_scores", mode="history", B=B, V=V, MB_read_per_pass=round(B * V * 2 / 1e6, 2))
        for k in sorted({0, K}):
            out = G.TokenScores.buffers(B, S, k, DEV)
            F.token_scores_(logits, hist, hist_len, out, k)
            r[f"us_k{k}"] = round(_events_time(lambda: F.token_scores_(logits, hist, hist_len, out, k), iters), 2)
        rows.append(r)
        R = 4096
        big = (torch.randn(R, V, generator=g, device=DEV) * 4).to(torch.bfloat16)
        tok = torch.randint(0, V, (R,), generator=g, device=DEV, dtype=torch.int32)
        r = dict(kernel="tn_token_scores", mode="token", R=R, V=V)
        for k in sorted({0, K}):
            F.token_scores(big, tok, k)
            us = _events_time(lambda: F.token_scores(big, tok, k), 20)
            r[f"us_k{k}"], r[f"rows_per_s_k{k}"] = round(us, 1), round(R / us * 1e6)
            r[f"TBps_one_pass_k{k}"] = round(R * V * 2 / us / 1e6, 3)
        rows.append(r)
        del big
        torch.cuda.empty_cache()
    V, P = 156032, 300
    gc = torch.Generator().manual_seed(0)
    prompts = G.Prompts([torch.randint(0, 150000, (P,), generator=gc) for _ in range(B)])
    text = DecoderConfig.from_dict(dict(model_type="qwen2", hidden_size=4096, intermediate_size=11008, num_attention_heads=32,
                                        num_key_value_heads=32, head_dim=128, num_hidden_layers=32, vocab_size=V,
                                        rope_theta=10000.0, rms_norm_eps=1e-5, tie_word_embeddings=False,
                                        initializer_range=0.02, eos_token_id=151643, pad_token_id=151643))
    torch.manual_seed(0)
    with torch.device(DEV):
        lm = PackedCausalLM(text)
    lm.post_init()
    lm = lm.to(torch.bfloat16).eval()
    keys = torch.arange(B, device=DEV)
    cache = G.KVCache.allocate(32, B, P + 8 * steps + 8, 32, 128, DEV)
    out = G.TokenScores.buffers(B, cache.capacity, K, DEV)
    sample = lambda lg: F.sample_step(lg, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                                      1.1, True, 0.7, 50, 0.9, 1, [151643, 151645], 151643, row_key=keys)
    with torch.no_grad():
        sample(G._prefill(lm, None, prompts, cache, DEV))

        def step_plain():
            sample(G.decode_logits(lm, cache))

        def step_scored():
            lg = G.decode_logits(lm, cache)
            sample(lg)
            F.token_scores_(lg, cache.hist, cache.hist_len, out, K)
        step_plain(), step_scored()
        ab = [[_events_time(step_plain, steps - 2) / 1e3, _events_time(step_scored, steps - 2) / 1e3] for _ in range(2)]
        lg = G.decode_logits(lm, cache)
        us = _events_time(lambda: F.token_scores_(lg, cache.hist, cache.hist_len, out, K), iters)
    ms = min(a for a, _ in ab)
    rows.append(dict(e2e="qwen2_audio_7b_decode_step", B=B, V=V, k=K, ms_per_step_without_scores=round(ms, 3),
                     ms_per_step_with_scores=round(min(b for _, b in ab), 3),
                     ab_runs_ms=[[round(a, 3), round(b, 3)] for a, b in ab], token_scores_us=round(us, 2),
                     token_scores_share_of_step=round(us / (ms * 1e3), 4)))
    return rows


DECODER_WIDTHS = {      # (model_type, H, I, heads, kv heads, head_dim, layers, V) of the three decoders modelled above
    "llama_asr_1b": ("llama", 2048, 8192, 32, 8, 64, 16, 128256),
    "qwen2_audio_7b": ("qwen2", 4096, 11008, 32, 32, 128, 32, 156032),
    "kimi_audio_7b": ("qwen2", 3584, 18944, 28, 4, 128, 28, 168448),
}
COPY_RATE = 6.3e12      # bytes / s: the copy rate DESIGN.md §9 measures every byte bound against


def bench_decode_gemm(name, B, steps=24, iters=40):
    """TN_DECODE_GEMM own against lib, and the FP8 weight variant of the small-M kernel against both, at one decoder's
    widths: every product family of a decode step at M = 1, 12, 48, 64, 96, 128, 192, 256 (weights cycled through > 768 MB of
    bf16 copies and their FP8 codes, so no call finds its weights in L2 / MALL) — from 48 rows on with the mid-M kernel's
    bf16 and FP8 entries (csrc/gemm_midm.hip) beside the library route, and beside the small-M kernel up to its 128 rows —, then the whole step at B rows with the arms alternated
    lib, own, fp8, lib, own, fp8, .. inside this process (fp8: a copy of the model after `quantize_decoder_weights`), and
    the decoder weight bytes resident before and after."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G, library as L
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    kind, H, I, Nh, Nkv, D, layers, V = DECODER_WIDTHS[name]
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    bias = kind == "qwen2"
    rows = []

    def copies(*shapes):            # enough sets of the family's weights that a set has left the caches when its turn returns
        per = sum(n * k * 2 for n, k in shapes)
        return [[rnd(n, k) for n, k in shapes] for _ in range(max(2, min(48, -(-768 * 2 ** 20 // per))))]

    def timed(fn, sets):
        it = [0]

        def call():
            fn(sets[it[0] % len(sets)])
            it[0] += 1
        for _ in range(len(sets) + 2):      # every set and every shape warm before the window
            call()
        torch.cuda.synchronize()
        return _events_time(call, iters)

    with torch.no_grad():
        fp8_sets = {}
        fam_sets = {"qkv+rope": copies((Nh * D, H), (Nkv * D, H), (Nkv * D, H)), "o": copies((H, Nh * D)),
                    "gate/up+swiglu": copies((I, H), (I, H)), "down": copies((H, I)), "lm_head": copies((V, H))}
        # what one call costs the host and the queue with next to nothing to compute: a family at this figure is launch-bound
        F.DECODE_GEMM = "own"
        tiny = timed(lambda ws: F.linear_smallm(ws[0][:1], [(ws[0], None)]), [[rnd(16, 64)]] * 2)
        print(json.dumps(dict(decode_gemm=name, launch_floor_us=round(tiny, 2))), flush=True)
        for M in (1, 12, 48, 64, 96, 128, 192, 256):
            small, mid = M <= F.SMALLM_MAX_ROWS, M >= 48
            x, xi, xo = rnd(M, H), rnd(M, I), rnd(M, Nh * D)
            pos = torch.arange(M, device=DEV)[None] + 300
            cos, sin = F.rope_tables(pos, F.rope_inv_freq(D, 10000.0, device=DEV), torch.bfloat16)
            bs = [rnd(n) if bias else None for n in (Nh * D, Nkv * D, Nkv * D)]
            # own: the kernel's entry itself, whatever the router's row limit; lib: `linear_group` with the switch at lib
            pair = lambda inp, rope=None, b=(None,) * 3: ((lambda ws: F.linear_smallm(inp, list(zip(ws, b)), rope)),
                                                          (lambda ws: F.linear_group(inp, list(zip(ws, b)), rope=rope)))
            # the current route of `swiglu_mlp`: the node's library body at M % 8 == 0, else composed of the single ops
            lib_swiglu = (lambda ws: L.swiglu_fwd_t(torch.nn.functional.linear(x, ws[0]), torch.nn.functional.linear(x, ws[1]))) \
                if M % 8 == 0 else (lambda ws: F.swiglu(*F.linear_group(x, [(ws[0], None), (ws[1], None)])))
            fp8 = lambda inp, rope=None, b=(None,) * 3: (lambda ws: F.linear_smallm_fp8(inp, list(zip(ws, b)), rope))
            mids = lambda inp, rope=None, b=(None,) * 3: ((lambda ws: F.linear_midm(inp, list(zip(ws, b)), rope)),
                                                          (lambda ws: F.linear_midm_fp8(inp, list(zip(ws, b)), rope)))
            mid_fams = {"qkv+rope": mids(x, (cos, sin, D, (0, 1)), bs), "o": mids(xo), "down": mids(xi), "lm_head": mids(x),
                        "gate/up+swiglu": (lambda ws: F.swiglu_midm(x, *ws), lambda ws: F.swiglu_midm_fp8(x, *ws))}
            fams = {"qkv+rope": (*pair(x, (cos, sin, D, (0, 1)), bs), fp8(x, (cos, sin, D, (0, 1)), bs), x, (Nh + 2 * Nkv) * D),
                    "o": (*pair(xo), fp8(xo), xo, H),
                    "gate/up+swiglu": (lambda ws: F.swiglu_smallm(x, *ws), lib_swiglu, lambda ws: F.swiglu_smallm_fp8(x, *ws), x, I),
                    "down": (*pair(xi), fp8(xi), xi, H), "lm_head": (*pair(x), fp8(x), x, V)}
            F.DECODE_GEMM = "lib"
            for fam, (own_fn, lib_fn, fp8_fn, inp, n_out) in fams.items():
                sets = fam_sets[fam]
                if fam not in fp8_sets:
                    fp8_sets[fam] = [[F.quantize_weight_fp8(w) for w in ws] for ws in sets]
                nbytes = sum(w.numel() for w in sets[0]) * 2 + inp.numel() * 2 + M * n_out * 2
                nbytes8 = nbytes - sum(w.numel() for w in sets[0]) + 4 * sum(w.shape[0] for w in sets[0])
                if mid:         # every arm twice, alternated: lib, mid-M, mid-M FP8, (small-M FP8,) and again
                    arms = {"lib": (lib_fn, sets), "midm": (mid_fams[fam][0], sets), "midm_fp8": (mid_fams[fam][1], fp8_sets[fam])}
                    if small:
                        arms["smallm_fp8"] = (fp8_fn, fp8_sets[fam])
                    us = {a: [] for a in arms}
                    for _ in range(2):
                        for a, (fn, ws) in arms.items():
                            us[a].append(round(timed(fn, ws), 2))
                    rows.append(dict(decode_gemm=name, family=fam, M=M, bytes=nbytes, bytes_fp8=nbytes8,
                                     **{"us_" + a: v for a, v in us.items()},
                                     midm_over_lib=round(min(us["midm"]) / min(us["lib"]), 3)))
                    print(json.dumps(rows[-1]), flush=True)
                if not small:
                    continue
                us_own = timed(own_fn, sets)
                us_fp8 = timed(fp8_fn, fp8_sets[fam])
                us_lib = timed(lib_fn, sets)
                us_own2 = timed(own_fn, sets)                  # (the bf16 arm again: the spread the fp8 figure is read against)
                us_fp8_2 = timed(fp8_fn, fp8_sets[fam])
                rows.append(dict(decode_gemm=name, family=fam, M=M, bytes=nbytes, us_own=round(us_own, 2),
                                 tbps_own=round(nbytes / us_own / 1e6, 3), us_at_copy_rate=round(nbytes / COPY_RATE * 1e6, 2),
                                 us_lib=round(us_lib, 2), own_over_lib=round(us_own / us_lib, 3), bytes_fp8=nbytes8,
                                 us_fp8=round(us_fp8, 2), tbps_fp8=round(nbytes8 / us_fp8 / 1e6, 3),
                                 us_own_again=round(us_own2, 2), us_fp8_again=round(us_fp8_2, 2),
                                 fp8_over_own=round(us_fp8 / us_own, 3)))
                print(json.dumps(rows[-1]), flush=True)
        del fam_sets, fp8_sets
        torch.cuda.empty_cache()
        text = DecoderConfig.from_dict(dict(model_type=kind, hidden_size=H, intermediate_size=I, num_attention_heads=Nh,
                                            num_key_value_heads=Nkv, head_dim=D, num_hidden_layers=layers, vocab_size=V,
                                            rope_theta=10000.0, rms_norm_eps=1e-5, tie_word_embeddings=kind == "llama",
                                            initializer_range=0.02, eos_token_id=1, pad_token_id=1))
        torch.manual_seed(0)
        with torch.device(DEV):
            lm = PackedCausalLM(text)
        lm.post_init()
        lm = lm.to(torch.bfloat16).eval()
        prompts = G.Prompts([torch.randint(2, 100000, (300,)) for _ in range(B)])
        cache = G.KVCache.allocate(layers, B, 300 + 10 * steps + 8, Nkv, D, DEV)
        logits = G._prefill(lm, None, prompts, cache, DEV)
        greedy = lambda lg: F.greedy_step(lg, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                                          1.0, 0, -1, 1)
        greedy(logits)
        import copy
        lm8 = copy.deepcopy(lm)
        linear_bytes = lambda m: sum(p.numel() * p.element_size() for n, p in m.named_parameters()
                                     if "embed_tokens" not in n and p.dim() == 2)
        before = linear_bytes(lm8) + (lm8.lm_head.weight.numel() * 2 if kind == "llama" else 0)      # (a tied head counts once more)
        G.quantize_decoder_weights(lm8)
        after = sum(m.weight.codes.numel() + 4 * m.weight.scale.numel() for m in lm8.modules() if isinstance(m, G.Fp8Linear)) \
            + linear_bytes(lm8)
        arms = []
        for arm in ("lib", "own", "fp8") * 4:              # the first round warms the arms' shapes and is not reported
            F.DECODE_GEMM = "lib" if arm == "fp8" else arm
            m = lm8 if arm == "fp8" else lm
            greedy(G.decode_logits(m, cache))
            arms.append((arm, round(_events_time(lambda: greedy(G.decode_logits(m, cache)), steps) / 1e3, 3)))
        F.DECODE_GEMM = "lib"
    lib_ms, own_ms, fp8_ms = ([t for a, t in arms[3:] if a == arm] for arm in ("lib", "own", "fp8"))
    rows.append(dict(e2e=f"{name}_decode_step", B=B, layers=layers, ms_lib=lib_ms, ms_own=own_ms, ms_fp8=fp8_ms,
                     own_worst_beats_lib_best=max(own_ms) < min(lib_ms), fp8_worst_beats_own_best=max(fp8_ms) < min(own_ms),
                     decoder_linear_bytes_bf16=before, decoder_linear_bytes_fp8=after))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_decode_gemm_mxfp4(name, B, steps=24, iters=200):
    """The MXFP4 arm against the FP8 arm per call — every product family of a decode step at M = 1, 12, 48, 96 on the small-M
    kernel and M = 256 on the mid-M kernel, each arm twice, alternated, on weight sets that outgrow L2 / MALL — then the whole
    step at B rows with the arms alternated lib, own, fp8, mxfp4 (copies of the model after `quantize_decoder_weights`)."""
    import copy

    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    kind, H, I, Nh, Nkv, D, layers, V = DECODER_WIDTHS[name]
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    bias = kind == "qwen2"

    def timed(fn, sets):
        it = [0]

        def call():
            fn(sets[it[0] % len(sets)])
            it[0] += 1
        for _ in range(len(sets) + 2):
            call()
        torch.cuda.synchronize()
        return round(_events_time(call, iters), 2)

    with torch.no_grad():
        shapes = {"qkv+rope": ((Nh * D, H), (Nkv * D, H), (Nkv * D, H)), "o": ((H, Nh * D),), "gate/up+swiglu": ((I, H), (I, H)),
                  "down": ((H, I),), "lm_head": ((V, H),)}
        sets = {}
        for fam, sh in shapes.items():      # (the bf16 weights are dropped as soon as both sets of codes exist)
            n = max(2, min(48, -(-768 * 2 ** 20 // sum(a * b for a, b in sh))))
            ws = [[rnd(a, b) for a, b in sh] for _ in range(n)]
            sets[fam] = ([[F.quantize_weight_fp8(w) for w in s] for s in ws], [[F.quantize_weight_mxfp4(w) for w in s] for s in ws])
            del ws
        for M in (1, 12, 48, 96, 256):
            kern = "smallm" if M <= F.SMALLM_MAX_ROWS else "midm"
            x, xi, xo = rnd(M, H), rnd(M, I), rnd(M, Nh * D)
            pos = torch.arange(M, device=DEV)[None] + 300
            rope = (*F.rope_tables(pos, F.rope_inv_freq(D, 10000.0, device=DEV), torch.bfloat16), D, (0, 1))
            bs = [rnd(n) if bias else None for n in (Nh * D, Nkv * D, Nkv * D)]
            for fam, (inp, r, b) in {"qkv+rope": (x, rope, bs), "o": (xo, None, [None]), "gate/up+swiglu": (x, None, None),
                                     "down": (xi, None, [None]), "lm_head": (x, None, [None])}.items():
                def arm(fmt, inp=inp, r=r, b=b):
                    if b is None:
                        return lambda ws: getattr(F, f"swiglu_{kern}_{fmt}")(inp, *ws)
                    return lambda ws: getattr(F, f"linear_{kern}_{fmt}")(inp, list(zip(ws, b)), r)
                us = {"fp8": [], "mxfp4": []}
                for _ in range(2):
                    us["fp8"].append(timed(arm("fp8"), sets[fam][0]))
                    us["mxfp4"].append(timed(arm("mxfp4"), sets[fam][1]))
                elems = sum(a * b for a, b in shapes[fam])
                io = inp.numel() * 2 + M * (I if b is None else sum(a for a, _ in shapes[fam])) * 2
                b8, b4 = elems + 4 * sum(a for a, _ in shapes[fam]) + io, elems // 2 + elems // 32 + io
                print(json.dumps(dict(decode_gemm_mxfp4=name, kernel=kern, family=fam, M=M, bytes_fp8=b8, bytes_mxfp4=b4,
                                      us_fp8=us["fp8"], us_mxfp4=us["mxfp4"], tbps_mxfp4=round(b4 / min(us["mxfp4"]) / 1e6, 3),
                                      mxfp4_over_fp8=round(min(us["mxfp4"]) / min(us["fp8"]), 3),
                                      bytes_ratio=round(b4 / b8, 3))), flush=True)
        del sets
        torch.cuda.empty_cache()
        text = DecoderConfig.from_dict(dict(model_type=kind, hidden_size=H, intermediate_size=I, num_attention_heads=Nh,
                                            num_key_value_heads=Nkv, head_dim=D, num_hidden_layers=layers, vocab_size=V,
                                            rope_theta=10000.0, rms_norm_eps=1e-5, tie_word_embeddings=kind == "llama",
                                            initializer_range=0.02, eos_token_id=1, pad_token_id=1))
        torch.manual_seed(0)
        with torch.device(DEV):
            lm = PackedCausalLM(text)
        lm.post_init()
        lm = lm.to(torch.bfloat16).eval()
        cache = G.KVCache.allocate(layers, B, 300 + 20 * steps + 8, Nkv, D, DEV)
        logits = G._prefill(lm, None, G.Prompts([torch.randint(2, 100000, (300,)) for _ in range(B)]), cache, DEV)
        greedy = lambda lg: F.greedy_step(lg, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                                          1.0, 0, -1, 1)
        greedy(logits)
        models = {"lib": lm, "own": lm, "fp8": copy.deepcopy(lm), "mxfp4": copy.deepcopy(lm)}
        G.quantize_decoder_weights(models["fp8"], "fp8_e4m3")
        G.quantize_decoder_weights(models["mxfp4"], "mxfp4")
        code_bytes = lambda m: sum(w.codes.numel() + F._scales_of(w).numel() * F._scales_of(w).element_size()
                                   for w in (mod.weight for mod in m.modules() if isinstance(mod, (G.Fp8Linear, G.Mxfp4Linear))))
        ms = {a: [] for a in models}
        for rnd_i in range(4):              # the first round warms the arms' shapes and is not reported
            for a, m in models.items():
                F.DECODE_GEMM = "own" if a == "own" else "lib"
                greedy(G.decode_logits(m, cache))
                t = round(_events_time(lambda: greedy(G.decode_logits(m, cache)), steps) / 1e3, 3)
                if rnd_i:
                    ms[a].append(t)
        F.DECODE_GEMM = "lib"
    print(json.dumps(dict(e2e=f"{name}_decode_step", B=B, layers=layers, **{"ms_" + a: v for a, v in ms.items()},
                          mxfp4_over_fp8=round(min(ms["mxfp4"]) / min(ms["fp8"]), 3),
                          mxfp4_over_own=round(min(ms["mxfp4"]) / min(ms["own"]), 3),
                          code_bytes_fp8=code_bytes(models["fp8"]), code_bytes_mxfp4=code_bytes(models["mxfp4"]))), flush=True)


def bench_attn_extend(layers, rounds=5, iters=100):
    """tn_attn_extend per call at the rescoring shape (48 continuations of 32 rows behind 12 shared prompts of 750 rows) at
    both head geometries and at one 750-row turn behind an 8 192-row prefix; then `score_continuations` with and without
    `cache=` at the rescoring shape on the LlamaForASR-1B-width model, alternated in one process (median of `rounds`).
    bytes = the cache bytes the launch's workgroups read: per sequence, tiles x prefix_len x Nkv x D x 2 (K, V) x 2 bytes is
    what is ASKED of L2; `cache_bytes` counts every prefix once per sequence (what a one-tile-per-sequence kernel would read)
    and the rate is quoted on that."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    bf = dict(device=DEV, dtype=torch.bfloat16)
    for name, n_seq, n_new, P, B in (("rescoring", 48, 32, 750, 12), ("turn", 1, 750, 8192, 1)):
        for Nh, Nkv, D in ((32, 8, 64), (28, 4, 128)):
            T = n_seq * n_new
            q, kn, vn = (torch.randn(T, h, D, **bf) for h in (Nh, Nkv, Nkv))
            kc, vc = torch.randn(B, P, Nkv, D, **bf), torch.randn(B, P, Nkv, D, **bf)
            start = torch.arange(n_seq + 1, dtype=torch.int32, device=DEV) * n_new
            pre = torch.full((n_seq,), P, dtype=torch.int32, device=DEV)
            row = torch.arange(n_seq, dtype=torch.int32, device=DEV) % B
            call = lambda: F.attn_extend(q, kn, vn, kc, vc, start, pre, None, row)
            with torch.no_grad():
                for _ in range(10):
                    call()
                torch.cuda.synchronize()
                us = _events_time(call, iters)
            nbytes = n_seq * P * Nkv * D * 2 * 2
            tiles = n_seq * ((n_new + 15) // 16)
            yield dict(what="attn_extend", shape=name, sequences=n_seq, new_rows=n_new, prefix=P, Nh=Nh, Nkv=Nkv, D=D,
                       workgroups=tiles * Nkv, cache_bytes=nbytes, us=round(us, 2), tbps=round(nbytes / us / 1e6, 3),
                       tbps_asked_of_l2=round(nbytes * ((n_new + 15) // 16) / us / 1e6, 3))
    m, _ = _model(layers)
    g = torch.Generator().manual_seed(0)
    prompts = G.Prompts([torch.randint(0, 128000, (750,), generator=g) for _ in range(12)])
    conts = [torch.randint(0, 128000, (32,), generator=g) for _ in range(48)]
    rows = [i % 12 for i in range(48)]
    repeated = G.Prompts([prompts.input_ids[r] for r in rows])
    _, cache = G.generate(m, prompts, G.GenerationConfig(max_new_tokens=2), return_cache=True)
    packed = lambda: G.score_continuations(m, repeated, conts)
    cached = lambda: G.score_continuations(m, prompts, conts, cache=cache, cache_row=rows)
    times = {"packed": [], "cached": []}
    for i in range(rounds + 1):
        for label, fn in (("packed", packed), ("cached", cached)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i:                                   # (round 0 warms both up)
                times[label].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    yield dict(what="score_continuations", layers=layers, prompts=12, prompt_rows=750, continuations=48, rows_each=32,
               ms_packed=round(med["packed"], 2), ms_with_cache=round(med["cached"], 2),
               ms_packed_all=[round(t, 2) for t in times["packed"]], ms_with_cache_all=[round(t, 2) for t in times["cached"]])


def _alternate(calls, rounds=5, iters=50):
    """{label: fn} -> {label: median over `rounds` of the µs per call}, the labels alternated round by round in one process"""
    with torch.no_grad():
        for fn in calls.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                t[k].append(_events_time(fn, iters))
    return {k: round(sorted(v)[len(v) // 2], 2) for k, v in t.items()}


def _random_fp8(*shape):
    """codes without the two NaN patterns, scales 2^-4 .. 2^-1"""
    codes = torch.randint(0, 256, shape, device=DEV, dtype=torch.uint8) & 0xF7
    return codes, torch.exp2(-torch.randint(1, 5, shape[:-1], device=DEV).float())


def bench_kv_fp8(B, rounds=5):
    """The FP8 KV cache beside the bf16 kernels, alternated in one process (medians of `rounds`): tn_attn_decode(_fp8) at B
    rows behind 750 and 8 192 positions at both head geometries, tn_attn_extend(_fp8) at bench_attn_extend's two shapes,
    tn_kv_quantize at a 12 x 750-row prefill, the whole decode step at Qwen2-Audio-7B's widths, and the largest logit
    difference between an fp8 and a bf16 cache over one teacher-forced generation of a random-weight two-layer model.
    bytes: the cache bytes a call must read (K and V, codes and scales)."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    bf = dict(device=DEV, dtype=torch.bfloat16)
    geoms = ((32, 8, 64), (28, 4, 128))
    for L in (750, 8192):
        for Nh, Nkv, D in geoms:
            S = L + 1
            q, kn = torch.randn(B, Nh, D, **bf), torch.randn(B, Nkv, D, **bf)
            kc, vc = torch.randn(B, S, Nkv, D, **bf), torch.randn(B, S, Nkv, D, **bf)
            (k8, ks), (v8, vs) = _random_fp8(B, S, Nkv, D), _random_fp8(B, S, Nkv, D)
            cl = torch.full((B,), L - 1, dtype=torch.int32, device=DEV)
            us = _alternate({"bf16": lambda: F.attn_decode(q, kn, kn, kc, vc, cl),
                             "fp8": lambda: F.attn_decode_fp8(q, kn, kn, k8, v8, ks, vs, cl)}, rounds, 100)
            nb = B * L * Nkv * 2
            yield dict(what="attn_decode", B=B, L=L, Nh=Nh, Nkv=Nkv, D=D, us_bf16=us["bf16"], us_fp8=us["fp8"],
                       fp8_over_bf16=round(us["fp8"] / us["bf16"], 3), tbps_bf16=round(nb * 2 * D / us["bf16"] / 1e6, 3),
                       tbps_fp8=round(nb * (D + 4) / us["fp8"] / 1e6, 3))
    for name, n_seq, n_new, P, rows in (("rescoring", 48, 32, 750, 12), ("turn", 1, 750, 8192, 1)):
        for Nh, Nkv, D in geoms:
            T = n_seq * n_new
            q, kn, vn = (torch.randn(T, h, D, **bf) for h in (Nh, Nkv, Nkv))
            kc, vc = torch.randn(rows, P, Nkv, D, **bf), torch.randn(rows, P, Nkv, D, **bf)
            (k8, ks), (v8, vs) = _random_fp8(rows, P, Nkv, D), _random_fp8(rows, P, Nkv, D)
            (kn8, kns), (vn8, vns) = F.kv_quantize(kn), F.kv_quantize(vn)
            start = torch.arange(n_seq + 1, dtype=torch.int32, device=DEV) * n_new
            pre = torch.full((n_seq,), P, dtype=torch.int32, device=DEV)
            row = torch.arange(n_seq, dtype=torch.int32, device=DEV) % rows
            us = _alternate({"bf16": lambda: F.attn_extend(q, kn, vn, kc, vc, start, pre, None, row),
                             "fp8": lambda: F.attn_extend_fp8(q, kn8, vn8, kns, vns, k8, v8, ks, vs, start, pre, None, row),
                             "fp8_with_quantize": lambda: (F.kv_quantize(kn), F.kv_quantize(vn), F.attn_extend_fp8(
                                 q, kn8, vn8, kns, vns, k8, v8, ks, vs, start, pre, None, row))}, rounds, 50)
            yield dict(what="attn_extend", shape=name, sequences=n_seq, new_rows=n_new, prefix=P, Nh=Nh, Nkv=Nkv, D=D,
                       us_bf16=us["bf16"], us_fp8=us["fp8"], us_fp8_with_quantize=us["fp8_with_quantize"],
                       fp8_over_bf16=round(us["fp8"] / us["bf16"], 3))
    for Nh, Nkv, D in geoms + ((32, 32, 128),):
        x = torch.randn(12 * 750, Nkv, D, **bf)
        us = _alternate({"q": lambda: F.kv_quantize(x)}, rounds, 100)["q"]
        yield dict(what="kv_quantize", rows=12 * 750, Nkv=Nkv, D=D, us=us,
                   tbps_read_and_written=round(x.numel() * (3 + 4 / D) / us / 1e6, 3))
    # the largest logit difference over one teacher-forced greedy generation (random weights, LlamaForASR-1B widths, 2 layers)
    m, _ = _model(2)
    g = torch.Generator().manual_seed(0)
    prompts = G.Prompts([torch.randint(0, 128000, (n,), generator=g) for n in (300, 750, 520)])
    lens = [300, 750, 520]
    with torch.no_grad():
        caches = {d: G.KVCache.allocate(2, 3, 750 + 34, 8, 64, DEV, kv_dtype=d) for d in G.KV_CACHE_DTYPES}
        logits = {d: G._prefill(m.language_model, None, prompts, c, DEV).float() for d, c in caches.items()}
        worst, scale, flips = 0.0, 0.0, 0
        for _ in range(32):
            worst = max(worst, float((logits["bf16"] - logits["fp8_e4m3"]).abs().max()))
            scale = max(scale, float(logits["bf16"].abs().max()))
            tok = logits["bf16"].argmax(1).to(torch.int32)                   # both caches follow the bf16 run's tokens
            flips += int((logits["fp8_e4m3"].argmax(1) != tok).sum())
            for c in caches.values():
                c.hist.scatter_(1, c.hist_len.to(torch.int64)[:, None], tok[:, None])
                c.hist_len += 1
                c.cache_len += 1
            logits = {d: G.decode_logits(m.language_model, c).float() for d, c in caches.items()}
    yield dict(what="logit_difference_fp8_vs_bf16_cache", model="random weights, 2 layers, hidden 2048, 32 / 8 heads, D 64",
               prompts=lens, steps=32, max_abs_difference=round(worst, 4), largest_logit=round(scale, 3),
               argmax_flips=flips, of=32 * 3)
    del m, caches, logits
    # the whole decode step at Qwen2-Audio-7B's widths, B rows behind 750 and 8 192 cached positions (random cache contents)
    text = DecoderConfig.from_dict(dict(model_type="qwen2", hidden_size=4096, intermediate_size=11008, num_attention_heads=32,
                                        num_key_value_heads=32, head_dim=128, num_hidden_layers=32, vocab_size=156032,
                                        rope_theta=10000.0, rms_norm_eps=1e-5, tie_word_embeddings=False,
                                        initializer_range=0.02, eos_token_id=151643, pad_token_id=151643))
    torch.manual_seed(0)
    with torch.device(DEV):
        lm = PackedCausalLM(text)
    lm.post_init()
    lm = lm.to(torch.bfloat16).eval()
    for P in (750, 8192):
        caches = {}
        for d in G.KV_CACHE_DTYPES:
            c = G.KVCache.allocate(32, B, P + 8, 32, 128, DEV, kv_dtype=d)
            for i in range(32):
                if d == "bf16":
                    c.k[i].normal_(), c.v[i].normal_()
                else:
                    (c.k[i], c.k_scale[i]), (c.v[i], c.v_scale[i]) = _random_fp8(B, P + 8, 32, 128), _random_fp8(B, P + 8, 32, 128)
            c.hist_len.fill_(P + 1), c.cache_len.fill_(P)
            caches[d] = c
        us = _alternate({d: (lambda c=c: G.decode_logits(lm, c)) for d, c in caches.items()}, 3, 8)
        kv_gb = lambda d: round(B * P * 32 * 32 * 2 * (256 if d == "bf16" else 132) / 1e9, 2)
        yield dict(what="decode_step_qwen2_audio_7b_widths", B=B, prefix=P, ms_bf16=round(us["bf16"] / 1e3, 3),
                   ms_fp8=round(us["fp8_e4m3"] / 1e3, 3), fp8_over_bf16=round(us["fp8_e4m3"] / us["bf16"], 3),
                   cache_gb_bf16=kv_gb("bf16"), cache_gb_fp8=kv_gb("fp8_e4m3"))
        del caches


def bench_prefill_codes(name, rounds=2):
    """Per format and M: µs of one layer's seven products on the parent route (a: `_CODES_PREFILL_MAX_ROWS` = 256) and on the
    prefill kernel for codes (b: unbounded), each `rounds` times, alternated a b a b; b / a from the minima."""
    import touchnet_amd.functional as F
    kind, H, I, Nh, Nkv, D, _, _ = DECODER_WIDTHS[name]
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    shapes = ((Nh * D, H), (Nkv * D, H), (Nkv * D, H), (H, Nh * D), (I, H), (I, H), (H, I))
    elems = sum(a * b for a, b in shapes)
    bound = F._CODES_PREFILL_MAX_ROWS
    with torch.no_grad():
        for fmt, quant in (("fp8", F.quantize_weight_fp8), ("mxfp4", F.quantize_weight_mxfp4)):
            nsets = max(2, -(-512 * 2 ** 20 // (elems if fmt == "fp8" else elems // 2)))      # codes cycled past the 256 MB MALL
            sets = [[quant(rnd(a, b)) for a, b in shapes] for _ in range(nsets)]
            wbytes = elems + 4 * sum(a for a, _ in shapes) if fmt == "fp8" else elems // 2 + elems // 32
            for M in (257, 512, 1024, 2048, 4096, 8192):
                x, xo = rnd(M, H), rnd(M, Nh * D)
                pos = torch.arange(M, device=DEV)[None] % 750
                rope = (*F.rope_tables(pos, F.rope_inv_freq(D, 10000.0, device=DEV), torch.bfloat16), D, (0, 1))
                bs = [rnd(n) if kind == "qwen2" else None for n in (Nh * D, Nkv * D, Nkv * D)]
                it = [0]

                def layer():
                    q, k, v, o, wg, wu, wd = sets[it[0] % nsets]
                    it[0] += 1
                    F.linear_group(x, [(q, bs[0]), (k, bs[1]), (v, bs[2])], rope=rope)
                    F.linear_group(xo, [(o, None)])
                    F.swiglu_mlp(x, wg, wu, wd)
                flop = 2 * M * elems
                iters = max(10, min(400, int(2e14 / flop)))       # windows of 0.1 s and more
                us = {"a": [], "b": []}
                for _ in range(rounds):
                    for arm, rows in (("a", 256), ("b", 1 << 30)):
                        F._CODES_PREFILL_MAX_ROWS = rows
                        for _ in range(nsets + 1):
                            layer()
                        torch.cuda.synchronize()
                        us[arm].append(round(_events_time(layer, iters), 1))
                F._CODES_PREFILL_MAX_ROWS = bound
                b = min(us["b"])
                print(json.dumps(dict(prefill_codes=name, fmt=fmt, M=M, us_dequant_then_bf16=us["a"], us_codes_kernel=us["b"],
                                      b_over_a=round(b / min(us["a"]), 3), tflops_codes_kernel=round(flop / b / 1e6, 1),
                                      weight_tbps_codes_kernel=round(wbytes / b / 1e6, 3))), flush=True)
            del sets
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-hf", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--qwen2-audio-7b", action="store_true")
    ap.add_argument("--num-beams", type=int, default=0, help="K > 1: the beam-search measurements")
    ap.add_argument("--kimi-audio-7b", action="store_true")
    ap.add_argument("--hotwords", type=int, default=0, help="N > 0: tn_logits_constrain with N phrases x 4 prefixes")
    ap.add_argument("--token-scores", type=int, nargs="?", const=8, default=None, metavar="K",
                    help="tn_token_scores with k = 0 and k = K (default 8) alternatives")
    ap.add_argument("--decode-gemm", nargs="?", const="all", default=None, metavar="DECODER",
                    help="TN_DECODE_GEMM own against lib: per product family and per step (one of DECODER_WIDTHS, default all)")
    ap.add_argument("--decode-gemm-mxfp4", nargs="?", const="qwen2_audio_7b", default=None, metavar="DECODER",
                    help="the MXFP4 arms against the FP8 arms per call, and the whole step (profiles/decode_gemm_mxfp4_bench.log)")
    ap.add_argument("--prefill-codes", nargs="?", const="all", default=None, metavar="DECODER",
                    help="the prefill kernel for codes against dequantise + bf16 per layer (profiles/prefill_codes_bench.log)")
    ap.add_argument("--attn-extend", action="store_true",
                    help="tn_attn_extend per call and score_continuations with / without cache= (profiles/attn_extend_bench.log)")
    ap.add_argument("--kv-fp8", action="store_true",
                    help="the FP8 KV cache beside the bf16 kernels, alternated in one process (profiles/kv_fp8_bench.log)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs the MI355X")
    from touchnet_amd import build
    build.build()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0))), flush=True)
    if a.kv_fp8:
        for r in bench_kv_fp8(a.batch):
            print(json.dumps(r), flush=True)
        return
    if a.attn_extend:
        for r in bench_attn_extend(a.layers):
            print(json.dumps(r), flush=True)
        return
    if a.prefill_codes is not None:
        for name in (DECODER_WIDTHS if a.prefill_codes == "all" else [a.prefill_codes]):
            bench_prefill_codes(name)
        return
    if a.decode_gemm_mxfp4 is not None:
        bench_decode_gemm_mxfp4(a.decode_gemm_mxfp4, a.batch)
        return
    if a.decode_gemm is not None:
        for name in (DECODER_WIDTHS if a.decode_gemm == "all" else [a.decode_gemm]):
            bench_decode_gemm(name, a.batch)
        return
    if a.token_scores is not None:
        for r in bench_token_scores(a.token_scores, a.batch):
            print(json.dumps(r), flush=True)
        return
    if a.hotwords > 0:
        for r in bench_hotwords(a.hotwords, a.batch):
            print(json.dumps(r), flush=True)
        return
    if a.num_beams > 1:
        for r in bench_beams(a.num_beams, a.batch):
            print(json.dumps(r), flush=True)
        return
    if a.kimi_audio_7b:
        for r in bench_kimi_audio_7b(a.batch):
            print(json.dumps(r), flush=True)
        return
    if a.qwen2_audio_7b:
        for r in bench_qwen2_audio_7b(a.batch):
            print(json.dumps(r), flush=True)
        return
    for B, L in ((64, 8192), (12, 600)):
        for Nh, Nkv, D in ((32, 8, 64), (28, 4, 128)):
            r = bench_kernel(B, L, Nh, Nkv, D)
            print(json.dumps(r), flush=True)
    if not a.skip_e2e:
        for r in bench_e2e(a.layers, a.batch, a.new, a.skip_hf):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
