"""KV-cache decoding on one MI355X: tn_attn_decode per call (µs, achieved TB/s) and greedy ASR decoding end to end on
LlamaForASR-1B (random weights, eos unreachable: every run decodes max_new_tokens), against transformers' own bf16
generate() (sdpa, same knobs, same weights).  Prints one JSON object per measurement.

    python scripts/decode_bench.py [--skip-hf] [--layers 16] [--batch 12] [--new 256]
    python scripts/decode_bench.py --qwen2-audio-7b [--batch 12]
    python scripts/decode_bench.py --num-beams 4 [--batch 12]
    python scripts/decode_bench.py --kimi-audio-7b [--batch 12]
    python scripts/decode_bench.py --hotwords 1024 [--batch 12]
    python scripts/decode_bench.py --token-scores [K] [--batch 12]

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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs the MI355X")
    from touchnet_amd import build
    build.build()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0))), flush=True)
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
