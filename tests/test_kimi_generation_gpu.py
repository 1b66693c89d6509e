"""Kimi-Audio decoding on the MI355X: tn_kimi_text_step against the plain-torch restatement
(tests/kimi_generate_reference.py), its draws' distribution and keying, and generate_kimi end to end — on the weights and the
recorded run of the reference's own generate() (tests/golden/kimi_generate.npz), against the packed forward that recomputes
the prefix, under cache growth and through the command line."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kimi_generate_reference as KR  # noqa: E402

fixture_model, cases = KR.fixture_model, KR.cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 3e-2        # of the logits' scale: the bound of test_reference_fixtures_gpu.py for kimi_decoder_dev on the device


def _state(hists, prompt_lens, S_hist=96, finished=()):
    B = len(hists)
    hist = torch.zeros(B, S_hist, dtype=torch.int32)
    for b, h in enumerate(hists):
        hist[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
    hl = torch.tensor([len(h) for h in hists], dtype=torch.int32)
    fin = torch.zeros(B, dtype=torch.int32)
    for b in finished:
        fin[b] = 1
    return dict(hist=hist, hl=hl, cl=hl - 1, fin=fin, nu=torch.tensor([B - len(finished)], dtype=torch.int32),
                pl=torch.tensor(prompt_lens, dtype=torch.int32))


def _run_both(logits, st, embed, penalty, W, T, k, eos, blank, uniforms=None, row_key=None, seed=0):
    """One step on the device and in the restatement from the same state -> (device state + x_next, reference state +
    x_next, reference tokens)."""
    import touchnet_amd.functional as F
    d = {n: v.clone().to(DEV) for n, v in st.items()}
    x = torch.full((logits.shape[0], embed.shape[1]), float("nan"), dtype=torch.bfloat16, device=DEV)
    F.kimi_text_step(logits.to(DEV), d["hist"], d["hl"], d["cl"], d["fin"], d["nu"], d["pl"], embed.to(DEV), x, penalty, W,
                     T, k, seed, eos, blank, blank, row_key=None if row_key is None else row_key.to(DEV),
                     uniforms=None if uniforms is None else uniforms.to(DEV))
    torch.cuda.synchronize()
    r = {n: v.clone() for n, v in st.items()}
    toks, xr = KR.text_step(logits, r["hist"], r["hl"], r["cl"], r["fin"], r["nu"], r["pl"], embed, penalty, W, T, k, eos,
                            blank, blank, uniforms)
    d = {n: v.cpu() for n, v in d.items()}
    d["x"], r["x"] = x.cpu(), xr
    return d, r, toks


def _assert_same(d, r, tag=""):
    for n in ("hist", "hl", "cl", "fin", "nu"):
        assert torch.equal(d[n], r[n]), (tag, n, d[n], r[n])
    assert torch.equal(d["x"].view(torch.int16), r["x"].view(torch.int16)), (tag, "x_next")


# ------------------------------------------------------------------------------------------- (1) kernel vs restatement
@pytest.mark.parametrize("B,V,H,dtype,W", [(1, 64, 64, torch.float32, 1), (3, 1003, 64, torch.bfloat16, 4),
                                           (12, 1003, 64, torch.float32, 16), (3, 1003, 64, torch.bfloat16, 64),
                                           (12, 168448, 64, torch.bfloat16, 16), (3, 64, 3584, torch.float32, 4),
                                           (12, 1003, 64, torch.bfloat16, 1), (1, 1003, 64, torch.float32, 64)])
def test_greedy_step_matches_the_restatement(B, V, H, dtype, W):
    g = torch.Generator().manual_seed(B * 1000 + V + W)
    eos, blank, pen = V - 3, V - 2, 1.1
    embed = (torch.randn(V, H, generator=g) * 0.5).to(torch.bfloat16)
    S = 2 * W + 40
    for trial in range(3):
        # generated counts around the threshold: W (penalty off), W + 1 (on), more
        gens = [(W, W + 1, W + 7, 0, W - 1 if W > 1 else 2)[(b + trial) % 5] for b in range(B)]
        prompts = [int(torch.randint(1, 20, (1,), generator=g)) for _ in range(B)]
        hists = [torch.randint(0, V, (p + n,), generator=g).tolist() for p, n in zip(prompts, gens)]
        logits = (torch.randn(B, V, generator=g) * 2.0).to(dtype)
        for b in range(B):                  # window ids among the largest logits, so that the penalty decides
            top = float(logits[b].float().max())
            for j, t in enumerate(hists[b][-min(3, len(hists[b])):]):
                logits[b, t] = top + 0.3 - 0.25 * j
        finished = [b for b in range(B) if (b + trial) % 7 == 6]
        d, r, toks = _run_both(logits, _state(hists, prompts, S, finished), embed, pen, W, 0.0, 5, eos, blank)
        _assert_same(d, r, (trial,))
        assert all(int(toks[b]) == blank for b in finished)


def test_planted_situations():
    """Every row is one situation; the expected token is stated here and must also be the restatement's."""
    V, H, W, pen, eos, blank = 1003, 64, 4, 1.1, 1000, 1001
    g = torch.Generator().manual_seed(7)
    embed = (torch.randn(V, H, generator=g) * 0.5).to(torch.bfloat16)
    for dtype in (torch.float32, torch.bfloat16):
        rows, hists, prompts, want, fin = [], [], [], [], []

        def add(values, hist, prompt, expect, finished=False, fill=-4.0):
            row = torch.full((V,), fill)
            for i, v in values.items():
                row[i] = v
            rows.append(row)
            hists.append(hist)
            prompts.append(prompt)
            want.append(expect)
            if finished:
                fin.append(len(rows) - 1)
        p = [900, 901, 902]                                          # a prompt: never penalised
        add({10: 5.0, 20: 4.75}, p + [10, 11, 12, 13], 3, 10)        # generated == W: the penalty is not in force yet
        add({10: 5.0, 20: 4.75}, p + [30, 10, 11, 12, 13], 3, 20)    # W + 1 generated, 10 in the window: 4.545 < 4.75
        add({10: 5.0, 20: 4.75}, p + [10, 30, 11, 12, 13], 3, 10)    # 10 was generated but has left the window
        add({10: 8.0, 20: 4.75}, p + [30, 10, 11, 12, 13], 3, 10)    # in the window and keeps the lead (7.27)
        add({900: 5.0, 20: 4.75}, p + [30, 31, 11, 12, 13], 3, 900)  # a prompt id is not penalised
        add({10: -1.0, 20: -1.0625}, p + [30, 10, 11, 12, 13], 3, 20, fill=-9.0)      # negative: -1.0 * 1.1 < -1.0625
        add({10: 5.0, 20: 4.25}, p + [30, 10, 10, 12, 10], 3, 10)    # three times in the window, penalised once (4.545)
        add({40: 3.5, 15: 3.5, 700: 3.5}, p + [30, 31, 11, 12, 13], 3, 15)            # exact tie: the lowest id
        # 2.0 / 1.1 = 1.81818.. rounds to bf16 1.8203125: id 10 ties with id 20 there and wins as the lower id; in fp32
        # it stays below and id 20 wins
        add({10: 2.0, 20: 1.8203125}, p + [30, 10, 11, 12, 13], 3, 10 if dtype == torch.bfloat16 else 20)
        add({10: 5.0}, p + [30, 10, 11, 12, 13], 3, blank, finished=True)             # a finished row emits the blank
        add({eos: 5.0, 20: 4.75}, p + [30, 31, 11, 12, 13], 3, eos)                   # eos at this step
        add({10: 5.0, 20: 4.75}, [900] * 16, 3, 10)                                   # a full history (S_hist = 16)
        logits = torch.stack(rows).to(dtype)
        st = _state(hists, prompts, 16, fin)
        d, r, toks = _run_both(logits, st, embed, pen, W, 0.0, 5, eos, blank)
        assert toks.tolist() == want, (dtype, toks.tolist(), want)
        _assert_same(d, r, (dtype,))
        B = len(rows)
        got = [int(d["hist"][b, len(hists[b])]) for b in range(B - 1)]
        assert got == want[:-1]
        assert d["hl"][-1] == 16 and d["cl"][-1] == 15                               # the full row did not advance
        assert torch.equal(d["x"][-1], (embed[10].float() + embed[blank].float()).to(torch.bfloat16))
        assert d["fin"].tolist() == [0] * 9 + [1, 1, 0] and int(d["nu"]) == B - 1 - 1
    # penalty <= 1 switches the penalty off whatever the window holds
    d, r, toks = _run_both(torch.stack(rows[1:2]), _state(hists[1:2], prompts[1:2], 16), embed, 1.0, W, 0.0, 5, eos, blank)
    assert toks.tolist() == [10]
    _assert_same(d, r)


def test_refusals():
    from touchnet_amd import _C
    import touchnet_amd.functional as F
    V, H, B = 100, 64, 2
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    lg = torch.zeros(B, V, device=DEV)
    emb = torch.zeros(V, H, dtype=torch.bfloat16, device=DEV)
    x = torch.zeros(B, H, dtype=torch.bfloat16, device=DEV)
    good = lambda: [i32(B, 8), i32(B), i32(B), i32(B), i32(1), i32(B), emb, x]
    F.kimi_text_step(lg, *good(), eos=1, blank=2)
    for kw in (dict(window=0), dict(window=65), dict(top_k=65), dict(top_k=-1), dict(penalty=0.0), dict(penalty=-2.0),
               dict(temperature=0.5, top_k=0), dict(blank=V), dict(blank=-1), dict(audio_token=V)):
        with pytest.raises(_C.KernelError, match="-22"):
            F.kimi_text_step(lg, *good(), **{"eos": 1, "blank": 2, **kw})
    with pytest.raises(_C.KernelError, match="-22"):                                  # H not a multiple of 8
        F.kimi_text_step(lg, *good()[:6], torch.zeros(V, 60, dtype=torch.bfloat16, device=DEV),
                         torch.zeros(B, 60, dtype=torch.bfloat16, device=DEV), eos=1, blank=2)
    with pytest.raises(_C.KernelError, match="-22"):                                  # V beyond the kernel's bitmap
        F.kimi_text_step(torch.zeros(1, 262145, device=DEV), i32(1, 8), i32(1), i32(1), i32(1), i32(1), i32(1),
                         torch.zeros(262145, 8, dtype=torch.bfloat16, device=DEV),
                         torch.zeros(1, 8, dtype=torch.bfloat16, device=DEV), eos=1, blank=2)
    with pytest.raises(_C.KernelError, match="prompt_len"):
        F.kimi_text_step(lg, i32(B, 8), i32(B), i32(B), i32(B), i32(1), i32(B + 1), emb, x, eos=1, blank=2)
    with pytest.raises(_C.KernelError, match="embed"):
        F.kimi_text_step(lg, *good()[:6], emb.float(), x, eos=1, blank=2)
    with pytest.raises(_C.KernelError, match="uniforms"):
        F.kimi_text_step(lg, *good(), eos=1, blank=2, uniforms=torch.zeros(B, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------- (2) sampled mode
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_injected_uniforms_draw_the_restatements_token(k, dtype):
    V, H, B, W, pen, T = 1003, 64, 12, 4, 1.1, 0.8
    g = torch.Generator().manual_seed(100 + k)
    embed = (torch.randn(V, H, generator=g) * 0.5).to(torch.bfloat16)
    prompts = [3] * B
    hists = [torch.randint(0, V, (3 + 6,), generator=g).tolist() for _ in range(B)]
    logits = (torch.randn(B, V, generator=g) * 1.5).to(dtype)
    for b in range(B):
        logits[b, hists[b][-1]] = float(logits[b].float().max()) + 0.2             # a window id among the candidates
    logits[0, 50] = logits[0, 60] = float(logits[0].float().max()) + 1.0            # tied candidates: the lower id first
    uni = torch.zeros(B)
    for b in range(B):
        row = KR.penalised(logits[b], KR.window_of(torch.tensor(hists[b]), len(hists[b]), 3, W, pen), pen)
        edges = torch.cat([torch.zeros(1, dtype=torch.float64), KR.boundaries(row, T, k)])
        width = edges[1:] - edges[:-1]
        pick = [j for j in range(width.numel()) if float(width[j]) > 4e-3]          # room for 1e-3 on either side
        j = pick[b % len(pick)]
        uni[b] = float(edges[j] + (0.25 + 0.5 * ((b * 7) % 3) / 2) * width[j])
        assert min(abs(float(uni[b]) - float(e)) for e in edges[1:-1].tolist() + [-1.0]) >= 1e-3
    d, r, toks = _run_both(logits, _state(hists, prompts), embed, pen, W, T, k, V - 1, V - 2, uniforms=uni)
    _assert_same(d, r, (k, dtype))


def test_seeded_draws_follow_the_distribution_and_are_keyed():
    from scipy.stats import chi2
    import touchnet_amd.functional as F
    V, N, H, W, pen, T = 4096, 20000, 64, 2, 1.2, 0.9
    g = torch.Generator().manual_seed(1)
    row = torch.randn(V, generator=g) * 2.0
    hist0 = [3, 17, 5, int(row.argmax())]                                            # prompt of 1, 3 generated > W
    embed = torch.zeros(V, H, dtype=torch.bfloat16, device=DEV)
    for k in (5, 20, 64):
        pr = KR.penalised(row, KR.window_of(torch.tensor(hist0), 4, 1, W, pen), pen)
        cv, ci = KR.candidates(pr, k)
        w = torch.exp((cv - torch.logsumexp(pr.double(), 0)) / T)
        probs = torch.zeros(V, dtype=torch.float64).index_add_(0, ci, w / w.sum())
        st = {n: v.to(DEV) for n, v in _state([hist0] * N, [1] * N, 8).items()}
        keys = torch.arange(N, dtype=torch.int64, device=DEV) * 7919 + 11
        x = torch.empty(N, H, dtype=torch.bfloat16, device=DEV)
        F.kimi_text_step(row.to(DEV)[None].expand(N, V).contiguous(), st["hist"], st["hl"], st["cl"], st["fin"], st["nu"],
                         st["pl"], embed, x, pen, W, T, k, 1234, -1, 0, row_key=keys)
        tok = st["hist"][:, len(hist0)].cpu().to(torch.int64)
        counts = torch.bincount(tok, minlength=V).double()
        support = probs > 0
        assert bool((counts[~support] == 0).all())
        exp, obs = probs[support] * N, counts[support]
        rare = exp < 5                                                               # pool the rare categories into one
        e = torch.cat([exp[~rare], exp[rare].sum()[None]]) if rare.any() else exp
        o = torch.cat([obs[~rare], obs[rare].sum()[None]]) if rare.any() else obs
        stat = float(((o - e) ** 2 / e.clamp_min(1e-12)).sum())
        pval = float(chi2.sf(stat, max(1, e.numel() - 1)))
        print(f"top_k {k}: chi2 {stat:.1f}, p {pval:.3g}")
        assert pval > 1e-3
    # keying: the same (seed, row_key, step) draws the same token under any permutation; another seed changes the draws
    B, V2 = 64, 8192
    logits = torch.randn(B, V2, generator=g)
    keys = torch.randint(0, 2 ** 40, (B,), generator=g)
    hists = [[int(t) for t in torch.randint(0, V2, (int(n),), generator=g)] for n in torch.randint(4, 40, (B,), generator=g)]
    emb2 = torch.zeros(V2, H, dtype=torch.bfloat16, device=DEV)

    def draw(perm, seed):
        hs = [hists[i] for i in perm.tolist()]
        st = {n: v.to(DEV) for n, v in _state(hs, [1] * B, 64).items()}
        x = torch.empty(B, H, dtype=torch.bfloat16, device=DEV)
        F.kimi_text_step(logits[perm].to(DEV), st["hist"], st["hl"], st["cl"], st["fin"], st["nu"], st["pl"], emb2, x, 1.1,
                         2, 1.0, 20, seed, -1, 0, row_key=keys[perm].to(DEV))
        return torch.tensor([int(st["hist"][i, len(h)]) for i, h in enumerate(hs)])
    ident = torch.arange(B)
    a = draw(ident, 99)
    perm = torch.randperm(B, generator=g)
    assert torch.equal(a[perm], draw(perm, 99))
    assert int((a != draw(ident, 100)).sum()) > B // 4


def test_a_step_repeats_bit_for_bit():
    import touchnet_amd.functional as F
    V, H, B, W = 168448, 3584, 12, 16
    g = torch.Generator().manual_seed(5)
    gd = torch.Generator(device=DEV).manual_seed(5)
    logits = torch.randn(B, V, generator=gd, device=DEV).to(torch.bfloat16)
    embed = (torch.randn(V, H, generator=gd, device=DEV) * 0.1).to(torch.bfloat16)
    hists = [torch.randint(0, V, (30 + b,), generator=g).tolist() for b in range(B)]
    outs = []
    for T, k in ((0.0, 5), (0.8, 5)):
        for _ in range(2):
            st = {n: v.to(DEV) for n, v in _state(hists, [5] * B, 64).items()}
            x = torch.empty(B, H, dtype=torch.bfloat16, device=DEV)
            F.kimi_text_step(logits, st["hist"], st["hl"], st["cl"], st["fin"], st["nu"], st["pl"], embed, x, 1.1, W, T, k, 3,
                             V - 1, V - 2)
            outs.append((st["hist"].clone(), st["hl"].clone(), x.clone()))
        assert all(torch.equal(a, b) for a, b in zip(outs[-1], outs[-2]))
        tok = outs[-1][0].gather(1, torch.tensor([[len(h)] for h in hists], device=DEV))[:, 0].long()
        assert torch.equal(outs[-1][2], (embed[tok].float() + embed[V - 2].float()).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------- (3) the reference's run
def _case_prompts(g, c):
    from touchnet_amd.models.kimi_audio.inference_kimi_audio import KimiPrompts
    text, audio = torch.tensor(g[f"{c}/text_ids"]), torch.tensor(g[f"{c}/audio_ids"])
    return KimiPrompts(text_ids=list(text), audio_ids=list(audio))


def _kimi_cfg(g, W, **kw):
    from touchnet_amd.generation import KimiGenerationConfig
    blank, eos, _, max_new = (int(x) for x in g["special"])
    return KimiGenerationConfig(text_repetition_window_size=W, max_new_tokens=max_new, kimia_text_blank=blank,
                                kimia_text_eos=eos, **kw)


def test_fixture_teacher_forced_and_free_running(golden):
    """The fixture's weights in bf16 on the device, teacher-forced with the reference's raw tokens, then free-running.
    Observed on the MI355X: logits within 5.7e-3 / 4.0e-3 / 4.5e-3 / 8.6e-3 of their scale (b1_w16, b1_w4, b2_w16, b2_w4;
    bound 3e-2), 2 near-tie steps of 166 (one each in the two window-16 cases), free-running cases b1_w4 and b2_w4."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    from touchnet_amd.models.kimi_audio import inference_kimi_audio as KI
    g = golden("kimi_generate.npz")
    blank, eos, offset, max_new = (int(x) for x in g["special"])
    m = fixture_model(g).to(DEV).to(torch.bfloat16)
    E = m.model.embed_tokens.weight.detach()
    lm = KI._TextDecoder(m)
    total = near_total = 0
    clean = []
    with torch.no_grad():
        for c in cases(g):
            W = int(g[f"{c}/window"])
            raw, ref_logits, margin, live = (torch.tensor(g[f"{c}/{n}"]) for n in ("raw", "logits", "margin", "live"))
            B, steps = raw.shape
            scale = float(ref_logits.abs().max())
            prompts = _case_prompts(g, c)
            lens = [int(t.numel()) for t in prompts.text_ids]
            cache = G.KVCache.allocate(len(lm.model.layers), B, max(lens) + steps, m.config.num_key_value_heads,
                                       m.config.head_dim, DEV)
            pl = torch.tensor(lens, dtype=torch.int32, device=DEV)
            x = torch.empty(B, m.config.hidden_size, dtype=torch.bfloat16, device=DEV)
            logits = G._prefill(lm, None, G.Prompts(input_ids=list(prompts.text_ids)), cache, DEV,
                                KI.kimi_embedder(m, prompts))
            worst, near = 0.0, 0
            for s in range(steps):
                # the device's own choice, on a copy of the state; the state itself advances with the reference's token
                st = [t.clone() for t in (cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished)]
                F.kimi_text_step(logits, *st, pl, E, x, 1.1, W, 0.0, 5, 0, eos, blank, blank)
                got = st[0].gather(1, cache.hist_len.long()[:, None])[:, 0].cpu()
                diff = (logits.float().cpu() - ref_logits[s]).abs().amax(1)               # [B]
                for b in range(B):
                    if not bool(live[b, s]):
                        assert int(got[b]) == blank == int(raw[b, s])                    # a finished row
                        continue
                    total += 1
                    worst = max(worst, float(diff[b]) / scale)
                    if float(margin[s, b]) > 2 * float(diff[b]):
                        assert int(got[b]) == int(raw[b, s]), (c, s, b, int(got[b]), int(raw[b, s]))
                    else:
                        near += 1
                tok = raw[:, s].to(DEV)
                cache.hist.scatter_(1, cache.hist_len.long()[:, None], tok.to(torch.int32)[:, None])
                cache.hist_len += 1
                cache.cache_len += 1
                cache.finished.copy_((~live[:, s]) | (raw[:, s] == eos))
                if s + 1 < steps:
                    logits = G.decode_logits(lm, cache, inputs_embeds=(E[tok].float() + E[blank].float()).to(torch.bfloat16))
            print(f"{c}: {steps} steps, logits within {worst:.2e} of their scale (bound {LOGIT_TOL}), {near} near-tie steps")
            assert worst < LOGIT_TOL, (c, worst)
            near_total += near
            if near == 0:
                clean.append(c)
        print(f"near-tie steps: {near_total} of {total}; free-running cases: {clean}")
        assert near_total <= 0.05 * total
        for c in clean:
            out, got_raw, _ = KI.generate_kimi(m, _case_prompts(g, c), _kimi_cfg(g, int(g[f"{c}/window"]), check_every=4),
                                               return_raw=True)
            B = len(out)
            assert out == [g[f"{c}/returned{b}"].tolist() for b in range(B)], c
            n = g[f"{c}/raw"].shape[1]
            assert got_raw.shape[1] >= n and torch.equal(got_raw[:, :n].cpu(), torch.tensor(g[f"{c}/raw"]).long())
            assert bool((got_raw[:, n:] == blank).all())                     # steps between the last eos and the host's check


def test_cache_growth_gives_the_tokens_of_full_preallocation(golden):
    from touchnet_amd.models.kimi_audio import inference_kimi_audio as KI
    g = golden("kimi_generate.npz")
    m = fixture_model(g).to(DEV).to(torch.bfloat16)
    c = "b2_w16"
    W = int(g[f"{c}/window"])
    a = KI.generate_kimi(m, _case_prompts(g, c), _kimi_cfg(g, W, cache_chunk=1024), return_raw=True)
    b = KI.generate_kimi(m, _case_prompts(g, c), _kimi_cfg(g, W, cache_chunk=8), return_raw=True)
    assert a[2].capacity == 24 + 40 and b[2].capacity == 24 + 40 and a[0] == b[0] and torch.equal(a[1], b[1])
    small = KI.generate_kimi(m, _case_prompts(g, c), _kimi_cfg(g, W, cache_chunk=8, check_every=1), return_raw=True)
    assert small[0] == a[0]


# ------------------------------------------------------------------------------------------- (4) with the audio-input side
def _tiny_whisper_kimi(frames, mels, vocab=1024, begin=5, end=6, seed=0):
    from touchnet_amd.models.kimi_audio import KimiAudioConfig, KimiAudioPackedForCausalLM
    kw = dict(vocab_size=vocab, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
              num_key_value_heads=1, head_dim=64, kimia_mimo_layers=1, kimia_mimo_transformer_from_layer_index=0,
              kimia_token_offset=512, kimia_media_begin=begin, kimia_media_end=end, use_whisper_feature=True,
              kimia_adaptor_input_dim=512, initializer_range=0.1,
              speech_encoder_config=dict(num_mel_bins=mels, d_model=128, encoder_layers=1, encoder_attention_heads=2,
                                         encoder_ffn_dim=128, max_source_positions=frames // 2),
              speech_tokenizer_config=dict(num_mel_bins=mels, d_model=128, encoder_attention_heads=2, encoder_ffn_dim=128,
                                           max_source_positions=frames // 2, pooling_position=2, quantize_position=2,
                                           quantize_vocab_size=64, quantize_causal_block_size=50))
    torch.manual_seed(seed)
    m = KimiAudioPackedForCausalLM(KimiAudioConfig(**kw))
    m.post_init()
    return m.to(DEV).to(torch.bfloat16).eval(), kw


def test_cached_decoding_equals_the_packed_forward_that_recomputes_the_prefix():
    from touchnet_amd.generation import KimiGenerationConfig
    from touchnet_amd.models.kimi_audio import inference_kimi_audio as KI
    m, _ = _tiny_whisper_kimi(320, 16)
    blank, eos, W, steps = 7, 8, 4, 24
    # a head that speaks (a Gaussian head leaves most steps without a clear margin): row j holds the embedding of the id
    # before it in its group of three, so an input carrying embed[t] scores t's successor far above the rest and the row
    # walks in circles through its own penalty window; the blank's group has no row, and the layers are damped so that the
    # input token leads the residual stream
    with torch.no_grad():
        E0 = m.model.embed_tokens.weight
        pred = torch.arange(1023) // 3 * 3 + (torch.arange(1023) + 2) % 3
        m.lm_head.weight[:1023].copy_(E0[pred.to(DEV)])
        m.lm_head.weight[6:9].zero_()
        for layer in m.model.layers:
            layer.self_attn.o_proj.weight.mul_(0.05)
            layer.mlp.down_proj.weight.mul_(0.05)
    g = torch.Generator().manual_seed(2)
    valid = [160, 72]                                                    # two clips of different length: 20 and 9 ids
    text, audio = [], []
    for L in valid:
        n = KI.audio_token_count(L)
        a = [blank, blank, blank, 5] + [blank] * n + [6, 9, 10, 11]
        audio.append(torch.tensor(a))
        text.append(torch.cat([torch.randint(12, 500, (3,), generator=g), torch.full((len(a) - 3,), blank)]))
    prompts = KI.KimiPrompts(text_ids=text, audio_ids=audio, whisper_input_features=torch.randn(2, 16, 320, generator=g),
                             valid_frames=valid)
    cfg = KimiGenerationConfig(text_repetition_window_size=W, max_new_tokens=steps, kimia_text_blank=blank,
                               kimia_text_eos=eos, check_every=100)
    _, raw, _ = KI.generate_kimi(m, prompts, cfg, return_raw=True)
    raw = raw.cpu()
    assert raw.shape == (2, steps)
    # ONE packed causal forward over prompt + generated inputs: position n - 1 + s holds the logits of step s
    E = m.model.embed_tokens.weight.detach()
    lens = [int(t.numel()) for t in text]
    T = sum(lens)
    Tp = (T + 255) // 256 * 256
    ids = torch.zeros(Tp, dtype=torch.int64)
    ids[:T] = torch.cat(text)
    with torch.no_grad():
        pe = KI.kimi_embedder(m, prompts)(ids.to(DEV), lens, Tp)
        rows, pos, doc, keep, o = [], [], [], [], 0
        for b, n in enumerate(lens):
            gen = (E[raw[b, :-1].to(DEV)].float() + E[blank].float()).to(torch.bfloat16)
            start = sum(r.shape[0] for r in rows)
            rows += [pe[o:o + n], gen]
            pos.append(torch.arange(n + steps - 1))
            doc.append(torch.full((n + steps - 1,), b + 1))
            keep.append(torch.arange(steps) + start + n - 1)
            o += n
        x = torch.cat(rows)
        pad = (x.shape[0] + 255) // 256 * 256 - x.shape[0]
        x = torch.cat([x, x.new_zeros(pad, x.shape[1])])
        pos = torch.cat(pos + [torch.zeros(pad, dtype=torch.int64)]).to(DEV)
        doc = torch.cat(doc + [torch.zeros(pad, dtype=torch.int64)]).to(torch.int32).to(DEV)
        h, _ = m.model(x[None], position_ids=pos[None], attention_mask=doc[None], keep_rows=torch.cat(keep).to(DEV))
        logits = m.lm_head(h[0]).view(2, steps, -1).cpu()
    scale = float(logits.float().abs().max())
    clear = checked = 0
    for b in range(2):
        hist = text[b].tolist()
        for s in range(steps):
            if s and int(raw[b, s - 1]) == eos:
                break
            row = KR.penalised(logits[b, s], KR.window_of(torch.tensor(hist), len(hist), lens[b], W, 1.1), 1.1)
            top = row.float().topk(2).values
            checked += 1
            if float(top[0] - top[1]) > 2 * LOGIT_TOL * scale:           # beyond twice the logits' own error bound
                clear += 1
                assert KR.choose(row, 0.0, 0) == int(raw[b, s]), (b, s)
            hist.append(int(raw[b, s]))
    print(f"cached vs recomputed: {clear} of {checked} steps at clear margins")
    assert clear >= checked // 2


def _wavs(seconds, seed):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy((rng.randn(int(s * 16000)) * 3000).astype(np.int16)) for s in seconds]


def test_infer_kimi_audio_command_line(tmp_path):
    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import AutoTokenizer, PreTrainedTokenizerFast
    from touchnet_amd.bin import infer_kimi_audio as cli
    from touchnet_amd.generation import KimiGenerationConfig
    from touchnet_amd.models.kimi_audio import inference_kimi_audio as KI
    vocab = {"[UNK]": 0}
    for i in range(1, 290):
        vocab[f"w{i}"] = i
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    special = ["<|im_kimia_user_msg_start|>", "<|im_kimia_text_blank|>", "<|im_media_begin|>", "<|im_media_end|>",
               "<|im_kimia_speech_ct_id|>", "<|im_msg_end|>", "<|im_kimia_assistant_msg_start|>", "<|im_kimia_text_eos|>"]
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="[UNK]", additional_special_tokens=special)
    ckpt = tmp_path / "ckpt"
    fast.save_pretrained(str(ckpt))
    t = AutoTokenizer.from_pretrained(str(ckpt))
    sid = {s: int(t.convert_tokens_to_ids(s)) for s in special}
    m, kw = _tiny_whisper_kimi(3000, 128, begin=sid["<|im_media_begin|>"], end=sid["<|im_media_end|>"], seed=4)
    save_file({k: v.contiguous() for k, v in m.state_dict().items()}, str(ckpt / "model.safetensors"))
    (ckpt / "config.json").write_text(json.dumps(kw))
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
    out = cli.main(["--model_path", str(ckpt), "--data_list", str(tmp_path / "data.list"), "--instruct", "w3 w4",
                    "--batch_size", "2", "--max_new_tokens", "12", "--output_dir", str(tmp_path / "out")])
    assert os.path.basename(out) == "part_1_of_1"
    recs = [json.loads(x) for x in open(out)]
    assert [json.loads(r["label"])["key"] for r in recs] == ["u0", "u1"]
    cfg = KimiGenerationConfig(max_new_tokens=12, kimia_text_blank=sid["<|im_kimia_text_blank|>"],
                               kimia_text_eos=sid["<|im_kimia_text_eos|>"])
    model = cli.load_model(str(ckpt), DEV)
    ids, texts = KI.transcribe(model, wavs, t, "w3 w4", cfg, row_keys=torch.tensor([0, 1]))
    assert [r["predict"] for r in recs] == texts
    assert all(len(r) <= 12 and all(x < kw["kimia_token_offset"] for x in r) for r in ids)
