"""Beam search on the MI355X: tn_attn_decode_beam bit for bit against tn_attn_decode on the gathered cache, tn_beam_step
against the torch restatement of transformers' `_beam_search` (tests/beam_search_reference.py, fp64), generate() with
num_beams > 1 against a reference loop built from existing parts, and the two command lines."""
import json
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_search_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------- (1) attention
@pytest.fixture(scope="module")
def attn_case():
    """R = 6 rows (B 2 x K 3), S_max 200: four key splits at every geometry below; lengths {0, 63, 64, 130}."""
    R, S = 6, 200
    lens = [0, 63, 64, 130, 130, 63]
    g = torch.Generator().manual_seed(3)
    table = torch.empty(R, S, dtype=torch.int32)
    for b in range(2):                                  # a valid table: any row of the same utterance, per position
        table[b * 3:b * 3 + 3] = torch.randint(0, 3, (3, S), generator=g, dtype=torch.int32) + b * 3
    # ... but never the slot a shorter row appends to in the same call (the entry point's precondition: that read would
    # race with the store): where a consulted entry names such a slot, the row reads its own
    for r in range(R):
        for r2, L2 in enumerate(lens):
            if L2 < lens[r] and int(table[r, L2]) == r2:
                table[r, L2] = r
    assert not any(L2 < lens[r] and int(table[r, L2]) == r2 for r in range(R) for r2, L2 in enumerate(lens))
    return R, S, lens, table


@pytest.mark.parametrize("Nh,Nkv,D", [(4, 1, 64), (14, 2, 128), (16, 1, 64)])
def test_attn_decode_beam_equals_attn_decode_on_the_gathered_cache(attn_case, Nh, Nkv, D):
    import touchnet_amd.functional as F
    from touchnet_amd import _C
    R, S, lens, table = attn_case
    assert _C.lib().tn_attn_decode_workspace_bytes(R, Nh, Nkv, D, S) > 0            # more than one key split
    g = torch.Generator().manual_seed(Nh + D)
    n, guard = R * S * Nkv * D, 4096
    kbuf = torch.randn(n + guard, generator=g).to(torch.bfloat16).to(DEV)
    vbuf = torch.randn(n + guard, generator=g).to(torch.bfloat16).to(DEV)
    kc, vc = kbuf[:n].view(R, S, Nkv, D), vbuf[:n].view(R, S, Nkv, D)
    q = torch.randn(R, Nh, D, generator=g).to(torch.bfloat16).to(DEV)
    kn = torch.randn(R, Nkv, D, generator=g).to(torch.bfloat16).to(DEV)
    vn = torch.randn(R, Nkv, D, generator=g).to(torch.bfloat16).to(DEV)
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    src = table.to(DEV)
    # entries at and behind cache_len are never consulted: make them invalid
    junk = src.clone()
    for r, L in enumerate(lens):
        junk[r, L:] = 1 << 20
    pos = torch.arange(S, device=DEV)
    kd = kc[src.long(), pos[None]].contiguous()                                   # the dense cache the table names
    vd = vc[src.long(), pos[None]].contiguous()
    k0, v0 = kbuf.clone(), vbuf.clone()
    with torch.no_grad():
        want = F.attn_decode(q, kn, vn, kd, vd, cl)
        got = F.attn_decode_beam(q, kn, vn, kc, vc, cl, junk)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the appended slot lands in row r; every other cache byte and the guard are untouched
    ke, ve = k0.clone(), v0.clone()
    for r, L in enumerate(lens):
        ke[:n].view(R, S, Nkv, D)[r, L] = kn[r]
        ve[:n].view(R, S, Nkv, D)[r, L] = vn[r]
    assert torch.equal(kbuf.view(torch.int16), ke.view(torch.int16))
    assert torch.equal(vbuf.view(torch.int16), ve.view(torch.int16))
    with torch.no_grad():
        again = F.attn_decode_beam(q, kn, vn, kc, vc, cl, junk)                   # (the slot now holds what it is given)
    assert torch.equal(again.view(torch.int16), got.view(torch.int16))
    # an out-of-range entry among the consulted ones: NaN for that row only, nothing else changes
    for bad_row, bad_pos, value in ((3, 129, R), (1, 0, -1)):
        poisoned = junk.clone()
        poisoned[bad_row, bad_pos] = value
        with torch.no_grad():
            o = F.attn_decode_beam(q, kn, vn, kc, vc, cl, poisoned)
        torch.cuda.synchronize()
        assert torch.isnan(o[bad_row].float()).all()
        keep = [r for r in range(R) if r != bad_row]
        assert torch.equal(o[keep].view(torch.int16), got[keep].view(torch.int16))
        assert torch.equal(kbuf.view(torch.int16), ke.view(torch.int16))


# ---------------------------------------------------------------------------------------------------- (2) step kernel
def _state_to(st, device, float_dtype):
    out = {}
    for k, v in st.items():
        out[k] = v.to(device=device, dtype=float_dtype if v.is_floating_point() else v.dtype).contiguous()
    return out


class _S:                                               # the attribute view functional.beam_step takes
    def __init__(self, d, K):
        self.__dict__.update(d)
        self.num_beams = K


def _spiked_logits(rows, V, n_spk, g, forced, dtype):
    """[rows, V]: a background in [-4, -2] and, per row, n_spk spikes on distinct ids, 8 down to 0 in equal steps of at
    least 0.28 (distinct in bf16 too); `forced[r]`: ids that get the largest spikes of row r, in that order."""
    x = torch.rand(rows, V, generator=g) * 2 - 4
    for r in range(rows):
        ids = list(dict.fromkeys(forced.get(r, [])))
        for i in torch.randperm(V, generator=g).tolist():
            if len(ids) == n_spk:
                break
            if i not in ids:
                ids.append(i)
        x[r, ids] = 8.0 - 0.5 * torch.arange(n_spk, dtype=torch.float32) * (16.0 / n_spk)
    return x.to(dtype)


def _mid_search_state(B, K, S, V, n_new, eos, g):
    """Utterances in the middle of a search, one per branch of the step (see the test)."""
    st = ref.new_state([[1]] * B, K, S)
    R = B * K
    for b in range(B):
        L = 9 + 2 * b                                   # history length (prompt 5 + generated), different per utterance
        for k in range(K):
            r = b * K + k
            h = torch.randint(0, V, (L,), generator=g)
            for e in eos:
                h[h == e] = (e + 7) % V
            h[L - 1] = h[3]                             # the bigram (h[3], h[4]) bans h[4]
            st["hist"][r, :L] = h.to(torch.int32)
            st["hist_len"][r], st["cache_len"][r] = L, L - 1
            st["src"][r, :L - 1] = torch.randint(0, K, (L - 1,), generator=g, dtype=torch.int32) + b * K
        st["run_score"][b * K:b * K + K] = -torch.sort(torch.rand(K, generator=g, dtype=torch.float64) * 3 + 2).values
        st["gen"][b] = L - 5
    return st


def _hold(st, b, K, scores, g, V):
    """Put finished hypotheses with the given scores (descending) into utterance b's set."""
    for j, s in enumerate(scores):
        r = b * K + j
        n = 6 + j
        st["fin_ids"][r, :n] = torch.randint(0, V, (n,), generator=g, dtype=torch.int32)
        st["fin_len"][r], st["fin_flag"][r], st["fin_score"][r] = n, 1, s


def _torch_fp32_error(logits, st, K, K_in, penalty, ngram):
    """max |acc of torch's fp32 path on the device - the fp64 restatement| over every finite candidate."""
    B = st["hist"].shape[0] // K
    worst = 0.0
    for b in range(B):
        for k in range(K_in):
            r = b * K + k
            h = st["hist"][r, :int(st["hist_len"][r])].tolist()
            row = logits[b * K_in + k]
            lp32 = torch.log_softmax(row.to(DEV).float(), -1)
            if penalty != 1.0:
                idx = torch.tensor(sorted(set(h)), device=DEV)
                lp32[idx] = torch.where(lp32[idx] < 0, lp32[idx] * penalty, lp32[idx] / penalty)
            base = float(st["run_score"][r].float())                       # the fp32 value both sides start from
            acc32 = (lp32 + base).cpu().double()
            acc64 = ref.processed_log_probs(row, h, penalty, 0, torch.float64) + base
            worst = max(worst, float((acc32 - acc64).abs().max()))
    return worst


def _compare(got, want, before, K, live, bound, all_hit):
    R = want["hist"].shape[0]
    B = R // K
    g = {k: v.cpu() for k, v in got.items()}
    for b in range(B):
        rows = slice(b * K, b * K + K)
        if not live[b]:                                 # frozen: byte-identical
            for k, v in before.items():
                sel = rows if v.shape[0] == R else (slice(b, b + 1) if v.shape[0] == B else slice(None))
                if k != "n_unfinished":
                    assert torch.equal(g[k][sel].view(torch.int32), v[sel].view(torch.int32)), (b, k)
            continue
        L, cl = int(want["hist_len"][b * K]), int(want["cache_len"][b * K])
        for k in ("hist_len", "cache_len", "out_ids", "out_parent", "fin_flag"):
            assert torch.equal(g[k][rows], want[k][rows]), (b, k, g[k][rows], want[k][rows])
        for k in ("gen", "unsat", "done"):
            assert int(g[k][b]) == int(want[k][b]), (b, k)
        assert torch.equal(g["hist"][rows, :L], want["hist"][rows, :L]), b
        assert torch.equal(g["src"][rows, :cl], want["src"][rows, :cl]), b
        for j in range(K):
            r = b * K + j
            if int(want["fin_flag"][r]):
                n = int(want["fin_len"][r])
                assert int(g["fin_len"][r]) == n and torch.equal(g["fin_ids"][r, :n], want["fin_ids"][r, :n]), (b, j)
                assert abs(float(g["fin_score"][r]) - float(want["fin_score"][r])) <= bound, (b, j)
            else:
                assert float(g["fin_score"][r]) == ref.EMPTY
            tol = 64.0 if all_hit[b] else bound         # (a beam that hit runs on at acc - 1e9: one fp32 ulp there is 64)
            assert abs(float(g["run_score"][r]) - float(want["run_score"][r])) <= tol, (b, j)
    assert int(g["n_unfinished"][0]) == int(want["n_unfinished"][0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,n_eos", [(2, 0), (3, 1), (8, 2)])
@pytest.mark.parametrize("V", [64, 1003, 151936])
def test_beam_step_matches_the_restatement(V, K, n_eos, dtype):
    """One step from hand-made states, penalty 1.5 / n-gram 2, every history holding a penalised and a banned spike.
    Utterances: 0 plain; 1 every one of the first K candidates is an eos; 2 K - 1 hypotheses held and one more arrives
    (full: done under early_stopping True); 3 a full set no running beam can beat (heuristic satisfied); 4 budget reached
    (every candidate hits); 5 done before the call (must stay byte-identical).  Then the first step after a prefill
    (K_in = 1).  Ids, parents, permuted history and table, finished slots and counters are exact.

    Scores: the bound is 4 x the error of torch's own fp32 path (log_softmax on the device, penalty, + running score)
    against the fp64 restatement on the same inputs, the factor covering another summation order.  It is measured in the
    test, per case; on the MI355X at these shapes: 1.1e-6 to 3.5e-6 (no trend in V: the running score, 2 to 5 in size,
    sets the rounding step), so bounds of 4.3e-6 to 1.4e-5.  The logits are drawn so that every decision of the
    restatement has a margin above the bound, which is asserted."""
    import touchnet_amd.functional as F
    g = torch.Generator().manual_seed(V + 10 * K + n_eos)
    eos = [5, 9][:n_eos]
    B, S, n_new, penalty, ngram = 6, 32, 20, 1.5, 2
    keep = max(2, 1 + n_eos) * K
    n_spk = min(keep + 4, V // 2)
    st = _mid_search_state(B, K, S, V, n_new, eos, g)
    _hold(st, 2, K, [-0.9 - 0.05 * j for j in range(K - 1)], g, V)
    _hold(st, 3, K, [-0.01 - 0.001 * j for j in range(K)], g, V)
    st["gen"][4] = n_new - 1
    st["done"][5], st["unsat"][5] = 1, 0
    _hold(st, 5, K, [-1.0], g, V)
    st["n_unfinished"][0] = B - 1
    forced = {}
    for b in range(B):
        for k in range(K):
            r = b * K + k
            h = st["hist"][r].tolist()
            forced[r] = [h[4], h[1]]                     # the banned id first (it would win), then a penalised one
            if eos and b in (1, 2):
                forced[r] = [eos[0]] + forced[r]         # 1: an eos on top of every row; 2: at least one among the first K
    if eos:                                              # 1: the K eos candidates come first whatever the running scores
        st["run_score"][K:2 * K] = -2.0 - 0.01 * torch.arange(K, dtype=torch.float64)
    logits = _spiked_logits(B * K, V, n_spk, g, forced, dtype)
    kw = dict(penalty=penalty, ngram=ngram, eos=eos, n_new=n_new, length_penalty=0.6, early_stopping=True)
    measured = _torch_fp32_error(logits, st, K, K, penalty, ngram)
    bound = 4 * measured
    print(f"V={V} K={K} n_eos={n_eos} {dtype}: torch fp32 path error {measured:.2e}, bound {bound:.2e}")
    dev = _state_to(st, DEV, torch.float32)
    before = {k: v.clone() for k, v in _state_to(st, "cpu", torch.float32).items()}
    live = [not int(d) for d in st["done"]]
    want = {k: v.clone() for k, v in st.items()}
    for k in ("run_score", "fin_score"):                 # the restatement starts from the fp32 values the kernel sees
        want[k] = want[k].float().double()
    margin = ref.beam_step(want, logits, K, dtype=torch.float64, **kw)
    assert margin > bound, (margin, bound)
    with torch.no_grad():
        F.beam_step(logits.to(DEV), _S(dev, K), **kw)
    torch.cuda.synchronize()
    all_hit = [b == 4 for b in range(B)]
    _compare(dev, want, before, K, live, bound, all_hit)
    # the branches were reached
    assert int(want["done"][4]) == 1 and int(want["done"][3]) == 1 and int(want["done"][0]) == 0
    assert all(int(want["fin_flag"][4 * K + j]) for j in range(K))
    if eos:
        assert all(int(want["fin_flag"][K + j]) for j in range(K)) and int(want["done"][2]) == 1
    assert int(want["n_unfinished"][0]) == (1 if eos else 3)

    # the first step after a prefill: one live row per utterance
    prompts = [torch.randint(0, V, (n,), generator=g).tolist() for n in (3, 7, 4)]
    for p in prompts:
        p[-1] = p[1]                                      # (a bigram to ban)
    st1 = ref.new_state(prompts, K, S)
    forced = {b: ([eos[0]] if eos and b == 1 else []) + [p[2], p[0]] for b, p in enumerate(prompts)}
    logits1 = _spiked_logits(3, V, n_spk, g, forced, dtype)
    kw1 = dict(kw, early_stopping="never", length_penalty=2.0)
    bound1 = 4 * _torch_fp32_error(logits1, st1, K, 1, penalty, ngram)
    dev1 = _state_to(st1, DEV, torch.float32)
    before1 = {k: v.clone() for k, v in _state_to(st1, "cpu", torch.float32).items()}
    margin1 = ref.beam_step(st1, logits1, K, dtype=torch.float64, **kw1)
    assert margin1 > bound1, (margin1, bound1)
    with torch.no_grad():
        F.beam_step(logits1.to(DEV), _S(dev1, K), **kw1)
    torch.cuda.synchronize()
    _compare(dev1, st1, before1, K, [True] * 3, bound1, [False] * 3)
    assert torch.equal(st1["out_parent"], torch.arange(3 * K, dtype=torch.int32) // K * K)
    if eos:
        assert int(st1["fin_flag"][K]) == 1 and int(st1["fin_len"][K]) == len(prompts[1]) + 1


# ---------------------------------------------------------------------------------------------------- (3) end to end
def _tiny_model(kind, seed):
    from touchnet_amd.models.llama import DecoderConfig
    from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
    if kind == "llama":
        text = dict(model_type="llama", hidden_size=256, intermediate_size=512, num_attention_heads=8, num_key_value_heads=2,
                    head_dim=64, num_hidden_layers=2, vocab_size=128, rope_theta=500000.0, tie_word_embeddings=True,
                    rms_norm_eps=1e-5)
    else:
        text = dict(model_type="qwen2", hidden_size=512, intermediate_size=768, num_attention_heads=4, num_key_value_heads=1,
                    head_dim=128, num_hidden_layers=2, vocab_size=128, rope_theta=1000000.0, tie_word_embeddings=False,
                    rms_norm_eps=1e-6)
    text.update(initializer_range=0.08, pad_token_id=1, bos_token_id=2, eos_token_id=3)
    cfg = TouchAudioConfig(text_config=DecoderConfig.from_dict(text), input_size=80, pad_token_id=1)
    torch.manual_seed(seed)
    m = TouchAudioForCausalLM(cfg)
    m.post_init()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_(0, 0.1)
    return m.to(DEV).to(torch.bfloat16).eval()


def reference_beam_search(model, prompts, cfg, K, eos):
    """Beam search from existing parts: dense [R, S] caches (KVCache), decode_logits without a table, HF's reorder_cache as
    index_select, and the restatement (fp64, on the CPU) on the device's logits.  -> (best hypotheses, smallest decision
    margin, per-step logits of the rows that were live)."""
    from touchnet_amd import generation as G
    lm, proj = G._parts(model)
    P = [int(t.numel()) for t in prompts.input_ids]
    B, n_new = len(P), cfg.new_tokens(max(P))
    R, S = B * K, max(P) + n_new
    c = lm.config
    small = G.KVCache.allocate(len(lm.model.layers), B, S, c.num_key_value_heads, c.head_dim, DEV)
    logits = G._prefill(lm, proj, prompts, small, DEV)
    rep = torch.arange(R, device=DEV) // K
    dense = G.KVCache.allocate(len(lm.model.layers), R, S, c.num_key_value_heads, c.head_dim, DEV)
    dense.k = [t.index_select(0, rep) for t in small.k]
    dense.v = [t.index_select(0, rep) for t in small.v]
    st = ref.new_state([t.tolist() for t in prompts.input_ids], K, S)
    kw = dict(K=K, penalty=float(cfg.repetition_penalty), ngram=int(cfg.no_repeat_ngram_size), eos=eos, n_new=n_new,
              length_penalty=float(cfg.length_penalty), early_stopping=cfg.early_stopping, dtype=torch.float64)
    margin, seen = math.inf, []
    for step in range(n_new):
        live = [b for b in range(B) if not int(st["done"][b])]
        if not live:
            break
        K_in = 1 if step == 0 else K
        seen.append((live, torch.stack([logits[b * K_in + k] for b in live for k in range(K_in)]).clone()))
        margin = min(margin, ref.beam_step(st, logits.float().cpu(), **kw))
        # reorder_cache: every layer's keys and values follow their beams (rows of done utterances stay)
        parent = torch.arange(R)
        for b in live:
            parent[b * K:b * K + K] = st["out_parent"][b * K:b * K + K].long()
        parent = parent.to(DEV)
        dense.k = [t.index_select(0, parent) for t in dense.k]
        dense.v = [t.index_select(0, parent) for t in dense.v]
        dense.hist = st["hist"].to(DEV)
        dense.hist_len = st["hist_len"].to(DEV)
        dense.cache_len = st["cache_len"].to(DEV)
        if step + 1 < n_new:
            logits = G.decode_logits(lm, dense)
    return ref.best_hypotheses(st, K, P), margin, seen


E2E = {  # (kind, run) -> model / prompt seed whose reference run has every decision margin above 1e-3 on the MI355X
         # (scanned seeds 0 .. 31: margins 1.3e-3, 4.2e-3, 3.0e-3, 1.6e-3; each run reaches an eos and the budget)
    ("llama", "penalties"): 17, ("llama", "growing"): 13, ("qwen2", "penalties"): 10, ("qwen2", "growing"): 23,
}


def e2e_config(run):
    from touchnet_amd.generation import GenerationConfig
    if run == "penalties":
        return GenerationConfig(max_new_tokens=24, repetition_penalty=1.5, no_repeat_ngram_size=2, num_beams=3)
    return GenerationConfig(max_new_tokens=24, repetition_penalty=1.0, no_repeat_ngram_size=0, num_beams=3,
                            length_penalty=0.6, early_stopping=True, cache_chunk=8)


def e2e_prompts(seed):
    from touchnet_amd import generation as G
    g = torch.Generator().manual_seed(1000 + seed)
    return G.Prompts([torch.randint(4, 128, (n,), generator=g) for n in (9, 4, 14)])


STEP_BOUND = 8.6e-6          # the step test's largest bound for bf16 logits at V <= 1003 (4 x torch's fp32 error), per step


@pytest.mark.parametrize("kind,run", list(E2E))
def test_generate_with_beams_equals_the_reference_loop(kind, run):
    """B 3 prompts of different lengths, K 3, 24 new tokens, vocab 128 with a reachable eos (id 3).  The reference loop
    reorders dense caches; the product follows the table, prefills once per utterance and (second run) grows caches,
    history and table mid-run.  Both see bit-identical logits; the reference's decisions all have margins > 1e-3 (two
    candidates of one row with the same bf16 logit are no decision of the arithmetic: beam_search_reference._gaps)."""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    K, eos = 3, [3]
    model = _tiny_model(kind, E2E[(kind, run)])
    cfg, prompts = e2e_config(run), e2e_prompts(E2E[(kind, run)])
    P = [int(t.numel()) for t in prompts.input_ids]
    with torch.no_grad():
        want, margin, seen = reference_beam_search(model, prompts, cfg, K, eos)
        print(f"{kind} / {run}: smallest decision margin {margin:.3g}; lengths {[len(w[0]) for w in want]}; "
              f"{len(seen)} steps")
        assert margin > 1e-3, margin
        # the product's own parts in lockstep: bit-identical logits at every step, for every live utterance
        lm, proj = G._parts(model)
        n_new = cfg.new_tokens(max(P))
        st = G.BeamState.allocate(len(lm.model.layers), 3, K, max(P) + n_new, lm.config.num_key_value_heads,
                                  lm.config.head_dim, DEV)
        kw = dict(penalty=cfg.repetition_penalty, ngram=cfg.no_repeat_ngram_size, eos=eos, n_new=n_new,
                  length_penalty=cfg.length_penalty, early_stopping=cfg.early_stopping)
        logits = G._prefill(lm, proj, prompts, st, DEV, row_stride=K)
        for step, (live, ref_logits) in enumerate(seen):
            K_in = 1 if step == 0 else K
            mine = torch.stack([logits[b * K_in + k] for b in live for k in range(K_in)])
            assert torch.equal(mine.view(torch.int16), ref_logits.view(torch.int16)), step
            F.beam_step(logits, st, **kw)
            if step + 1 < len(seen):
                logits = G.decode_logits(lm, st, table=st.src)
        assert int(st.n_unfinished.item()) == 0
        out, state = G.generate(model, prompts, cfg, return_cache=True)
    ids, scores = state.best(P, pad=1)
    assert torch.equal(ids, out)
    lock_ids, lock_scores = st.best(P, pad=1)
    for b, (w_ids, w_score) in enumerate(want):
        assert out[b, :len(w_ids)].tolist() == w_ids and (out[b, len(w_ids):] == 1).all(), (b, out[b].tolist(), w_ids)
        assert lock_ids[b, :len(w_ids)].tolist() == w_ids
        assert abs(float(scores[b]) - w_score) <= STEP_BOUND * len(seen), (b, float(scores[b]), w_score)
        assert float(lock_scores[b]) == float(scores[b])
    if run == "growing":
        assert state.capacity > max(P) + 8 and state.src.shape == state.hist.shape == state.fin_ids.shape
        assert state.k[0].shape[1] == state.capacity


# ---------------------------------------------------------------------------------------------------- (4) command lines
def _wav_list(tmp_path, secs, seed):
    rng = np.random.RandomState(seed)
    lines = []
    for i, sec in enumerate(secs):
        p = tmp_path / f"u{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes((rng.randn(int(sec * 16000)) * 3000).clip(-32768, 32767).astype(np.int16).tobytes())
        lines.append({"key": f"u{i}", "wav": str(p), "txt": "x"})
    (tmp_path / "data.list").write_text("".join(json.dumps(x) + "\n" for x in lines))
    return lines


def test_infer_asr_command_line_with_beams(tmp_path):
    from safetensors.torch import save_file
    from test_generation_gpu import _tiny_touch_audio
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
    lines = _wav_list(tmp_path, [1.3, 0.4, 2.1], 0)
    args = ["--model_path", str(ckpt), "--data_list", str(tmp_path / "data.list"), "--data_config",
            str(tmp_path / "data_config.json"), "--batch_size", "2", "--max_new_tokens", "12"]
    out = infer_asr.main(args + ["--output_dir", str(tmp_path / "out"), "--num_beams", "2", "--length_penalty", "0.8",
                                 "--early_stopping", "true"])
    recs = [json.loads(x) for x in open(out)]
    assert [json.loads(r["label"])["key"] for r in recs] == ["u0", "u1", "u2"]
    model = infer_asr.load_model(str(ckpt), DEV)
    dcfg = infer_asr.data_config(type("A", (), {"data_config": str(tmp_path / "data_config.json"),
                                                "model_path": str(ckpt)})(), model)
    feats = infer_asr.features([infer_asr.read_wav(x["wav"]) for x in lines], dcfg)
    cfg = GenerationConfig(max_new_tokens=12, num_beams=2, length_penalty=0.8, early_stopping=True)
    assert [r["predict_ids"] for r in recs] == transcribe(model, feats[:2], cfg) + transcribe(model, feats[2:], cfg)
    greedy = infer_asr.main(args + ["--output_dir", str(tmp_path / "out1")])      # the defaults are today's greedy search
    cfg1 = GenerationConfig(max_new_tokens=12)
    assert [json.loads(x)["predict_ids"] for x in open(greedy)] == \
        transcribe(model, feats[:2], cfg1) + transcribe(model, feats[2:], cfg1)


def test_infer_qwen2_audio_command_line_with_beams(tmp_path):
    from safetensors.torch import save_file
    from test_sampling_gpu import _tiny_qwen2_audio, _tiny_tokenizer, _wavs
    from touchnet_amd.bin import infer_qwen2_audio as cli
    from touchnet_amd.generation import GenerationConfig
    from touchnet_amd.models.qwen2_audio import inference_qwen2_audio as Q
    tok, _ = _tiny_tokenizer(tmp_path)
    hf, _, d, eos = _tiny_qwen2_audio(tok, seed=6)
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    save_file({k: v.contiguous() for k, v in hf.state_dict().items()}, str(ckpt / "model.safetensors"))
    (ckpt / "config.json").write_text(json.dumps(d))
    gen = {"repetition_penalty": 1.1, "eos_token_id": eos, "pad_token_id": eos[0]}    # (beam sampling is refused)
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
    out = cli.main(["--model_path", str(ckpt), "--data_list", str(tmp_path / "data.list"), "--instruct", "w3",
                    "--batch_size", "2", "--max_length", "400", "--max_new_tokens", "10", "--num_beams", "2",
                    "--output_dir", str(tmp_path / "out")])
    recs = [json.loads(x) for x in open(out)]
    model = cli.load_model(str(ckpt), DEV)
    cfg = GenerationConfig.from_hf(str(ckpt), max_length=400, num_beams=2)
    cfg.max_new_tokens = 10
    assert cfg.num_beams == 2 and not cfg.do_sample
    assert [r["predict"] for r in recs] == Q.transcribe(model, wavs, tok, "w3", cfg)[1]
