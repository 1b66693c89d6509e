"""generation.extend and what is built on it — score_continuations(cache=), generate(past=), chunked prefill — against the
packed forward, on the tiny Llama (GQA, D 64) and Qwen2 (biases, D 128) of tests/test_generation_gpu.py.  The bound is that
file's cached-versus-packed bound: logits within 3e-2 of their scale (`scale`: the largest packed logit over the prompts'
last rows); a log-probability is a logit minus a log-sum-exp of logits, so it may move by twice that.  The top alternative
must be the same wherever the packed path's top-2 margin exceeds twice the observed difference."""
import functools

import pytest
import torch

from test_generation_gpu import DEV, _tiny_touch_audio

pytestmark = pytest.mark.gpu
KINDS = pytest.mark.parametrize("kind", ["llama", "qwen2"])


@functools.lru_cache(maxsize=None)
def _setup(kind):
    from touchnet_amd import generation as G
    m, _ = _tiny_touch_audio(kind, seed=21)
    m = m.to(DEV).to(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(3)
    draw = lambda lens: [torch.randint(4, 500, (n,), generator=g) for n in lens]
    prompts = G.Prompts(draw((70, 33, 97)))
    with torch.no_grad():
        c = m.language_model.config
        whole = G.KVCache.allocate(c.num_hidden_layers, 3, 97, c.num_key_value_heads, c.head_dim, DEV)
        logits = G._prefill(m.language_model, None, prompts, whole, DEV).float()
    return m, prompts, draw, logits, whole


def _judge(packed, cached, scale, what):       # (logp, alt_logp [.., 2], alt_id [.., 2]) of the same tokens, twice
    d_lp = float((packed[0] - cached[0]).abs().max())
    d_all = max(d_lp, float((packed[1] - cached[1]).abs().max()))
    print(f"measured: {what}: |d logp| {d_lp:.3g}, with alternatives {d_all:.3g}, bound {2 * 3e-2 * scale:.3g}")
    assert d_lp <= 2 * 3e-2 * scale
    sure = (packed[1][..., 0] - packed[1][..., 1] > 2 * d_all) & (packed[2][..., 0] >= 0)
    assert bool(sure.any()) and torch.equal(packed[2][..., 0][sure], cached[2][..., 0][sure])


@KINDS
def test_scores_behind_a_cache_equal_the_packed_scores(kind):
    from touchnet_amd import generation as G
    m, prompts, draw, logits, _ = _setup(kind)
    _, cache = G.generate(m, prompts, G.GenerationConfig(max_new_tokens=4), return_cache=True)
    conts, rows = draw((9, 0, 17, 5, 12)), [0, 1, 2, 0, 2]                   # more continuations than prompts, one empty
    a = G.score_continuations(m, G.Prompts([prompts.input_ids[r] for r in rows]), conts, k=2)
    b = G.score_continuations(m, prompts, conts, k=2, cache=cache, cache_row=rows)
    assert float(b.logp[1].abs().max()) == 0.0 and float(b.confidence[1]) == 1.0
    _judge((a.logp, a.alt_logp, a.alt_id), (b.logp, b.alt_logp, b.alt_id), float(logits.abs().max()), f"{kind} rescoring")


@KINDS
def test_a_second_turn_behind_the_cache_equals_one_generate_over_all_ids(kind):
    from touchnet_amd import generation as G
    m, prompts, draw, logits, _ = _setup(kind)
    cfg = G.GenerationConfig(max_new_tokens=5, top_alternatives=2)
    _, cache = G.generate(m, prompts, G.GenerationConfig(max_new_tokens=5), return_cache=True)
    ids2 = G.next_turn(cache, draw((6, 11, 3)), [3], 1)
    hist, kept = cache.hist.cpu(), cache.hist_len.tolist()
    whole = G.Prompts([torch.cat([hist[b, :kept[b] - 1].to(torch.int64), ids2.input_ids[b]]) for b in range(3)])
    got, gs = G.generate(m, ids2, cfg, past=cache, return_scores=True)
    ref, rs = G.generate(m, whole, cfg, return_scores=True)
    assert torch.equal(cache.cache_len, cache.hist_len - 1)
    n = min(got.shape[1], ref.shape[1])
    same = (got[:, :n] == ref[:, :n]).cumprod(1).bool()       # teacher-forced: the columns up to which both runs agree
    assert int(same.sum()) >= 3
    pick = lambda s: (s.logp[:, :n][same], s.alt_logp[:, :n][same], s.alt_id[:, :n][same])
    _judge(pick(rs), pick(gs), float(logits.abs().max()), f"{kind} second turn ({int(same.sum())} tokens)")


@KINDS
def test_prefill_in_two_chunks_gives_the_logits_of_one(kind):
    from touchnet_amd import generation as G
    m, prompts, _, ref, whole = _setup(kind)
    lm, c = m.language_model, m.language_model.config
    half = [int(t.numel()) // 2 for t in prompts.input_ids]
    with torch.no_grad():
        cache = G.KVCache.allocate(c.num_hidden_layers, 3, 50, c.num_key_value_heads, c.head_dim, DEV)     # extend grows it
        G._prefill(lm, None, G.Prompts([t[:h] for t, h in zip(prompts.input_ids, half)]), cache, DEV)
        h = G.extend(m, cache, range(3), [t[n:] for t, n in zip(prompts.input_ids, half)], prefix_len=half)
        got = lm.lm_head(h).float()
    err = (got - ref).abs().max(1).values
    print(f"measured: {kind} chunked prefill: logits differ by {float(err.max()):.3g} at scale {float(ref.abs().max()):.3g}")
    assert float(err.max()) < 3e-2 * float(ref.abs().max())
    sure = -torch.topk(ref, 2, dim=1).values.diff(dim=1)[:, 0] > 2 * err           # top-2 margin above the observed error
    assert torch.equal(got.argmax(1)[sure], ref.argmax(1)[sure])
    assert torch.equal(cache.hist_len, whole.hist_len) and torch.equal(cache.cache_len, whole.cache_len)
