"""tests/loss_reference.py is a reference and its budgets can fail: the restatements against torch.autograd in float64
(F.linear + F.cross_entropy(reduction="none") written out with the per-sentence normalisation) and against oracle.loss;
a bf16-storage / fp32-arithmetic emulation of the chunked lm_head + CE passes `check`; the same emulation with one
planted error each fails it.  No GPU."""
import pytest
import torch
import torch.nn.functional as TF

import loss_reference as R
from oracle import loss as oloss

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
NS, G = 7, 1.0 / 3.0
N, H, V, CHUNK = 300, 64, 2056, 128                    # the ragged all-library shape of the GPU test


def _close(a, b, what, rel=1e-12):
    a, b = a.to(F64).flatten(), b.to(F64).flatten()
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max()) / scale
    assert err <= rel, f"{what}: {err:.3e} of its largest element"


def _autograd(x_or_hw, lab, sl, g):
    """float64 autograd of g * sum(nll / sentence_lens) / num_sentence -> (nll, loss, gradients of the leaves)"""
    leaves = [t.detach().to(F64).requires_grad_(True) for t in x_or_hw]
    x = leaves[0] if len(leaves) == 1 else TF.linear(leaves[0], leaves[1])
    nll = TF.cross_entropy(x, lab, reduction="none", ignore_index=-100)
    loss = (nll / sl.to(F64)).sum() / NS
    (g * loss).backward()
    return nll.detach(), loss.detach(), [t.grad for t in leaves], x.detach()


def _kernel_rows(dtype):
    """rows with a label in the first / last column, ignored rows, a tie, -inf entries (index 0, a stripe, half the row)"""
    gen = torch.Generator().manual_seed(5)
    n, Vk = 12, 1003
    x = (3 * torch.randn(n, Vk, generator=gen)).to(dtype)
    lab = torch.randint(0, Vk, (n,), generator=gen)
    lab[0], lab[1], lab[4], lab[7] = 0, Vk - 1, -100, -100
    x[2, 9] = x[2, 700] = 40.0
    lab[2] = 9
    x[3, 0] = float("-inf")
    x[5, 256:512] = float("-inf")
    x[6, ::2] = float("-inf")
    x[7, 0] = float("-inf")                               # in an ignored row: never read
    lab[3], lab[5], lab[6] = 17, 600, 1
    sl = torch.randint(1, 10, (n,), generator=gen)
    return x, lab, sl


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ce_rows_is_float64_autograd_and_the_oracle(dtype):
    x, lab, sl = _kernel_rows(dtype)
    r = R.ce_rows(x, lab, sl, NS, G)
    nll, loss, (dx,), _ = _autograd([x], lab, sl, G)
    valid = lab != -100
    _close(r["nll"].value, nll, "nll")
    _close(r["lse"].value[valid], torch.logsumexp(x.to(F64), 1)[valid], "lse")
    _close(r["per_sample"].value, loss, "per_sample")
    _close(r["per_token"].value, nll.sum() / valid.sum(), "per_token")
    _close(r["dlogits"].value, dx, "dlogits")
    assert bool((r["dlogits"].value[~torch.isfinite(x)] == 0).all()) and bool((r["dlogits"].value[~valid] == 0).all())
    assert float(r["hit"].value[2]) == 1.0                                       # the tie: first index
    assert float(r["n_valid"].value) == float(valid.sum())
    # the oracle computes in fp32 whatever it is given (token_nll upcasts with .float()): held at that precision, 1e-5, not
    # at the 1e-12 of the float64 autograd above; its accuracy is exact
    ps, pt = oloss.cross_entropy_loss(x[None], lab[None], sl[None].float(), NS)
    _close(r["per_sample"].value, ps, "oracle per_sample", rel=1e-5)
    _close(r["per_token"].value, pt, "oracle per_token", rel=1e-5)
    assert float(oloss.accuracy(x[None], lab[None])) == pytest.approx(float(r["accuracy"].value), abs=1e-7)
    for k in ("lse", "nll", "dlogits", "per_sample"):
        assert bool(torch.isfinite(R.budget(r[k], dtype)).all()), k


def test_ce_stats_small_sum_and_nothing_labelled():
    n = 40
    lab = torch.arange(n)
    sl = torch.full((n,), 3)
    s = R.ce_stats(torch.full((n,), 1e-9), torch.ones(n), lab, sl, NS)
    assert float(s["per_token"].value) == 0.0 and float(s["per_sample"].value) > 0 and float(s["accuracy"].value) == 1.0
    none = torch.full((n,), -100)
    s = R.ce_stats(torch.zeros(n), torch.zeros(n), none, sl, NS)
    assert [float(s[k].value) for k in ("per_sample", "per_token", "accuracy", "n_valid")] == [0.0, 0.0, 0.0, 0.0]
    ps, pt = oloss.cross_entropy_loss(torch.randn(1, n, 4), none[None], sl[None].float(), NS)
    assert float(ps) == 0.0 and float(pt) == 0.0 and float(oloss.accuracy(torch.randn(1, n, 4), none[None])) == 0.0


@pytest.fixture(scope="module")
def case():
    h, w, lab, sl = R.fused_inputs(N, H, V, n_ignored=40, row0_labelled=True, seed=3)
    ref = R.fused_linear_ce(h, w, lab, sl, NS, G)
    return h, w, lab, sl, ref


def test_fused_linear_ce_is_float64_autograd_and_the_oracle(case):
    h, w, lab, sl, ref = case
    nll, loss, (dh, dw), x = _autograd([h, w], lab, sl, G)
    assert 8 < float(x.abs().max()) <= 16                   # logits of the magnitude the budget was made for
    _close(ref["nll"].value, nll, "nll")
    _close(ref["per_sample"].value, loss, "loss")
    _close(ref["dhidden"].value, dh, "d(hidden)")
    _close(ref["dweight"].value, dw, "d(weight)")
    assert bool((ref["dhidden"].value[lab == -100] == 0).all())
    ps, pt = oloss.cross_entropy_loss(x[None], lab[None], sl[None].float(), NS)
    _close(ref["per_sample"].value, ps, "oracle per_sample", rel=1e-5)
    _close(ref["per_token"].value, pt, "oracle per_token", rel=1e-5)
    assert float(oloss.accuracy(x[None], lab[None])) == pytest.approx(float(ref["accuracy"].value), abs=1e-7)


# ------------------------------------------------------------------------------------------------------ emulation
def _emulate(h, w, lab, sl, g, chunk, plant=None):
    """_FusedLinearCE with bf16 storage and fp32 arithmetic on the CPU, optionally with one planted error"""
    n, Vv = h.shape[0], w.shape[0]
    h32, w32 = h.float(), w.float()
    lab = lab.clone()
    if plant == "label+1":
        lab = torch.where(lab != -100, (lab + 1) % Vv, lab)
    if plant == "sentence_lens rolled":
        sl = sl.roll(1)
    if plant == "last row dropped":
        lab[n - 1] = -100
    valid = lab != -100
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    dh = torch.zeros(n, h.shape[1], dtype=BF16)
    dw = None
    nll, hit = torch.zeros(n), torch.zeros(n)
    for k, s in enumerate(range(0, n, chunk)):
        e = min(s + chunk, n)
        x = (h32[s:e] @ w32.t()).to(BF16).float()
        lse = torch.logsumexp(x, 1)
        vc = valid[s:e]
        nll[s:e] = torch.where(vc, lse - x.gather(1, safe[s:e, None])[:, 0], torch.zeros(()))
        hit[s:e] = ((x.argmax(1) == lab[s:e]) & vc).float()
        p = torch.exp(x - lse[:, None])
        p[torch.arange(e - s), safe[s:e]] -= 1.0
        dl = (p * (vc.float() / (sl[s:e].float() * NS))[:, None]).to(BF16).float()
        dh[s:e] = (dl @ w32).to(BF16)
        if plant == "chunk's d(weight) dropped" and k == 1:
            continue
        part = dl.t() @ h32[s:e]
        dw = part if dw is None else part + dw        # fp32 over the chunks, one rounding (through bf16 per chunk, three
        #                                               chunks sit AT the budget: 1.03 x here, not a dependable failure)
    v = valid.float()
    tot, cnt = (nll * v).sum(), v.sum()
    stats = dict(per_sample=(nll * v / sl.float()).sum() / NS, per_token=tot / cnt, accuracy=(hit * v).sum() / cnt,
                 n_valid=cnt)
    gb = torch.tensor(g, dtype=F32).to(BF16)
    return dict(nll=nll, dhidden=dh * gb, dweight=dw.to(BF16) * gb, **stats)


def _failures(got, ref):
    bad = []
    for k, dtype, r in (("nll", F32, 1), ("per_sample", F32, 1), ("per_token", F32, 1), ("accuracy", F32, 1),
                        ("n_valid", F32, 1), ("dhidden", BF16, 2), ("dweight", BF16, 2)):
        try:
            R.check(got[k], ref[k], dtype, f"emulated {k}", roundings=r)
        except AssertionError:
            bad.append(k)
    return bad


def test_emulated_fused_path_is_within_budget(case):
    h, w, lab, sl, ref = case
    assert _failures(_emulate(h, w, lab, sl, G, CHUNK), ref) == []


@pytest.mark.parametrize("plant, seen_in", [("label+1", "dweight"), ("sentence_lens rolled", "dhidden"),
                                            ("last row dropped", "dhidden"), ("chunk's d(weight) dropped", "dweight")])
def test_planted_errors_of_the_fused_path_fail(case, plant, seen_in):
    h, w, lab, sl, ref = case
    bad = _failures(_emulate(h, w, lab, sl, G, CHUNK, plant), ref)
    print(plant, "->", bad)
    assert seen_in in bad


def test_planted_tie_to_the_higher_index_fails():
    x, lab, sl = _kernel_rows(BF16)
    r = R.ce_rows(x, lab, sl, NS, G)
    last = x.shape[1] - 1 - x.float().flip(1).argmax(1)                          # the LAST index among equal values
    hit = ((last == lab) & (lab != -100)).float()
    with pytest.raises(AssertionError):
        R.check(hit, r["hit"], F32, "hit, tie to the higher index")
    stats = R.ce_stats(r["nll"].value, hit, lab, sl, NS)
    with pytest.raises(AssertionError):
        R.check(stats["accuracy"].value, r["accuracy"], F32, "accuracy, tie to the higher index")


def test_planted_reduction_that_stops_at_row_1024_fails():
    gen = torch.Generator().manual_seed(9)
    n = 1025
    nll = (torch.rand(n, generator=gen) * 5).float()
    hit = (torch.rand(n, generator=gen) < 0.5).float()
    lab = torch.arange(n)
    sl = torch.randint(1, 10, (n,), generator=gen)
    ref = R.ce_stats(nll, hit, lab, sl, NS)
    cut = R.ce_stats(nll[:1024], hit[:1024], lab[:1024], sl[:1024], NS)
    for k in ("per_sample", "n_valid"):
        with pytest.raises(AssertionError):
            R.check(cut[k].value, ref[k], F32, f"{k} of 1024 of 1025 rows")
    whole = {k: v.value.float() for k, v in ref.items()}                        # and the full sum in fp32 passes
    for k in whole:
        R.check(whole[k], ref[k], F32, f"{k} in fp32")
