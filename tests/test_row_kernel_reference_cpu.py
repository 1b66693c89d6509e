"""tests/row_kernel_reference.py against torch's own operations in float64 (no GPU): with float64 inputs the restated
roundings are the identity, so every restatement must reproduce torch.nn.functional / oracle.nn / torch.optim to
float64 accuracy, gradients (by autograd) included.  This is what entitles the GPU tests to use it as the reference."""
import math

import pytest
import torch
import torch.nn.functional as TF

import row_kernel_reference as R
from oracle import nn as onn

F64 = torch.float64


def _rand(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F64) * scale + shift


def _same(a, b, tol=1e-11):
    a, b = a.detach(), b.detach()
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), err


@pytest.mark.parametrize("residual", [False, True])
def test_rmsnorm_restatement_is_torch_rms_norm_with_its_gradients(residual):
    rows, H, eps = 7, 24, 1e-5
    x, res = _rand(rows, H, seed=1, shift=0.3).requires_grad_(), (_rand(rows, H, seed=2) if residual else None)
    w = (1 + 0.5 * _rand(H, seed=3)).requires_grad_()
    dy, dres = _rand(rows, H, seed=4), _rand(rows, H, seed=5)
    h = x + res if residual else x
    if residual:
        h.retain_grad()
    y = TF.rms_norm(h, (H,), w, eps)
    torch.autograd.backward([y, h] if residual else [y], [dy, dres] if residual else [dy])
    f = R.rmsnorm_fwd(x, res, w, eps, F64)
    _same(f["y"].value, y)
    _same(f["rstd"].value, torch.rsqrt((h * h).mean(-1) + eps))
    if residual:
        _same(f["h"].value, h)
    else:
        assert f["h"] is None
    b = R.rmsnorm_bwd(dy, h, w, f["rstd"].value, dres if residual else None, F64)
    _same(b["dh"].value, x.grad)
    _same(b["dw"].value, w.grad)
    assert bool((b["dh"].scale >= b["dh"].value.abs() * (1 - 1e-12)).all())       # scale bounds the cancelled result
    assert bool((b["dw"].scale >= b["dw"].value.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shift", [0.0, 100.0])
def test_layernorm_restatement_is_torch_layer_norm_with_its_gradients(residual, shift):
    rows, H, eps = 6, 20, 1e-5
    x, res = _rand(rows, H, seed=1, shift=shift).requires_grad_(), (_rand(rows, H, seed=2) if residual else None)
    w, b = (1 + 0.5 * _rand(H, seed=3)).requires_grad_(), (0.3 * _rand(H, seed=6)).requires_grad_()
    dy, dres = _rand(rows, H, seed=4), _rand(rows, H, seed=5)
    h = x + res if residual else x
    y = TF.layer_norm(h, (H,), w, b, eps)
    torch.autograd.backward([y, h] if residual else [y], [dy, dres] if residual else [dy])
    f = R.layernorm_fwd(x, res, w, b, eps, F64)
    _same(f["y"].value, y, 1e-10)
    _same(f["mean"].value, h.mean(-1))
    _same(f["rstd"].value, torch.rsqrt(h.var(-1, unbiased=False) + eps), 1e-10)
    g = R.layernorm_bwd(dy, h, w, f["mean"].value, f["rstd"].value, dres if residual else None, F64)
    _same(g["dh"].value, x.grad, 1e-9)
    _same(g["dw"].value, w.grad, 1e-10)
    _same(g["db"].value, b.grad)
    assert bool((f["y"].scale >= f["y"].value.abs() * (1 - 1e-12)).all())
    assert bool((g["dh"].scale >= g["dh"].value.abs() * (1 - 1e-9)).all())


def test_swiglu_and_gelu_restatements_are_torch_with_their_gradients():
    g = torch.cat((_rand(500, seed=1, scale=3.0), torch.tensor([0.0, -0.0, 5.0, -5.0, 13.5, -13.5, 20.0, -20.0], dtype=F64)))
    g = g.requires_grad_()
    u, do = _rand(508, seed=2).requires_grad_(), _rand(508, seed=3)
    out = TF.silu(g) * u
    out.backward(do)
    _same(R.swiglu_fwd(g, u, F64).value, out)
    dg, du = R.swiglu_bwd(do, g, u, F64)
    _same(dg.value, g.grad)
    _same(du.value, u.grad)
    x = g.detach().clone().requires_grad_()
    y = TF.gelu(x)
    y.backward(do)
    _same(R.gelu_fwd(x).value, y)
    _same(R.gelu_bwd(do, x).value, x.grad)
    # the lower tail keeps its relative accuracy (1 + erf cancels there; the restatement goes through erfc)
    t = R.gelu_fwd(torch.tensor([-12.0], dtype=F64)).value
    assert float(t) == pytest.approx(-12.0 * 0.5 * math.erfc(12.0 / math.sqrt(2.0)), rel=1e-12)


def test_roundings_are_restated_where_the_kernels_round():
    """bf16 inputs: silu and xhat are rounded to bf16 before the second product, and only there"""
    g = torch.tensor([1.2345, -0.777, 3.3], dtype=torch.bfloat16)
    u = torch.tensor([0.9, 1.7, -2.2], dtype=torch.bfloat16)
    silu = (g.double() * torch.sigmoid(g.double())).float().bfloat16().double()
    assert torch.equal(R.swiglu_fwd(g, u, torch.bfloat16).value, silu * u.double())
    x = torch.tensor([[1.0, -2.0, 3.0, 0.5]], dtype=torch.bfloat16)
    w = torch.tensor([1.5, 0.5, -1.25, 2.0], dtype=torch.bfloat16)
    f = R.rmsnorm_fwd(x, None, w, 1e-5, torch.bfloat16)
    xhat = (x.double() * f["rstd"].value[:, None]).float().bfloat16().double()
    assert torch.equal(f["y"].value, w.double() * xhat)
    res = torch.tensor([[0.0039, 1.0, 1.0, 1.0]], dtype=torch.bfloat16)
    f2 = R.rmsnorm_fwd(x, res, w, 1e-5, torch.bfloat16)
    h = (x.double() + res.double()).float().bfloat16().double()                    # 1.0039 is no bf16 number
    assert float(h[0, 0]) == 1.0
    assert float(f2["rstd"].value) == pytest.approx(float(torch.rsqrt((h * h).mean() + 1e-5)), rel=1e-14)


def test_rope_restatement_is_the_oracle():
    n, hq, hk, D = 9, 3, 2, 16
    pos = torch.tensor([0, 1, 2, 3, 40, 41, 4095, 65535, 131071])
    inv = onn.rope_inv_freq(D, 10000.0)
    c, s = R.rope_table(pos, inv, 1.0)
    oc, osn = onn.rope_cos_sin(pos[None], inv, torch.float32)                      # [1, n, D]: both halves alike
    # the oracle takes cos / sin in fp32 of the same fp32 angle
    assert float((c.value - oc[0, :, :D // 2].double()).abs().max()) < 1e-6
    assert float((s.value - osn[0, :, :D // 2].double()).abs().max()) < 1e-6
    c5, _ = R.rope_table(pos, inv, 0.5)
    _same(c5.value, 0.5 * c.value)
    q, k = _rand(n, hq, D, seed=1).requires_grad_(), _rand(n, hk, D, seed=2).requires_grad_()
    cc, ss = torch.cat((c.value, c.value), -1)[None], torch.cat((s.value, s.value), -1)[None]
    oq, ok = onn.apply_rope(q.transpose(0, 1)[None], k.transpose(0, 1)[None], cc, ss)    # [1, heads, n, D]
    _same(R.rope_apply(q, c.value, s.value).value, oq[0].transpose(0, 1))
    _same(R.rope_apply(k, c.value, s.value).value, ok[0].transpose(0, 1))
    dq, dk = _rand(n, hq, D, seed=3), _rand(n, hk, D, seed=4)
    torch.autograd.backward([oq, ok], [dq.transpose(0, 1)[None], dk.transpose(0, 1)[None]])
    _same(R.rope_apply(dq, c.value, s.value, backward=True).value, q.grad)
    _same(R.rope_apply(dk, c.value, s.value, backward=True).value, k.grad)


def test_adamw_restatement_is_torch_adamw_with_clip_and_skip():
    lr, b1, b2, eps, wd, max_norm = 3e-3, 0.9, 0.95, 1e-8, 0.1, 0.7
    shapes = [(33,), (5, 7), (1,)]
    ps = [torch.nn.Parameter(_rand(*s, seed=i)) for i, s in enumerate(shapes)]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    step = 0
    for it in range(6):                                                            # 5 applied steps and a skipped one
        gs = [_rand(*s, seed=100 + 10 * it + i, scale=(0.05 if it % 2 else 2.0)) for i, s in enumerate(shapes)]
        if it == 2:
            gs[1][0, 0] = float("nan")
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        if bool(torch.isfinite(norm)):                                            # the reference's skip (bin/train.py)
            opt.step()
        nsq = sum(float(R.sumsq(g).value) for g in gs)
        new_step, bc1, bc2, clip, skip = R.adamw_prepare(step, nsq, b1, b2, max_norm)
        assert skip == (it == 2) and new_step == step + (0 if skip else 1)
        if not skip:
            assert math.sqrt(nsq) == pytest.approx(float(norm), rel=1e-12)
            assert bc1 == pytest.approx(1 - b1 ** new_step) and bc2 == pytest.approx(1 - b2 ** new_step)
            mine = [R.adamw_step(p, m, v, g, new_step, lr, b1, b2, eps, wd, clip)[:3] for (p, m, v), g in zip(mine, gs)]
        step = new_step
        for (p, m, v), q in zip(mine, ps):
            _same(p, q.data, 1e-12)
            if step:
                _same(m, opt.state[q]["exp_avg"], 1e-12)
                _same(v, opt.state[q]["exp_avg_sq"], 1e-12)
    assert step == 5
    assert R.adamw_prepare(3, None, b1, b2, max_norm)[3:] == (1.0, False)          # NULL norm: no clip, no skip
    assert R.adamw_prepare(3, 4.0, b1, b2, 0.0)[3] == 1.0
    assert R.adamw_prepare(3, 0.1225, b1, b2, 0.7)[3] == 1.0                       # norm = max_norm / 2
    assert R.adamw_prepare(3, 1.96, b1, b2, 0.7)[3] == pytest.approx(0.7 / (1.4 + 1e-6), rel=1e-15)
    assert R.adamw_prepare(3, float("inf"), b1, b2, 0.7)[0::4] == (3, True)
    sh = R.adamw_step(*mine[0], gs[0], 6, lr, b1, b2, eps, wd, 1.0)
    assert sh[3].dtype == torch.bfloat16 and torch.equal(sh[3], sh[0].float().bfloat16())


def test_budget_and_check_helper(capsys):
    assert float(R.ulp(torch.tensor([1.0], dtype=F64), torch.bfloat16)) == 2.0 ** -7
    assert float(R.ulp(torch.tensor([-0.99], dtype=F64), torch.bfloat16)) == 2.0 ** -8
    assert float(R.ulp(torch.tensor([3.0], dtype=F64), torch.float32)) == 2.0 ** -22
    assert float(R.ulp(torch.tensor([0.0], dtype=F64), torch.float32)) == 2.0 ** -149
    v = torch.tensor([1.0, -2.0, 100.0], dtype=F64)
    ref = R.Ref(v, v.abs() * 3, torch.zeros(3, dtype=F64), torch.zeros(3, dtype=F64))
    b = R.budget(ref, torch.bfloat16)
    assert b.tolist() == pytest.approx([2.0 ** -8 + 3e-5, 2.0 ** -7 + 6e-5, 0.25 + 3e-3], rel=1e-9)
    assert R.check(v + 0.999 * b, ref, torch.bfloat16, "inside") == pytest.approx(0.999, rel=1e-6)
    with pytest.raises(AssertionError) as e:
        R.check(v + torch.tensor([0.0, 0.0, 0.3]), ref, torch.bfloat16, "outside")
    msg = str(e.value)
    assert "1/3 elements over budget" in msg and "worst at (2,)" in msg and "got 100.3" in msg and "ref 100.0" in msg
    assert "budget 0.253" in msg
    # an allowance that carries the value over a power of two: the output rounding is that of the coarser side
    # (w x xhat = 1.9963, xhat one bf16 ulp up: 2.008 rounds to 2.015625)
    near2 = R.Ref(torch.tensor([1.996337890625], dtype=F64), torch.tensor([2.0], dtype=F64),
                  torch.tensor([0.01171875], dtype=F64), torch.zeros(1, dtype=F64))
    assert float(R.budget(near2, torch.bfloat16)) == pytest.approx(2.0 ** -7 + 0.01171875 + 2e-5, rel=1e-6)
    R.check(torch.tensor([2.015625]), near2, torch.bfloat16, "over a power of two")
    with pytest.raises(AssertionError):
        R.check(torch.tensor([2.03125]), near2, torch.bfloat16, "one more ulp")
    with pytest.raises(AssertionError):
        R.check(torch.tensor([1.0, float("nan"), 100.0]), ref, torch.bfloat16, "nan")
    with pytest.raises(AssertionError):
        R.check(torch.tensor([1.0, -2.0, float("inf")]), ref, torch.bfloat16, "inf")
    assert "measured: inside [bf16] worst error = 0.999 x budget" in capsys.readouterr().out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_budget_at_the_edge_values_is_the_half_ulp_and_the_fp32_allowance(dtype):
    """The flush allowance exists only where a factor really is denormal (sigmoid below -87.3, e^{-x^2 / 2} beyond 13.2)
    and is that factor times its co-factors; at every other edge, the largest finite value of the dtype included, the
    budget is half an ulp + 1e-5 of the terms (+ one silu flip in swiglu_fwd) + 2^-126 and nothing else."""
    big = float(torch.finfo(dtype).max)
    x = torch.tensor([big, -big, 1e4, -1e4, 88.0, 20.0, -20.0, 13.0, -13.0, 5.0, -5.0, 1e-3, 0.0]).to(dtype)
    u, do = torch.full_like(x, 0.75), torch.full_like(x, -0.625)
    dg, du = R.swiglu_bwd(do, x, u, dtype)
    refs = {"swiglu_fwd": R.swiglu_fwd(x, u, dtype), "swiglu_bwd.dgate": dg, "swiglu_bwd.dup": du,
            "gelu_fwd": R.gelu_fwd(x), "gelu_bwd": R.gelu_bwd(do, x)}
    keep = (x.double().abs() <= 5) | (x.double().abs() >= 88)        # e^{-x^2 / 2}: normal, or zero in float64 too
    for what in ("gelu_fwd", "gelu_bwd"):
        assert bool((refs[what].flush[~keep] < 1e-36).all())          # +-13, +-20: a denormal factor, and that small
        refs[what] = R.Ref(*(t[keep] for t in refs[what]))
    for what, ref in refs.items():
        assert not ref.flush.any(), what
        plain = 0.5 * R.ulp(ref.value.abs() + R.FP32_REL * ref.scale + ref.flip + R.TINY, dtype) \
            + R.FP32_REL * ref.scale + ref.flip + R.TINY
        assert torch.allclose(R.budget(ref, dtype), plain, rtol=1e-12, atol=0.0), what
        rel = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
        # at most: the output's half ulp (twice, across a power of two) + 1e-5 + a silu flip of one ulp
        assert bool((R.budget(ref, dtype) <= (4 * rel + 2e-5) * ref.scale + 2 * R.TINY).all()), what
    # at the largest finite value: a wrong finite answer is over budget
    # (1 + erf cancels at -max: the fp32 allowance is of the uncancelled 1/2 + |erf|/2, 1e-5 x |dout|, and that is all)
    assert float(R.budget(refs["gelu_bwd"], dtype)[1]) < 1e-5 and float(refs["gelu_bwd"].value[1]) == 0.0
    assert float(R.budget(dg, dtype)[0]) < 0.0025 * 0.47 and float(dg.value[0]) == pytest.approx(-0.46875)
    assert float(R.budget(du, dtype)[0]) < 0.004 * 0.625 * big
    # a denormal silu (gate 2^-126) may be lost whole, and that is all
    tiny = R.swiglu_fwd(torch.tensor([2.0 ** -126]).to(dtype), torch.tensor([0.75]).to(dtype), dtype)
    assert float(tiny.flush) == 0.75 * 2.0 ** -127
    # inside the window the allowance is the denormal factor times its co-factors, no more
    g = torch.tensor([-88.0, -100.0, -700.0]).to(dtype)
    s = torch.sigmoid(g.double())
    assert bool((s < R.TINY).all()) and bool((s > 0).all())
    one = torch.ones_like(g)
    f = R.swiglu_fwd(g, one, dtype)
    assert bool((f.flush >= g.double().abs() * s).all()) and bool((f.flush <= 2 * g.double().abs() * s).all())
    t = R.gelu_fwd(torch.tensor([-13.5, -20.0, -38.0]).to(dtype))
    assert bool((t.flush > 0).all()) and float(t.flush.max()) < 1e-38


@pytest.mark.parametrize("H", [260, 520, 2052, 4104])
def test_layernorm_budget_tells_the_two_pass_variance_from_the_one_pass_form(H):
    """rows at 100 +- 1.3, float32 arithmetic on the CPU: the two-pass variance (what norm_fwd_kernel does for LayerNorm) is inside
    the rstd budget, E[h^2] - mean^2 is not"""
    g = torch.Generator().manual_seed(H)
    h = 1.3 * torch.randn(33, H, generator=g) + 100.2
    ref = R.layernorm_fwd(h, None, torch.ones(H), torch.zeros(H), 1e-5, torch.float32)
    mean = h.sum(-1) / H
    two = torch.rsqrt(((h - mean[:, None]) ** 2).sum(-1) / H + 1e-5)
    one = torch.rsqrt((h * h).sum(-1) / H - mean * mean + 1e-5)
    assert R.check(two, ref["rstd"], torch.float32, "two-pass rstd") < 0.5
    with pytest.raises(AssertionError):
        R.check(one, ref["rstd"], torch.float32, "one-pass rstd")
