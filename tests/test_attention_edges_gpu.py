"""The packed attention kernels (csrc/attn_fwd_stream.hip, attn_bwd_dq_stream.hip, attn_bwd.hip's attn_bwd_kv_kernel
<64, 2> / <128, 0> / <128, 1>, attn_bwd_fused.hip) against the float64 reference and the derived error budget of
tests/attention_reference.py, on layouts whose document boundaries sit at chosen places against a wave's 32 rows, a
64-key tile and a workgroup's 128 rows, with inputs that make one lost or leaked key visible (attention_reference.py
`_plant`, `_spike`).  Through touchnet_amd.library, where lse2 is visible; the backward gets the forward kernel's own
o and lse2.  tests/test_attention_reference_cpu.py shows on the CPU that a correct kernel can meet this budget and that
kernels wrong by one key, one rescale, one delta, one head or one pad row cannot.

MEASURED on an MI355X, the worst error as a multiple of the budget over all 76 cases, and the case it occurred in:
    O     0.921   edges, D = 128, causal, planted, 14 x 2 heads
    lse2  0.017   revisit, D = 64, bidirectional, sharp, 4 x 1 heads
    dQ    0.610   revisit, D = 64, causal, planted, 14 x 2 heads
    dK    0.700   edges, D = 64, causal, planted, 3 x 3 heads
    dV    0.947   edges, D = 64, causal, planted, 3 x 3 heads
(the fp32 model of test_attention_reference_cpu.py reaches 0.921 / 0.036 / 0.610 / 0.700 / 0.947, in the same cases but for
lse2: the worst elements are decided by where bf16 roundings fall, which the model reproduces.)
The file's 82 tests take 7.5 s, the largest (long_list, T = 4352) 0.95 s.  Every case passed on the first run on the
device: no budget term was added after it, and no kernel was changed.  One constant differs from the issue that asked
for this file — bf16's unit roundoff is 2^-8, not 2^-9 — and was settled on the CPU before that run
(attention_reference.py, UBF)."""
import functools
import math

import pytest
import torch

import attention_reference as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
_IDS = [A.case_id(c) for c in A.CASES]


def _dev(inp):
    return tuple(t.to(DEV) for t in (inp.q, inp.k, inp.v, inp.do, inp.doc))


@functools.lru_cache(maxsize=None)
def _run(idx):
    """forward and backward of CASES[idx] at the library level -> (o, lse2, dq, dk, dv) on the CPU"""
    import touchnet_amd.library as L
    case = A.CASES[idx]
    inp, _ = A.problem(idx)
    q, k, v, do, doc = _dev(inp)
    meta = L.attn_build_meta(doc)
    fwd, bwd = (L.attn_fwd, L.attn_bwd) if case.causal else (L.attn_fwd_bidir, L.attn_bwd_bidir)
    o, lse2 = fwd(q, k, v, doc, meta, case.scale)
    dq, dk, dv = bwd(q, k, v, o, do, lse2, doc, meta, case.scale)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (o, lse2, dq, dk, dv))


def _zeros(case, inp, o, lse2, dq, dk, dv):
    """exact zeros: O and dQ of pad rows (lse2 = +inf there), dK and dV of pad keys and of keys no query may see, and
    everything in a batch row that is all pad"""
    pad = inp.doc == 0
    unseen = ~A.allow_mask(inp.doc, case.causal).any(1)
    assert bool((pad <= unseen).all())
    for name, t, where in (("O", o, pad), ("dQ", dq, pad), ("dK", dk, unseen), ("dV", dv, unseen)):
        if where.any():
            assert float(t.float()[where].abs().max()) == 0.0, f"{name} is not exactly 0 where nothing may be seen"
    if pad.any():
        assert bool((lse2.transpose(1, 2)[pad] == math.inf).all()), "lse2 of a pad row is not +inf"
    for b in torch.nonzero(pad.all(1)).flatten().tolist():
        assert all(float(t[b].float().abs().max()) == 0.0 for t in (o, dq, dk, dv)) and bool((lse2[b] == math.inf).all())


@pytest.mark.parametrize("idx", range(len(A.CASES)), ids=_IDS)
def test_kernels_stay_inside_the_derived_budget(idx):
    case = A.CASES[idx]
    inp, ref = A.problem(idx)
    o, lse2, dq, dk, dv = _run(idx)
    what = A.case_id(case)
    A.check(o, ref["o"], f"O of {what}")
    A.check(lse2, ref["lse2"], f"lse2 of {what}", torch.float32)
    A.check(dq, ref["dq"], f"dQ of {what}")
    A.check(dk, ref["dk"], f"dK of {what}")
    A.check(dv, ref["dv"], f"dV of {what}")
    _zeros(case, inp, o, lse2, dq, dk, dv)


def _case(layout, D, causal):
    return next(i for i, c in enumerate(A.CASES) if (c.layout, c.D, c.causal, c.kind) == (layout, D, causal, "planted"))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
def test_the_python_surface_returns_the_bits_of_the_library_calls(D, causal):
    """functional.packed_attention / bidirectional_attention under autograd (causal with Nh == Nkv: the stacked gradient
    buffer) against attn_fwd + attn_bwd called by hand: the same bits, so the surface cannot hide a difference"""
    import touchnet_amd.functional as F
    idx = _case("edges", D, causal)
    case = A.CASES[idx]
    inp, _ = A.problem(idx)
    q, k, v, do, doc = _dev(inp)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    attend = F.packed_attention if causal else F.bidirectional_attention
    out = attend(q, k, v, F.build_packed_mask(doc), scale=case.scale)
    out.backward(do)
    torch.cuda.synchronize()
    o, _, dq, dk, dv = _run(idx)
    for name, a, b in (("O", out, o), ("dQ", q.grad, dq), ("dK", k.grad, dk), ("dV", v.grad, dv)):
        assert torch.equal(a.detach().cpu(), b), name


@pytest.mark.parametrize("D", [64, 128])
def test_the_rotary_backward_with_an_identity_rotation(D):
    """attn_bwd_rope with cos = 1, sin = 0 (the rotation's backward is then the identity, exactly: x 1 + y 0 of bf16 values)
    against the same reference: D = 128 rotates in the dQ and the fused dK / dV kernels' epilogues, D = 64 runs the row
    kernel behind the launch.  `pads`, causal; the geometry decides between the stacked and the flat buffer."""
    import touchnet_amd.library as L
    idx = _case("pads", D, True)
    case = A.CASES[idx]
    inp, ref = A.problem(idx)
    q, k, v, do, doc = _dev(inp)
    B, T = doc.shape
    meta = L.attn_build_meta(doc)
    o, lse2 = L.attn_fwd(q, k, v, doc, meta, case.scale)
    cos = torch.ones(B * T, D // 2, dtype=torch.bfloat16, device=DEV)
    sin = torch.zeros_like(cos)
    stacked = case.Nh == case.Nkv
    buf = L.attn_bwd_rope(q, k, v, o, do, lse2, doc, meta, case.scale, cos, sin, stacked)
    torch.cuda.synchronize()
    dq, dk, dv = (t.cpu() for t in L.attn_grads(q, k, "stacked" if stacked else "flat", buf)[1])
    what = f"{A.case_id(case)} through attn_bwd_rope"
    A.check(dq, ref["dq"], f"dQ of {what}")
    A.check(dk, ref["dk"], f"dK of {what}")
    A.check(dv, ref["dv"], f"dV of {what}")
    _zeros(case, inp, o.cpu(), lse2.cpu(), dq, dk, dv)
