"""tn_attn_extend (csrc/attn_extend.hip) through touchnet_amd.functional against the float64 restatement and the derived
budget of tests/attn_extend_reference.py (one ragged call over every prefix and row-count edge, shared cache rows, NaN in
every cache position no sequence may read); the poison rule; and the n_r = 1 case beside tn_attn_decode."""
import pytest
import torch

import attn_extend_reference as X
import inference_attention_reference as IR

pytestmark = pytest.mark.gpu
DEV, I16 = "cuda", torch.int16


def _run(q, kn, vn, kc, vc, start, pre, row, scale):
    """two calls on device copies -> o on the CPU; the caches bit-identical afterwards, the second call bit-identical"""
    import touchnet_amd.functional as F
    dq, dkn, dvn, dkc, dvc = (t.to(DEV) for t in (q, kn, vn, kc, vc))
    with torch.no_grad():
        o = F.attn_extend(dq, dkn, dvn, dkc, dvc, start, pre, scale, row)
        again = F.attn_extend(dq, dkn, dvn, dkc, dvc, start.to(DEV), pre.to(DEV), scale, None if row is None else row.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(o.view(I16), again.view(I16)), "a second call differs"
    assert torch.equal(dkc.cpu().view(I16), kc.view(I16)) and torch.equal(dvc.cpu().view(I16), vc.view(I16)), "caches written"
    return o.cpu()


@pytest.mark.parametrize("kind", ["gauss", "sharp"])
@pytest.mark.parametrize("Nh,Nkv", [(1, 1), (8, 2), (28, 4), (16, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_extend_meets_the_float64_reference(D, Nh, Nkv, kind):
    inp = X.inputs(D, Nh, Nkv, kind, seed=100 * D + Nh)
    IR.check(_run(*inp), X.extend(*inp[:7], inp[8], inp[7]), f"attn_extend D{D} {Nh}x{Nkv} {kind}")


def test_out_of_range_prefix_or_row_poisons_exactly_its_sequence():
    seqs = ((5, 17, 0), (X.S_MAX + 1, 3, 1), (64, 16, 2), (-1, 1, 0), (9, 2, X.B), (3, 20, -1), (X.S_MAX, 1, 3))
    inp = X.inputs(64, 8, 2, "sharp", seed=7, seqs=seqs)
    ref = X.extend(*inp[:7], inp[8], inp[7])
    o = _run(*inp)
    bad = torch.isnan(ref.value)
    assert int(bad[:, 0, 0].sum()) == 3 + 1 + 2 + 20 and torch.equal(torch.isnan(o.float()), bad)
    ok = ~bad[:, 0, 0]
    IR.check(o[ok], IR.Ref(ref.value[ok], ref.slack[ok]), "attn_extend beside poisoned sequences")


@pytest.mark.parametrize("idx", [i for i, c in enumerate(IR.DECODE_CASES) if c.name in ("len0", "len2", "sharp")])
def test_one_new_row_meets_the_decode_reference_as_attn_decode_does(idx):
    """n_r = 1 everywhere: both kernels meet the SAME float64 values, each within its own budget (bits may differ)."""
    import touchnet_amd.functional as F
    case = IR.DECODE_CASES[idx]
    inp, dref, _, _ = IR.decode_problem(idx)
    start = torch.arange(case.B + 1, dtype=torch.int32)
    args = (inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, start, inp.cache_len, None, case.scale)
    xref = X.extend(*args[:7], case.scale)
    assert torch.allclose(xref.value, dref.value, rtol=1e-9, atol=1e-12)        # two float64 restatements of one rule
    IR.check(_run(*args), xref, f"attn_extend on {IR.dcase_id(case)}")
    with torch.no_grad():
        od = F.attn_decode(*(t.to(DEV) for t in (inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, inp.cache_len)),
                           case.scale)
    IR.check(od.cpu(), dref, f"attn_decode on {IR.dcase_id(case)}")
