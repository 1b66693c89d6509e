"""tests/attention_reference.py is a reference, and its budget is neither loose nor tight (no GPU).

1. Its values agree with torch autograd in float64 over a masked softmax written independently (`torch.softmax` of a
   `masked_fill`), to float64 roundoff, on every layout and both directions (long_list, one document of 4352 keys, is left
   to the emulation: it is one_over with more tiles); rows without an allowed key give O = 0, lse2 = +inf and zero
   gradients.
2. `emulate` is a plain-torch fp32 model of the kernels with exactly the rounding points the budget names (online
   softmax over 64-key tiles with the rescale deferred per 32-row wave, P and dS through bf16, fp32 sums, bf16 stores,
   delta from the bf16 O, the backward on the emulated o / lse2).  It stays inside the budget on every case the GPU test
   runs: what the budget allows, a correct kernel can meet.
3. Each mutant of the emulation — a kernel that is subtly wrong in one way — exceeds the budget on the case aimed at it:
   what the budget allows, a wrong kernel cannot meet."""
import math

import pytest
import torch

import attention_reference as A

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ 1. the reference
def _autograd(inp, case):
    q, k, v, do = (A.d(t).requires_grad_(True) for t in (inp.q, inp.k, inp.v, inp.do))
    G = case.Nh // case.Nkv
    doc = inp.doc.long()
    T = doc.shape[1]
    same = (doc[:, :, None] == doc[:, None, :]) & (doc[:, :, None] > 0)
    if case.causal:
        same = same & (torch.arange(T)[:, None] >= torch.arange(T)[None, :])
    kk, vv = (t.repeat_interleave(G, dim=2) for t in (k, v))
    s = torch.einsum("bihd,bjhd->bhij", q, kk) * case.scale
    s = s.masked_fill(~same[:, None], -math.inf)
    dead = ~same.any(-1)[:, None, :, None]
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    o = torch.einsum("bhij,bjhd->bihd", p, vv)
    lse2 = torch.logsumexp(s.masked_fill(dead, 0.0), dim=-1) / math.log(2.0)
    lse2 = lse2.masked_fill(dead[..., 0], math.inf)
    o.backward(do.detach())
    return dict(o=o.detach(), lse2=lse2.detach(), dq=q.grad, dk=k.grad, dv=v.grad), ~same.any(-1)


_LAYOUT_CASES = [i for i, c in enumerate(A.CASES) if c.layout != "long_list" and c.D == 64 and c.kind == "planted"]


@pytest.mark.parametrize("idx", _LAYOUT_CASES, ids=lambda i: A.case_id(A.CASES[i]))
def test_reference_agrees_with_float64_autograd(idx):
    """Bound: float64 roundoff.  A sum of n terms carries n 2^-53 of the sum of their magnitudes; the gradients chain four
    such sums (logits, softmax, dP, the product), n <= 540 keys or D = 64 terms each, and the planted logits reach 40, whose
    exponentials lose 40 2^-53 relative: 2^-53 x (4 x 540 + 40) < 2.5e-13 of the largest magnitude in play, which the
    test takes as max |reference| + 1 per quantity."""
    case = A.CASES[idx]
    inp, ref = A.problem(idx)
    auto, dead_rows = _autograd(inp, case)
    for name in ("o", "lse2", "dq", "dk", "dv"):
        r, a = ref[name].value, auto[name]
        fin = torch.isfinite(r)
        assert torch.equal(fin, torch.isfinite(a)) and torch.equal(r[~fin], a[~fin]), name
        tol = 2.5e-13 * (float(r[fin].abs().max()) + 1.0 if fin.any() else 1.0)
        err = float((r[fin] - a[fin]).abs().max()) if fin.any() else 0.0
        print(f"measured: {name} vs float64 autograd: {err:.3g} (bound {tol:.3g})")
        assert err <= tol, (name, err, tol)
    dead = dead_rows                                                    # [B, T]
    if dead.any():
        assert float(ref["o"].value[dead].abs().max()) == 0.0 and float(ref["dq"].value[dead].abs().max()) == 0.0
        assert float(ref["o"].slack[dead].abs().max()) == 0.0 and float(ref["dq"].slack[dead].abs().max()) == 0.0
        assert bool((ref["lse2"].value.transpose(1, 2)[dead] == math.inf).all())
    unseen = ~A.allow_mask(inp.doc, case.causal).any(1)                 # keys no query may see
    if unseen.any():
        for name in ("dk", "dv"):
            assert float(ref[name].value[unseen].abs().max()) == 0.0 and float(ref[name].slack[unseen].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. the emulation
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in float64; one rounding back"""
    return (a.double() * b - c.double()).float()


def emulate(inp, case, mutant=None, arg=None, backward=True):
    """The kernels' arithmetic in fp32 on the CPU.  `mutant`:
         drop / leak (arg: Plants)   the pair (i, j) of that head is masked / allowed against the predicate
         diagonal                    no row sees its own key
         skip_rescale (arg: Plant)   at the tile of key j the wave of row i updates m and l but leaves O unscaled
         lse2                        lse2 x (1 + 2^-10)
         delta (arg: (b, h, i))      delta of that row from the unrounded O, sign flipped
         pad_rows                    the dK / dV pass takes pad rows for a document (lse2 = 0 where the forward left +inf)
         gqa                         dK / dV sum one query head too few"""
    f32 = torch.float32
    B, T, Nh, D = inp.q.shape
    G = Nh // case.Nkv
    qf, dof = (t.float().transpose(1, 2) for t in (inp.q, inp.do))
    kf, vf = (t.float().transpose(1, 2).repeat_interleave(G, dim=1) for t in (inp.k, inp.v))
    allow = A.allow_mask(inp.doc, case.causal)[:, None].expand(B, Nh, T, T).clone()
    if mutant in ("drop", "leak"):
        for pl in arg:
            allow[pl.b, pl.h, pl.i, pl.j] = mutant == "leak"
    if mutant == "diagonal":
        allow &= ~torch.eye(T, dtype=torch.bool)
    c = torch.tensor(case.scale, dtype=f32) * torch.tensor(A.LOG2E, dtype=f32)
    Tp = (T + 31) // 32 * 32
    m = torch.full((B, Nh, T), -1e30, dtype=f32)
    l = torch.zeros(B, Nh, T, dtype=f32)
    o = torch.zeros(B, Nh, T, D, dtype=f32)
    skipped = False
    for j0 in range(0, T, 64):
        al = allow[..., j0:j0 + 64]
        if not bool(al.any()):
            continue
        s = torch.where(al, qf @ kf[:, :, j0:j0 + 64].transpose(-1, -2), torch.tensor(-math.inf))
        mx = s.amax(-1) * c
        grow = torch.nn.functional.pad(mx - m > A.DEFER, (0, Tp - T))
        trig = grow.view(B, Nh, Tp // 32, 32).any(-1, keepdim=True).expand(B, Nh, Tp // 32, 32).reshape(B, Nh, Tp)[..., :T]
        m_new = torch.where(trig, torch.maximum(m, mx), m)
        alpha = torch.exp2(m - m_new)
        l = l * alpha
        if mutant == "skip_rescale" and arg.j // 64 * 64 == j0:
            w0 = arg.i // 32 * 32
            skipped = bool(trig[arg.b, arg.h, arg.i]) and float(alpha[arg.b, arg.h, arg.i]) < 1.0
            alpha = alpha.clone()
            alpha[arg.b, arg.h, w0:w0 + 32] = 1.0
        o = o * alpha[..., None]
        m = m_new
        p = torch.exp2(_fma(s, c, m[..., None]))
        l = l + p.sum(-1)
        o = o + p.to(BF).float() @ vf[:, :, j0:j0 + 64]
    if mutant == "skip_rescale":
        assert skipped, "the mutant found no rescale to skip"
    live = l > 0
    inv = torch.where(live, 1.0 / l, torch.zeros_like(l))
    o32 = o * inv[..., None]
    ob = o32.to(BF)
    lse2 = torch.where(live, m + torch.log2(torch.where(live, l, torch.ones_like(l))), torch.tensor(math.inf))
    if mutant == "lse2":
        lse2 = lse2 * (1 + 2.0 ** -10)
    out = dict(o=ob.transpose(1, 2), lse2=lse2)
    if not backward:
        return out
    delta = (dof * ob.float()).sum(-1)
    if mutant == "delta":
        b, h, i = arg
        delta[b, h, i] = -(dof[b, h, i] * o32[b, h, i]).sum()
    if mutant == "pad_rows":
        pad = inp.doc == 0
        extra = pad[:, :, None] & pad[:, None, :]
        if case.causal:
            extra = extra & torch.ones(T, T, dtype=torch.bool).tril()
        allow_kv = allow | extra[:, None]
        lse_kv = torch.where(torch.isfinite(lse2), lse2, torch.zeros_like(lse2))
    else:
        allow_kv, lse_kv = allow, lse2
    s = qf @ kf.transpose(-1, -2)
    dp = dof @ vf.transpose(-1, -2)

    def scores(al, lse):
        p = torch.where(al, torch.exp2(s * c - lse[..., None]), torch.zeros_like(s))
        return p, p * (dp - delta[..., None])

    p, ds = scores(allow, lse2)
    scale = torch.tensor(case.scale, dtype=f32)
    dq = ((ds.to(BF).float() @ kf) * scale).to(BF)
    if allow_kv is not allow:
        p, ds = scores(allow_kv, lse_kv)
    dvh = p.to(BF).float().transpose(-1, -2) @ dof
    dkh = ds.to(BF).float().transpose(-1, -2) @ qf
    heads = slice(0, G - 1) if mutant == "gqa" else slice(0, G)
    group = lambda t: t.view(B, case.Nkv, G, T, D)[:, :, heads].sum(2).transpose(1, 2)
    out.update(dq=dq.transpose(1, 2), dk=(group(dkh) * scale).to(BF), dv=group(dvh).to(BF))
    return out


_DTYPE = dict(o=BF, lse2=torch.float32, dq=BF, dk=BF, dv=BF)


def _worst(got, ref, names=("o", "lse2", "dq", "dk", "dv")):
    return {n: float(A.ratios(got[n], ref[n], _DTYPE[n]).max()) for n in names if n in got}


@pytest.mark.parametrize("idx", range(len(A.CASES)), ids=lambda i: A.case_id(A.CASES[i]))
def test_emulation_stays_inside_the_budget(idx):
    """worst ratio <= 1 per quantity, on every case tests/test_attention_edges_gpu.py runs"""
    case = A.CASES[idx]
    inp, ref = A.problem(idx)
    got = emulate(inp, case)
    for name in ("o", "lse2", "dq", "dk", "dv"):
        A.check(got[name], ref[name], f"emulated {name} of {A.case_id(case)}", _DTYPE[name])


# ------------------------------------------------------------------------------------------------ 3. the mutants
def _find(kind_of, wanted, causal=None, pred=lambda c: True):
    """the first planted / sharp case that holds a plant of kind `wanted` -> (idx, plants of that kind)"""
    rank = {"edges": 0, "pads": 1, "revisit": 2}                        # the layouts with the most boundaries first
    for idx, c in sorted(enumerate(A.CASES), key=lambda ic: rank.get(ic[1].layout, 3)):
        if c.layout == "long_list" or (causal is not None and c.causal != causal) or not pred(c):
            continue
        inp, _ = A.problem(idx)
        hit = [pl for pl in getattr(inp, kind_of) if pl.kind == wanted]
        if hit:
            return idx, hit
    raise AssertionError(f"no case plants a {wanted}")


def _exceeds(idx, names, mutant, arg=None, backward=False):
    case = A.CASES[idx]
    inp, ref = A.problem(idx)
    w = _worst(emulate(inp, case, mutant, arg, backward=backward), ref, names)
    print(f"measured: mutant {mutant} on {A.case_id(case)}: " + ", ".join(f"{n} {v:.3g} x budget" for n, v in w.items()))
    return w


@pytest.mark.parametrize("kind", ["tile_first", "tile_last", "diagonal", "doc_first", "single"])
def test_a_dropped_anchor_key_exceeds_the_budget(kind):
    """EVERY anchor of the kind, one at a time, in the first causal and the first bidirectional case that plants it"""
    for causal in (True, False):
        idx, plants = _find("anchors", kind, causal)
        for pl in plants:
            w = _exceeds(idx, ("o", "lse2"), "drop", [pl])
            assert w["o"] > 1.0 and w["lse2"] > 1.0, (kind, pl, w)


def test_a_dropped_key_in_a_long_document_exceeds_the_budget():
    """long_list (one document of 4352 keys, 68 KV tiles): the first, a middle and the last tile anchor, one at a time — the
    single-key fault in a long document that random inputs hide under any tolerance"""
    idx = next(i for i, c in enumerate(A.CASES) if c.layout == "long_list" and c.kind == "planted")
    inp, _ = A.problem(idx)
    plants = [pl for pl in inp.anchors if pl.kind in ("tile_first", "tile_last")]
    assert len(plants) >= 100
    for pl in (plants[0], plants[len(plants) // 2], plants[-1]):
        w = _exceeds(idx, ("o", "lse2"), "drop", [pl])
        assert w["o"] > 1.0 and w["lse2"] > 1.0, (pl, w)


@pytest.mark.parametrize("kind,causal", [("causal_next", True), ("prev_doc_last", True), ("prev_doc_last", False),
                                         ("next_doc_first", False), ("pad_key", True), ("pad_key", False),
                                         ("other_id_same_tile", True), ("other_id_same_tile", False)])
def test_a_leaked_bait_key_exceeds_the_budget(kind, causal):
    idx, plants = _find("baits", kind, causal)
    for pl in plants:
        w = _exceeds(idx, ("o", "lse2"), "leak", [pl])
        assert w["o"] > 1.0 and w["lse2"] > 1.0, (kind, pl, w)


def test_a_dropped_diagonal_exceeds_the_budget():
    for kind in ("planted", "gauss", "sharp"):
        idx = next(i for i, c in enumerate(A.CASES) if c.causal and c.kind == kind and c.layout in ("edges", "pads"))
        w = _exceeds(idx, ("o", "lse2"), "diagonal")
        assert w["o"] > 1.0 and w["lse2"] > 1.0, (kind, w)


def test_a_skipped_rescale_exceeds_the_budget():
    for causal in (True, False):
        idx, spikes = _find("spikes", "spike", causal)
        for pl in spikes:
            w = _exceeds(idx, ("o",), "skip_rescale", pl)
            assert w["o"] > 1.0, (pl, w)


def _backward_case(causal, pred=lambda c: True):
    return next(i for i, c in enumerate(A.CASES) if c.causal == causal and c.layout == "pads" and pred(c))


@pytest.mark.parametrize("causal", [True, False])
def test_lse2_off_by_one_part_in_1024_exceeds_the_budget(causal):
    """in lse2 itself.  (The gradients are printed: P recomputed from such an lse2 is off by 2^-10 |lse2| ln 2, about what its
    bf16 rounding costs, so they need not leave their budgets.)"""
    w = _exceeds(_backward_case(causal), ("lse2", "dq", "dk", "dv"), "lse2", backward=True)
    assert w["lse2"] > 1.0, w


@pytest.mark.parametrize("causal", [True, False])
def test_delta_from_the_unrounded_o_with_a_flipped_sign_exceeds_the_budget(causal):
    """on the one-token document of `pads` (position 255): there dP = delta exactly and dS = 0, so dQ and dK of that position
    are 0 with next to no budget, and a delta of the other sign makes dS = 2 delta"""
    idx = _backward_case(causal)
    inp, _ = A.problem(idx)
    assert inp.doc[0, 254:257].tolist() == [0, 4, 0]
    w = _exceeds(idx, ("dq", "dk"), "delta", (0, 0, 255), backward=True)
    assert w["dq"] > 1.0 and w["dk"] > 1.0, w


@pytest.mark.parametrize("causal", [True, False])
def test_unmasked_do_of_pad_rows_exceeds_the_budget(causal):
    w = _exceeds(_backward_case(causal, lambda c: c.kind == "planted"), ("dk", "dv"), "pad_rows", backward=True)
    assert w["dk"] > 1.0 and w["dv"] > 1.0, w


@pytest.mark.parametrize("causal", [True, False])
def test_a_gqa_sum_one_head_short_exceeds_the_budget(causal):
    w = _exceeds(_backward_case(causal, lambda c: c.Nh > c.Nkv), ("dk", "dv"), "gqa", backward=True)
    assert w["dk"] > 1.0 and w["dv"] > 1.0, w
