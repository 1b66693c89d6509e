"""tests/gemm_reference.py on the CPU: the float64 reference is exact (equal to an int64 product), the regime S data keep
their condition (every expected value an integer of magnitude <= 256: a bf16 number), the fp32 model of the kernel's
structure reproduces the expected bits on every case, and each of ten small mistakes — one stage, one contraction row,
one tile, one term — breaks bit equality on the case aimed at it.  The last test shows why tests/test_gemm_edges_gpu.py
exists: two of those mistakes pass the tolerance the older GEMM tests judge with."""
import dataclasses

import pytest
import torch

import gemm_reference as R

_checked = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want):
    return got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_float64_reference_equals_the_int64_product(case):
    for sub, p in R.sub_problems(case):
        key = R._data_key(sub)
        if key not in _checked:                 # (cases that differ in options only share their data: one product each)
            ak, bk = R.MODES[sub.mode]
            exact = 0
            for a, b in zip(p.A, p.B):
                a64, b64 = R._logical(a.view(), ak).to(torch.int64), R._logical(b.view(), bk).to(torch.int64)
                assert torch.equal(a64.to(torch.bfloat16), R._logical(a.view(), ak))        # integers, as stored
                exact = exact + a64.contiguous() @ b64.t().contiguous()
            _checked[key] = torch.equal(exact, p.exact.to(torch.int64)) and torch.equal(exact.double(), p.exact)
        assert _checked[key], R.case_id(sub)


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_regime_s_expected_values_are_bf16_integers(case):
    for sub, p in R.sub_problems(case):
        assert p.unrepresentable == 0
        e = p.expected(sub)
        if sub.regime == "S":
            assert R._s_violations(e.double()) == 0
            assert _same(e, e.double().to(e.dtype)) and _same(e.to(torch.bfloat16).to(e.dtype), e)
            if sub.bias_grad:
                assert R._s_violations(p.colsum) == 0
        else:
            assert float(p.exact.abs().max()) < 2 ** 24
            wide, thin = (p.A, p.B) if sub.regime == "WA" else (p.B, p.A)
            assert all(float(o.view().abs().max()) == 255 for o in wide)        # all eight significand bits in use
            assert all(float(o.view().abs().max()) == 1 for o in thin)
            assert int((p.exact.float().to(torch.bfloat16).double() != p.exact).sum()) > 0      # and the rounding is at work


def _agrees(case, out):
    ok = True
    for (sub, p), o in zip(R.sub_problems(case), out):
        ok = ok and _same(o["C"], p.expected(sub))
        if sub.out_t:
            ok = ok and _same(o["Ct"], p.expected(sub).t())
        if sub.bias_grad:
            ok = ok and _same(o["bias_grad"], p.expected_bias_grad())
    return ok


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_the_model_of_the_kernel_reproduces_the_expected_bits(case):
    out = R.emulate(case)
    assert _agrees(case, out)
    for (sub, p), o in zip(R.sub_problems(case), out):            # the restated tile walk is a bijection
        nbm, nbn = -(-p.exact.shape[0] // R.BM), -(-p.exact.shape[1] // R.BN)
        assert set(o["visits"].values()) == {1} and {(tm, tn) for tm, tn, _ in o["visits"]} == {
            (tm, tn) for tm in range(nbm) for tn in range(nbn)}


def test_the_persistent_cases_are_what_they_are_listed_for():
    """tile counts against 256 CUs: more than one tile per workgroup, three for some at 529, a short last panel group"""
    for c in R.CASES:
        if c.group == "persist":
            nbm, nbn = -(-c.M // 256), -(-c.N // 256)
            assert nbm * nbn > R.NCU
            assert (nbm * nbn > 2 * R.NCU) == (c.M == 5640)
            assert (nbm > 8 and nbm % 8 != 0) and (c.M != 16392 or nbm % 8 == 1)
        if c.group == "tail":
            assert 0 < (-(-c.M // 256) * -(-c.N // 256)) % R.NCU
        if c.group == "grouped" and c.device_ref:
            tiles = sum(-(-m // 256) * -(-n // 256) for m, n, _ in c.products)
            assert R.grouped_split(tiles, 16) == (2, 74)


def _case(**kw):
    found = [c for c in R.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    assert found, kw
    return found[0]


_PLAIN = dict(group="plain", regime="S", bias=False, accumulate=False)
MUTANT_CASES = [
    ("a", dict(_PLAIN, mode="fwd", M=129, N=264, Ks=(320,))),                      # five stages: the ring's first wrap
    ("a", dict(_PLAIN, mode="dgrad", M=129, N=264, Ks=(320,))),
    ("b", dict(_PLAIN, mode="wgrad", M=136, N=264, Ks=(65,))),
    ("b", dict(_PLAIN, mode="wgrad", M=8, N=8, Ks=(321,))),
    ("c", dict(_PLAIN, mode="fwd", M=129, N=264, Ks=(320,))),
    ("c", dict(_PLAIN, mode="wgrad", M=136, N=264, Ks=(1,))),
    ("d", dict(_PLAIN, mode="dgrad", M=129, N=264, Ks=(128,))),
    ("e", dict(_PLAIN, mode="fwd", M=129, N=264, Ks=(320,), bias=True)),
    ("f", dict(group="persist", mode="fwd", M=4104, Ks=(64,), accumulate=True, persist=True)),
    ("g", dict(group="splitk", mode="wgrad", M=264, Ks=(129,), entry="splitk", bias=False)),
    ("g", dict(group="splitk", mode="fwd", M=264, Ks=(384,), entry="splitk", bias=False)),
    ("h", dict(group="out_t", mode="fwd", M=264, N=72, bias=False)),
    ("h", dict(group="out_t", mode="wgrad", M=520, N=264, bias=True)),
    ("i", dict(_PLAIN, mode="fwd", M=1, N=8, Ks=(320,))),
    ("i", dict(_PLAIN, mode="fwd", M=264, N=264, Ks=(320,))),
    ("j", dict(group="overlap", mode="fwd", M=40, overlap=64)),
    ("j", dict(group="overlap", mode="fwd", M=264, overlap=128)),
]


@pytest.mark.parametrize("mutant,where", MUTANT_CASES, ids=[f"{m}-{R.case_id(_case(**w))}" for m, w in MUTANT_CASES])
def test_each_mutant_breaks_bit_equality_on_its_case(mutant, where):
    case = _case(**where)
    assert _agrees(case, R.emulate(case))
    assert not _agrees(case, R.emulate(case, mutant)), R.MUTANTS[mutant]


def test_every_mutant_is_aimed_at_some_case():
    assert {m for m, _ in MUTANT_CASES} == set(R.MUTANTS)


def test_the_overlapping_row_mutant_misses_exactly_the_last_rows():
    """mutant j is the suspected defect of Stream::open: the tails of the last ceil((K - ld) / ld) rows read as zeros"""
    for case in (c for c in R.CASES if c.group == "overlap" and c.mode == "fwd"):
        p = R.build(case)
        bad = (R.emulate(case, "j")[0]["C"] != p.expected(case)).any(1).nonzero().flatten().tolist()
        n_rows = -(-(case.Ks[0] - case.overlap) // case.overlap)
        assert bad and set(bad) <= set(range(case.M - n_rows, case.M)), (R.case_id(case), bad)


def test_what_the_older_tolerance_sees_of_a_dropped_term_and_a_dropped_row():
    """THE GAP: the uniform(-1, 1) data of test_gemm_operand_modes_match_fp64_reference at (1280, 520, 3000), judged with
    that test's own criterion (_close: atol = max|ref| 2^-8 = 0.34 here, rtol = 2^-7).
      mutant i, one term (0.33 x 0.155 = 0.05) dropped in one element (-33.25, bf16 spacing 0.25): PASSES — it does not
                even reach the rounded output, and no single term (at most 1) is told from the half spacing plus the 0.34
                unless it is above about 0.5, which one term in seven is; in regime S the same mistake changes the
                expected bits (the test above).
      mutant c, the whole last contraction row dropped: does NOT pass at this shape — but it is seen in fewer than one
                in four of the 557602 output elements it changes (122123); the other 435479 are inside the tolerance, and
                so is every element of an output small enough to hold none of the large terms.  (The issue that asked for this
                file expected mutant c to pass as well; it does not, and this test asserts what is the case.)"""
    import test_kernels_gpu as TK
    M, N, K = 1280, 520, 3000
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    r = lambda *sh: (torch.rand(*sh, generator=g) * 2 - 1).to(torch.bfloat16)
    a, b = r(K, M), r(K, N)
    ref = a.double().t() @ b.double()
    case = R.Case("plain", "wgrad", M, N, (K,), regime="uniform")
    z = torch.zeros(M, N)
    p = R.assemble(case, [a.double()], [b.double()], torch.zeros(N), z, z)
    atol, rtol = float(ref.abs().max()) * 2 ** -8, 2 ** -7
    whole = R.emulate(case, None, problem=p)[0]["C"]
    TK._close(whole, ref, atol, rtol, "the unmutated model")
    one_term = R.emulate(case, "i", problem=p)[0]["C"]
    f32 = dataclasses.replace(case, f32=True)                         # (the accumulators, unrounded)
    lost = R.emulate(f32, None, problem=p)[0]["C"] - R.emulate(f32, "i", problem=p)[0]["C"]
    assert int((lost != 0).sum()) == 1 and 0.04 < float(lost.abs().max()) < 0.06      # the mistake is there ...
    TK._close(one_term, ref, atol, rtol, "mutant i")                  # ... and the older criterion does not see it
    no_last_row = R.emulate(case, "c", problem=p)[0]["C"]
    wrong = no_last_row != whole
    seen = (no_last_row.double() - ref).abs() > atol + rtol * ref.abs()
    print(f"mutant c: {int(wrong.sum())} elements differ, {int(seen.sum())} of {seen.numel()} outside the tolerance")
    assert bool((seen <= wrong).all()) and 0 < int(seen.sum()) < int(wrong.sum()) / 4
    with pytest.raises(AssertionError):
        TK._close(no_last_row, ref, atol, rtol, "mutant c")
