"""The restatement of tn_sample_step (tests/sampling_reference.py) held to transformers' warpers and to rows computed by
hand, and the planted cases of the device test held to the margins that let it ask for exact equality: every top_p and
every uniform at least 5e-5 from the nearest decision boundary of the fp64 restatement.

Where 5e-5 comes from: the kernel's sums are exact fixed point; its errors are per weight — d = max - l rounded in fp32,
d * log2(e) rounded in fp32 (<= 28 * 1.4427 * 2^-24 ~ 2.4e-6 in the exponent, ~1.7e-6 relative), the exp instruction, and
the truncation to an integer (V * 2^-40 of the mass at worst, 2.4e-7 at V = 262144): ~4e-6 relative together, inside the
1e-5 band test_sample_step_matches_transformers_warpers grants.  5e-5 is five times that band."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kimi_generate_reference as KR  # noqa: E402
import sampling_reference as SR  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]


def _hf(logits_row, hist_row, penalty, T, k, p):
    """HF's pipeline: RepetitionPenalty and Temperature in fp32 (generate()'s dtype), TopK, TopP and softmax in fp64 ->
    (fp32 values, probabilities [V])."""
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    ids = torch.tensor([hist_row], dtype=torch.int64)
    s = logits_row.float()[None].clone()
    if penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty)(ids, s)
    if T != 1.0:
        s = TemperatureLogitsWarper(T)(ids, s)
    v = s[0].clone()
    s = s.double()
    if k > 0:
        s = TopKLogitsWarper(k)(ids, s)
    if p < 1.0:
        s = TopPLogitsWarper(p)(ids, s)
    return v, torch.softmax(s[0], dim=-1)


# ---------------------------------------------------------------------------------------------------- vs transformers
@pytest.mark.parametrize("dtype", DTYPES)
def test_kept_set_and_draw_against_transformers_warpers(dtype):
    """fp32 Gaussian rows are tie-free: the kept set equals HF's.  bf16 rows tie: HF's sort cuts a tied group at the
    top-k / top-p boundary in an arbitrary place, the threshold rule keeps the whole group — HF's set is a subset and what
    is missing from it has the one value of the lowest kept token."""
    g = torch.Generator().manual_seed(3)
    V = 3000
    rows = 0
    for trial in range(4):
        pen, T = (1.3, 0.8) if trial % 2 else (1.0, 1.0)
        logits = (torch.randn(V, generator=g) * (1.0 + trial)).to(dtype)
        hist = torch.randint(0, V, (20,), generator=g).tolist() + [int(logits.float().argmax())] * 2
        v = SR.values(logits, hist, pen, T, True)
        for k in (0, 1, 20, 700, V - 1, V, V + 5):
            for frac in (None, 0.3, 0.9):
                p = 1.0 if frac is None else SR.mid_top_p(v, k, frac)
                dec = SR.decide(v, k, p)
                hv, probs = _hf(logits, hist, pen, T, min(k, V), p)
                assert torch.equal(hv.view(torch.int32), v.view(torch.int32))          # bit-equal values
                hf_kept = probs > 0
                rows += 1
                if dtype == torch.float32:
                    assert v.unique().numel() == V
                    assert torch.equal(hf_kept, dec["kept"]), (trial, k, p)
                else:
                    assert bool((hf_kept <= dec["kept"]).all()), (trial, k, p)
                    extra = dec["kept"] & ~hf_kept
                    if bool(extra.any()):
                        assert v[extra].unique().numel() == 1 and float(v[extra][0]) == float(v[dec["kept"]].min())
                if dtype == torch.float32:
                    # the draw: HF's multinomial over these probabilities, by inverse cdf at the same u
                    cdf = torch.cumsum(probs, 0)
                    for u in SR.mid_uniforms(v, k, p, 3):
                        want = int(torch.searchsorted(cdf, torch.tensor([u], dtype=torch.float64), right=True))
                        assert SR.decide(v, k, p, u)["token"] == want
    assert rows == 4 * 7 * 3


# ---------------------------------------------------------------------------------------------------- by hand
def test_hand_computed_rows():
    ln = math.log
    # weights 8 4 2 1 1 (total 16) at ids 2 0 4 1 3; mass strictly above each value: 8: 0, 4: 1/2, 2: 3/4, 1: 7/8
    v = torch.tensor([ln(4.0), 0.0, ln(8.0), 0.0, ln(2.0)])
    for p, kept in ((0.4, [2]), (0.5, [2]), (0.51, [0, 2]), (0.75, [0, 2]), (0.76, [0, 2, 4]), (0.875, [0, 2, 4]),
                    (0.88, [0, 1, 2, 3, 4]), (1.0, [0, 1, 2, 3, 4])):
        assert SR.decide(v, 0, p)["kept"].nonzero().reshape(-1).tolist() == kept, p
    # top-k: ties at the k-th value stay; k >= V is off
    for k, n in ((1, 1), (2, 2), (3, 3), (4, 5), (5, 5), (0, 5), (9, 5)):
        assert SR.decide(v, k, 1.0)["n_kept"] == n, k
    # top-k first, top-p over the survivors: k = 3 leaves 8 4 2 (total 14): above 4 is 8/14, above 2 is 12/14
    assert SR.decide(v, 3, 0.58)["kept"].nonzero().reshape(-1).tolist() == [0, 2]
    assert SR.decide(v, 3, 0.57)["kept"].nonzero().reshape(-1).tolist() == [2]
    d = SR.decide(v, 3, 0.7)
    assert abs(d["p_margin"] - (0.7 - 8 / 14)) < 1e-7 and d["thr_d"] == pytest.approx(ln(2.0))
    # the draw in id order: cumulative 4 5 13 14 16 of 16 -> edges 1/4 5/16 13/16 7/8
    for u, tok in ((0.0, 0), (0.2, 0), (0.26, 1), (0.32, 2), (0.8, 2), (0.82, 3), (0.9, 4), (1.0, 4)):
        assert SR.decide(v, 0, 1.0, u)["token"] == tok, u
    assert SR.decide(v, 0, 1.0, 0.5)["u_margin"] == pytest.approx(0.1875)
    assert SR.decide(v, 0, 0.51, 0.7)["token"] == 2                       # kept 0 and 2: edges 1/3, 1
    # weights that vanish in 2^-40 fixed point are kept but never drawn, at either end
    v = torch.tensor([-50.0, 0.0, -1.0, float("-inf"), -45.0, -60.0])
    d0, d1 = SR.decide(v, 0, 1.0, 0.0), SR.decide(v, 0, 1.0, 1.0)
    assert d0["n_kept"] == 6 and d0["token"] == 1 and d1["token"] == 2 and not d0["exact_count"]
    assert SR.decide(v, 4, 1.0, 0.5)["n_kept"] == 4 and SR.decide(v, 4, 1.0, 0.5)["thr_d"] == 50.0
    # the penalty: once per distinct id of [0, V), negative * p, others / p; then the temperature — in fp32
    v = SR.values(torch.tensor([2.0, -2.0, 0.0, 3.0, 1.0]), [0, 0, 1, 2, -1, 5, 2 ** 30, 0], 2.0, 0.5, True)
    assert v.tolist() == [2.0, -8.0, 0.0, 6.0, 2.0]
    assert SR.values(torch.tensor([2.0, -2.0]), [0, 1], 2.0, 0.5, False).tolist() == [1.0, -4.0]
    # rows without a finite maximum
    nan, inf = float("nan"), float("inf")
    assert SR.argmax(torch.tensor([1.0, inf, nan, nan])) == 2 and SR.argmax(torch.tensor([1.0, inf, 3.0, inf])) == 1
    assert SR.argmax(torch.tensor([-inf, -inf])) == 0 and SR.argmax(torch.tensor([1.0, 3.0, 3.0])) == 1


def test_hand_computed_bookkeeping():
    S = 4
    logits = torch.full((5, 6), -50.0)
    logits[:, 2] = 1.0                                                      # every live row draws 2, the eos
    hist = torch.zeros(5, S, dtype=torch.int32)
    hl = torch.tensor([1, S, S + 3, 2, -2], dtype=torch.int32)
    cl = torch.tensor([0, 3, 6, 1, 9], dtype=torch.int32)
    fin = torch.tensor([0, 0, 0, 1, 0], dtype=torch.int32)
    nu = torch.tensor([4], dtype=torch.int32)
    rows = SR.step(logits, hist, hl, cl, fin, nu, 1.0, True, 1.0, 0, 1.0, [2], 5, torch.full((5,), 0.5))
    assert [r["token"] for r in rows] == [2, 2, 2, 5, 2] and [r["n_kept"] for r in rows] == [6, 6, 6, 0, 6]
    assert hist.tolist() == [[0, 2, 0, 0], [0] * 4, [0] * 4, [0, 0, 5, 0], [2, 0, 0, 0]]
    assert hl.tolist() == [2, S, S + 3, 3, 1] and cl.tolist() == [1, 3, 6, 2, 10]
    assert fin.tolist() == [1] * 5 and int(nu) == 0                         # the full rows finished too; row 3 once only
    rows = SR.step(logits, hist, hl, cl, fin, nu, do_sample=False)
    assert [r["token"] for r in rows] == [0] * 5 and int(nu) == 0


# ---------------------------------------------------------------------------------------------------- the planted cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_cases_keep_their_margins(dtype):
    cases = SR.edge_cases(dtype)
    for c in cases:
        for b, r in enumerate(c["rows"]):
            if "kept" not in r:
                continue                                     # greedy, finished, or no finite maximum: nothing is weighed
            tag = (c["name"], b)
            assert r["p_margin"] >= SR.MARGIN, (tag, r["p_margin"])
            if r["exact_count"]:
                assert r["d_gap_ok"], tag                    # fp32 d separates the lowest kept from the highest dropped
            u = c["uniforms"][b]
            if c["planted_u"] and u in (0.0, 1.0, SR.ONE_BELOW):
                # the first / last kept token of nonzero weight is unambiguous: no kept token between d = 20 and d = 40
                d = r["d"][r["kept"]]
                assert bool(((d <= 20.0) | (d >= 40.0)).all()), tag
                # and the last unit of mass below 1 belongs to a token whose share is far above 2^-24
                assert float(1.0 - r["edges"][-2] if r["edges"].numel() > 1 else 1.0) >= 1e-4, tag
            else:
                assert r["u_margin"] >= SR.MARGIN, (tag, r["u_margin"])
            if c.get("floor_uV"):
                assert r["token"] == int(math.floor(u * c["logits"].shape[1])) and r["n_kept"] == c["logits"].shape[1]
        # (at T = 0.02 the 8th largest of a Gaussian row lies ~50 below the maximum: weight zero, but short of the last bin)
        if c["name"].startswith("far_tail") and not c["name"].endswith("_p") and c["name"] != "far_tail_T0.02_k8":
            assert all(not r["exact_count"] for r in c["rows"]), c["name"]
    # what the rows were planted for, by the reference's own numbers
    by = {c["name"]: c for c in cases}
    assert by["tied_bin_k1500"]["rows"][0]["n_kept"] == 3001 and by["tied_bin_k600"]["rows"][0]["n_kept"] == 3001
    assert by["tied_bin_k3500"]["rows"][0]["n_kept"] == 5501 and by["tied_bin_p"]["rows"][0]["n_kept"] == 3001
    assert by["compact_overflow"]["rows"][0]["n_kept"] == 2300
    assert by["top_k_V-1"]["rows"][0]["n_kept"] == 1499 and by["top_k_V+1"]["rows"][0]["n_kept"] == 1500
    assert [r["token"] for r in by["neg_inf_one_finite"]["rows"]] == [37] * 3
    assert [r["token"] for r in by["neg_inf_all"]["rows"]] == [0, 0] and by["one_nan"]["rows"][0]["token"] == 55
    assert by["nans_and_inf"]["rows"][0]["token"] == 20 and by["pos_inf"]["rows"][0]["token"] == 9
    assert by["nans_and_inf_greedy"]["rows"][0]["token"] == 20 and by["neg_inf_all_greedy"]["rows"][0]["token"] == 0
    for k in (0, 40):
        r = by[f"top_p_tiny_k{k}"]["rows"]
        assert [x["token"] for x in r] == [7, 2995] and r[0]["n_kept"] == 2
    for k in (50, 0, 1100):
        r = by[f"draw_edges_k{k}"]["rows"]
        assert [x["token"] for x in r[:3]] == [3, 2996, 2996] and bool(r[0]["kept"][0]) and bool(r[0]["kept"][2999])
    for n in ("neg_inf_half_k1500", "neg_inf_half_k1010", "neg_inf_half_plain", "neg_inf_from_constrain"):
        r = by[n]["rows"]
        assert all(math.isfinite(float(x["values"][x["token"]])) for x in r), n
        assert r[0]["n_kept"] == 2000 or n == "neg_inf_from_constrain"          # (that one also cuts with top_p)
        assert r[0]["token"] < r[1]["token"] == r[2]["token"]
    if dtype == torch.float32:
        for k in (1000, 1024, 1025, 3000):
            assert by[f"three_levels_k{k}"]["rows"][0]["n_kept"] == k
            assert k // 4 < by[f"three_levels_k{k}_p"]["rows"][0]["n_kept"] < k
    h = by["history_pen1.75"]
    assert sorted(h["rows"][0]["kept"].nonzero().reshape(-1).tolist()) == [5, 11, 20, 30, 40]
    assert [r["token"] for r in h["rows"][2:5]] == [777, 777, 3] and h["want"]["hl"].tolist()[2:5] == [12, 15, 3]
    assert int(h["want"]["nu"]) == 3 and h["want"]["fin"].tolist() == [0, 0, 1, 1, 1, 0]
    assert by["history_greedy_pen1.75"]["rows"][0]["token"] == 5 and by["history_greedy_pen0.5"]["rows"][0]["token"] == 5
    assert sorted(by["history_pen0.5"]["rows"][0]["kept"].nonzero().reshape(-1).tolist()) == [5, 9, 11, 20, 30]


@pytest.mark.parametrize("dtype", DTYPES)
def test_kimi_planted_cases_keep_their_margins(dtype):
    for c in SR.kimi_edge_cases(dtype):
        k = c["top_k"]
        for b, row in enumerate(c["rows"]):
            edges = KR.boundaries(row, c["T"], k)
            u = c["uniforms"][b]
            assert min([abs(u - float(e)) for e in edges[:-1].tolist()] + [1.0]) >= SR.KIMI_MARGIN, (c["name"], b)
    by = {c["name"]: c for c in SR.kimi_edge_cases(dtype)}
    # the tied maximum: the candidates are the k lowest of its ids, in id order
    for k in (32, 64):
        c = by[f"kimi_3000_tied_k{k}"]
        cv, ci = KR.candidates(c["rows"][0], k)
        tied = (c["rows"][0].double() == cv[0]).nonzero().reshape(-1)
        assert tied.numel() >= 2990 and ci.tolist() == tied[:k].tolist() and len(set((tied % 1024).tolist())) == 20
    cv, ci = KR.candidates(by["kimi_3000_ranked_k64"]["rows"][0], 64)
    assert bool((cv[1:] <= cv[:-1]).all()) and len(set((ci % 1024).tolist())) <= 20
    cv, _ = KR.candidates(by["kimi_neg_inf_k5"]["rows"][0], 5)
    assert int(torch.isinf(cv).sum()) == 2
