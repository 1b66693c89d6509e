"""csrc/edit_align.hip (tn_edit_align) on the device: the scorer's edit-distance alignment, exact arcs and counts.

Everything here is integer and exact: there is no tolerance.  The yardsticks are the reference's own arcs
(tests/golden/error_rate/edit_align.npz) and, for the shapes the fixture does not hold, the plain-Python restatement of its
tie rule (tests/edit_align_reference.py; tests/test_error_rate_cpu.py holds the restatement to the fixture).  The shapes sit
where the kernel changes behaviour: the 64-column strip (H = 63, 64, 65, 127, 128, 129), the 16-row packed word (R = 15,
16, 17), a single row, the 64-row chunk of the carry column (R = 63, 64, 65, 200), an empty hypothesis (no forward launch),
more than one workgroup, and R > 2048 (the carry column in the workspace rather than LDS) once, in a pair checked by
invariants.  Two-symbol alphabets make ties in almost every cell, so a tie-breaking mistake shows there."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import edit_align_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "error_rate")
EDGE_R = (1, 15, 16, 17, 63, 64, 65, 200)
EDGE_H = (0, 1, 63, 64, 65, 127, 128, 129)


def _F():
    import touchnet_amd.functional as F
    return F


def _check(got, ref, hyp, what):
    """one device result against the restatement"""
    ops, counts, _ = R.align(ref, hyp)
    assert got[4].tolist() == ops, what
    assert tuple(got[:4]) == counts, what


def _rand(rng, alphabet, n):
    return [rng.randrange(alphabet) for _ in range(n)]


def test_every_fixture_pair_equals_the_reference(golden):
    g = golden(os.path.join("error_rate", "edit_align.npz"))
    out = _F().edit_align(torch.from_numpy(g["ref_tok"]), torch.from_numpy(g["hyp_tok"]), g["ref_off"], g["hyp_off"])
    assert len(out) == g["counts"].shape[0]
    for p, (c, s, i, d, ops) in enumerate(out):
        assert ops.tolist() == g["ops"][g["ops_off"][p]:g["ops_off"][p + 1]].tolist(), p
        assert (c, s, i, d) == tuple(g["counts"][p].tolist()) and -float(s + i + d) == float(g["score"][p]), p
    assert R.letters(out[0][4]) == "DCI" and R.letters(out[1][4]) == "CDC"          # the two witnesses of the tie rule


@pytest.mark.parametrize("alphabet", [2, 50])
def test_shape_edges_against_the_restatement(alphabet):
    rng = random.Random(100 + alphabet)
    refs, hyps = [], []
    for r in EDGE_R:
        for h in EDGE_H:
            refs.append(_rand(rng, alphabet, r))
            hyps.append(_rand(rng, alphabet, h))
    out = _F().edit_align(refs, hyps)
    for ref, hyp, got in zip(refs, hyps, out):
        _check(got, ref, hyp, (len(ref), len(hyp), alphabet))


def test_identical_disjoint_and_empty_hypotheses():
    rng = random.Random(7)
    same = [_rand(rng, 3, n) for n in (1, 16, 64, 65, 200)]
    refs = same + same + same
    hyps = [list(s) for s in same] + [[t + 10 for t in s[:max(1, len(s) - 3)]] for s in same] + [[] for _ in same]
    out = _F().edit_align(refs, hyps)
    for k, s in enumerate(same):
        n = len(s)
        assert out[k][:4] == (n, 0, 0, 0) and out[k][4].tolist() == [R.C] * n                       # identical: all C
        _check(out[5 + k], refs[5 + k], hyps[5 + k], ("disjoint", n))
        assert out[5 + k][0] == 0 and out[5 + k][1] + out[5 + k][3] == n                             # disjoint: no C
        assert out[10 + k][:4] == (0, 0, 0, n) and out[10 + k][4].tolist() == [R.D] * n              # empty hypothesis: all D


def test_a_700_by_700_pair_of_two_symbols():
    rng = random.Random(700)
    ref, hyp = _rand(rng, 2, 700), _rand(rng, 2, 700)
    _check(_F().edit_align([ref], [hyp])[0], ref, hyp, "700 x 700")


def _levenshtein(ref, hyp):
    """row-vectorised: the diagonal and deletion candidates at once, the insertion chain as a running minimum"""
    ref, hyp = np.asarray(ref), np.asarray(hyp)
    j = np.arange(hyp.size + 1)
    row = j.copy()
    for r in range(ref.size):
        cand = np.minimum(row[1:] + 1, row[:-1] + (hyp != ref[r]))
        cand = np.concatenate([[row[0] + 1], cand])
        row = np.minimum.accumulate(cand - j) + j
    return int(row[-1])


def _check_invariants(ref, hyp, got):
    """what every alignment of minimal cost has: the counts add up to the two lengths, the edits to the edit distance, and
    replaying the arcs regenerates both sequences"""
    c, s, i, d, ops = got
    assert c + s + d == len(ref) and c + s + i == len(hyp) and ops.size == c + s + i + d
    assert np.bincount(ops, minlength=4).tolist() == [c, s, i, d]
    assert s + i + d == _levenshtein(ref, hyp)
    r = h = 0
    for code in ops.tolist():
        if code in (R.C, R.S):
            assert (ref[r] == hyp[h]) == (code == R.C), (r, h)
        r += code != R.I
        h += code != R.D
    assert (r, h) == (len(ref), len(hyp))


def test_a_1500_by_1300_pair_by_invariants():
    assert _levenshtein(list(b"kitten"), list(b"sitting")) == 3 and _levenshtein([1, 2], []) == 2
    rng = random.Random(1501)
    ref, hyp = _rand(rng, 2, 1500), _rand(rng, 2, 1300)
    _check_invariants(ref, hyp, _F().edit_align([ref], [hyp])[0])


def test_a_pair_with_more_rows_than_the_lds_carry_column_by_invariants():
    """2100 x 1300, a noisy copy: above 2048 rows the carry column between the 21 strips lives in the workspace"""
    rng = random.Random(2100)
    ref = _rand(rng, 4, 2100)
    hyp = [t if rng.random() > 0.3 else rng.randrange(4) for t in ref if rng.random() > 0.2][:1300]
    hyp += _rand(rng, 4, 1300 - len(hyp))
    _check_invariants(ref, hyp, _F().edit_align([ref], [hyp])[0])


def test_a_shuffled_batch_split_into_several_launches(monkeypatch):
    import touchnet_amd.library as L
    rng = random.Random(300)
    refs, hyps = [], []
    for n in range(300):
        alphabet = (2, 5, 50)[n % 3]
        r = rng.choice((1, 3, 16, 17, 40, 64, 90, 130))
        ref = _rand(rng, alphabet, r)
        hyp = [t for t in ref if rng.random() > 0.15] if n % 2 else _rand(rng, alphabet, rng.choice((0, 1, 30, 64, 65, 150)))
        refs.append(ref)
        hyps.append(hyp)
    launches = []
    real = L.edit_align
    monkeypatch.setattr(L, "edit_align", lambda *a: (launches.append(a[2].shape[0]), real(*a))[1])
    cap = 4 * 9 * 192 * 3                                   # three of the heaviest pairs (130 x 150: 9 x 192 words) per launch
    out = _F().edit_align(refs, hyps, workspace_bytes=cap)
    assert len(launches) > 3 and sum(launches) == 300
    assert len(out) == 300
    launches.clear()
    for n, (ref, hyp, got) in enumerate(zip(refs, hyps, out)):
        alone = _F().edit_align([ref], [hyp])[0]
        assert got[:4] == alone[:4] and got[4].tolist() == alone[4].tolist(), n        # and so in the input order
        assert got[0] + got[1] + got[3] == len(ref) and got[0] + got[1] + got[2] == len(hyp), n
    for n in range(0, 300, 7):
        _check(out[n], refs[n], hyps[n], n)


def test_nothing_is_written_outside_the_arcs_and_the_workspace():
    """the bytes of `ops` left of each pair's right-aligned arcs, a canary after `ops`, after the workspace and after
    `counts`, and the token arrays come back as they went in"""
    from touchnet_amd import _C
    lib = _C.lib()
    rng = random.Random(11)
    shapes = [(200, 129), (65, 64), (17, 0), (1, 1), (64, 65), (16, 200)]
    refs = [_rand(rng, 2, r) for r, _ in shapes]
    hyps = [_rand(rng, 2, h) for _, h in shapes]
    words = [lib.tn_edit_align_ws_words(r, h) for r, h in shapes]
    gap = 5                                                 # unused words / bytes between the pairs' ranges
    desc, ws_base, ops_base, r0, h0 = [], 0, 0, 0, 0
    for (r, h), w in zip(shapes, words):
        desc.append([r0, r, h0, h, ws_base, ops_base])
        ws_base, ops_base, r0, h0 = ws_base + w + gap, ops_base + r + h + gap, r0 + r, h0 + h
    ws_words, n_ops, P, tail = ws_base, ops_base, len(shapes), 64
    CANARY_W, CANARY_B = 0x5A5A5A5A, 0xA5
    ws = torch.full((ws_words + tail,), CANARY_W, dtype=torch.int32, device=DEV)
    ops = torch.full((n_ops + tail,), CANARY_B, dtype=torch.uint8, device=DEV)
    counts = torch.full((P * 5 + tail,), -7, dtype=torch.int32, device=DEV)
    ref_tok = torch.tensor(sum(refs, []), dtype=torch.int32, device=DEV)
    hyp_tok = torch.tensor(sum(hyps, []), dtype=torch.int32, device=DEV)
    ref_before, hyp_before = ref_tok.clone(), hyp_tok.clone()
    desc_dev = torch.empty(P, 6, dtype=torch.int32, device=DEV)
    host = torch.tensor(desc, dtype=torch.int32)
    rc = lib.tn_edit_align(_C.ptr(ref_tok), ref_tok.numel(), _C.ptr(hyp_tok), hyp_tok.numel(), C.c_void_p(host.data_ptr()),
                           _C.ptr(desc_dev), P, _C.ptr(ws), ws_words, _C.ptr(ops), n_ops, _C.ptr(counts), _C.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(desc_dev.cpu(), host) and torch.equal(ref_tok, ref_before) and torch.equal(hyp_tok, hyp_before)
    ws, ops, counts = ws.cpu().numpy(), ops.cpu().numpy(), counts.cpu().numpy()
    assert (ws[ws_words:] == CANARY_W).all() and (ops[n_ops:] == CANARY_B).all() and (counts[P * 5:] == -7).all()
    for p, ((r, h), w, row) in enumerate(zip(shapes, words, desc)):
        want, (c, s, i, d), _ = R.align(refs[p], hyps[p])
        n = len(want)
        assert counts[p * 5:p * 5 + 5].tolist() == [c, s, i, d, n], p
        lo, hi = row[5], row[5] + r + h
        assert ops[hi - n:hi].tolist() == want, p
        assert (ops[lo:hi - n] == CANARY_B).all() and (ops[hi:hi + gap] == CANARY_B).all(), p
        assert (ws[row[4] + w:row[4] + w + gap] == CANARY_W).all(), p
    # a refused table leaves everything as it is: pair 1's workspace one word into pair 0's
    bad = host.clone()
    bad[1, 4] -= gap + 1
    before = ops.copy()
    rc = lib.tn_edit_align(_C.ptr(ref_tok), ref_tok.numel(), _C.ptr(hyp_tok), hyp_tok.numel(), C.c_void_p(bad.data_ptr()),
                           _C.ptr(desc_dev), P, _C.ptr(torch.from_numpy(ws).to(DEV)), ws_words, _C.ptr(torch.from_numpy(ops).to(DEV)),
                           n_ops, _C.ptr(torch.from_numpy(counts).to(DEV)), _C.stream())
    torch.cuda.synchronize()
    assert rc == -22 and torch.equal(desc_dev.cpu(), host) and (ops == before).all()


@pytest.mark.parametrize("tokenizer", ["whitespace", "char"])
def test_corpus_details_are_the_reference_programs(tokenizer, tmp_path):
    from touchnet_amd.metrics import error_rate as E
    res = E.evaluate(E.load_utterances(os.path.join(GOLD, "ref.txt")), E.load_utterances(os.path.join(GOLD, "hyp.txt")), tokenizer)
    out = tmp_path / "DETAILS.txt"
    with open(out, "w+", encoding="utf8") as f:
        res.write_details(f)
    assert out.read_bytes() == open(os.path.join(GOLD, f"DETAILS_{tokenizer}.txt"), "rb").read()
    assert (res.to_json() + "\n" + res.to_kaldi() + "\n").encode("utf8") == open(os.path.join(GOLD, f"stdout_{tokenizer}.txt"),
                                                                                "rb").read()


def test_opcheck_of_the_op():
    from torch.library import opcheck
    ref = torch.tensor([0, 1, 0, 1, 1, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV)
    hyp = torch.tensor([1, 0, 1, 1, 0, 0, 1], dtype=torch.int32, device=DEV)
    desc = torch.tensor([[0, 6, 0, 4, 0, 0], [6, 4, 4, 3, 64, 10]], dtype=torch.int32)
    opcheck(torch.ops.mi355_touch.edit_align.default, (ref, hyp, desc))
    counts, ops = torch.ops.mi355_touch.edit_align(ref, hyp, desc)
    for p, (r0, r, h0, h, _, o0) in enumerate(desc.tolist()):
        want, n4, _ = R.align(ref[r0:r0 + r].tolist(), hyp[h0:h0 + h].tolist())
        assert counts[p].tolist() == [*n4, len(want)]
        assert ops[o0 + r + h - len(want):o0 + r + h].tolist() == want and not ops[o0:o0 + r + h - len(want)].any()
