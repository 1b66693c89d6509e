"""The loss path — csrc/cross_entropy.hip and functional._FusedLinearCE — against the float64 restatements of
tests/loss_reference.py.  Every comparison goes through `check` (half an ulp of the output's dtype, the project's fp32
allowance of the uncancelled terms, the documented roundings of the path) and prints its `measured:` line; DESIGN.md 5,
"Measured error of the loss path", is filled from those lines.

A row block has 256 threads that read 16 bytes (N = 8 bf16 / 4 fp32 elements) per step: one lap is 256 N elements, a row
takes the vector path when V % N == 0 and its base is 16-byte aligned, else the scalar one (thread = index % 256).
tests/test_loss_reference_cpu.py shows that these checks fail on a wrong label, a neighbour's sentence_lens, a dropped
row or chunk, a tie resolved upwards and a reduction that stops at row 1024."""
import functools

import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
VEC = R.VEC
NS, G = 7, 1.0 / 3.0
IGN = -100
GUARD = 777.0
NEG = float("-inf")


def _F():
    import touchnet_amd.functional as F
    return F


def _L():
    import touchnet_amd.library as L
    return L


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _scalars(g=G):
    return torch.tensor([float(NS)], device=DEV), torch.tensor([g], dtype=F32, device=DEV)


def _place(x, offset):
    """x [n, V] on the device as a view that starts `offset` elements into a buffer, with GUARD on either side"""
    flat = torch.full((offset + x.numel() + 8,), GUARD, dtype=x.dtype, device=DEV)
    view = flat[offset:offset + x.numel()].view(x.shape)
    view.copy_(x)
    return flat, view


def _guards_ok(flat, offset, numel):
    return bool((flat[:offset] == GUARD).all()) and bool((flat[offset + numel:] == GUARD).all())


def _rows(dtype, V, n=8, seed=0, spread=3.0):
    """n rows of logits, a label in the first and in the last column, rows 3 and 6 ignored, sentence_lens 1 .. 9"""
    gen = torch.Generator().manual_seed(seed * 1000003 + V)
    x = (spread * torch.randn(n, V, generator=gen)).to(dtype)
    lab = torch.randint(0, V, (n,), generator=gen)
    lab[0], lab[1] = 0, V - 1
    lab[3] = lab[6] = IGN
    sl = torch.randint(1, 10, (n,), generator=gen)
    sl[2] = 9
    return x, lab, sl


def _run_ce(x, lab, sl, what, offset=0):
    """Every entry point of the kernels on one set of rows against ce_rows; the in-place and the autograd forms must give
    the bits of the plain ones, a second launch the bits of the first, and nothing outside the rows may be written."""
    F, L = _F(), _L()
    dtype = x.dtype
    what = f"{'bf16' if dtype == BF16 else 'fp32'} logits, {what}"
    flat, xd = _place(x, offset)
    lab_d, sl_d = _dev(lab, sl)
    ns, g = _scalars()
    loss, stats, lse = L.ce_fwd(xd, lab_d, sl_d, ns, IGN)
    nll, lse_r, hit = L.ce_fwd_rows(xd, lab_d, sl_d, ns, IGN)
    r = R.ce_rows(x, lab, sl, NS, G, lse=lse)
    R.check(lse, r["lse"], F32, f"{what} lse")
    R.check(nll, r["nll"], F32, f"{what} nll")
    assert torch.equal(hit.cpu().to(R.F64), r["hit"].value), f"{what}: hit"
    for i, k in enumerate(("per_sample", "per_token", "accuracy")):
        R.check(stats[i:i + 1], r[k], F32, f"{what} {k}")
    assert float(stats[3]) == float(r["n_valid"].value), f"{what}: n_valid"
    hits, cnt = torch.tensor(float(r["hit"].value.sum()), dtype=F32), torch.tensor(float(r["n_valid"].value), dtype=F32)
    assert float(stats[2]) == float(hits / cnt), f"{what}: accuracy"           # exact: one fp32 division of two counts
    assert torch.equal(loss, stats[0]) and torch.equal(lse, lse_r)
    assert torch.equal(L.ce_reduce(nll, hit, lab_d, sl_d, ns, IGN), stats)
    again = L.ce_fwd(xd, lab_d, sl_d, ns, IGN)
    assert all(torch.equal(a, b) for a, b in zip(again, (loss, stats, lse))), f"{what}: forward not repeatable"

    dl = L.ce_bwd(xd, lab_d, sl_d, lse, ns, g, IGN)
    R.check(dl, r["dlogits"], dtype, f"{what} dlogits")
    dl_c = dl.cpu()
    assert bool((dl_c[lab == IGN] == 0).all()), f"{what}: gradient of an ignored row"
    assert bool((dl_c[x == NEG] == 0).all()), f"{what}: gradient at a -inf logit"
    assert torch.equal(L.ce_bwd(xd, lab_d, sl_d, lse, ns, g, IGN), dl), f"{what}: backward not repeatable"
    assert torch.equal(xd.cpu(), x) and _guards_ok(flat, offset, x.numel()), f"{what}: forward / backward wrote outside"

    flat2, x2 = _place(x, offset)                              # in place, same alignment
    L.ce_bwd_(x2, lab_d, sl_d, lse, ns, g, IGN)
    assert torch.equal(x2, dl), f"{what}: ce_bwd_ differs from ce_bwd"
    assert _guards_ok(flat2, offset, x.numel()), f"{what}: ce_bwd_ wrote outside the rows"

    for inplace in (False, True):                              # autograd: packed_cross_entropy
        flat3, x3 = _place(x, offset)
        leaf = x3.requires_grad_()
        l3, st3 = F.packed_cross_entropy(leaf, lab_d, sl_d, NS, IGN, inplace_grad=inplace)
        assert torch.equal(l3.detach(), loss) and torch.equal(st3, stats)
        (l3 * G).backward()
        assert torch.equal(leaf.grad, dl), f"{what}: packed_cross_entropy(inplace_grad={inplace}) differs from ce_bwd"
        assert _guards_ok(flat3, offset, x.numel())
    return r


# ------------------------------------------------------------------------------------------------------ widths
# bf16: 1 lap = 2048; fp32: 1 lap = 1024.  One element, one short of a vector, one vector; one vector short of a lap, one
# element short (scalar), the lap, one vector more, two laps and a vector; an odd width; the largest vocabulary in use.
WIDTHS = [(BF16, V) for V in (1, 7, 8, 2040, 2047, 2048, 2056, 4104, 1003, 168448)] + \
         [(F32, V) for V in (1, 3, 4, 1020, 1023, 1024, 1028, 2052, 1003)]


@pytest.mark.parametrize("dtype, V", WIDTHS, ids=lambda p: str(p).replace("torch.", ""))
def test_ce_vocabulary_widths(dtype, V):
    x, lab, sl = _rows(dtype, V)
    _run_ce(x, lab, sl, f"V={V}")


@pytest.mark.parametrize("dtype, V", [(BF16, 2056), (F32, 1028)], ids=["bf16", "fp32"])
def test_ce_misaligned_base(dtype, V):
    """V % N == 0 but the rows start one element past a 16-byte boundary: the scalar branch of the forward, of both
    backward forms and of the zero fill, and not one element before or after the rows is touched"""
    x, lab, sl = _rows(dtype, V, seed=1)
    assert V % VEC[dtype] == 0
    _run_ce(x, lab, sl, "misaligned", offset=1)


# ------------------------------------------------------------------------------------------------------ ties
def _tie_rows(dtype, V, pairs):
    """per pair (lo, hi) two rows with the row's largest value at both: label lo (hit) and label hi (no hit); then two
    rows of all-equal logits, label 0 (hit) and label 5 (no hit)"""
    gen = torch.Generator().manual_seed(11)
    n = 2 * len(pairs) + 2
    x = torch.randn(n, V, generator=gen).to(dtype)
    lab = torch.zeros(n, dtype=torch.int64)
    for k, (lo, hi) in enumerate(pairs):
        for j in (0, 1):
            x[2 * k + j, lo] = x[2 * k + j, hi] = 40.0
            lab[2 * k + j] = (lo, hi)[j]
    x[-2:] = 1.5
    lab[-2], lab[-1] = 0, 5
    sl = torch.randint(1, 10, (n,), generator=gen)
    expect = torch.tensor([1.0, 0.0] * (len(pairs) + 1), dtype=R.F64)
    return x, lab, sl, expect


# (lo, hi): the LOWER index sits in the HIGHER thread, so a merge that ignored the index would keep `hi`.
#   vector path, thread of index i = (i // N) % 256:
#     bf16  9 -> thread 1, 2050 -> thread 0 (second lap): same wave;   513 -> thread 64 (wave 1), 2072 -> thread 3 (wave 0)
#     fp32  5 -> thread 1, 1026 -> thread 0 (second lap): same wave;   257 -> thread 64 (wave 1), 1036 -> thread 3 (wave 0)
#   scalar path (V = 1003), thread = i % 256:  9 -> thread 9, 258 -> thread 2;   70 -> thread 70 (wave 1), 259 -> thread 3
TIES = [(BF16, 4104, [(9, 2050), (513, 2072)]), (F32, 2052, [(5, 1026), (257, 1036)]),
        (BF16, 1003, [(9, 258), (70, 259)]), (F32, 1003, [(9, 258), (70, 259)])]


@pytest.mark.parametrize("dtype, V, pairs", TIES, ids=["bf16-vec", "fp32-vec", "bf16-scalar", "fp32-scalar"])
def test_ce_ties_go_to_the_first_index(dtype, V, pairs):
    N = VEC[dtype]
    thread = (lambda i: (i // N) % 256) if V % N == 0 else (lambda i: i % 256)
    (a, b), (c, e) = pairs
    assert thread(a) > thread(b) and thread(a) // 64 == thread(b) // 64                # same wave
    assert thread(c) // 64 > thread(e) // 64                                           # across waves
    x, lab, sl, expect = _tie_rows(dtype, V, pairs)
    r = _run_ce(x, lab, sl, "ties")
    assert torch.equal(r["hit"].value, expect) and float(r["accuracy"].value) == 0.5


# ------------------------------------------------------------------------------------------------------ extremes
@pytest.mark.parametrize("dtype, V", [(BF16, 4104), (BF16, 1003), (F32, 2052), (F32, 1003)],
                         ids=["bf16-vec", "bf16-scalar", "fp32-vec", "fp32-scalar"])
def test_ce_extreme_logits_and_minus_infinity(dtype, V):
    """Logits over the whole range a model can produce, and -inf (masked / padded vocabulary entries) where a thread's
    running max is still -inf: index 0, the first element of a thread's second lap, every other column.  Finite results
    equal to the reference, gradient exactly 0 at the -inf entries (asserted in _run_ce)."""
    N = VEC[dtype]
    lap = 256 * N if V % N == 0 else 256
    gen = torch.Generator().manual_seed(13)
    n = 10
    x = (3 * torch.randn(n, V, generator=gen)).to(dtype)
    lab = torch.randint(0, V, (n,), generator=gen)
    sl = torch.randint(1, 10, (n,), generator=gen)
    if dtype == BF16:
        x[0] = (torch.rand(V, generator=gen) * 6e4 - 3e4).to(dtype)    # +-3e4, label anywhere
        x[1] = (torch.rand(V, generator=gen) * 6e4 - 3e4).to(dtype)
    else:
        x[0] = torch.rand(V, generator=gen) * 160 - 80                  # +-80
        x[1] = torch.rand(V, generator=gen) * 5.9e4 - 3e4               # +-3e4, the row's maximum at the label
        x[1, lab[1]] = 3e4
    x[2, 0] = NEG                                                       # thread 0's first element
    x[3, lap] = NEG                                                     # thread 0's first element of its second lap
    x[3, :N] = NEG                                                      # ... after a first lap of -inf only
    x[4, 0] = x[4, lap] = NEG
    x[5, ::2] = NEG                                                     # half of all columns
    x[6, :lap] = NEG                                                    # every thread starts on -inf
    lab[2], lab[3], lab[4], lab[5], lab[6] = V - 1, lap + 1, 1, 1, lap + 1     # labels on finite logits
    lab[7] = IGN
    x[7, 0] = NEG
    assert bool(torch.isfinite(x[torch.arange(n)[lab != IGN], lab[lab != IGN]]).all())
    r = _run_ce(x, lab, sl, "extremes")
    assert bool(torch.isfinite(r["nll"].value).all())


# ------------------------------------------------------------------------------------------------------ reduction
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2500])
def test_ce_reduction_over_more_rows_than_threads(n):
    """ce_reduce_kernel is one block of 1024 threads that strides over the rows"""
    L = _L()
    V = 8
    gen = torch.Generator().manual_seed(n)
    x = (3 * torch.randn(n, V, generator=gen)).to(BF16)
    lab = torch.randint(0, V, (n,), generator=gen)
    lab[torch.randperm(n, generator=gen)[:n // 7]] = IGN
    lab[n - 1] = 3                                                      # the last row counts
    sl = torch.randint(1, 10, (n,), generator=gen)
    xd, lab_d, sl_d = _dev(x, lab, sl)
    ns, _ = _scalars()
    loss, stats, lse = L.ce_fwd(xd, lab_d, sl_d, ns, IGN)
    r = R.ce_rows(x, lab, sl, NS, G)
    for i, k in enumerate(("per_sample", "per_token", "accuracy")):
        R.check(stats[i:i + 1], r[k], F32, f"n={n} {k}")
    assert float(stats[3]) == float((lab != IGN).sum())
    # the reduction alone, from given rows
    nll = (torch.rand(n, generator=gen) * 5).float()
    hit = (torch.rand(n, generator=gen) < 0.5).to(torch.int32)
    s = R.ce_stats(nll, hit, lab, sl, NS)
    out = L.ce_reduce(*_dev(nll, hit, lab, sl), ns, IGN)
    for i, k in enumerate(("per_sample", "per_token", "accuracy")):
        R.check(out[i:i + 1], s[k], F32, f"n={n} ce_reduce {k}")
    assert float(out[3]) == float(s["n_valid"].value)
    assert torch.equal(L.ce_reduce(*_dev(nll, hit, lab, sl), ns, IGN), out)


def test_ce_reduction_small_sum_and_nothing_labelled():
    F, L = _F(), _L()
    n = 1025
    ns, g = _scalars()
    lab = torch.arange(n) % 8
    sl = torch.full((n,), 3)
    nll = torch.full((n,), 1e-10)                                      # sum 1.0e-7 <= 1e-6: per_token is 0
    hit = torch.ones(n, dtype=torch.int32)
    s = R.ce_stats(nll, hit, lab, sl, NS)
    out = L.ce_reduce(*_dev(nll, hit, lab, sl), ns, IGN)
    assert float(s["per_token"].value) == 0.0 and float(out[1]) == 0.0
    R.check(out[0:1], s["per_sample"], F32, "small sum per_sample")
    assert float(out[0]) > 0 and float(out[2]) == 1.0 and float(out[3]) == n
    # everything ignored
    none = torch.full((n,), IGN)
    x = torch.randn(n, 8).to(BF16).to(DEV).requires_grad_()
    loss, stats = F.packed_cross_entropy(x, none.to(DEV), sl.to(DEV), NS)
    (loss * G).backward()
    assert stats.tolist() == [0.0, 0.0, 0.0, 0.0] and float(loss) == 0.0 and bool((x.grad == 0).all())
    out = L.ce_reduce(*_dev(nll, hit, none, sl), ns, IGN)
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------------ lm_head + CE
# name: (n, H, V, chunk, ignored rows).  Which GEMM takes each product of each chunk when ALL rows run (`compact` False;
# confirmed from F._own / F.split_k by test_fused_shapes_take_the_routes_they_are_here_for — the compacted forms run the
# labelled rows only, in chunks of 512 + 19 ("own"), 128 + 128 + 4 ("lib") and 76 ("one") rows plus fillers, on whatever
# those sizes are routed to):
#   own   chunks of 512 + 89 rows.  logits: own kernel both chunks (2 x 96 and 1 x 96 tiles); d(weight): own kernel both
#         chunks (96 tiles), ACCUMULATING in the epilogue into the fp32 buffer, the second with an odd contraction depth
#         of 89; d(hidden): own kernel cut 48 ways along V on the full chunk (2 tiles x 48), the library on the last one
#         (1 tile x 48 < 96)
#   lib   chunks of 128 + 128 + 44 rows, every product on the library (9 tiles; V = 2056 is no multiple of 64)
#   one   one chunk of 96 rows, library
SHAPES = {"own": (601, 256, 24576, 512, 70), "lib": (300, 64, 2056, 128, 40), "one": (96, 64, 1000, 4096, 20)}


def test_fused_shapes_take_the_routes_they_are_here_for():
    F = _F()
    route = lambda m, H, V: (F._own(m, V, (H,)), F._own(m, H, (V,)), F._own(V, H, (m,), True, True))
    n, H, V, chunk, _ = SHAPES["own"]
    assert F.LINEAR_GEMM == "own" and F.SPLIT_K
    assert route(chunk, H, V) == (True, True, True) and route(n - chunk, H, V) == (True, False, True)
    assert (n - chunk) % 2 == 1 and F.split_k(chunk, H, V, False, True) == 48 and F.split_k(chunk, V, H, False, False) == 1
    for name in ("lib", "one"):
        n, H, V, chunk, _ = SHAPES[name]
        for m in {min(chunk, n), n % chunk or min(chunk, n)}:
            assert route(m, H, V) == (False, False, False)


def _compact_forms(n, count):
    return {"False": False, "True": True, "count": count, "count-up-256": -(-count // 256) * 256, "n+100": n + 100}


@functools.lru_cache(maxsize=1)          # (the case at hand: its compact forms come one after the other)
def _fused_case(name, row0, g):
    n, H, V, chunk, n_ign = SHAPES[name]
    h, w, lab, sl = R.fused_inputs(n, H, V, n_ign, row0, seed=list(SHAPES).index(name))
    return h, w, lab, sl, R.fused_linear_ce(h, w, lab, sl, NS, g)


def _fused(h, w, lab, sl, chunk, compact, g):
    F = _F()
    hd, wd = h.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    loss, stats = F.fused_linear_cross_entropy(hd, wd, lab.to(DEV), sl.to(DEV), NS, IGN, chunk_tokens=chunk,
                                               compact=compact)
    (loss if g == 1.0 else loss * g).backward()
    return loss.detach(), stats, hd.grad, wd.grad


@pytest.mark.parametrize("form", ["False", "True", "count", "count-up-256", "n+100"])     # (varies fastest)
@pytest.mark.parametrize("g", [1.0, G], ids=["g=1", "g=1/3"])
@pytest.mark.parametrize("row0", [True, False], ids=["row0-labelled", "row0-ignored"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_linear_ce(name, form, row0, g):
    n, H, V, chunk, n_ign = SHAPES[name]
    compact = _compact_forms(n, n - n_ign)[form]
    h, w, lab, sl, ref = _fused_case(name, row0, g)
    loss, stats, dh, dw = _fused(h, w, lab, sl, chunk, compact, g)
    what = f"fused {name} compact={form}"
    assert torch.equal(loss, stats[0])
    for i, k in enumerate(("per_sample", "per_token", "accuracy")):
        R.check(stats[i:i + 1], ref[k], F32, f"{what} {k}")
    assert float(stats[3]) == n - n_ign
    R.check(dh, ref["dhidden"], BF16, f"{what} d(hidden)", roundings=2)
    R.check(dw, ref["dweight"], BF16, f"{what} d(weight)", roundings=2)
    assert dh.dtype == BF16 and dw.dtype == BF16
    assert bool((dh.cpu()[lab == IGN] == 0).all()), "d(hidden) of an ignored row"


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_linear_ce_bound_too_small_and_nothing_labelled(name):
    n, H, V, chunk, n_ign = SHAPES[name]
    h, w, lab, sl, _ = _fused_case(name, True, 1.0)
    loss, stats, dh, dw = _fused(h, w, lab, sl, chunk, n - n_ign - 1, 1.0)      # one below the count
    assert all(bool(torch.isnan(t.float()).all()) for t in (loss, stats, dh, dw))
    none = torch.full_like(lab, IGN)
    for compact in (False, True, 64):
        loss, stats, dh, dw = _fused(h, w, none, sl, chunk, compact, G)
        assert float(loss) == 0.0 and stats.tolist() == [0.0, 0.0, 0.0, 0.0]
        assert bool((dh == 0).all()) and bool((dw == 0).all())
