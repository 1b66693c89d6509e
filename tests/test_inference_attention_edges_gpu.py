"""The three inference attention entry points — tn_attn_decode, tn_attn_decode_beam (csrc/attn_decode.hip) and
tn_attn_block_causal_fwd (csrc/attn_block_causal.hip) — against the float64 references and the derived error budgets of
tests/inference_attention_reference.py, through touchnet_amd.library.  Decode: every G in 1..16 at both D on the split
path, the length and split-count edges, a scale that is not D^-0.5 and logits of deviation 16, dense and through an
ancestry table, on planted inputs in which one lost key is worth O(1) and with NaN in every cache position at or past
cache_len and junk in every table entry there; the caches and a guard behind them bit for bit, cache_len untouched, a
second call bit-identical; refused lengths and out-of-range table entries.  Block-causal: single and packed clips whose
boundaries sit off the tile and block grids, with anchors and finite baits, exact zeros on rows without keys.
tests/test_inference_attention_reference_cpu.py shows on the CPU that a correct kernel can meet these budgets and that
kernels wrong by one key, one split weight, one table position, one block boundary or one rescale cannot.

MEASURED on an MI355X, the worst error as a multiple of the budget, and the case it occurred in:
    dense decode   0.995   units512: B = 64, 8 x 8 heads, D = 64, S_max = 140, one split, planted
    beam decode    0.996   the same case through its table
    block-causal   0.860   packed, T = 400, block = 50, six clips per row, B = 2, Nh = 3, planted
(the fp32 models of test_inference_attention_reference_cpu.py reach 0.995 / 0.996 / 0.860 in the same cases: decode's
budget is half a bf16 ulp of the output plus fp32 terms, so its worst ratio over some 10^5 outputs is that of the
unluckiest final rounding, which the model reproduces.)  The file's 191 tests take 5.3 s, the largest (the first, which
loads the library) 2.0 s and every other below 0.1 s.  Every test passed on the first run on the device: no budget term
was added after it, and no kernel was changed.  Two things differ from the issue that asked for this file, both settled
on the CPU before that run: the caches of the B Nkv = 171 and 256 cases cannot be smaller than 5.7 and 4.6 MB (three /
two splits need S_max >= 129 / 65), and the claim that one key lost among 1000 Gaussian keys passes the old decode
tolerance holds for about one loss in four only (test_inference_attention_reference_cpu.py states what is true)."""
import functools

import pytest
import torch

import inference_attention_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
I16 = torch.int16
_DIDS = [R.dcase_id(c) for c in R.DECODE_CASES]
_BIDS = [R.bcase_id(c) for c in R.BLOCK_CAUSAL_CASES]


# ------------------------------------------------------------------------------------------------ decode
def _guarded(cache):
    """-> (buffer, view): the cache as a view of a longer device buffer whose last GUARD elements are NaN as well"""
    buf = torch.cat([cache.flatten().view(I16), torch.full((R.GUARD,), R.NAN_BITS, dtype=I16)]).to(DEV).view(torch.bfloat16)
    return buf, buf[:cache.numel()].view(cache.shape)


def _call(inp, scale, cache_len=None, src=None, surface=None):
    """one call on fresh device copies -> (o, k buffer, v buffer, cache_len), all on the CPU"""
    import touchnet_amd.library as L
    kbuf, kc = _guarded(inp.k_cache)
    vbuf, vc = _guarded(inp.v_cache)
    q, kn, vn = (t.to(DEV) for t in (inp.q, inp.k_new, inp.v_new))
    cl = (inp.cache_len if cache_len is None else cache_len).to(DEV)
    src = inp.src if src is None else src
    with torch.no_grad():
        if surface is not None:
            o = surface(q, kn, vn, kc, vc, cl, scale) if src is None else surface(q, kn, vn, kc, vc, cl, src.to(DEV), scale)
        elif src is None:
            o = L.attn_decode_(q, kn, vn, kc, vc, cl, scale)
        else:
            o = L.attn_decode_beam_(q, kn, vn, kc, vc, cl, src.to(DEV), scale)
        if surface is None:                                 # a second call on the state the first one left
            again = L.attn_decode_(q, kn, vn, kc, vc, cl, scale) if src is None else \
                L.attn_decode_beam_(q, kn, vn, kc, vc, cl, src.to(DEV), scale)
            nan = torch.isnan(o.float())                    # (a poisoned row is NaN both times; NaN payloads are not compared)
            assert torch.equal(torch.isnan(again.float()), nan), "a second call differs"
            assert torch.equal(again.view(I16)[~nan], o.view(I16)[~nan]), "a second call differs"
    torch.cuda.synchronize()
    return o.cpu(), kbuf.cpu(), vbuf.cpu(), cl.cpu()


def _expect_buffer(cache):
    return torch.cat([cache.flatten().view(I16), torch.full((R.GUARD,), R.NAN_BITS, dtype=I16)])


def _caches_are(kbuf, vbuf, k_exp, v_exp):
    assert torch.equal(kbuf.view(I16), _expect_buffer(k_exp)), "k_cache or the guard behind it"
    assert torch.equal(vbuf.view(I16), _expect_buffer(v_exp)), "v_cache or the guard behind it"


@functools.lru_cache(maxsize=None)
def _run(idx, beam):
    case = R.DECODE_CASES[idx]
    return _call(R.decode_problem(idx, beam)[0], case.scale)


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
@pytest.mark.parametrize("idx", range(len(R.DECODE_CASES)), ids=_DIDS)
def test_decode_stays_inside_the_derived_budget(idx, beam):
    from touchnet_amd import _C
    case = R.DECODE_CASES[idx]
    inp, ref, k_exp, v_exp = R.decode_problem(idx, beam)
    ns = R.num_splits(case.B, case.Nkv, case.S_max)
    nbytes = int(_C.lib().tn_attn_decode_workspace_bytes(case.B, case.Nh, case.Nkv, case.D, case.S_max))
    assert nbytes == (case.B * case.Nh * ns * (case.D + 1) * 4 if ns > 1 else 0)       # the split count is the library's
    if case.name.startswith("allG"):
        assert nbytes > 0                                                               # the split path is really taken
    o, kbuf, vbuf, cl = _run(idx, beam)
    R.check(o, ref, f"{'beam' if beam else 'dense'} decode of {R.dcase_id(case)}")
    _caches_are(kbuf, vbuf, k_exp, v_exp)
    assert torch.equal(cl, inp.cache_len)


def _base(name, D):
    return next(i for i, c in enumerate(R.DECODE_CASES) if c.name == name and c.D == D)


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
@pytest.mark.parametrize("bad", [-1, "S_max", "S_max + 1", R.INT32_MAX, R.INT32_MIN])
@pytest.mark.parametrize("name,D", [("smax64", 64), ("scale", 64)], ids=["one_split", "four_splits"])
def test_a_refused_length_poisons_its_row_only(name, D, bad, beam):
    """row 1's cache_len outside [0, S_max), beside two good rows: NaN for that row, the bits of the good run for the
    others, and a cache (with its guard) in which only the good rows' slots changed"""
    idx = _base(name, D)
    case = R.DECODE_CASES[idx]
    inp = R.decode_problem(idx, beam)[0]
    lens = inp.cache_len.clone()
    lens[1] = {"S_max": case.S_max, "S_max + 1": case.S_max + 1}.get(bad, bad)
    ref, k_exp, v_exp = R.decode(inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, lens, case.scale, inp.src)
    assert bool(torch.isnan(ref.value[1]).all()) and torch.equal(k_exp[1].view(I16), inp.k_cache[1].view(I16))
    o, kbuf, vbuf, cl = _call(inp, case.scale, cache_len=lens)
    good = _run(idx, beam)[0]
    assert bool(torch.isnan(o[1].float()).all())
    assert torch.equal(o[[0, 2]].view(I16), good[[0, 2]].view(I16))
    _caches_are(kbuf, vbuf, k_exp, v_exp)
    assert torch.equal(cl, lens)


@pytest.mark.parametrize("where", ["split_first", "last_cached", "split_first_and_filler", "one_split_first", "one_split_last"])
def test_an_out_of_range_table_entry_poisons_its_row_only(where):
    """one consulted entry of the longest row (row 0: 199 cached keys in splits [0, 64), [64, 128), [128, 192), [192, 200), or
    63 in one split) outside [0, R): position 64 opens a full split; 198 is the last cached key; 192 opens the tail split,
    whose invalid lanes load it again as their filler"""
    idx = _base("smax64" if where.startswith("one_split") else "scale", 64)
    case = R.DECODE_CASES[idx]
    inp, ref, _, _ = R.decode_problem(idx, True)
    n = int(inp.cache_len[0])
    assert n == (63 if where.startswith("one_split") else 199)
    pos = {"split_first": 64, "last_cached": n - 1, "split_first_and_filler": 192, "one_split_first": 0, "one_split_last": 62}[where]
    if where == "split_first_and_filler":
        assert R.split_keys(n + 1, R.num_splits(case.B, case.Nkv, case.S_max)) == 64
    good = _run(idx, True)[0]
    for value in (case.B, -1, R.INT32_MIN, R.INT32_MAX):
        src = inp.src.clone()
        src[0, pos] = value
        want, k_exp, v_exp = R.decode(inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, inp.cache_len, case.scale, src)
        assert bool(torch.isnan(want.value[0]).all())
        o, kbuf, vbuf, _ = _call(inp, case.scale, src=src)
        assert bool(torch.isnan(o[0].float()).all()), (where, value)
        assert torch.equal(o[1:].view(I16), good[1:].view(I16)), (where, value)
        _caches_are(kbuf, vbuf, k_exp, v_exp)


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
def test_the_decode_surface_returns_the_bits_of_the_library_call(beam):
    import touchnet_amd.functional as F
    for idx in (_base("allG7", 64), _base("scale", 128)):
        case = R.DECODE_CASES[idx]
        inp = R.decode_problem(idx, beam)[0]
        o, kbuf, vbuf, _ = _call(inp, case.scale, surface=F.attn_decode_beam if beam else F.attn_decode)
        want = _run(idx, beam)
        assert torch.equal(o.view(I16), want[0].view(I16))
        assert torch.equal(kbuf.view(I16), want[1].view(I16)) and torch.equal(vbuf.view(I16), want[2].view(I16))


def _args(B=2, Nh=4, Nkv=2, D=64, S=70):
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    return [z(B, Nh, D), z(B, Nkv, D), z(B, Nkv, D), z(B, S, Nkv, D), z(B, S, Nkv, D),
            torch.zeros(B, dtype=torch.int32, device=DEV)]


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
@pytest.mark.parametrize("what", ["D32", "D96", "G17", "Nh%Nkv", "strided_cache", "int64_len"])
def test_decode_refuses_what_it_cannot_run(what, beam):
    import touchnet_amd.library as L
    from touchnet_amd import _C
    a = _args(**{"D32": dict(D=32), "D96": dict(D=96), "G17": dict(Nh=34), "Nh%Nkv": dict(Nh=5)}.get(what, {}))
    if what == "strided_cache":
        a[3] = torch.zeros(2, 70, 2, 128, dtype=torch.bfloat16, device=DEV)[..., :64]
    if what == "int64_len":
        a[5] = a[5].long()
    table = [torch.zeros(2, 70, dtype=torch.int32, device=DEV)] if beam else []
    with pytest.raises(_C.KernelError), torch.no_grad():
        (L.attn_decode_beam_ if beam else L.attn_decode_)(*a, *table, 0.125)


@pytest.mark.parametrize("what", ["short_table", "wide_table", "int64_table", "strided_table"])
def test_the_beam_entry_refuses_a_wrong_table(what):
    import touchnet_amd.library as L
    from touchnet_amd import _C
    table = {"short_table": lambda: torch.zeros(2, 69, dtype=torch.int32, device=DEV),
             "wide_table": lambda: torch.zeros(3, 70, dtype=torch.int32, device=DEV),
             "int64_table": lambda: torch.zeros(2, 70, dtype=torch.int64, device=DEV),
             "strided_table": lambda: torch.zeros(2, 140, dtype=torch.int32, device=DEV)[:, ::2]}[what]()
    with pytest.raises(_C.KernelError), torch.no_grad():
        L.attn_decode_beam_(*_args(), table, 0.125)


# ------------------------------------------------------------------------------------------------ block-causal
@functools.lru_cache(maxsize=None)
def _run_bc(idx):
    import touchnet_amd.library as L
    case = R.BLOCK_CAUSAL_CASES[idx]
    inp = R.bc_problem(idx)[0]
    q, k, v, ss, ke = (t.to(DEV) for t in (inp.q, inp.k, inp.v, inp.seg_start, inp.key_end))
    with torch.no_grad():
        o = L.attn_block_causal_fwd(q, k, v, ss, ke, case.block, case.scale)
        again = L.attn_block_causal_fwd(q, k, v, ss, ke, case.block, case.scale)
    torch.cuda.synchronize()
    assert torch.equal(o.view(I16), again.view(I16)), "a second call differs"
    return o.cpu()


@pytest.mark.parametrize("idx", range(len(R.BLOCK_CAUSAL_CASES)), ids=_BIDS)
def test_block_causal_stays_inside_the_derived_budget(idx):
    case = R.BLOCK_CAUSAL_CASES[idx]
    inp, ref = R.bc_problem(idx)
    o = _run_bc(idx)
    R.check(o, ref, f"block-causal attention of {R.bcase_id(case)}")
    dead = ~R.bc_allow(inp.seg_start, inp.key_end, case.block).any(-1)
    if dead.any():
        assert float(o.float()[dead].abs().max()) == 0.0, "a row without keys is not exactly 0"


def test_the_block_causal_surface_returns_the_bits_of_the_library_call():
    import touchnet_amd.functional as F
    for idx, case in enumerate(R.BLOCK_CAUSAL_CASES):
        if case.name in ("packed", "dead_wg") and case.block in (50, 7):
            inp = R.bc_problem(idx)[0]
            mask = F.block_causal_mask(inp.seg_start.to(DEV), inp.key_end.to(DEV), case.block)
            with torch.no_grad():
                o = F.block_causal_attention(*(t.to(DEV) for t in (inp.q, inp.k, inp.v)), mask, scale=case.scale)
            assert torch.equal(o.cpu().view(I16), _run_bc(idx).view(I16))
