"""tests/inference_attention_reference.py is a reference, and its budgets are neither loose nor tight (no GPU).

1. Each reference agrees with an independently written torch float64 masked softmax on every case; the block-causal mask
   is the reference project's (`_ref_mask` of test_speech_tokenizer_gpu.py) on single-clip layouts; the split geometry
   restated in Python is the kernel header's.
2. `emulate_decode` / `emulate_block_causal` are plain-torch fp32 models of the kernels in the kernels' own order (decode:
   D / 8 lanes per key, 8 or 4 keys per wave, per-lane online softmax, lane-group, wave and split merges; block-causal:
   64-key tiles, P through bf16).  They stay inside the budget on every case the GPU test runs.
3. Each mutant of an emulation exceeds the budget on the case aimed at it.
4. The two claims the new tests rest on: one key dropped from a row of 1000 Gaussian keys stays inside the old decode
   tolerance, and a block index taken from the absolute position computes the old packed-clip layout correctly."""
import math
import os
import re

import pytest
import torch

import inference_attention_reference as R

BF = torch.bfloat16
F32 = torch.float32
_DIDS = [R.dcase_id(c) for c in R.DECODE_CASES]
_BIDS = [R.bcase_id(c) for c in R.BLOCK_CAUSAL_CASES]
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "touchnet_amd", "csrc")


# ------------------------------------------------------------------------------------------------ 1. the references
def test_split_geometry_is_the_kernel_headers():
    src = open(os.path.join(_CSRC, "attn_decode.hip")).read()
    const = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (k\w+) = (\d+);", src)}
    assert (const["kThreads"], const["kMinKeysPerSplit"], const["kMaxSplits"], const["kTargetWorkgroups"]) == (256, 64, 64, 512)
    assert "constexpr int LPK = D / 8;" in src and "constexpr int KPW = 64 / LPK;" in src and "constexpr int U = 2;" in src
    assert R.lane_geometry(64) == (8, 8, 32) and R.lane_geometry(128) == (16, 4, 16)

    def header_num_splits(B, Nkv, S_max):                  # transcribed line by line
        units = B * Nkv
        s = (512 + units - 1) // units
        by_len = (S_max + 64 - 1) // 64
        if s > by_len:
            s = by_len
        if s > 64:
            s = 64
        return 1 if s < 1 else s

    def header_split_keys(total, nsplit):
        c = (total + nsplit - 1) // nsplit
        c = (c + 64 - 1) // 64 * 64
        return 64 if c < 64 else c

    for units in (1, 2, 6, 7, 8, 9, 170, 171, 172, 255, 256, 257, 511, 512, 513, 4096):
        for S in (1, 63, 64, 65, 128, 129, 200, 4095, 4096, 4097, 4160, 8192):
            assert R.num_splits(units, 1, S) == header_num_splits(units, 1, S)
    for total in (1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097, 8191):
        for ns in (1, 2, 3, 4, 63, 64):
            assert R.split_keys(total, ns) == header_split_keys(total, ns)
    want = {"allG1": 4, "len0": 4, "short_long": 64, "smax1": 1, "smax63": 1, "smax64": 1, "smax65": 2, "units512": 1,
            "units171": 3, "units256": 2, "cap64_full": 64, "cap64_33": 64, "cap64_1": 64, "scale": 4, "sharp": 4}
    for c in R.DECODE_CASES:
        if c.name in want:
            assert R.num_splits(c.B, c.Nkv, c.S_max) == want[c.name], c
    used = lambda n, S: -(-(n + 1) // R.split_keys(n + 1, R.num_splits(1, 1, S)))
    assert (used(4095, 4160), used(4096, 4160), used(0, 4160)) == (64, 33, 1)
    assert {c.Nh // c.Nkv for c in R.DECODE_CASES if c.name.startswith("allG") and c.D == 64} == set(range(1, 17))
    assert {c.Nh // c.Nkv for c in R.DECODE_CASES if c.name.startswith("allG") and c.D == 128} == set(range(1, 17))


def _softmax_decode(inp, case):
    """dense float64 softmax over [B, S_max + 1] positions with a -inf mask (stale entries zeroed first: 0 x NaN)"""
    B, Nh, D = inp.q.shape
    S, Nkv = case.S_max, case.Nkv
    lens = inp.cache_len.long()
    pos = torch.arange(S)
    live = pos[None, :] < lens[:, None]
    rows = torch.arange(B)[:, None].expand(B, S) if inp.src is None else torch.where(live, inp.src.long(), torch.zeros(B, S, dtype=torch.long))
    k, v = (torch.where(live[:, :, None, None], c[rows, pos[None, :]].double(), torch.zeros((), dtype=torch.float64))
            for c in (inp.k_cache, inp.v_cache))
    k = torch.cat([k, inp.k_new.double()[:, None]], 1).repeat_interleave(Nh // Nkv, dim=2)
    v = torch.cat([v, inp.v_new.double()[:, None]], 1).repeat_interleave(Nh // Nkv, dim=2)
    s = torch.einsum("bhd,bnhd->bhn", inp.q.double(), k) * R.f32(case.scale)
    mask = torch.cat([live, torch.ones(B, 1, dtype=torch.bool)], 1)
    return torch.einsum("bhn,bnhd->bhd", torch.softmax(s.masked_fill(~mask[:, None], -math.inf), -1), v)


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
@pytest.mark.parametrize("idx", range(len(R.DECODE_CASES)), ids=_DIDS)
def test_decode_reference_agrees_with_a_float64_softmax(idx, beam):
    """Bound: float64 roundoff, 2^-53 x (keys + D + the exponent's argument, below 200) of the largest magnitude in play,
    below 1e-12 (max |reference| + 1).  Stale NaN (every cache position >= cache_len, every junk table entry) does not
    enter: the reference is finite.  The expected cache differs from the given one in the written slots only."""
    case = R.DECODE_CASES[idx]
    inp, ref, k_exp, v_exp = R.decode_problem(idx, beam)
    assert bool(torch.isfinite(ref.value).all()) and bool(torch.isfinite(ref.slack).all())
    lens = inp.cache_len.tolist()
    assert sorted(lens) == sorted(case.lens)
    for b, n in enumerate(lens):
        assert bool(torch.isnan(inp.k_cache[b, n:].float()).all()) and bool(torch.isnan(inp.v_cache[b, n:].float()).all())
        if beam:
            assert bool((inp.src[b, n:] == R.beam_variant(idx)[1]).all())
            assert all(lens[int(r)] > s for s, r in enumerate(inp.src[b, :n].tolist()))
    want = _softmax_decode(inp, case)
    err = float((ref.value - want).abs().max())
    tol = 1e-12 * (float(want.abs().max()) + 1.0)
    print(f"measured: decode reference vs float64 softmax: {err:.3g} (bound {tol:.3g})")
    assert err <= tol
    changed = (k_exp.view(torch.int16) != inp.k_cache.view(torch.int16)).any(-1).any(-1)
    slots = torch.zeros_like(changed)
    slots[torch.arange(case.B), inp.cache_len.long()] = True
    assert torch.equal(changed, slots)
    for b, n in enumerate(lens):
        assert torch.equal(k_exp[b, n], inp.k_new[b]) and torch.equal(v_exp[b, n], inp.v_new[b])


def test_decode_reference_refuses_what_the_kernel_refuses():
    idx = next(i for i, c in enumerate(R.DECODE_CASES) if c.name == "smax64")
    case = R.DECODE_CASES[idx]
    inp, ref, _, _ = R.decode_problem(idx, True)
    for bad in (-1, case.S_max, case.S_max + 1, R.INT32_MAX, R.INT32_MIN):
        lens = inp.cache_len.clone()
        lens[1] = bad
        r, k_exp, v_exp = R.decode(inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, lens, case.scale, inp.src)
        assert bool(torch.isnan(r.value[1]).all()) and torch.equal(r.value[[0, 2]], ref.value[[0, 2]])
        assert torch.equal(k_exp[1].view(torch.int16), inp.k_cache[1].view(torch.int16))
    src = inp.src.clone()
    src[0, 5] = case.B
    r, k_exp, _ = R.decode(inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, inp.cache_len, case.scale, src)
    assert bool(torch.isnan(r.value[0]).all()) and torch.equal(r.value[1:], ref.value[1:])
    assert torch.equal(k_exp[0, int(inp.cache_len[0])], inp.k_new[0])


def _softmax_block_causal(inp, case, allowed):
    qh, kh, vh = (t.double().transpose(1, 2) for t in (inp.q, inp.k, inp.v))
    s = (qh @ kh.transpose(-1, -2)) * R.f32(case.scale)
    dead = ~allowed.any(-1)[:, None, :, None]
    s = s.masked_fill(~allowed[:, None], -math.inf).masked_fill(dead, 0.0)
    return (torch.softmax(s, -1).masked_fill(dead, 0.0) @ vh).transpose(1, 2)


def _loop_mask(case):
    """the predicate of the issue, one (i, j) at a time"""
    ss, ke = R.bc_layout(case.rows)
    B, T = ss.shape
    out = torch.zeros(B, T, T, dtype=torch.bool)
    for b in range(B):
        for i in range(T):
            s, e = int(ss[b, i]), int(ke[b, i])
            for j in range(s, min(e, T)):
                out[b, i, j] = (j - s) // case.block <= (i - s) // case.block
    return out


@pytest.mark.parametrize("idx", range(len(R.BLOCK_CAUSAL_CASES)), ids=_BIDS)
def test_block_causal_reference_agrees_with_a_float64_softmax(idx, monkeypatch):
    """Bound as above (at most 400 keys).  The mask is the loop's; on single-clip layouts it is `_ref_mask`, the
    repository's restatement of the reference project's mask (causal | same block, key < length).  Rows without a key are
    exactly 0 with no slack.  Packed clips start and end away from multiples of 32, 64, 128 and the block."""
    case = R.BLOCK_CAUSAL_CASES[idx]
    inp, ref = R.bc_problem(idx)
    B, T = inp.seg_start.shape
    allowed = _loop_mask(case)
    assert torch.equal(allowed, R.bc_allow(inp.seg_start, inp.key_end, case.block))
    if case.name == "one":
        import test_speech_tokenizer_gpu as S
        monkeypatch.setattr(S, "DEV", "cpu")
        assert torch.equal(allowed, S._ref_mask([r[0][1] for r in case.rows], T, case.block))
    if case.name == "packed":
        for clips in case.rows:
            s = 0
            for f, L in clips:
                for x in {s, s + L, s + f} - {0, T}:
                    assert all(x % m for m in (32, 64, 128, case.block) if m <= T), (case, x)
                s += f
    if case.name == "dead_wg":
        assert not bool(allowed[0, 128:256].any()) and bool(allowed[0, :128].any()) and bool(allowed[0, 256:].any())
    want = _softmax_block_causal(inp, case, allowed)
    err = float((ref.value - want).abs().max())
    tol = 1e-12 * (float(want.abs().max()) + 1.0)
    print(f"measured: block-causal reference vs float64 softmax: {err:.3g} (bound {tol:.3g})")
    assert err <= tol
    dead = ~allowed.any(-1)
    if dead.any():
        assert float(ref.value[dead].abs().max()) == 0.0 and float(ref.slack[dead].abs().max()) == 0.0
    for pl in inp.anchors:
        assert bool(allowed[pl.b, pl.i, pl.j])
    for pl in inp.baits:
        assert not bool(allowed[pl.b, pl.i, pl.j])
    assert bool(torch.isfinite(inp.k.float()).all()) and bool(torch.isfinite(inp.v.float()).all())


# ------------------------------------------------------------------------------------------------ 2. the emulations
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in float64; one rounding back"""
    return (a.double() * b.double() + c.double()).float()


def _exp2_or_zero(x, dead):
    return torch.where(dead, torch.zeros_like(x), torch.exp2(torch.where(dead, torch.zeros_like(x), x)))


def emulate_decode(case, inp, mutant=None, arg=None):
    """attn_decode.hip in fp32, in its order -> o bf16 [B, Nh, D].  `mutant`:
         drop (arg: (b, j))      key j of row b is skipped
         new_from_cache          the key at index cache_len is read from the cache slot, not from k_new / v_new
         extra_key               key cache_len + 1 is included
         empty_weight_1          an empty split enters the combine with weight 1
         unweighted              the splits are averaged without their lse weights
         lse                     lse x (1 + 2^-10)
         gqa                     query head h reads kv head h % Nkv
         no_table / late_table   beam: the table is ignored / read one position late
         no_log2e                scale without log2(e)"""
    B, Nh, Nkv, D, S = case.B, case.Nh, case.Nkv, case.D, case.S_max
    G = Nh // Nkv
    lpk, kpw, kpi = R.lane_geometry(D)
    ns = R.num_splits(B, Nkv, S)
    c = torch.tensor(case.scale, dtype=F32) * (1.0 if mutant == "no_log2e" else torch.tensor(R.LOG2E, dtype=F32))
    hmap = torch.arange(Nh) % Nkv if mutant == "gqa" else torch.arange(Nh) // G
    ninf = torch.tensor(-math.inf)
    out = torch.full((B, Nh, D), math.nan).to(BF)
    for b in range(B):
        n = int(inp.cache_len[b])
        if not 0 <= n < S:
            continue
        total = n + 1 + (mutant == "extra_key")
        chunk = R.split_keys(total, ns)
        nit = chunk // kpi
        j = (torch.arange(ns)[:, None, None, None] * chunk + torch.arange(nit)[None, :, None, None] * kpi
             + torch.arange(4)[None, None, :, None] * kpw + torch.arange(kpw))                  # [ns, nit, 4, kpw]
        k1 = torch.clamp((torch.arange(ns) + 1) * chunk, max=total)[:, None, None, None]
        valid = j < k1
        if mutant == "drop" and arg[0] == b:
            valid = valid & (j != arg[1])
        js = torch.where(valid, j, torch.zeros_like(j)).flatten().clamp_max(S - 1)
        new = (js == n) & (mutant != "new_from_cache")
        rows = torch.full_like(js, b)
        if inp.src is not None and mutant != "no_table":
            rows = inp.src[b, (js + (mutant == "late_table")).clamp_max(S - 1)].long()
            rows = torch.where(new, torch.full_like(rows, b), rows)
            if bool((((rows < 0) | (rows >= B)) & valid.flatten()).any()):
                continue                                                                        # poisoned row
            rows = rows.clamp(0, B - 1)
        kf = torch.where(new[:, None, None], inp.k_new[b][None], inp.k_cache[rows, js]).float()[:, hmap]   # [N, Nh, D]
        vf = torch.where(new[:, None, None], inp.v_new[b][None], inp.v_cache[rows, js]).float()[:, hmap]
        qs = (inp.q[b].float() * c).view(1, Nh, lpk, 8)
        kl = kf.view(-1, Nh, lpk, 8)
        s = torch.zeros(kl.shape[:3])
        for e in range(8):
            s = _fma(qs[..., e], kl[..., e], s)
        off = lpk // 2
        while off:
            s = s + s[..., torch.arange(lpk) ^ off]
            off //= 2
        s = s[..., 0].view(ns, nit, 4, kpw, Nh)
        vf = vf.view(ns, nit, 4, kpw, Nh, D)
        m = torch.full((ns, 4, kpw, Nh), -math.inf)
        l = torch.zeros(ns, 4, kpw, Nh)
        acc = torch.zeros(ns, 4, kpw, Nh, D)
        for it in range(nit):
            ok = valid[:, it][..., None]
            mn = torch.maximum(m, s[:, it])
            alpha = _exp2_or_zero(m - mn, m == ninf)
            p = torch.exp2(s[:, it] - mn)
            l = torch.where(ok, _fma(l, alpha, p), l)
            acc = torch.where(ok[..., None], _fma(acc, alpha[..., None], p[..., None] * vf[:, it]), acc)
            m = torch.where(ok, mn, m)
        o = 1
        while o < kpw:
            idx = torch.arange(kpw) ^ o
            mo, lo, ao = m[:, :, idx], l[:, :, idx], acc[:, :, idx]
            mn = torch.maximum(m, mo)
            a = _exp2_or_zero(m - mn, (mn == ninf) | (m == ninf))
            cc = _exp2_or_zero(mo - mn, (mn == ninf) | (mo == ninf))
            l = l * a + lo * cc
            acc = acc * a[..., None] + ao * cc[..., None]
            m = mn
            o *= 2
        m, l, acc = m[:, :, 0], l[:, :, 0], acc[:, :, 0]                                       # [ns, 4, Nh(, D)]
        mx = m.amax(1)
        lt, ot = torch.zeros(ns, Nh), torch.zeros(ns, Nh, D)
        for w in range(4):
            cw = _exp2_or_zero(m[:, w] - mx, m[:, w] == ninf)
            lt = _fma(l[:, w], cw, lt)
            ot = _fma(acc[:, w], cw[..., None], ot)
        live = (lt > 0) | torch.isnan(lt)
        on = torch.where(live[..., None], ot / torch.where(live, lt, torch.ones_like(lt))[..., None], torch.zeros_like(ot))
        if ns == 1:
            out[b] = on[0].to(BF)
            continue
        lse = torch.where(live, mx + torch.log2(torch.where(live, lt, torch.ones_like(lt))), ninf)
        if mutant == "lse":
            lse = lse * (1 + 2.0 ** -10)
        mxs = lse.amax(0)
        wsum, acc = torch.zeros(Nh), torch.zeros(Nh, D)
        for sp in range(ns):
            empty = lse[sp] == ninf
            w = _exp2_or_zero(lse[sp] - mxs, empty)
            if mutant == "unweighted":
                w = torch.where(empty, w, torch.ones_like(w))
            if mutant == "empty_weight_1":
                w, empty = torch.where(empty, torch.ones_like(w), w), torch.zeros_like(empty)
            wsum = torch.where(empty, wsum, wsum + w)
            acc = torch.where(empty[:, None], acc, _fma(w[:, None], on[sp], acc))
        out[b] = (acc / wsum[:, None]).to(BF)
    return out


def emulate_block_causal(case, inp, mutant=None, arg=None):
    """attn_block_causal.hip in fp32: 64-key tiles, P through bf16, the row sum from the unrounded p -> o bf16.  `mutant`:
         abs_block       the block index from the absolute position (qi / block, key / block)
         end_inclusive   key_end taken as inclusive
         late_boundary   the block boundary one key late
         seg0            seg_start taken as 0
         drop (arg: BPlant)   key j is skipped by row i of head h
         skip_rescale    O is never rescaled
         invalid_rows_zero    rows at or past their clip's valid length write 0"""
    B, T, Nh, D = inp.q.shape
    qf, kf, vf = (t.float().transpose(1, 2) for t in (inp.q, inp.k, inp.v))
    i, j = torch.arange(T)[None, :, None], torch.arange(T)[None, None, :]
    s, e = inp.seg_start.long()[:, :, None], inp.key_end.long()[:, :, None]
    if mutant == "seg0":
        s = torch.zeros_like(s)
    if mutant == "abs_block":
        allow = (j >= s) & (j < e) & (j // case.block <= i // case.block)
    else:
        bend = s + ((i - s) // case.block + 1) * case.block + (mutant == "late_boundary")
        allow = (j >= s) & (j < torch.minimum(e + (mutant == "end_inclusive"), bend))
    allow = allow[:, None].expand(B, Nh, T, T).clone()
    if mutant == "drop":
        allow[arg.b, arg.h, arg.i, arg.j] = False
    c = torch.tensor(case.scale, dtype=F32) * torch.tensor(R.LOG2E, dtype=F32)
    ninf = torch.tensor(-math.inf)
    m = torch.full((B, Nh, T), -math.inf)
    l = torch.zeros(B, Nh, T)
    o = torch.zeros(B, Nh, T, D)
    for j0 in range(0, T, 64):
        al = allow[..., j0:j0 + 64]
        sv = torch.where(al, (qf @ kf[:, :, j0:j0 + 64].transpose(-1, -2)) * c, ninf)
        m_new = torch.maximum(m, sv.amax(-1))
        m_use = torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_use)
        p = torch.exp2(sv - m_use[..., None])
        l = l * alpha + p.sum(-1)
        o = (o if mutant == "skip_rescale" else o * alpha[..., None]) + p.to(BF).float() @ vf[:, :, j0:j0 + 64]
        m = m_new
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    out = (o * inv[..., None]).to(BF).transpose(1, 2)
    if mutant == "invalid_rows_zero":
        out = torch.where((torch.arange(T)[None, :] >= inp.key_end.long())[:, :, None, None], torch.zeros_like(out), out)
    return out


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
@pytest.mark.parametrize("idx", range(len(R.DECODE_CASES)), ids=_DIDS)
def test_decode_emulation_stays_inside_the_budget(idx, beam):
    case = R.DECODE_CASES[idx]
    inp, ref, _, _ = R.decode_problem(idx, beam)
    R.check(emulate_decode(case, inp), ref, f"emulated {'beam' if beam else 'dense'} decode of {R.dcase_id(case)}")


@pytest.mark.parametrize("idx", range(len(R.BLOCK_CAUSAL_CASES)), ids=_BIDS)
def test_block_causal_emulation_stays_inside_the_budget(idx):
    case = R.BLOCK_CAUSAL_CASES[idx]
    inp, ref = R.bc_problem(idx)
    R.check(emulate_block_causal(case, inp), ref, f"emulated block-causal attention of {R.bcase_id(case)}")


# ------------------------------------------------------------------------------------------------ 3. the mutants
def _dcase(name, D=None, pred=lambda c: True):
    return next(i for i, c in enumerate(R.DECODE_CASES) if c.name == name and (D is None or c.D == D) and pred(c))


def _dworst(idx, beam, mutant, arg=None, row=None):
    case = R.DECODE_CASES[idx]
    inp, ref, _, _ = R.decode_problem(idx, beam)
    r = R.ratios(emulate_decode(case, inp, mutant, arg), ref, BF)
    w = float((r if row is None else r[row]).max())
    print(f"measured: decode mutant {mutant} {arg if arg is not None else ''} on {R.dcase_id(case)}: {w:.3g} x budget")
    return w


@pytest.mark.parametrize("kind", ["first", "last_cached", "new", "split_first", "split_last", "wave_first", "wave_last", "tail"])
@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
def test_a_dropped_decode_anchor_exceeds_the_budget(kind, beam):
    """EVERY anchor of the kind, one at a time, at the head that owns it: in an all-G case of each D (G = 7 and 16), in
    the 64-split rows, and in the short row of a long cache"""
    picks = [_dcase("allG7", 64), _dcase("allG16", 128), _dcase("cap64_full"), _dcase("cap64_33"), _dcase("short_long"),
             _dcase("units171"), _dcase("len3", 64)]
    seen = 0
    for idx in picks:
        inp = R.decode_problem(idx, beam)[0]
        hits = [a for a in inp.anchors if kind in a.kinds]
        for a in hits[:6] + hits[-6:]:
            w = _dworst(idx, beam, "drop", (a.b, a.j), row=(a.b, a.h))
            assert w > 1.0, (kind, a, w)
            seen += 1
    assert seen >= 6


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
@pytest.mark.parametrize("mutant", ["new_from_cache", "extra_key", "gqa", "no_log2e", "lse"])
def test_a_wrong_decode_kernel_exceeds_the_budget(mutant, beam):
    for idx in (_dcase("allG7", 64), _dcase("allG3", 128)):
        assert _dworst(idx, beam, mutant) > 1.0


def test_wrong_split_weights_exceed_the_budget():
    """an empty split with weight 1: rows with empty splits (len 0 and 63 of 4 splits; 63 of 64 empty).  No lse weights:
    splits of different mass."""
    for idx in (_dcase("allG5", 64), _dcase("cap64_1"), _dcase("cap64_33")):
        assert _dworst(idx, False, "empty_weight_1") > 1.0
    for idx in (_dcase("allG5", 64), _dcase("sharp", 128), _dcase("cap64_33")):
        assert _dworst(idx, False, "unweighted") > 1.0


def test_a_wrong_beam_table_read_exceeds_the_budget():
    """in every all-G case of D = 64 (and three more) whose table sends a consulted entry to another row"""
    for mutant in ("no_table", "late_table"):
        hit = 0
        for idx, c in enumerate(R.DECODE_CASES):
            if not (c.name.startswith("allG") and c.D == 64) and c.name not in ("len1", "len2", "units256"):
                continue
            inp = R.decode_problem(idx, True)[0]
            live = torch.arange(c.S_max)[None, :] < inp.cache_len[:, None]
            if bool(((inp.src != torch.arange(c.B, dtype=torch.int32)[:, None]) & live).any()):
                assert _dworst(idx, True, mutant) > 1.0, (mutant, c)
                hit += 1
        assert hit >= 12


def _bworst(idx, mutant, arg=None, row=None):
    case = R.BLOCK_CAUSAL_CASES[idx]
    inp, ref = R.bc_problem(idx)
    r = R.ratios(emulate_block_causal(case, inp, mutant, arg), ref, BF)
    w = float((r if row is None else r[row]).max())
    print(f"measured: block-causal mutant {mutant} {arg if arg is not None else ''} on {R.bcase_id(case)}: {w:.3g} x budget")
    return w


@pytest.mark.parametrize("kind", ["clip_first", "last_allowed", "tile_first", "tile_last", "diagonal"])
def test_a_dropped_block_causal_anchor_exceeds_the_budget(kind):
    """EVERY anchor of the kind, one at a time, in every planted case, at the row and head that own it"""
    seen = 0
    for idx, case in enumerate(R.BLOCK_CAUSAL_CASES):
        for pl in (a for a in R.bc_problem(idx)[0].anchors if a.kind == kind):
            w = _bworst(idx, "drop", pl, row=(pl.b, pl.i, pl.h))
            assert w > 1.0, (case, pl, w)
            seen += 1
    assert seen >= 10


@pytest.mark.parametrize("mutant,bait", [("abs_block", "next_block"), ("end_inclusive", "key_end"),
                                         ("late_boundary", "next_block"), ("seg0", "prev_clip_last")])
def test_a_wrong_block_causal_mask_exceeds_the_budget(mutant, bait):
    """at the row of EVERY bait the mutant lets in (abs_block: in the packed cases, whose clips start off the block grid)"""
    seen = 0
    for idx, case in enumerate(R.BLOCK_CAUSAL_CASES):
        if case.kind != "planted" or (mutant in ("abs_block", "seg0") and case.name != "packed"):
            continue
        inp, ref = R.bc_problem(idx)
        hits = [pl for pl in inp.baits if pl.kind == bait]
        if mutant == "abs_block":                           # the baits this mutant reaches: the key's absolute block is the row's
            hits = [pl for pl in hits if pl.j // case.block <= pl.i // case.block]
        if mutant == "end_inclusive":                       # ... and this one: key_end lies inside the row's block range
            start = lambda pl: int(inp.seg_start[pl.b, pl.i])
            hits = [pl for pl in hits if pl.j < start(pl) + ((pl.i - start(pl)) // case.block + 1) * case.block]
        if not hits:
            continue
        r = R.ratios(emulate_block_causal(case, inp, mutant), ref, BF)
        for pl in hits:
            assert float(r[pl.b, pl.i, pl.h].max()) > 1.0, (mutant, case, pl)
            seen += 1
        print(f"measured: block-causal mutant {mutant} on {R.bcase_id(case)}: {float(r.max()):.3g} x budget, {len(hits)} baits")
    assert seen >= 5


def test_a_skipped_rescale_exceeds_the_budget():
    idx = next(i for i, c in enumerate(R.BLOCK_CAUSAL_CASES) if c.kind == "sharp")
    assert _bworst(idx, "skip_rescale") > 1.0


def test_zeroed_rows_past_the_valid_length_exceed_the_budget():
    """padded query rows are ordinary rows: they see the valid keys of their block range"""
    hit = 0
    for idx, c in enumerate(R.BLOCK_CAUSAL_CASES):
        if c.name == "one" and any(0 < r[0][1] < r[0][0] for r in c.rows):
            assert _bworst(idx, "invalid_rows_zero") > 1.0
            hit += 1
    assert hit >= 10


# ------------------------------------------------------------------------------------------------ 4. the "why" claims
def _single_key_losses(n):
    """A row of n cached Gaussian keys (test_generation_gpu.py's inputs: randn, nothing planted).  Without key j the output
    is (o - p_j v_j) / (1 - p_j): in float64, for every j at once -> (error / old tolerance, error / derived budget), the
    worst element per (key, head), and the problem"""
    case = R.DCase("old", 1, 8, 2, 64, n + 3, (n,), "gauss", 64 ** -0.5)
    inp = R.decode_inputs(case, 7)
    ref, _, _ = R.decode(inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, inp.cache_len, case.scale)
    k = torch.cat([inp.k_cache[0, :n], inp.k_new]).double().repeat_interleave(4, dim=1)             # [n + 1, Nh, D]
    v = torch.cat([inp.v_cache[0, :n], inp.v_new]).double().repeat_interleave(4, dim=1)
    p = torch.softmax(torch.einsum("hd,nhd->hn", inp.q[0].double(), k) * R.f32(case.scale), -1).t()[:, :, None]
    err = (p * (ref.value[0][None] - v) / (1 - p)).abs()
    old = (err / (4e-3 + 8e-3 * ref.value[0].abs())[None]).amax(-1)
    new = (err / R.budget(R.Ref(ref.value[0], ref.slack[0]), BF)[None]).amax(-1)
    return old, new, case, inp, ref


def test_a_dropped_key_in_gaussian_keys_and_the_old_tolerance():
    """The claim behind these tests was that ONE key lost from a row of 1000 Gaussian keys passes the old bound
    4e-3 + 8e-3 |ref|.  What is true: such a loss moves the output by p_j |v_j - o|, about 1e-3 x 3 at the worst of a head's
    64 elements, and a key's weight is several times the mean as often as not — so at 1000 keys a loss passes in a head
    more often than it fails, passes in all 8 heads at once for a good part of the keys (more than one in five), and the
    worst is a small multiple of the bound; at 8191 keys, the longest row of the old test, nearly every loss passes
    (more than nine in ten, in all heads).  Every one of them leaves the derived budget, at either length.  The emulation
    without key 500, the last cached key and the new key agrees with the float64 count."""
    old, new, case, inp, ref = _single_key_losses(1000)
    all_heads, per_head = float((old.amax(-1) <= 1.0).double().mean()), float((old <= 1.0).double().mean())
    print(f"measured: 1000 keys: {all_heads:.1%} of the single-key losses pass the old tolerance in all 8 heads, {per_head:.1%} "
          f"per head (worst {float(old.max()):.1f} x); the least visible one is {float(new.amax(-1).min()):.0f} x the budget")
    assert all_heads > 0.2 and per_head > 0.5 and float(new.amax(-1).min()) > 1.0
    for j in (500, 999, 1000):
        got = emulate_decode(case, inp, "drop", (0, j)).double()
        o = float(((got - ref.value).abs() / (4e-3 + 8e-3 * ref.value.abs())).max())
        n = float(R.ratios(got, ref, BF).max())
        print(f"measured: emulation without key {j}: {o:.3f} x the old tolerance, {n:.1f} x the derived budget")
        assert n > 1.0 and (o <= 1.0) == bool(old[j].max() <= 1.0)
    old, new, _, _, _ = _single_key_losses(8191)
    all_heads = float((old.amax(-1) <= 1.0).double().mean())
    print(f"measured: 8191 keys: {all_heads:.1%} pass in all 8 heads (worst {float(old.max()):.1f} x); the least visible "
          f"one is {float(new.amax(-1).min()):.0f} x the budget")
    assert all_heads > 0.9 and float(new.amax(-1).min()) > 1.0


def test_the_absolute_position_mutant_is_right_on_the_old_packed_layout():
    """test_speech_tokenizer_gpu.py's packed clips (150, 100, 200, 50 frames, block 50) all start on a multiple of the
    block, where (j - s) // block <= (i - s) // block and j // block <= i // block are the same predicate: the mutant
    returns the correct kernel's bits, so no tolerance could tell them apart"""
    case = R.BCase("old", (((150, 150), (100, 37), (200, 1), (50, 50)),), 50, 2, "gauss", R.S0)
    inp = R.bc_inputs(case, 3)
    assert torch.equal(emulate_block_causal(case, inp, "abs_block").view(torch.int16),
                       emulate_block_causal(case, inp).view(torch.int16))
    ref = R.block_causal(inp.q, inp.k, inp.v, inp.seg_start, inp.key_end, case.block, case.scale)
    err = (emulate_block_causal(case, inp, "abs_block").double() - ref.value).abs()
    assert bool((err <= 2e-2 + 2e-2 * ref.value.abs()).all())
