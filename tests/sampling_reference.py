"""tn_sample_step restated in plain torch — what csrc/sample.hip is held to at its edges — and the planted rows that reach
every branch of its selection and of its two draws.  No kernel, no transformers, no device: tensors in, tensors out.

step        one decoding step with the arguments of functional.sample_step, on the CPU.  Per row:
              values   fp32 of the logits; the penalty once per distinct history id in [0, V): l < 0 ? l * p : l / p; then
                       l / T — all in fp32, as the kernel and HF compute them, so the values are bit-equal; fp64 from there
              top-k    keep l >= the k-th largest (ties stay); k == 0 or k >= V: off
              top-p    keep a value iff the softmax mass (over the top-k survivors) strictly above it is < top_p; 1: off
              draw     the first kept token, in id order, whose running sum of exp(l - max) exceeds u * total; u == 1 (nothing
                       exceeds) draws the last kept token of positive weight.  A weight below 2^-40 counts as zero, as the
                       kernel's fixed-point masses have it ("can be kept but are never drawn"): d = max - l > 40 ln 2
              no finite maximum, or greedy mode: a NaN wins (the lowest id among NaNs), else the first largest value
                       (torch.argmax): the first +inf, id 0 of a row of -inf
              books    a finished row emits `pad`; the token is appended unless len >= S_hist, len clamped to [0, S_hist];
                       an eos finishes a live row even when it could not be appended
            and the decision data the tests need: the kept mask, the distance of the threshold from the maximum, and the
            two margins — for top-p min |above(v) - top_p| over the distinct values v below the maximum (the maximum has
            nothing above it: an empty sum, 0 < top_p in the kernel as here, no decision), for the draw min |u - edge| over
            the interior cumulative edges.
edge_cases  the planted rows, each with a name, the arguments and the expected result; the CPU test checks their margins,
            the device test runs them.  kimi_edge_cases does the same for tn_kimi_text_step's sampled mode, whose
            restatement is kimi_generate_reference.text_step.
"""
import functools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kimi_generate_reference as KR  # noqa: E402

NEG_INF = float("-inf")
TAIL_D = 1023.0 / 16.0             # level 0 of the kernel's selection: everything at or beyond this d shares the last bin
ZERO_D = 40.0 * math.log(2.0)      # exp(-d) * 2^40 < 1: the fixed-point weight is zero
MARGIN = 5e-5                      # what the planted top_p and u keep from every decision boundary
ONE_BELOW = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------ values
def values(logits_row, hist_ids, penalty, temperature, do_sample):
    """The fp32 row the thresholds and the draw see."""
    v = logits_row.detach().to(torch.float32).clone()
    V = v.numel()
    ids = sorted({int(t) for t in hist_ids if 0 <= int(t) < V})
    if penalty != 1.0 and ids:
        ids = torch.tensor(ids, dtype=torch.int64)
        p = torch.tensor(penalty, dtype=torch.float32)
        s = v[ids]
        v[ids] = torch.where(s < 0, s * p, s / p)
    if do_sample:
        v = v / torch.tensor(temperature, dtype=torch.float32)
    return v


def argmax(v):
    """torch.argmax's token: a NaN wins, the lowest id among NaNs; else the first largest value."""
    nan = torch.isnan(v)
    if bool(nan.any()):
        return int(nan.nonzero()[0])
    return int((v == v.max()).nonzero()[0])


def decide(v, top_k, top_p, u=None):
    """v: fp32 values of a row with a finite maximum -> dict(kept, n_kept, thr_d, exact_count, p_margin, above, edges,
    ids, token, u_margin, d_gap_ok).  `above`: (distinct values of the top-k survivors, descending; mass strictly above
    each, as a fraction of the survivors' mass).  `edges`: the cumulative fractions of the kept tokens of positive weight,
    in id order, with `ids` their tokens (interval j is [edges[j-1], edges[j]))."""
    V = v.numel()
    x = v.double()
    M = float(x.max())
    top_p = f32(top_p)
    keep = torch.ones(V, dtype=torch.bool)
    k = top_k if 0 < top_k < V else 0
    if k:
        keep = x >= torch.sort(x, descending=True).values[k - 1]
    d = M - x                                                              # +inf at -inf logits
    w = torch.where(d <= ZERO_D, torch.exp(-d), torch.zeros_like(d))
    # top-p over the survivors, in exact-softmax masses (the cut-off weights are below 2^-40 of the maximum's)
    e = torch.where(keep, torch.exp(-d), torch.zeros_like(d))
    vals, inv = torch.unique(x, sorted=True, return_inverse=True)          # ascending
    mass = torch.zeros(vals.numel(), dtype=torch.float64).index_add_(0, inv, e)
    above = (mass.flip(0).cumsum(0).flip(0) - mass) / mass.sum()
    present = torch.zeros(vals.numel(), dtype=torch.bool)
    present[inv[keep]] = True
    p_margin = float("inf")
    if top_p < 1.0:
        keep = keep & (above[inv] < top_p)
        below_max = present.clone()
        below_max[-1] = False
        if bool(below_max.any()):
            p_margin = float((above[below_max] - top_p).abs().min())
    kept_vals = x[keep]
    thr_d = M - float(kept_vals.min())
    # does fp32 rounding of d = M - l merge the lowest kept value with the highest dropped one?
    dropped = x[~keep]
    d_gap_ok = True
    if dropped.numel():
        m32 = torch.tensor(M, dtype=torch.float32)
        hi = dropped.max().to(torch.float32)
        lo = kept_vals.min().to(torch.float32)
        d_gap_ok = bool((m32 - hi) > (m32 - lo))
    ids = (keep & (w > 0)).nonzero().reshape(-1)
    cum = torch.cumsum(w[ids], 0)
    edges = cum / cum[-1]
    out = dict(kept=keep, n_kept=int(keep.sum()), thr_d=thr_d, exact_count=thr_d < TAIL_D, p_margin=p_margin,
               above=(vals.flip(0)[present.flip(0)], above.flip(0)[present.flip(0)]), edges=edges, ids=ids, d=d,
               d_gap_ok=d_gap_ok)
    if u is not None:
        u = min(max(f32(u), 0.0), 1.0)
        hit = (cum > u * float(cum[-1])).nonzero()
        out["token"] = int(ids[int(hit[0])] if hit.numel() else ids[-1])
        out["u_margin"] = float((edges[:-1] - u).abs().min()) if edges.numel() > 1 else float("inf")
    return out


def step(logits, hist, hist_len, cache_len, finished, n_unfinished, penalty=1.0, do_sample=True, temperature=1.0, top_k=0,
         top_p=1.0, eos=(), pad=0, uniforms=None):
    """functional.sample_step on the CPU: hist / hist_len / cache_len / finished / n_unfinished are updated in place.
    -> one dict per row: token, n_kept, and for a sampled row with a finite maximum the decision data of `decide`."""
    B, V = logits.shape
    S = hist.shape[1]
    eos = [int(e) for e in ([eos] if isinstance(eos, int) else eos)]
    rows = []
    for b in range(B):
        n = min(max(int(hist_len[b]), 0), S)
        done = bool(int(finished[b]))
        if done:
            r = dict(token=int(pad), n_kept=0)
        else:
            v = values(logits[b], hist[b, :n].tolist(), penalty, temperature, do_sample)
            tok = argmax(v)
            if do_sample and math.isfinite(float(v[tok])):
                r = decide(v, top_k, top_p, float(uniforms[b]))
            else:
                r = dict(token=tok, n_kept=1)
            r["values"] = v
        if n < S:
            hist[b, n] = r["token"]
            hist_len[b] = n + 1
            cache_len[b] += 1
        if not done and r["token"] in eos:
            finished[b] = 1
            n_unfinished[0] -= 1
        rows.append(r)
    return rows


# ------------------------------------------------------------------------------------------- mid-gap top_p and uniforms
def mid_top_p(v, top_k, frac):
    """An fp32 top_p in the middle of a gap between two neighbouring `above` values of the row, the gap near `frac` of the
    survivors' mass that is at least 4 * MARGIN wide and the widest of the few around it."""
    above = decide(v, top_k, 1.0)["above"][1]
    a = torch.cat([above, torch.ones(1, dtype=torch.float64)])
    width = a[1:] - a[:-1]
    ok = (width >= 4 * MARGIN).nonzero().reshape(-1)
    assert ok.numel(), "no gap wide enough for a top_p"
    j = int(ok[int(((a[:-1][ok] + a[1:][ok]) / 2 - frac).abs().argmin())])
    return f32(float(a[j] + a[j + 1]) / 2)


def mid_uniforms(v, top_k, top_p, n, planted=()):
    """n fp32 uniforms for one row: the planted ones first, then the middles of the widest intervals of the draw at least
    4 * MARGIN wide, spread over the id range (the first, the last, then the widest remaining)."""
    dec = decide(v, top_k, top_p)
    e = torch.cat([torch.zeros(1, dtype=torch.float64), dec["edges"]])
    width = e[1:] - e[:-1]
    ok = (width >= 4 * MARGIN).nonzero().reshape(-1).tolist()
    assert ok, "no interval wide enough for a uniform"
    order = [ok[0], ok[-1]] + sorted(ok[1:-1], key=lambda j: -float(width[j]))
    order = list(dict.fromkeys(order))
    us = list(planted)
    i = 0
    while len(us) < n:
        j = order[i % len(order)]
        t = (0.5, 0.3, 0.7)[(i // len(order)) % 3]
        us.append(f32(float(e[j]) + t * float(width[j])))
        i += 1
    return us


# ------------------------------------------------------------------------------------------------------- the cases
def _case(name, dtype, row, top_k=0, top_p=1.0, T=1.0, n=3, planted=(), reach="", penalty=1.0, hist=(), frac=None):
    """One row repeated under n uniforms (the planted ones, then mid-interval ones).  frac: plant top_p mid-gap near that
    fraction of the mass instead of `top_p`."""
    row = row.to(dtype)
    v = values(row, hist, penalty, T, True)
    if math.isfinite(float(v[argmax(v)])):
        if frac is not None:
            top_p = mid_top_p(v, top_k, frac)
        us = mid_uniforms(v, top_k, top_p, n, planted)
    else:
        us = (list(planted) + [0.5] * n)[:n]
    B = len(us)
    return dict(name=name, logits=row[None].repeat(B, 1), hists=[list(hist) or [0]] * B, S_hist=16, penalty=penalty, T=T,
                top_k=top_k, top_p=f32(top_p), uniforms=us, planted_u=bool(planted), reach=reach)


def _finish(c):
    """Fill in the state tensors and the expected result of a case."""
    B = c["logits"].shape[0]
    S = c["S_hist"]
    hist = torch.zeros(B, S, dtype=torch.int32)
    for b, h in enumerate(c["hists"]):
        hist[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
    hl = c.get("hist_len") or [len(h) for h in c["hists"]]
    fin = torch.zeros(B, dtype=torch.int32)
    for b in c.get("finished", ()):
        fin[b] = 1
    c.setdefault("eos", [])
    c.setdefault("pad", 0)
    c.setdefault("do_sample", True)
    c["state"] = dict(hist=hist, hl=torch.tensor(hl, dtype=torch.int32), cl=torch.tensor(hl, dtype=torch.int32) - 1, fin=fin,
                      nu=torch.tensor([B - int(fin.sum())], dtype=torch.int32))
    want = {n: t.clone() for n, t in c["state"].items()}
    c["rows"] = step(c["logits"], want["hist"], want["hl"], want["cl"], want["fin"], want["nu"], c["penalty"],
                     c["do_sample"], c["T"], c["top_k"], c["top_p"], c["eos"], c["pad"],
                     torch.tensor(c["uniforms"], dtype=torch.float32))
    c["want"] = want
    return c


def _scatter(V, seed):
    """A fixed permutation of the ids, so that no planted row is sorted by value."""
    return torch.randperm(V, generator=torch.Generator().manual_seed(seed))


def _cluster_row(V, d_of_j, n_cluster, seed):
    """One logit 0.0, n_cluster logits -d_of_j(j), the rest at -30 and below (weight zero), at scattered ids."""
    perm = _scatter(V, seed)
    row = torch.empty(V, dtype=torch.float64)
    row[perm[0]] = 0.0
    j = torch.arange(n_cluster, dtype=torch.float64)
    row[perm[1:1 + n_cluster]] = -d_of_j(j)
    rest = V - 1 - n_cluster
    row[perm[1 + n_cluster:]] = -30.0 - 0.5 * (torch.arange(rest) % 40).double()
    out = row.float()
    assert torch.equal(out.double(), row)                                   # exact in fp32
    return out


def _tied_bins_row(V):
    """bf16-exact: 0.0 once, 500 x -0.5, 2500 x -1.0, 2500 x -1.0078125 (both in level-0 bin 16), the rest far below."""
    perm = _scatter(V, 11)
    row = torch.empty(V)
    row[perm[0]] = 0.0
    row[perm[1:501]] = -0.5
    row[perm[501:3001]] = -1.0
    row[perm[3001:5501]] = -1.0078125
    row[perm[5501:]] = -30.0 - 0.5 * (torch.arange(V - 5501) % 40).float()
    return row


def _gauss(V, seed, scale=1.5):
    return torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale


def _draw_edge_row(V):
    """30 head tokens within 10 of the maximum (the first at id 3, the last at id V - 4, both 1 below it); ids 0 and V - 1
    at -40, everything else at -41 and below in steps of 0.25: every kept token has d <= 20 or d >= 40."""
    g = torch.Generator().manual_seed(5)
    row = -41.0 - 0.25 * (torch.arange(V) % 77).float()
    row[0] = row[V - 1] = -40.0
    head = torch.randperm(V - 20, generator=g)[:28] + 10
    row[head] = -(torch.rand(28, generator=g) * 8).mul(4).round().div(4)    # steps of 0.25: bf16-exact
    row[int(head[0])] = 0.0
    row[3] = row[V - 4] = -1.0
    return row


def _sample_cases(dtype):
    fp32 = dtype == torch.float32
    C = []
    add = lambda *a, **kw: C.append(_case(a[0], dtype, *a[1:], **kw))
    # ---- selection levels ---------------------------------------------------------------------------------------------
    if fp32:
        # d = 2^-6 + j 2^-26: level 0 (16 per unit) bin 0; level 1 (2^14) 256 + j 2^-12: bin 256; level 2 (lo = 2^-6,
        # 2^24) j / 4: four per bin, gathered
        row = _cluster_row(8192, lambda j: 2.0 ** -6 + j * 2.0 ** -26, 4096, 1)
        for k in (1000, 1024, 1025, 3000, 0):
            if k:
                add(f"three_levels_k{k}", row, top_k=k, reach="select(count): levels 0, 1, 2 then the gather; draw: "
                    + ("compact" if k <= 1024 else "scan"))
            add(f"three_levels_k{k}_p", row, top_k=k, frac=0.5,
                reach="top-p cut inside the cluster: " + ("compact all-pairs" if 0 < k <= 1024 else
                                                          "select(mass): levels 0, 1, 2 then the gather"))
        # the same away from d = 0, so that every level's lower edge adds to the one above: d = 2^-4 + 2^-10 + j 2^-27:
        # level 0 bin 1 (lo = 2^-4); level 1 16 + j 2^-13: bin 16 (lo = 2^-4 + 2^-10); level 2 j / 8: eight per bin
        row = _cluster_row(8192, lambda j: 2.0 ** -4 + 2.0 ** -10 + j * 2.0 ** -27, 4096, 4)
        for k in (1000, 3000):
            add(f"three_levels_offset_k{k}", row, top_k=k, reach="select(count): levels 0, 1, 2 with lo > 0 at each")
            add(f"three_levels_offset_k{k}_p", row, top_k=k, frac=0.4, reach="compact top-p / select(mass), lo > 0")
        # d = 1 + 2^-5 + (j - 2048) 2^-18: level 0 bin 16 (16.5 +- 0.125); level 1 (lo = 1, 2^14) 512 + (j - 2048) / 16:
        # sixteen per bin, gathered
        row = _cluster_row(8192, lambda j: 1.0 + 2.0 ** -5 + (j - 2048) * 2.0 ** -18, 4096, 2)
        for k in (1000, 3000):
            add(f"two_levels_k{k}", row, top_k=k, reach="select(count): levels 0, 1 then the gather")
            add(f"two_levels_k{k}_p", row, top_k=k, frac=0.6, reach="select(mass) or compact top-p inside the cluster")
    # two values in one level-0 bin, each tied more than 2048 times: level 1 separates them, level 2 sees one value
    row = _tied_bins_row(8192)
    add("tied_bin_k1500", row, top_k=1500, reach="select(count): level 1 bin 0 holds 2500 > 2048, level 2: set_min == set_max")
    add("tied_bin_k3500", row, top_k=3500, reach="select(count): level 1 bin 128, level 2: set_min == set_max")
    add("tied_bin_k600", row, top_k=600, reach="the same early return, then the compact gather overflows (3001 > 2048)")
    add("tied_bin_p", row, frac=0.55, reach="select(mass): the cut between the two tied values; level 2 early return")
    add("tied_bin_k3500_p", row, top_k=3500, frac=0.55, reach="select(count) then select(mass) under dcap = dk")
    # ---- the whole row tied -------------------------------------------------------------------------------------------
    for V in (1000, 3000):
        row = torch.full((V,), 1.5)
        us = [f32((t + 0.5) / V) for t in (0, V // 2, V - 1)]
        for k, p in ((0, 1.0), (5, 1.0), (0, 1e-6), (5, 1e-6)):
            c = _case(f"all_tied_V{V}_k{k}_p{p:g}", dtype, row, top_k=k, top_p=p, n=3, planted=us,
                      reach="select: set_min == set_max at level 0" + ("; compact" if k and V <= 2048 else "; scan"))
            c["planted_u"] = False                                            # mid-interval: the margins hold
            c["floor_uV"] = True
            C.append(c)
    # ---- far tail -----------------------------------------------------------------------------------------------------
    V = 4096
    row = -65.0 - (torch.arange(V) % 131).float()
    row[[100, 2000, 4000, 17]] = torch.tensor([5.0, 3.0, 0.0, -2.0])
    for k in (8, 2000):
        add(f"far_tail_k{k}", row, top_k=k, reach="select(count): level 0 bin 1023, returns +inf; the scan draw")
        add(f"far_tail_k{k}_p", row, top_k=k, frac=0.9, reach="the same, then select(mass) over the whole row")
    row = _gauss(V, 21, 2.0)
    for k in (8, 2000):
        add(f"far_tail_T0.02_k{k}", row, top_k=k, T=0.02, reach="as far_tail: d = (max - l) / 0.02")
    # ---- compact overflow ---------------------------------------------------------------------------------------------
    perm = _scatter(V, 3)
    row = torch.empty(V)
    row[perm[:800]] = -(torch.arange(800) // 8).float() / 64
    row[perm[800:2300]] = -4.0
    row[perm[2300:]] = -6.0 - (torch.arange(V - 2300) % 32).float() / 16
    add("compact_overflow", row, top_k=1000, reach="k <= 1024, 2300 candidates > 2048: the scan draw with dk set")
    add("compact_overflow_p", row, top_k=1000, frac=0.7, reach="the same with select(mass) under dcap = dk")
    # ---- top_k edges --------------------------------------------------------------------------------------------------
    V = 1500
    row = _gauss(V, 22)
    row[777] = float(row.min()) - 1.0
    for k in (V - 1, V, V + 1):
        add(f"top_k_V{'%+d' % (k - V) if k != V else ''}", row, top_k=k, reach="k = V - 1 drops one token; k >= V is off")
    # ---- -inf logits --------------------------------------------------------------------------------------------------
    V = 2000
    row = _gauss(V, 23)
    dead = torch.arange(V) % 2 == 1
    dead[:4] = True
    dead[-4:] = True
    dead[1000:1010] = False
    row[dead] = NEG_INF
    row[4], row[1994] = 1.0, 2.0                      # the first and the last finite id carry a clear share of the mass
    for name, k, p in (("k1500", 1500, None), ("k1010", 1010, None), ("p", 0, 0.8), ("plain", 0, None), ("k1010_p", 1010, 0.8)):
        add(f"neg_inf_half_{name}", row, top_k=k, frac=p, n=4, planted=(0.0, 1.0, ONE_BELOW),
            reach="d = +inf members; " + ("k > the finite count: level 0 bin 1023; " if k else "")
            + ("compact with -inf candidates" if k == 1010 else "scan"))
    row = torch.full((100,), NEG_INF)
    row[37] = 0.25
    add("neg_inf_one_finite", row, n=3, planted=(0.0, 1.0, 0.5), reach="one token of weight")
    add("neg_inf_one_finite_k5_p", row, top_k=5, top_p=0.5, n=3, planted=(0.0, 1.0, 0.5), reach="compact, 100 candidates")
    add("neg_inf_all", torch.full((100,), NEG_INF), n=2, reach="no finite maximum: id 0")
    row = _gauss(100, 24)
    row[55] = float("nan")
    add("one_nan", row, top_k=5, top_p=0.9, n=2, reach="no finite maximum: the NaN")
    row = row.clone()
    row[20] = row[70] = float("nan")
    row[3] = float("inf")
    add("nans_and_inf", row, n=2, reach="the lowest NaN wins over +inf")
    add("nans_and_inf_greedy", row, n=2, reach="the same without do_sample")
    C[-1]["do_sample"] = False
    row = _gauss(100, 25)
    row[40] = row[9] = float("inf")
    add("pos_inf", row, top_k=5, n=2, reach="no finite maximum: the first +inf")
    add("neg_inf_all_greedy", torch.full((100,), NEG_INF), n=2, reach="argmax of a row of -inf: id 0")
    C[-1]["do_sample"] = False
    # ---- draw edges ---------------------------------------------------------------------------------------------------
    row = _draw_edge_row(3000)
    for k in (50, 0, 1100):
        add(f"draw_edges_k{k}", row, top_k=k, n=4, planted=(0.0, 1.0, ONE_BELOW),
            reach=("compact" if k == 50 else "scan") + " draw: target 0, the target >= Zk clamp, the last unit of mass")
    # ---- top_p edges --------------------------------------------------------------------------------------------------
    V = 3000
    row = _gauss(V, 26)
    row[7] = row[V - 5] = float(row.max()) + 1.0
    for k in (0, 40):
        add(f"top_p_tiny_k{k}", row, top_k=k, top_p=1e-6, n=2, planted=(0.25, 0.75),
            reach="only the maximum's tie group stays: " + ("compact" if k else "select(mass) gathers bin 0"))
        C[-1]["planted_u"] = False
    row = -(torch.arange(1000) % 3).float()
    for k in (0, 900):
        add(f"top_p_one_below_k{k}", row, top_k=k, top_p=ONE_BELOW, reach="top_p = nextafter(1, 0): everything stays")
    # ---- vocabulary edges ---------------------------------------------------------------------------------------------
    for V in (1, 2, 31, 33, 1023, 1025):
        row = _gauss(V, 30 + V)
        add(f"vocab_{V}", row, reach="V against the 1024 threads and the last bitmap word", penalty=1.3,
            hist=[V - 1, 0])
        add(f"vocab_{V}_k3_p", row, top_k=3, frac=0.6 if V > 1 else None, top_p=0.5, penalty=1.3, hist=[V - 1, 0],
            reach="the same through select and the compact draw")
    return C


def _history_cases(dtype):
    """Rows that differ in their history; one launch each."""
    V, S = 1000, 12
    base = torch.full((V,), -45.0) - (torch.arange(V) % 50).float()
    row = base.clone()
    for i, x in {5: 6.0, 20: 3.0, 30: 2.875, 9: -1.0, 11: 0.0, 40: -1.25}.items():
        row[i] = x
    eos_row = base.clone()
    eos_row[777] = 4.0
    out = []
    for pen in (1.75, 0.5):
        hists = [[-1, V, 2 ** 30, 5, 5, 5, 5, 5, 9, 11],            # ignored ids; 5 once; negative, zero, positive
                 [1, 2, 3],                                         # nothing of the row penalised
                 [777] * S,                                         # full: no append, eos still finishes
                 [777] * S,                                         # hist_len = S + 3: clamped
                 [4, 4],                                            # finished: pad, n_kept 0
                 [9, -5, 30]]
        logits = torch.stack([row, row, eos_row, eos_row, row, row]).to(dtype)
        k = 5
        us = []
        for b, h in enumerate(hists):
            v = values(logits[b], h, pen, 1.0, True)
            us.append(mid_uniforms(v, k, 1.0, 3)[b % 3])
        c = dict(name=f"history_pen{pen:g}", logits=logits, hists=hists, S_hist=S, penalty=pen, T=1.0, top_k=k, top_p=1.0,
                 uniforms=us, planted_u=False, hist_len=[10, 3, S, S + 3, 2, 3], finished=[4], eos=[777], pad=3,
                 reach="mark_seen's range check and bitmap; append_token's len < S_hist and eos rules")
        out.append(c)
        g = dict(c, name=f"history_greedy_pen{pen:g}", do_sample=False)
        out.append(g)
    return out


def _big_vocab_case(dtype):
    """V = 262144, the bitmap limit: penalised ids V - 1 and V - 32 (the last word), the maximum at V - 1."""
    V = 262144
    row = _gauss(V, 40, 2.0)
    row[V - 1] = 14.0 * 1.25
    row[V - 32] = 13.0 * 1.25
    row = row.to(dtype)
    hist = [V - 1, V - 32, V - 1]
    v = values(row, hist, 1.25, 1.0, True)
    out = []
    for name, frac in (("", None), ("_p", 0.8)):
        top_p = 1.0 if frac is None else mid_top_p(v, 0, frac)
        us = mid_uniforms(v, 0, top_p, 2)
        out.append(dict(name=f"vocab_262144{name}", logits=row[None].repeat(2, 1), hists=[hist] * 2, S_hist=8, penalty=1.25,
                        T=1.0, top_k=0, top_p=top_p, uniforms=us, planted_u=False,
                        reach="the last bitmap word; 256 elements per thread in the scan draw"))
    return out


def _constrain_case(dtype):
    """-inf as constrain_logits_ writes it: every odd id forbidden as a one-id sequence, and (12, 400) after a 12."""
    V = 2000
    pre = _gauss(V, 41)
    pre[0], pre[1998] = 1.0, 2.0
    pre = pre.to(dtype)
    forbid = {(i,): NEG_INF for i in range(1, V, 2)}
    forbid[(12, 400)] = NEG_INF
    forbid[(13, 402)] = NEG_INF                                              # not matched: the history ends in 12
    hist = [7, 12]
    row = pre.clone()
    row[1::2] = NEG_INF
    row[400] = NEG_INF
    c = _case("neg_inf_from_constrain", dtype, row, top_k=1010, frac=0.8, n=4, planted=(0.0, 1.0, ONE_BELOW), hist=hist,
              reach="the logits of constrain_logits_ into the compact draw")
    c["pre_logits"] = pre[None].repeat(4, 1)
    c["forbid"] = forbid
    return c


@functools.lru_cache(maxsize=None)
def edge_cases(dtype):
    """Every planted case of tn_sample_step for fp32 or bf16 logits, with its expected result.  Built once per dtype and
    shared: treat as read-only."""
    cases = _sample_cases(dtype) + _history_cases(dtype) + _big_vocab_case(dtype) + [_constrain_case(dtype)]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return tuple(_finish(c) for c in cases)


# ------------------------------------------------------------------------------------------------ Kimi's sampled mode
KIMI_MARGIN = 1e-3          # the room test_injected_uniforms_draw_the_restatements_token leaves: fp32 weights and sums of
                            # at most 64 candidates are within ~1e-5 of the fp64 restatement


def _kimi_uniforms(rows, T, k):
    """One uniform per row: the middle region of an interval of the draw at least 4 * KIMI_MARGIN wide."""
    us = []
    for b, row in enumerate(rows):
        edges = torch.cat([torch.zeros(1, dtype=torch.float64), KR.boundaries(row, T, k)])
        width = edges[1:] - edges[:-1]
        pick = [j for j in range(width.numel()) if float(width[j]) > 4 * KIMI_MARGIN]
        j = pick[(b * 5 + 1) % len(pick)] if b else pick[-1]
        us.append(f32(float(edges[j]) + (0.25 + 0.25 * (b % 3)) * float(width[j])))
    return us


def _kimi_case(name, dtype, logits, k, T=0.8, reach=""):
    """A window id among the candidates (penalty 1.1 over the last 4 generated ids), the rest as planted."""
    B, V = logits.shape
    W, pen, prompt = 4, 1.1, 3
    logits = logits.to(dtype)
    g = torch.Generator().manual_seed(V + k)
    hists = [torch.randint(0, V, (prompt + 6,), generator=g).tolist() for _ in range(B)]
    rows = [KR.penalised(logits[b], KR.window_of(torch.tensor(hists[b]), len(hists[b]), prompt, W, pen), pen)
            for b in range(B)]
    return dict(name=name, logits=logits, hists=hists, prompts=[prompt] * B, penalty=pen, window=W, T=T, top_k=k,
                uniforms=_kimi_uniforms(rows, T, k), rows=rows, reach=reach)


@functools.lru_cache(maxsize=None)
def kimi_edge_cases(dtype):
    C = []
    for V in (1024, 1025, 4099, 168448):
        B = 1 if V == 168448 else 4
        for k in (1, 5, 64):
            lg = _gauss(B * V, 50 + k, 1.5).view(B, V)
            lg[0, 50] = lg[0, min(60 + 1024, V - 1)] = float(lg[0].max()) + 1.0   # tied candidates: the lower id first
            C.append(_kimi_case(f"kimi_V{V}_k{k}", dtype, lg, k,
                                reach="the k-th best thread maximum bounds the row's k-th best; gather and rank in LDS"))
    # 3000 tokens tie for the maximum, all owned by 20 of the 1024 threads (ids = r mod 1024, r < 20): the 64th best
    # thread maximum lies below them, all 3000 are gathered, 3000 > 2048: one-by-one picks — the k lowest ids in id order
    V = 168448
    ids = (torch.arange(150)[:, None] * 1024 + torch.arange(20)[None] * 37 % 1024).reshape(-1)
    lg = _gauss(V, 60, 1.0).view(1, V).clamp(max=3.0)
    lg[0, ids] = 6.0
    for k in (32, 64):
        C.append(_kimi_case(f"kimi_3000_tied_k{k}", dtype, lg, k, reach="n_cand > 2048: the one-by-one fallback, ties"))
    # the same ids with 3000 descending values in scattered order: the fallback must order by value, then by id
    lg = lg.clone()
    lg[0, ids[_scatter(3000, 61)]] = 6.0 - torch.arange(3000).float() / 1024
    C.append(_kimi_case("kimi_3000_ranked_k64", dtype, lg, 64, reach="the one-by-one fallback on distinct and tied values"))
    C.append(_kimi_case("kimi_V3_k5", dtype, torch.tensor([[0.5, 1.25, -0.75], [2.0, 2.0, 1.0]]), 5, reach="k = min(top_k, V)"))
    lg = torch.full((3, 1500), NEG_INF)
    lg[:, [1400, 3, 700]] = torch.tensor([1.0, 0.5, 0.0])
    C.append(_kimi_case("kimi_neg_inf_k5", dtype, lg, 5, reach="fewer finite values than k: -inf candidates of weight 0"))
    C.append(_kimi_case("kimi_neg_inf_k64", dtype, lg, 64, reach="the same with most thread maxima at -inf"))
    return tuple(C)
