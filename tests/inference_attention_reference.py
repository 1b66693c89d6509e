"""Plain float64 restatements of the three inference attention entry points — tn_attn_decode and tn_attn_decode_beam
(csrc/attn_decode.hip), tn_attn_block_causal_fwd (csrc/attn_block_causal.hip) — the error budgets the GPU test holds the
kernels to, and the cases and inputs that tests/test_inference_attention_reference_cpu.py and
tests/test_inference_attention_edges_gpu.py share.  No GPU, no HIP: torch on the CPU only.  `Ref`, `budget`, `ratios`,
`check`, `ulp`, `d` and the roundoff constants are attention_reference.py's.

What is computed, over the kernels' own inputs (bf16 tensors widened to float64; `scale` as the fp32 number the entry
point receives):
  decode        row b, query head h (kv head h // G) attends to cache[src[b, s] if src is given else b, s] for
                s < cache_len[b], and to k_new / v_new[b] at index cache_len[b].  Only the consulted positions are gathered,
                so whatever else the caches or the table hold cannot enter.  cache_len[b] outside [0, S_max): NaN, cache
                untouched.  A consulted table entry outside [0, B): NaN (the slot is still written: the header promises an
                untouched cache for a refused LENGTH only).  Also returned: the caches after the call — slot
                [b, cache_len[b]] holds k_new / v_new[b], nothing else changes.
  block_causal  key j is allowed for query i iff seg_start[i] <= j < key_end[i] and
                (j - seg_start[i]) // block <= (i - seg_start[i]) // block; a row without an allowed key is exactly 0.

The budgets.  `budget(Ref(value, slack))` = half an ulp of bf16 at |value| + slack (the final `f2bf` / `pack2bf`) + slack.
Each term of `slack` is a unit roundoff (U32 = 2^-24 one fp32 operation, ULP32 = 2^-23 one MFMA term or one division,
EXP = 2^-23 v_exp_f32 / v_log_f32, UBF = 2^-8 P through bf16) times the magnitudes it acts on, to first order.

DECODE (LPK = D / 8 lanes per key, KPW = 64 / LPK keys per wave and iteration, KPI = 4 KPW; a2 = scale log2(e) q . k):
  logit   E_j = (1 + 8 + log2 LPK) U32 c sum_d |q_d| |k_d| + 2 U32 |a2_j|                             (log2 domain)
          one rounding of q_d * scale_log2, the 8 fmas of a lane, log2 LPK shuffle adds; scale_log2 = scale * kLog2e is
          an fp32 product of an fp32 constant (2 roundings, relative, on every logit)
  per key R_j = ln2 E_j + 2 ln2 U32 (max a2 - a2_j) + C_exp EXP + C_u32 U32        relative error of key j's share
          the subtraction s - mn in front of fast_exp2 (|s - mn| <= max a2 - a2_j), and the subtractions m - mn of every
          later rescale, lane-group merge, wave merge and split weight, which telescope to at most max a2 - a2_j again;
          C_exp = 1 (p) + n_lane (alpha of every later key of the lane) + log2 KPW (group merges) + 1 (wave merge)
          C_u32 = 1 (p * v) + n_lane (the fma on l / acc) + 2 log2 KPW (product and sum of a merge) + 4 (wave fma chain)
          n_lane = ceil(keys of the longest split / KPI), the keys one lane handles
  one split   slack = sum_j p_j R_j (|v_j| + |o|) + ULP32 |o| (ot / lt) + FLUSH
  more splits slack = sum_j p_j R_j (|v_j| + |on_s(j)|) + ULP32 sum_s W_s |on_s|            (each split's own ot / lt)
                    + sum_s (W_s w_s + sum_{j in s} p_j R_j) (|on_s| + |o|) + ULP32 |o| + FLUSH
          W_s the true weight of split s, on_s its normalised output; lse_s = mx + __log2f(lt) carries lt's relative
          error (the sum over j in s) and  w_s = ln2 (EXP log2 n_s + U32 |lse_s| + U32 (max lse - lse_s)) + EXP + nsplit U32:
          v_log_f32 (|log2 lt| <= log2 n_s), the add mx + ., the subtraction v - mx, fast_exp2, and the nsplit adds / fmas
          of wsum and acc; the last ULP32 |o| is acc / wsum
  FLUSH = n 2^-126 (max |v| + |o|): fast_exp2 flushes denormal results to 0
Decode never rounds P to bf16: there is no UBF term, and the budget is half a bf16 ulp plus fp32 terms.

BLOCK-CAUSAL (the packed forward's structure, D = 64, 64-key tiles, no deferred rescale):
  Ef_j = D ULP32 scale sum_d |q_d| |k_d| + ln2 U32 (3 |a2_j| + 2 (max a2 - a2_j)) + EXP
          mfma32 logits; s * scale_log2 (one product, two roundings inside scale_log2); the subtraction s - m_use and the
          telescoping m - m_use of the rescales; fast_exp2
  slack(O) = UBF A + sum_j p_j Ef_j (|v_j| + |O|) + ((n + 2 nt + 2) ULP32 + nt EXP) (A + |O|) + FLUSH,  A = sum_j p_j |v_j|
          pack2bf of p at an unknown binade (UBF); n MFMA terms of O and n adds of the row sum (taken from the unrounded p);
          per tile the row reads (nt of them) l * alpha, + ps, acc * alpha and alpha's own EXP; 1 / l and the product with it
There is no free multiplier in either.

Inputs.  gauss: randn.  sharp: q and k of deviation (16 / (scale sqrt D))^0.5, logits of deviation 16.  planted: gauss
plus ANCHORS (a key one query row must see: k = q_i ANCHOR_LOGIT / (scale |q_i|^2), v a constant of magnitude 2..3.75 —
`_plant`'s arithmetic) and, for block-causal, BAITS (a key the row must not see: logit 40, v = +-32, finite, because that
kernel multiplies masked keys by p = 0).  Decode's baits are NaN: every cache element at a position >= cache_len[b] (the
slot to be written included) is 0x7fc0 in K and V, and every table entry at s >= cache_len[r] is junk.  For the beam entry
the valid part of cache row r is s < cache_len[r], and a consulted table entry names a row that is valid at s (which also
keeps the entry point's precondition)."""
import functools
import math
from collections import namedtuple

import torch

from attention_reference import (ANCHOR_LOGIT, BAIT_LOGIT, BAIT_V, BF, EXP, F64, LN2, LOG2E, TINY, U32, UBF, ULP32, Ref,
                                 budget, check, d, ratios, ulp)

__all__ = ["Ref", "budget", "check", "d", "ratios", "ulp"]

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
NAN_BITS = 0x7fc0
JUNK = (1 << 20, -1, INT32_MIN)
GUARD = 4096


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# ================================================================================================ decode: geometry
def num_splits(B, Nkv, S_max):
    """attn_decode.hip: ceil(512 / (B Nkv)) workgroups' worth, at most ceil(S_max / 64), at most 64, at least 1"""
    units = B * Nkv
    return max(1, min((512 + units - 1) // units, (S_max + 63) // 64, 64))


def split_keys(total, nsplit):
    """keys per split of a row with `total` keys: a multiple of 64, at least 64"""
    c = (total + nsplit - 1) // nsplit
    return max(64, (c + 63) // 64 * 64)


def lane_geometry(D):
    """(LPK lanes per key row, KPW keys per wave per iteration, KPI keys per workgroup per iteration)"""
    lpk = D // 8
    return lpk, 64 // lpk, 4 * (64 // lpk)


# ================================================================================================ decode: reference
def decode(q, k_new, v_new, k_cache, v_cache, cache_len, scale, src=None):
    """-> (Ref of o [B, Nh, D], expected k_cache, expected v_cache)"""
    B, Nh, D = q.shape
    S_max, Nkv = k_cache.shape[1], k_cache.shape[2]
    G = Nh // Nkv
    c2 = f32(scale) * LOG2E
    ns = num_splits(B, Nkv, S_max)
    lpk, kpw, kpi = lane_geometry(D)
    val = torch.full((B, Nh, D), math.nan, dtype=F64)
    slack = torch.zeros(B, Nh, D, dtype=F64)
    k_exp, v_exp = k_cache.clone(), v_cache.clone()
    for b in range(B):
        n = int(cache_len[b])
        if not 0 <= n < S_max:
            continue
        k_exp[b, n], v_exp[b, n] = k_new[b], v_new[b]
        pos = torch.arange(n)
        rows = src[b, :n].long() if src is not None else torch.full((n,), b, dtype=torch.long)
        if bool(((rows < 0) | (rows >= B)).any()):
            continue
        kk = torch.cat([d(k_cache[rows, pos]), d(k_new[b])[None]]).repeat_interleave(G, dim=1).transpose(0, 1)
        vv = torch.cat([d(v_cache[rows, pos]), d(v_new[b])[None]]).repeat_interleave(G, dim=1).transpose(0, 1)
        qd = d(q[b])                                                                 # [Nh, D]; kk / vv [Nh, n + 1, D]
        a2 = c2 * torch.einsum("hd,hnd->hn", qd, kk)
        mag = c2 * torch.einsum("hd,hnd->hn", qd.abs(), kk.abs())
        mx = a2.amax(-1, keepdim=True)
        e = torch.exp2(a2 - mx)
        p = e / e.sum(-1, keepdim=True)
        o = torch.einsum("hn,hnd->hd", p, vv)
        total = n + 1
        chunk = split_keys(total, ns)
        n_lane = -(-min(chunk, total) // kpi)
        E = (9 + math.log2(lpk)) * U32 * mag + 2 * U32 * a2.abs()
        c_exp = 2 + n_lane + math.log2(kpw)
        c_u32 = 5 + n_lane + 2 * math.log2(kpw)
        pR = p * (LN2 * E + 2 * LN2 * U32 * (mx - a2) + c_exp * EXP + c_u32 * U32)
        av, ao = vv.abs(), o.abs()
        flush = total * TINY * (av.amax(1) + ao)
        if ns == 1:
            sl = torch.einsum("hn,hnd->hd", pR, av) + pR.sum(-1, keepdim=True) * ao + ULP32 * ao + flush
        else:
            M = torch.nn.functional.one_hot(torch.arange(total) // chunk, ns).to(F64)          # [total, ns]
            W = p @ M
            on = torch.einsum("hn,hnd,ns->hsd", p, vv, M) / W.clamp_min(TINY)[..., None]
            nk = M.sum(0)
            lse = mx + torch.log2((e @ M).clamp_min(TINY))
            lse_max = torch.where(nk > 0, lse, torch.full_like(lse, -math.inf)).amax(-1, keepdim=True)
            w = LN2 * (EXP * torch.log2(nk.clamp_min(1.0)) + U32 * lse.abs() + U32 * (lse_max - lse)) + EXP + ns * U32
            w = torch.where(nk > 0, w, torch.zeros_like(w))
            aon = on.abs()
            sl = (torch.einsum("hn,hnd->hd", pR, av) + torch.einsum("hn,ns,hsd->hd", pR, M, aon)
                  + ULP32 * torch.einsum("hs,hsd->hd", W, aon)
                  + torch.einsum("hs,hsd->hd", W * w + pR @ M, aon + ao[:, None, :]) + ULP32 * ao + flush)
        val[b], slack[b] = o, sl
    return Ref(val, slack), k_exp, v_exp


# ================================================================================================ block-causal: reference
def bc_allow(seg_start, key_end, block):
    """bool [B, T(query), T(key)]"""
    T = seg_start.shape[1]
    i, j = torch.arange(T)[None, :, None], torch.arange(T)[None, None, :]
    s, e = seg_start.long()[:, :, None], key_end.long()[:, :, None]
    return (j >= s) & (j < e) & ((j - s) // block <= (i - s) // block)


def block_causal(q, k, v, seg_start, key_end, block, scale):
    """-> Ref of o [B, T, Nh, D]"""
    B, T, Nh, D = q.shape
    scale = f32(scale)
    qh, kh, vh = (d(t).transpose(1, 2) for t in (q, k, v))
    al = bc_allow(seg_start, key_end, block)[:, None]
    a = scale * (qh @ kh.transpose(-1, -2))
    a = torch.where(al, a, torch.zeros_like(a))
    dead = ~al.any(-1, keepdim=True)
    inf = torch.tensor(math.inf, dtype=F64)
    mx = torch.where(al, a, -inf).amax(-1, keepdim=True)
    mx = torch.where(dead, torch.zeros_like(mx), mx)
    e = torch.where(al, torch.exp(a - mx), torch.zeros_like(a))
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(dead, torch.ones_like(l), l)
    o = p @ vh
    n = al.sum(-1, keepdim=True).to(F64)
    j = torch.arange(T)
    first = torch.where(al, j, torch.tensor(T)).amin(-1, keepdim=True)
    last = torch.where(al, j, torch.tensor(-1)).amax(-1, keepdim=True)
    nt = torch.where(dead, torch.zeros_like(first), last // 64 - first // 64 + 1).to(F64)
    a2 = a * LOG2E
    Ef = D * ULP32 * scale * (qh.abs() @ kh.abs().transpose(-1, -2)) + LN2 * U32 * (3 * a2.abs() + 2 * (mx * LOG2E - a2).abs()) + EXP
    pE = p * Ef
    av, ao = vh.abs(), o.abs()
    A = p @ av
    so = (UBF * A + pE @ av + pE.sum(-1, keepdim=True) * ao + ((n + 2 * nt + 2) * ULP32 + nt * EXP) * (A + ao)
          + n * TINY * (av.amax(2, keepdim=True) + ao))
    return Ref(o.transpose(1, 2), so.transpose(1, 2))


# ================================================================================================ decode: cases
DCase = namedtuple("DCase", ["name", "B", "Nh", "Nkv", "D", "S_max", "lens", "kind", "scale"])
DAnchor = namedtuple("DAnchor", ["kinds", "b", "h", "j"])            # key j (cache_len[b] = the new key) of row b, head h
DInputs = namedtuple("DInputs", ["q", "k_new", "v_new", "k_cache", "v_cache", "cache_len", "src", "anchors"])
DECODE_GEOMS = ((1, 1), (4, 1), (14, 2), (6, 3), (16, 1))
EDGE_LENS = (0, 1, 3, 4, 7, 8, 15, 16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 199)
TABLES = ("identity", "row0", "random", "mixed")


def _decode_cases():
    """allG: every G at both D on the split path (B Nkv = 6, S_max = 200: 4 splits of 64).  len: the edge lengths rotated
    through the five geometries, once per D, at S_max = 200 — 64, 128 and 192 put the new key first in its split (its only
    key), 63 and 127 last in a full one, 199 is the last legal slot.  short_long: len = 1 and 2000 at S_max = 4100 (64
    splits, 63 of them empty in row 0).  smax1 / 63 / 64: one split; smax65: two.  units512 / 171 / 256: the workgroup
    target caps the count at 1 / 3 / 2 (the two latter cannot have fewer than B Nkv S_max D 4 bytes = 5.7 / 4.6 MB of
    cache).  cap64: 64 full splits / 33 used / 1 used.  scale = 0.2 and sharp once per D."""
    out = []
    for D in (64, 128):
        for G in range(1, 17):
            out.append(DCase(f"allG{G}", 3, 2 * G, 2, D, 200, (0, 63, 130), "planted", D ** -0.5))
    for gi, (nh, nkv) in enumerate(DECODE_GEOMS):
        out.append(DCase(f"len{gi}", len(EDGE_LENS[gi::5]), nh, nkv, 64, 200, EDGE_LENS[gi::5], "planted", 64 ** -0.5))
        lens = EDGE_LENS[(gi + 2) % 5::5]
        out.append(DCase(f"len{gi}", len(lens), nh, nkv, 128, 200, lens, "planted", 128 ** -0.5))
    out.append(DCase("short_long", 2, 4, 1, 64, 4100, (1, 2000), "planted", 64 ** -0.5))
    out.append(DCase("smax1", 2, 4, 1, 64, 1, (0, 0), "planted", 64 ** -0.5))
    out.append(DCase("smax63", 3, 14, 2, 128, 63, (0, 62, 31), "planted", 128 ** -0.5))
    out.append(DCase("smax64", 3, 6, 3, 64, 64, (63, 0, 40), "planted", 64 ** -0.5))
    out.append(DCase("smax65", 3, 4, 1, 128, 65, (0, 63, 64), "planted", 128 ** -0.5))
    g = torch.Generator().manual_seed(512)
    lens = torch.randint(0, 140, (64,), generator=g).tolist()
    lens[:6] = [139, 0, 63, 64, 65, 128]
    out.append(DCase("units512", 64, 8, 8, 64, 140, tuple(lens), "planted", 64 ** -0.5))
    cyc = (0, 63, 64, 65, 127, 128, 129)
    out.append(DCase("units171", 171, 1, 1, 64, 130, tuple(cyc[i % 7] for i in range(171)), "planted", 64 ** -0.5))
    out.append(DCase("units256", 128, 4, 2, 64, 70, tuple((0, 63, 64, 69, 31)[i % 5] for i in range(128)), "planted", 64 ** -0.5))
    out.append(DCase("cap64_full", 1, 4, 1, 64, 4160, (4095,), "planted", 64 ** -0.5))
    out.append(DCase("cap64_33", 1, 1, 1, 128, 4160, (4096,), "planted", 128 ** -0.5))
    out.append(DCase("cap64_1", 1, 16, 1, 64, 4160, (0,), "planted", 64 ** -0.5))
    for D in (64, 128):
        out.append(DCase("scale", 3, 4, 1, D, 200, (5, 70, 199), "planted", 0.2))
        out.append(DCase("sharp", 3, 14, 2, D, 200, (5, 130, 199), "sharp", D ** -0.5))
    return tuple(out)


DECODE_CASES = _decode_cases()


def dcase_id(c):
    return f"{c.name}-D{c.D}-{c.Nh}x{c.Nkv}-B{c.B}-S{c.S_max}-{c.kind}-s{c.scale:.3g}"


def make_table(kind, lens, S_max, seed, junk):
    """int32 [R, S_max].  Consulted entries (s < lens[r]) name a row that is valid at s (lens[row] > s), the row itself
    where the rule would not — the repair of test_beam_search_gpu.py's fixture, which also keeps the precondition; every
    other entry is `junk`."""
    R = len(lens)
    L = torch.tensor(lens)[:, None]
    s = torch.arange(S_max)[None, :]
    own = torch.arange(R)[:, None].expand(R, S_max)
    if kind == "identity":
        want = own
    elif kind == "row0":
        want = torch.zeros(R, S_max, dtype=torch.long)
    elif kind == "random":                                  # any row of the same utterance (three beams each)
        g = torch.Generator().manual_seed(seed)
        want = torch.minimum(own // 3 * 3 + torch.randint(0, 3, (R, S_max), generator=g), torch.tensor(R - 1))
    elif kind == "mixed":                                   # rows of different lengths reading each other
        want = (own + 1 + s) % R
    else:
        raise ValueError(kind)
    want = torch.where(torch.tensor(lens)[want] > s, want, own)
    return torch.where(s < L, want, torch.tensor(junk)).to(torch.int32)


def decode_anchor_positions(n, ns, D):
    """{key index: kinds} of a row with n cached keys (index n = the new key)"""
    _, kpw, kpi = lane_geometry(D)
    total = n + 1
    chunk = split_keys(total, ns)
    out = {}

    def add(j, kind):
        if 0 <= j < total:
            out.setdefault(j, []).append(kind)

    add(0, "first")
    add(n - 1, "last_cached")
    add(n, "new")
    for s in range(ns):
        k0, k1 = s * chunk, min((s + 1) * chunk, total)
        if k0 < k1:
            add(k0, "split_first")
            add(k1 - 1, "split_last")
    for w in range(4):                                      # iteration 0 of split 0
        if w * kpw + kpw - 1 < min(chunk, total):
            add(w * kpw, "wave_first")
            add(w * kpw + kpw - 1, "wave_last")
    k0 = (total - 1) // chunk * chunk                       # the last split's tail iteration, when some lanes are invalid
    if (total - k0) % kpi:
        base = k0 + (total - k0) // kpi * kpi
        add(base + (total - base) // 2, "tail")
    return out


def plant_key(qrow, logit, scale):
    """`_plant`'s key: alpha q with scale * q . (alpha q) = logit"""
    qf = qrow.float()
    return (qf * (logit / (scale * float(qf.square().sum())))).to(BF)


def decode_inputs(case, seed, table=None, junk=JUNK[0]):
    B, Nh, Nkv, D, S = case.B, case.Nh, case.Nkv, case.D, case.S_max
    G = Nh // Nkv
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Nh, D, generator=g)
    kn, vn = torch.randn(B, Nkv, D, generator=g), torch.randn(B, Nkv, D, generator=g)
    kc, vc = torch.randn(B, S, Nkv, D, generator=g), torch.randn(B, S, Nkv, D, generator=g)
    if case.kind == "sharp":
        sd = math.sqrt(16.0 / (case.scale * math.sqrt(D)))
        q, kn, kc = q * sd, kn * sd, kc * sd
    q, kn, vn, kc, vc = (t.to(BF) for t in (q, kn, vn, kc, vc))
    # (through a table the longest row comes first: "every row reads row 0" then shares as much as can be shared)
    lens = sorted(case.lens, reverse=True) if table is not None else list(case.lens)
    src = make_table(table, lens, S, seed, junk) if table is not None else None
    anchors = []
    if case.kind == "planted":
        ns = num_splits(B, Nkv, S)
        want = [sorted(decode_anchor_positions(n, ns, D).items()) for n in lens]
        used, count, per_head = set(), 0, {}
        for i in range(max(len(w) for w in want)):          # request i of every row, the rows taking turns to go first
            for b in [(i + r) % B for r in range(B)]:
                if i >= len(want[b]):
                    continue
                j, kinds = want[b][i]
                hk = count % Nkv
                h = hk * G + (count // Nkv) % G
                new = j == lens[b]
                slot = ("new", b, hk) if new else (int(src[b, j]) if src is not None else b, j, hk)
                if slot in used:
                    continue
                used.add(slot)
                key = plant_key(q[b, h], ANCHOR_LOGIT, case.scale)
                # magnitude by the anchor's rank in its head, signs drawn per anchor: no two anchors a head sees agree
                nth = per_head[(b, h)] = per_head.get((b, h), -1) + 1
                signs = torch.randint(0, 2, (D,), generator=torch.Generator().manual_seed(count)) * 2.0 - 1.0
                value = ((2.0 + 0.25 * (nth % 8)) * signs).to(BF)
                if new:
                    kn[b, hk], vn[b, hk] = key, value
                else:
                    kc[slot[0], j, hk], vc[slot[0], j, hk] = key, value
                anchors.append(DAnchor(tuple(kinds), b, h, j))
                count += 1
    for b, n in enumerate(lens):                            # stale memory
        kc.view(torch.int16)[b, n:] = NAN_BITS
        vc.view(torch.int16)[b, n:] = NAN_BITS
    return DInputs(q, kn, vn, kc, vc, torch.tensor(lens, dtype=torch.int32), src, anchors)


def beam_variant(idx):
    """(table kind, junk value) of DECODE_CASES[idx] through the beam entry: both rotate"""
    return TABLES[idx % 4], JUNK[idx % 3]


@functools.lru_cache(maxsize=None)
def decode_problem(idx, beam=False):
    """(inputs, Ref, expected k_cache, expected v_cache) of DECODE_CASES[idx]: built once, shared, never modified"""
    case = DECODE_CASES[idx]
    table, junk = beam_variant(idx) if beam else (None, 0)
    inp = decode_inputs(case, 3000 + idx, table, junk)
    return (inp,) + decode(inp.q, inp.k_new, inp.v_new, inp.k_cache, inp.v_cache, inp.cache_len, case.scale, inp.src)


# ================================================================================================ block-causal: cases
BCase = namedtuple("BCase", ["name", "rows", "block", "Nh", "kind", "scale"])   # rows: per batch row, (frames, valid) clips
BPlant = namedtuple("BPlant", ["kind", "b", "h", "i", "j"])
BInputs = namedtuple("BInputs", ["q", "k", "v", "seg_start", "key_end", "anchors", "baits"])
CLIPS = ((37, 37), (91, 60), (1, 1), (130, 0), (74, 73), (67, 50))
S0 = 64 ** -0.5


def _one(T, *key_ends):
    return tuple(((T, e),) for e in key_ends)


def _pick(*idx):
    return tuple(CLIPS[i] for i in idx)


def _block_causal_cases():
    """T classes: below a tile (1, 31, 33), within a workgroup (127, 128, 129), several workgroups (200, 333, 400).  Block
    classes: 1; below a wave's rows (7); a wave / a tile (32, 50, 64); above a tile (100, 128); above T (T + 5).  Clip
    classes: one clip with key_end = T; one clip with key_end in {0, 1, block - 1, block, block + 1, T - 1}; packed clips;
    a workgroup that sees nothing.  Every T, every block and every key_end appears, and every pair of classes does."""
    c = []
    s = lambda name, rows, block, Nh, kind="planted", scale=S0: c.append(BCase(name, rows, block, Nh, kind, scale))
    s("one", _one(1, 1), 1, 1)
    s("one", _one(1, 0, 1), 6, 3)
    s("one", _one(31, 31, 30), 7, 3)
    s("one", _one(31, 1), 1, 1)
    s("one", _one(33, 33, 31), 32, 1)
    s("one", _one(33, 32, 1), 38, 3)
    s("one", _one(127, 127, 49), 50, 1)
    s("one", _one(127, 64, 65), 64, 3)
    s("one", _one(128, 128, 127), 128, 1)
    s("one", _one(128, 128, 0), 1, 3)
    s("one", _one(129, 129, 63), 64, 1)
    s("one", _one(129, 129, 128), 128, 3)
    s("one", _one(129, 101, 1), 100, 1)
    s("one", _one(129, 128, 8), 7, 1)
    s("one", _one(129, 129), 134, 1)
    s("one", _one(200, 200, 51), 50, 3)
    s("one", _one(200, 199, 6), 7, 1)
    s("one", _one(200, 200, 100), 205, 1)
    s("one", _one(200, 200, 49), 50, 1, "planted", 0.2)
    s("one", _one(333, 333, 100), 100, 1, "sharp")
    s("one", _one(333, 332, 33), 32, 1)
    s("one", _one(400, 400, 129), 128, 1)
    s("one", _one(400, 399, 0), 64, 3)
    s("one", _one(400, 400), 1, 1)
    s("one", _one(400, 400, 99), 100, 1)
    s("packed", (_pick(0, 2, 1, 3, 4, 5), _pick(4, 5, 3, 2, 0, 1)), 50, 3)
    s("packed", (_pick(0, 3, 1, 4, 2, 5),), 7, 1)
    s("packed", (_pick(5, 4, 3, 2, 1, 0), _pick(0, 2, 1, 3, 5, 4)), 64, 1)
    s("packed", (_pick(0, 2, 1, 3, 4), _pick(4, 3, 2, 0, 1)), 100, 3)
    s("packed", (_pick(5, 4, 3, 2, 0, 1),), 128, 1)
    s("packed", (_pick(0, 2, 1),), 32, 3)
    s("packed", (_pick(0, 2, 1, 4, 3, 5),), 405, 1)
    s("dead_wg", (((128, 100), (128, 0), (77, 77)),), 50, 1)
    return tuple(c)


BLOCK_CAUSAL_CASES = _block_causal_cases()


def bcase_id(c):
    T = sum(f for f, _ in c.rows[0])
    ends = "_".join(str(r[0][1]) for r in c.rows) if c.name == "one" else f"{len(c.rows[0])}clips"
    return f"{c.name}-T{T}-blk{c.block}-end{ends}-B{len(c.rows)}-Nh{c.Nh}-{c.kind}-s{c.scale:.3g}"


def bc_layout(rows):
    """-> (seg_start, key_end) int32 [B, T]"""
    ss, ke = [], []
    for clips in rows:
        s_row, e_row, off = [], [], 0
        for f, L in clips:
            s_row += [off] * f
            e_row += [off + L] * f
            off += f
        ss.append(s_row), ke.append(e_row)
    return torch.tensor(ss, dtype=torch.int32), torch.tensor(ke, dtype=torch.int32)


def _bc_plant(q, k, v, rows, block, scale):
    """Target rows per clip: its first and last row, the last valid and the first invalid one, the rows on either side of
    the first block edge, the first row of the last block, the middle, and the rows at absolute positions 63 / 64 mod 64.
    Target t owns head t % Nh.  First every target's BAITS — the first key of the next block, key key_end (the first
    invalid frame), the previous clip's last key and the next clip's first — then the ANCHORS of every target that is
    still quiet (no key it may see is within 3.5 of the anchor logit: other rows' baits are ordinary keys to it): the
    clip's first key, the row's last allowed key, the first and last key of each 64-key tile it reads, its own position."""
    B, T, Nh, D = q.shape
    ss, ke = bc_layout(rows)
    allow = bc_allow(ss, ke, block)
    anchors, baits, used, targets = [], [], set(), []

    def put(kind, b, h, i, j, logit, value, into):
        if (b, j, h) in used or not 0 <= j < T:
            return
        used.add((b, j, h))
        k[b, j, h] = plant_key(q[b, i, h], logit, scale)
        v[b, j, h] = torch.as_tensor(value, dtype=torch.float32).to(BF)
        into.append(BPlant(kind, b, h, i, j))

    for b, clips in enumerate(rows):
        s = 0
        for f, L in clips:
            cand = {s, s + f - 1, s + L - 1, s + L, s + block - 1, s + block, s + (f - 1) // block * block, s + f // 2}
            cand |= {p for p in range(s, s + f) if p % 64 in (0, 63)}
            for i in sorted(p for p in cand if s <= p < s + f):
                targets.append((b, len(targets) % Nh, i, s, f, L))
            s += f
    for b, h, i, s, f, L in targets:
        unseen = lambda j: not (0 <= j < T) or not bool(allow[b, i, j])
        signs = lambda: torch.randint(0, 2, (D,), generator=torch.Generator().manual_seed(len(baits))) * 2.0 - 1.0
        nb = s + ((i - s) // block + 1) * block
        wanted = [("next_block", nb if nb < s + L else -1), ("key_end", s + L if s + L < T else -1),
                  ("prev_clip_last", s - 1), ("next_clip_first", s + f if s + f < T else -1)]
        for kind, j in wanted:
            assert unseen(j), (kind, b, i, j)
            put(kind, b, h, i, j, BAIT_LOGIT, BAIT_V * signs(), baits)
    for b, h, i, s, f, L in targets:
        lo, hi = s, min(s + L, s + ((i - s) // block + 1) * block)
        if hi <= lo:
            continue
        cand = {lo: "clip_first", hi - 1: "last_allowed"}
        for t in range(lo // 64, (hi - 1) // 64 + 1):
            cand.setdefault(max(lo, 64 * t), "tile_first")
            cand.setdefault(min(hi - 1, 64 * t + 63), "tile_last")
        if lo <= i < hi:
            cand.setdefault(i, "diagonal")
        cand = {j: kind for j, kind in cand.items() if (b, j, h) not in used}
        rest = allow[b, i].clone()
        rest[list(cand)] = False
        a = scale * (k[b, :, h].float() @ q[b, i, h].float())[rest]
        if a.numel() and float(a.max()) > ANCHOR_LOGIT - 3.5:
            continue
        for j, kind in sorted(cand.items()):
            idx = len(anchors)
            put(kind, b, h, i, j, ANCHOR_LOGIT, (2.0 + 0.25 * (idx % 8)) * (-1.0) ** idx, anchors)
    return anchors, baits


def bc_inputs(case, seed):
    B, T = len(case.rows), sum(f for f, _ in case.rows[0])
    assert all(sum(f for f, _ in r) == T for r in case.rows)
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, T, case.Nh, 64, generator=g) for _ in range(3))
    if case.kind == "sharp":
        sd = math.sqrt(16.0 / (case.scale * 8.0))
        q, k = q * sd, k * sd
    q, k, v = (t.to(BF) for t in (q, k, v))
    anchors, baits = _bc_plant(q, k, v, case.rows, case.block, case.scale) if case.kind == "planted" else ([], [])
    ss, ke = bc_layout(case.rows)
    return BInputs(q, k, v, ss, ke, anchors, baits)


@functools.lru_cache(maxsize=None)
def bc_problem(idx):
    """(inputs, Ref) of BLOCK_CAUSAL_CASES[idx]: built once, shared, never modified"""
    case = BLOCK_CAUSAL_CASES[idx]
    inp = bc_inputs(case, 5000 + idx)
    return inp, block_causal(inp.q, inp.k, inp.v, inp.seg_start, inp.key_end, case.block, case.scale)
