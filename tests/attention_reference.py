"""Plain float64 restatement of packed (document-masked) attention, forward and backward, the error budget the GPU test
holds the kernels to (csrc/attn_fwd_stream.hip, attn_bwd_dq_stream.hip, attn_bwd.hip, attn_bwd_fused.hip), and the
layouts and inputs both attention-reference tests share.  No GPU, no HIP: torch on the CPU only.

What is computed (q [B, T, Nh, D], k / v [B, T, Nkv, D], dO like q: the kernels' own bf16 inputs widened to float64;
doc [B, T] ids, 0 = pad; query head h reads kv head h // (Nh / Nkv)):
    allow(i, j) = doc[i] == doc[j] > 0   (causal: and j <= i)
    P = softmax over the allowed j of scale * q_i . k_j          O = P V
    lse2 = log2 sum_j exp2(scale * log2(e) * q_i . k_j)          +inf on a row without an allowed key, whose O is 0
    delta = rowsum(dO o O)    dP = dO V^T    dS = P o (dP - delta)
    dV = P^T dO    dK = scale * dS^T Q    dQ = scale * dS K      (dK, dV summed over the query heads of a kv head)
tests/test_attention_reference_cpu.py holds these values to torch autograd over an independently written masked softmax.

The budget.  Every function returns `Ref(value, slack)`; `budget` = half an ulp of the stored type at |value| + slack
(the output's own rounding, taken where an error may have carried the result) + slack + TINY.  `slack` is the sum of
the terms below, each a unit roundoff times the sum of the absolute values it acts on.  The constants:
    UBF  = 2^-8   round-to-nearest to bf16 (8 significant bits), relative, at its worst (1 + 2^-8 -> 1): `pack2bf` of the
                  forward's P, whose binade is not known (it carries the unknown lag 2^(max2 - m) of the running maximum).
                  2^-9, half of it, is what the rounding costs at the TOP of a binade only: an fp32 model of the kernels
                  with honest roundings exceeds a 2^-9 budget (1.10 x in dV of one_tile63, D = 64, causal).  Where the
                  rounded value itself is known — P and dS of the backward — the term is half a bf16 ulp AT that value,
                  `hulp(x)`, between 2^-9 |x| and 2^-8 |x|
    U32  = 2^-24  one round-to-nearest fp32 operation (fma, add, multiply)
    ULP32 = 2^-23 one term of an MFMA sum: v_mfma_f32_32x32x16_bf16 multiplies exactly and adds in fp32, and its adder is
                  not documented to round to nearest, so each accumulated term is given a whole ulp
    EXP  = 2^-23  v_exp_f32 (`fast_exp2`) and v_log_f32 / log2f: one ulp of the result
    DEFER = 8     the forward's deferred rescale (attn_fwd_stream.hip "threshold 8 in the log2 domain"): the running
                  reference maximum may lag the true one by up to 8, so the exponent's argument reaches +8
Where they enter, read off the kernels:
  logits   s = q . k accumulated over D terms in fp32: |error of scale * s| <= D ULP32 scale sum_d |q_d| |k_d|    (L)
  forward  p~ = exp2(fma(s, c, -m)): relative error of p~ (before its bf16 rounding)
               Ef = L + ln2 U32 (|a2 - max2| + DEFER) + EXP            (a2 = scale log2(e) s; the fma rounds once)
           O = sum bf16(p~) v / sum p~ (the row sum adds the UNROUNDED p~), n allowed keys, A = sum_j p_j |v_j|:
               slack(O) = UBF A + sum_j p_j Ef_j (|v_j| + |O|) + (n + 3) ULP32 (A + |O|)
           (n terms in the accumulator and in the row sum, the reciprocal, the product with it, one rescale product)
           lse2 = m + log2f(l):  slack = (sum_j p_j Ef_j + n ULP32) / ln2 + 2 EXP (DEFER + log2 n)
           (l~ = sum exp2(a2 - m) lies in [1, n 2^DEFER], so |log2f| <= DEFER + log2 n, held to two ulps)
  backward runs on the FORWARD KERNEL's o and lse2 (the production pairing), so their budgets b(O), b(lse2) enter:
           delta = sum_d dO O~ in fp32:  b(delta) = sum_d |dO| b(O) + D U32 sum_d |dO| (|O| + b(O))
           p^ = exp2(s c - lse2~): relative error  Eb = L + ln2 (U32 (|a2| + |a2 - lse2|) + b(lse2)) + EXP
           (product and difference may round separately)
           dV = sum_i bf16(p^) dO:  slack = sum_i (p Eb + hulp(p (1 + Eb))) |dO| + n_q ULP32 sum_i p |dO|
           dP = dO . v over D terms: b(dP) = D ULP32 sum_d |dO_d| |v_d|
           dS~ = bf16(p^ (dP~ - delta~)):  e = p (b(dP) + b(delta)) + |dS| (Eb + 3 U32);  b(dS) = e + hulp(|dS| + e)
           dQ = scale sum_j dS~ k:  slack = scale (sum_j b(dS) |k| + n ULP32 sum_j |dS| |k|) + U32 |dQ|
           dK = scale sum_i dS~ q:  the same with q for k and the n_q queries (of every head of the group) that see the key
There is no free multiplier: a kernel that exceeds a budget has a bug or rounds somewhere this list does not name."""
import functools
import math
from collections import namedtuple

import torch

F64 = torch.float64
BF = torch.bfloat16
UBF, U32, ULP32, EXP = 2.0 ** -8, 2.0 ** -24, 2.0 ** -23, 2.0 ** -23
DEFER = 8.0
TINY = 2.0 ** -126
LOG2E, LN2 = 1.4426950408889634, math.log(2.0)
_MANT = {torch.bfloat16: 8, torch.float32: 24, F64: 53}

Ref = namedtuple("Ref", ["value", "slack"])


def d(t):
    return t.detach().cpu().to(F64)


def ulp(x, dtype):
    """spacing of `dtype` at |x| (at least that of the smallest normal)"""
    _, e = torch.frexp(x.abs().clamp_min(TINY))
    return torch.ldexp(torch.ones_like(x), e - _MANT[dtype])


def budget(ref, dtype):
    fin = torch.isfinite(ref.value)
    val = torch.where(fin, ref.value, torch.zeros_like(ref.value))
    other = ref.slack + TINY
    return 0.5 * ulp(val.abs() + other, dtype) + other


def ratios(got, ref, dtype):
    """error / budget per element; an infinite reference (lse2 of a row without keys) asks for the same infinity"""
    g = d(got).reshape(ref.value.shape)
    fin = torch.isfinite(ref.value)
    err = torch.where(fin, g - torch.where(fin, ref.value, torch.zeros_like(g)), torch.zeros_like(g)).abs()
    r = err / budget(ref, dtype)
    r = torch.where(torch.isfinite(g) | ~fin, r, torch.full_like(r, math.inf))
    return torch.where(~fin & (g != ref.value), torch.full_like(r, math.inf), r)


def check(got, ref, what, dtype=BF):
    """Every element of `got` within the budget of `ref`; prints and returns the worst error as a multiple of the budget"""
    r = ratios(got, ref, dtype)
    worst = float(r.max()) if r.numel() else 0.0
    print(f"measured: {what} worst error = {worst:.3f} x budget")
    bad = ~(r <= 1.0)
    if bool(bad.any()):
        i = int(r.flatten().argmax())
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))
        g = d(got).reshape(ref.value.shape)
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} elements over budget; worst at {idx}: got {float(g.flatten()[i])!r}, "
            f"ref {float(ref.value.flatten()[i])!r}, budget {float(budget(ref, dtype).flatten()[i]):.4g}")
    return worst


def allow_mask(doc, causal):
    """bool [B, T(query), T(key)]"""
    dd = doc.long()
    a = (dd[:, :, None] == dd[:, None, :]) & (dd[:, :, None] > 0)
    if causal:
        T = dd.shape[1]
        a = a & torch.ones(T, T, dtype=torch.bool).tril()
    return a


def attention(q, k, v, do, doc, causal, scale, block=512):
    """-> dict(o, lse2, dq, dk, dv) of Refs; o / dq [B, T, Nh, D], dk / dv [B, T, Nkv, D], lse2 [B, Nh, T].  Evaluated
    `block` query rows at a time (a [B, Nh, block, T] score matrix is the largest thing alive)."""
    B, T, Nh, D = q.shape
    Nkv = k.shape[2]
    G = Nh // Nkv
    qh, doh = (d(t).transpose(1, 2) for t in (q, do))                              # [B, Nh, T, D]
    kh, vh = (d(t).transpose(1, 2).repeat_interleave(G, dim=1) for t in (k, v))    # [B, Nh, T, D]
    allow = allow_mask(doc, causal)
    O, sO, LSE, sLSE, dQ, sdQ = [], [], [], [], [], []
    dK, sdK, adK, dV, sdV, adV = (torch.zeros(B, Nh, T, D, dtype=F64) for _ in range(6))
    inf = torch.tensor(math.inf, dtype=F64)
    for r0 in range(0, T, block):
        r1 = min(r0 + block, T)
        al = allow[:, None, r0:r1, :]
        qb, dob = qh[:, :, r0:r1], doh[:, :, r0:r1]
        a = scale * (qb @ kh.transpose(-1, -2))
        a = torch.where(al, a, torch.zeros_like(a))                                # (finite everywhere: the mask is `al`)
        dead = ~al.any(-1, keepdim=True)
        mx = torch.where(al, a, -inf).amax(-1, keepdim=True)
        mx = torch.where(dead, torch.zeros_like(mx), mx)
        e = torch.where(al, torch.exp(a - mx), torch.zeros_like(a))
        l = e.sum(-1, keepdim=True)
        p = e / torch.where(dead, torch.ones_like(l), l)
        lse2 = (mx + torch.log(torch.where(dead, torch.ones_like(l), l))) * LOG2E
        n = al.sum(-1, keepdim=True).to(F64)
        o = p @ vh
        # ---- forward budget
        L = D * ULP32 * scale * (qb.abs() @ kh.abs().transpose(-1, -2))
        a2 = a * LOG2E
        Ef = L + LN2 * U32 * ((a2 - mx * LOG2E).abs() + DEFER) + EXP
        pE = p * Ef
        A = p @ vh.abs()
        so = UBF * A + pE @ vh.abs() + pE.sum(-1, keepdim=True) * o.abs() + (n + 3) * ULP32 * (A + o.abs())
        slse = (pE.sum(-1, keepdim=True) + n * ULP32) / LN2 + 2 * EXP * (DEFER + torch.log2(n.clamp_min(1.0)))
        slse = torch.where(dead, torch.zeros_like(slse), slse)
        O.append(o), sO.append(so), sLSE.append(slse[..., 0])
        LSE.append(torch.where(dead, inf, lse2)[..., 0])
        # ---- backward on the forward kernel's o / lse2
        bO = budget(Ref(o, so), BF)
        delta = (dob * o).sum(-1, keepdim=True)
        bdelta = (dob.abs() * bO).sum(-1, keepdim=True) + D * U32 * (dob.abs() * (o.abs() + bO)).sum(-1, keepdim=True)
        blse = torch.where(dead, torch.zeros_like(slse), budget(Ref(lse2, slse), torch.float32))
        Eb = L + LN2 * (U32 * (a2.abs() + (a2 - lse2).abs()) + blse) + EXP
        dP = dob @ vh.transpose(-1, -2)
        bdP = D * ULP32 * (dob.abs() @ vh.abs().transpose(-1, -2))
        dS = p * (dP - delta)
        edS = p * (bdP + bdelta) + dS.abs() * (Eb + 3 * U32)
        bdS = edS + torch.where(al, 0.5 * ulp(dS.abs() + edS, BF), torch.zeros_like(edS))
        dq = scale * (dS @ kh)
        dQ.append(dq)
        sdQ.append(scale * (bdS @ kh.abs() + n * ULP32 * (dS.abs() @ kh.abs())) + U32 * dq.abs())
        pt, dst = p.transpose(-1, -2), dS.transpose(-1, -2)
        dV += pt @ dob
        adV += pt @ dob.abs()
        bp = p * Eb + torch.where(al, 0.5 * ulp(p * (1 + Eb), BF), torch.zeros_like(p))
        sdV += bp.transpose(-1, -2) @ dob.abs()
        dK += scale * (dst @ qb)
        adK += scale * (dst.abs() @ qb.abs())
        sdK += scale * (bdS.transpose(-1, -2) @ qb.abs())
    group = lambda t: t.view(B, Nkv, G, T, D).sum(2).transpose(1, 2)               # -> [B, T, Nkv, D]
    nq = allow.sum(1).to(F64)[:, :, None, None] * G                                # queries that see key j, all heads
    dK, sdK, adK, dV, sdV, adV = (group(t) for t in (dK, sdK, adK, dV, sdV, adV))
    cat = lambda ts: torch.cat(ts, dim=2).transpose(1, 2)                          # row blocks -> [B, T, Nh, D]
    return dict(o=Ref(cat(O), cat(sO)), lse2=Ref(torch.cat(LSE, dim=2), torch.cat(sLSE, dim=2)),
                dq=Ref(cat(dQ), cat(sdQ)), dk=Ref(dK, sdK + nq * ULP32 * adK + U32 * dK.abs()),
                dv=Ref(dV, sdV + nq * ULP32 * adV))


# ================================================================================================ layouts
def _runs(*pairs):
    out = []
    for ident, n in pairs:
        out += [ident] * n
    return out


def layout(name):
    """document ids int32 [B, T].  Boundaries are placed against 32 (a wave's query rows), 64 (a KV tile) and 128 (a
    workgroup's rows)."""
    if name == "one_row":
        rows = [[1]]
    elif name.startswith("one_tile"):                         # one_tile63 / one_tile64 / one_tile65
        rows = [[1] * int(name[len("one_tile"):])]
    elif name == "one_over":                                  # the last workgroup has one row
        rows = [[1] * 129]
    elif name == "edges":                                     # boundaries at 31, 32, 33, 63, 64, 65, 127, 128, 129
        rows = [_runs((1, 31), (2, 1), (3, 1), (4, 30), (5, 1), (6, 1), (7, 62), (8, 1), (9, 1), (10, 191))]
    elif name == "pads":
        # pad at 0 | doc | pads 60..70 (across a tile edge) | doc | the whole tile 128..191 | doc | pads | a one-token
        # document at 255 between two pad runs | pads | doc | padded tail
        rows = [_runs((0, 1), (1, 59), (0, 11), (2, 57), (0, 64), (3, 58), (0, 5), (4, 1), (0, 4), (5, 90), (0, 34))]
    elif name == "revisit":                                   # id 1 recurs after a gap (test_kernels_gpu._meta_cases)
        rows = [_runs((3, 100), (1, 200), (0, 10), (2, 150), (1, 60), (0, 20))]
    elif name == "dead_row":                                  # batch row 1 is all pad
        rows = [[1] * 200, [0] * 200]
    elif name == "long_list":                                 # 68 KV tiles > kListPre = 64: the kernel lists them itself
        rows = [[1] * 4352]
    else:
        raise ValueError(name)
    return torch.tensor(rows, dtype=torch.int32)


SMALL_LAYOUTS = ("one_row", "one_tile63", "one_tile64", "one_tile65", "one_over", "edges", "pads", "revisit", "dead_row")
GEOMS = ((1, 1), (3, 3), (4, 1), (14, 2))

Case = namedtuple("Case", ["layout", "D", "causal", "kind", "Nh", "Nkv", "scale"])


def case_id(c):
    return f"{c.layout}-D{c.D}-{'causal' if c.causal else 'bidir'}-{c.kind}-{c.Nh}x{c.Nkv}-s{c.scale:.3g}"


def _cases():
    """Every small layout at both D and both directions with `planted` inputs and once more with `sharp` or `gauss`; the
    four head geometries rotate so that each layout meets all of them.  long_list: both D, causal, one head.  One more
    case per direction at a scale that is not D^-0.5."""
    out, n = [], 0
    for li, lay in enumerate(SMALL_LAYOUTS):
        for D in (64, 128):
            for causal in (True, False):
                nh, nkv = GEOMS[(li + n) % 4]
                out.append(Case(lay, D, causal, "planted", nh, nkv, D ** -0.5))
                nh, nkv = GEOMS[(li + n + 2) % 4]
                out.append(Case(lay, D, causal, ("sharp", "gauss")[(li + n) % 2], nh, nkv, D ** -0.5))
                n += 1
    out += [Case("long_list", 64, True, "planted", 1, 1, 64 ** -0.5), Case("long_list", 128, True, "sharp", 1, 1, 128 ** -0.5)]
    out += [Case("edges", 64, True, "planted", 4, 1, 0.2), Case("pads", 128, False, "planted", 3, 3, 0.2)]
    return tuple(out)


CASES = _cases()

# ================================================================================================ inputs
Plant = namedtuple("Plant", ["kind", "b", "h", "i", "j"])     # query row i of head h and key j of kv head h // G
Inputs = namedtuple("Inputs", ["q", "k", "v", "do", "doc", "anchors", "baits", "spikes"])

ANCHOR_LOGIT, BAIT_LOGIT, BAIT_V, PAD_DO = 8.0, 40.0, 32.0, 32.0


def _doc_runs(row):
    """maximal runs (start, end, id) of one batch row's ids"""
    out, s = [], 0
    for t in range(1, len(row) + 1):
        if t == len(row) or row[t] != row[s]:
            out.append((s, t, row[s]))
            s = t
    return out


def _plant(q, k, v, doc, causal, scale):
    """Overwrite keys (and their values) in place.  An ANCHOR is a key row i must see: k_j = alpha q_i with
    alpha = ANCHOR_LOGIT / (scale |q_i|^2), a logit about 8 above the gauss rest (whose logits have unit deviation), and
    v_j = a constant of magnitude 2..3.75 that no other anchor of the row shares: losing the key moves O_i by O(1).  A
    BAIT is a key row i must NOT see: would-be logit 40, v_j = +-32 — one leaked bait takes the row over.  All planted
    values are finite (0 x NaN would be NaN in the reference too).  Every planted key serves one (row, head) pair; rows are
    not reused while another allowed row is free, so anchors do not dilute each other.  -> (anchors, baits), lists of
    Plant, so that a test can aim a mutant at each."""
    B, T, Nh, D = q.shape
    Nkv = k.shape[2]
    G = Nh // Nkv
    allow = allow_mask(doc, causal)
    anchors, baits, used_keys, used_rows = [], [], set(), set()
    pos = torch.arange(T)

    def put(kind, b, i, j, logit, value, into):
        if (b, j) in used_keys or not (0 <= i < T and 0 <= j < T):
            return False
        hk = len(used_keys) % Nkv
        h = hk * G + (len(used_keys) // Nkv) % G
        qi = q[b, i, h].float()
        k[b, j, hk] = (qi * (logit / (scale * float(qi.square().sum())))).to(BF)
        v[b, j, hk] = torch.as_tensor(value, dtype=torch.float32).to(BF)
        used_keys.add((b, j))
        used_rows.add((b, i))
        into.append(Plant(kind, b, h, i, j))
        return True

    def anchor(kind, b, rows, j):
        """on the first of `rows` that is QUIET: no key it may see has a logit within 3.5 of the anchor's yet (a bait key is
        seen rightfully by its own document, with logits of deviation 40 / sqrt D there, and would outweigh the anchor)"""
        if (b, j) in used_keys:
            return
        hk = len(used_keys) % Nkv
        h = hk * G + (len(used_keys) // Nkv) % G
        for i in rows:
            assert bool(allow[b, i, j]), (kind, b, i, j)
            a = (scale * (k[b, :, hk].float() @ q[b, i, h].float()))[allow[b, i] & (pos != j)]   # (key j is overwritten)
            if a.numel() == 0 or float(a.max()) <= ANCHOR_LOGIT - 3.5:
                idx = len(anchors)
                put(kind, b, i, j, ANCHOR_LOGIT, (2.0 + 0.25 * (idx % 8)) * (-1.0) ** idx, anchors)
                return

    def bait(kind, b, i, j):
        assert not bool(allow[b, i, j]), (kind, b, i, j)
        # +-32 per element, the signs drawn per bait: a row whose honest output is already near one bait's value (it may
        # see that key rightfully) still moves by 64 in half of its elements when another bait leaks
        signs = torch.randint(0, 2, (D,), generator=torch.Generator().manual_seed(len(baits))) * 2.0 - 1.0
        return put(kind, b, i, j, BAIT_LOGIT, BAIT_V * signs, baits)

    def free_rows(b, j):
        """the rows other than j that may see key j, last first, those not yet used in front"""
        rows = [i for i in torch.nonzero(allow[b, :, j]).flatten().tolist()[::-1] if i != j]
        return [i for i in rows if (b, i) not in used_rows] + [i for i in rows if (b, i) in used_rows]

    for b in range(B):
        row = doc[b].tolist()
        runs = _doc_runs(row)
        docs = [r for r in runs if r[2] > 0]
        first_of_id = {}
        for s, e, ident in docs:
            first_of_id.setdefault(ident, s)
        # ---- one-token documents first (their only key), then the baits (they want particular neighbours); the other
        # anchors take what is left
        for s, e, ident in docs:
            if e - s == 1 and first_of_id[ident] == s:
                anchor("single", b, [s], s)
        for s, e, ident in runs:
            if ident == 0:
                nxt = [r for r in docs if r[0] >= e]
                prv = [r for r in docs if r[1] <= s]
                if nxt:
                    bait("pad_key", b, nxt[0][0], e - 1)                # the pad just below the next document's first row
                    bait("pad_key", b, min(nxt[0][0] + 33, nxt[0][1] - 1), s)
                elif prv:
                    bait("pad_key", b, prv[-1][1] - 1, s)
                continue
            before = [r for r in docs if r[1] <= s and r[2] != ident]
            after = [r for r in docs if r[0] >= e and r[2] != ident]
            # (the nearest such document whose key is still free: a one-token neighbour's only key is an anchor)
            any(bait("prev_doc_last", b, s, r[1] - 1) for r in before[::-1])
            if not causal:
                any(bait("next_doc_first", b, e - 1, r[0]) for r in after)
        for s, e, ident in docs:
            if causal and e - s >= 2:
                if not bait("causal_next", b, e - 2, e - 1) and e - s >= 3:      # (the last key may be taken)
                    bait("causal_next", b, e - 3, e - 2)
                if e - s >= 70:
                    bait("causal_next", b, s + (63 - s) % 64, s + (63 - s) % 64 + 1)   # i ends a tile, j opens the next
        for s, e, ident in docs:                                    # a key of another id inside a tile the row reads
            for s2, e2, id2 in docs:
                if id2 != ident and s2 // 64 == (e - 1) // 64 and s2 >= e and e2 - s2 >= 2:
                    # row i of document id2 reads the tile for its own keys; key j, the last free one of `ident` there
                    if any(bait("other_id_same_tile", b, e2 - 1, j) for j in range(e - 1, max(s, (e - 1) // 64 * 64) - 1, -1)):
                        break
        # ---- anchors
        for s, e, ident in docs:
            if e - s > 1:
                anchor("doc_first", b, free_rows(b, first_of_id[ident]), first_of_id[ident])
        for t in range((T + 63) // 64):
            for kind, j in (("tile_first", 64 * t), ("tile_last", min(64 * t + 63, T - 1))):
                if row[j] > 0:
                    anchor(kind, b, free_rows(b, j), j)
        for s, e, ident in docs:
            for i in {e - 1, s + (e - s) // 2, s + (127 - s) % 128 if s + (127 - s) % 128 < e else e - 1}:
                anchor("diagonal", b, [i], i)
    return anchors, baits


def _spike(q, k, doc, sd):
    """test_packed_attention_online_softmax_rescale's row, per document of >= 130 positions: a quiet query row (deviation
    0.3 where the others have `sd`) with a key two tiles back that is 8 x the row — a logit of 0.72 scale D, some 3 to 6
    in the log2 domain above the row's other logits (deviation 0.3 sd): growth below 2^DEFER, the deferred path — and a
    key one tile back that is 40 x the row: a jump of 30 and more, the rescale branch."""
    out = []
    G = q.shape[2] // k.shape[2]
    for b in range(doc.shape[0]):
        for s, e, ident in _doc_runs(doc[b].tolist()):
            if ident > 0 and e - s >= 130:
                i, jm, js = e - 1, e - 1 - 128, e - 1 - 64
                q[b, i] = (q[b, i].float() * (0.3 / sd)).to(BF)
                k[b, jm] = (q[b, i, ::G].float() * 8).to(BF)
                k[b, js] = (q[b, i, ::G].float() * 40).to(BF)
                out.append(Plant("spike", b, 0, i, js))
    return out


def make_inputs(case, seed):
    """bf16 q, k, v, dO (CPU) of `case` and what was planted.  gauss: randn.  sharp: q and k of deviation
    (16 / (scale sqrt D))^0.5 — logits of deviation 16, a nearly one-hot softmax — plus `_spike`.  planted: gauss + `_plant`;
    pad query rows carry dO = 32, which dK / dV must not feel."""
    doc = layout(case.layout)
    B, T = doc.shape
    g = torch.Generator().manual_seed(seed)
    q, do = (torch.randn(B, T, case.Nh, case.D, generator=g) for _ in range(2))
    k, v = (torch.randn(B, T, case.Nkv, case.D, generator=g) for _ in range(2))
    anchors, baits, spikes = [], [], []
    if case.kind == "sharp":
        sd = math.sqrt(16.0 / (case.scale * math.sqrt(case.D)))
        q, k = q * sd, k * sd
    q, k, v, do = (t.to(BF) for t in (q, k, v, do))
    if case.kind == "sharp":
        spikes = _spike(q, k, doc, sd)
    if case.kind == "planted":
        anchors, baits = _plant(q, k, v, doc, case.causal, case.scale)
        do[doc == 0] = PAD_DO
    return Inputs(q, k, v, do, doc, anchors, baits, spikes)


@functools.lru_cache(maxsize=None)
def problem(idx):
    """(inputs, reference) of CASES[idx]: built once, shared by every test that needs it, never modified"""
    case = CASES[idx]
    inp = make_inputs(case, 1000 + idx)
    return inp, attention(inp.q, inp.k, inp.v, inp.do, inp.doc, case.causal, case.scale)
