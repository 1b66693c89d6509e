"""Exact-integer reference for the bf16 MFMA GEMM entry points (csrc/gemm_kernel.h, gemm.hip, gemm_table.hip).

A bf16 GEMM with fp32 accumulation is EXACT when its operands are small integers: every product and every partial sum
is an integer below 2^24, so the summation order, the split, the stage ring and the MFMA shape cannot change a bit of
the result.  This module builds such problems, states what every entry point has to return for them — bit for bit, no
tolerance anywhere — and lists the cases tests/test_gemm_edges_gpu.py runs on the device.  No GPU and no touchnet_amd
import here: tests/test_gemm_reference_cpu.py checks on the CPU that the reference is right (float64 == int64), that
the data keep the condition below, and that a model of the kernel's structure (`emulate`) reproduces the expected bits
while each of ten one-term / one-stage / one-tile mistakes does not.

Two data regimes, both from a seeded CPU generator (random, hence asymmetric: a swapped operand or a transposed tile
cannot pass):
  S   operands, bias, the accumulate target C0 and the addend uniform in {-1, 0, 1}.  CONDITION (asserted in `build`
      from the reference alone): every expected value is an integer with |value| <= 256, i.e. a bf16 number — one lost,
      doubled or misplaced term changes the expected bits.  A case that breaks it is repaired by thinning operand A
      (zeroing a seeded share of it), never by relaxing the condition.
  WA / WB   operand A (B) uniform integers in [-255, 255] — all eight significand bits in use — the other one in
      {-1, 0, 1}.  fp32 outputs equal the exact integer; bf16 outputs equal bf16(exact + bias), one round-to-nearest-even
      from float64 (integers below 2^24 survive double -> float), and with accumulate / addend
      bf16(bf16(exact + bias) + c0): the two roundings gemm_kernel.h documents for those epilogues.
Reference: torch.matmul in float64 of the operands as stored (with integer inputs any correct float64 product is exact).

Guards: every operand is a view with a row pitch above its row length inside a buffer whose other elements are NaN;
every output is a view (16-byte aligned start, pitch above its width) inside a buffer of a fixed sentinel bit pattern
that must come back unchanged; without accumulate the output region itself starts as the sentinel."""
import dataclasses
import functools
import zlib

import torch

BM = BN = 256
STAGE = 64
NCU = 256                                   # CUs of an MI355X: what the (D) cases' tile counts are chosen against
SENT16 = 0x7FC1                             # sentinel bit patterns (NaNs with a payload): compared as integers
SENT32 = 0x7FC00ACE
MODES = {"fwd": (False, False), "dgrad": (False, True), "wgrad": (True, True)}      # (a_kmaj, b_kmaj)


@dataclasses.dataclass(frozen=True)
class Case:
    group: str                  # plain seg out_t addend wgrad_out splitk persist tail grouped table overlap + the fused ones
    mode: str                   # fwd: A [M, K] B [N, K]; dgrad: A [M, K] B [K, N]; wgrad: A [K, M] B [K, N]
    M: int
    N: int
    Ks: tuple                   # depth of every segment
    regime: str = "S"
    bias: bool = False
    accumulate: bool = False
    out_t: bool = False
    addend: bool = False
    f32: bool = False
    bias_grad: bool = False
    entry: str = "gemm"         # gemm (functional.gemm) | splitk | wgrad_f32 | wgrad_bias (the C ABI)
    parts: int = 1
    tail: bool = False          # tail_only = 1
    persist: bool = True        # False: TN_GEMM_PERSIST=0
    device_ref: bool = False    # (D): the float64 reference product is formed on the device
    overlap: int = 0            # pitch of the overlapping-row operand (ld < K): A of fwd, B of wgrad
    products: tuple = ()        # grouped / table launches: ((M, N, K), ...)
    heads: int = 0              # gemm_rope: N = heads * head_dim
    head_dim: int = 0
    index: int = 0              # which product of a grouped / table launch this is (its data differ from its twins')


def case_id(c):
    if c.products:
        shape = "+".join("x".join(map(str, p)) for p in c.products[:3]) + ("+.." if len(c.products) > 3 else "")
    else:
        shape = f"{c.M}x{c.N}x" + "+".join(map(str, c.Ks))
    opts = [n for n in ("bias", "accumulate", "out_t", "addend", "f32", "bias_grad", "tail") if getattr(c, n)]
    if c.parts > 1:
        opts.append(f"{c.parts}parts")
    if c.entry != "gemm":
        opts.append(c.entry)
    if not c.persist:
        opts.append("per_tile")
    if c.overlap:
        opts.append(f"ld{c.overlap}")
    if c.heads:
        opts.append(f"{c.heads}heads{c.head_dim}")
    return "-".join([c.group, c.mode, shape, c.regime] + opts)


class Op:
    """a 2-D operand as stored: a view [rows, cols] of pitch `pitch` at element `offset` of a flat buffer"""

    def __init__(self, buf, offset, shape, pitch):
        self.buf, self.offset, self.shape, self.pitch = buf, offset, tuple(shape), pitch

    def view(self, device=None):
        buf = self.buf if device is None else self.buf.to(device)
        return buf.as_strided(self.shape, (self.pitch, 1), self.offset)


def _padded(x, extra, dtype=torch.bfloat16):
    """x [rows, cols] as a view of pitch > cols (a multiple of 8), 16-byte aligned start, everything around it NaN"""
    rows, cols = x.shape
    pitch = (cols + 7) // 8 * 8 + 8 * extra
    buf = torch.full((8 + (rows + 1) * pitch,), float("nan"), dtype=dtype)
    op = Op(buf, 8, (rows, cols), pitch)
    op.view().copy_(x)
    return op


def _ints(g, shape, hi):
    return torch.randint(-hi, hi + 1, shape, generator=g).double()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _logical(view, kmaj):
    """the operand as [rows, K], whatever its storage"""
    return view.t() if kmaj else view


class Problem:
    """operands (Op), bias [N], c0 [M, N] (accumulate target), addend (Op), exact [M, N] float64 (on `dev`)"""

    def expected(self, case):
        """the bits the entry point has to leave in C for `case`'s options"""
        e = self.exact + (self.bias.double().to(self.exact.device) if case.bias else 0)
        c0 = self.c0.to(self.exact.device)
        if case.f32:
            out = e.float()
            return out + c0.float() if case.accumulate else out
        out = e.float().to(torch.bfloat16)
        if case.accumulate:
            out = (out.float() + c0.float()).to(torch.bfloat16)
        if case.addend:
            out = (out.float() + self.add.view().float().to(out.device)).to(torch.bfloat16)
        return out

    def expected_bias_grad(self):
        return self.colsum.float().to(torch.bfloat16)


def _s_violations(*vals):
    """elements that are not integers of magnitude <= 256 (exactly representable in bf16)"""
    return sum(int(((v != v.round()) | (v.abs() > 256)).sum()) for v in vals)


def assemble(case, a_mats, b_mats, bias, c0, add, dev="cpu"):
    """a Problem from the operands AS STORED (one matrix per segment; mode's layout), any values"""
    ak, bk = MODES[case.mode]
    p = Problem()
    p.case = case
    p.unrepresentable = 0
    p.A = [m if isinstance(m, Op) else _padded(m, 1 + s) for s, m in enumerate(a_mats)]
    p.B = [m if isinstance(m, Op) else _padded(m, 2 + s) for s, m in enumerate(b_mats)]
    p.bias = bias.to(torch.bfloat16)
    p.c0 = c0.to(torch.bfloat16)
    p.add = _padded(add, 3)
    exact = 0
    for a, b in zip(p.A, p.B):
        exact = exact + torch.matmul(_logical(a.view(dev).double(), ak), _logical(b.view(dev).double(), bk).t())
    p.exact = exact
    p.colsum = sum(_logical(a.view().double(), ak).sum(1) for a in p.A)
    return p


def _overlapping(g, rows, ld, K):
    """rows of length K that begin `ld` < K apart in ONE flat integer sequence (the im2col view of a k = 3 convolution);
    behind the last row's start every element is non-zero"""
    n = (rows - 1) * ld + K
    flat = _ints(g, (n,), 1)
    tail = flat[(rows - 1) * ld:]
    tail[tail == 0] = 1.0
    buf = flat.to(torch.bfloat16)
    return Op(buf, 0, (rows, K), ld)


def _data_key(case):
    return dataclasses.replace(case, group="", bias=False, accumulate=False, out_t=False, addend=False, f32=False,
                               bias_grad=False, entry="gemm", parts=1, tail=False, persist=True, device_ref=False)


@functools.lru_cache(maxsize=6)
def _build(key, dev):
    case = key
    ak, bk = MODES[case.mode]
    M, N = case.M, case.N
    for thin in (0.0, 0.5, 0.75, 0.9):
        g = torch.Generator().manual_seed(_seed(key, thin))
        a_hi, b_hi = (255 if case.regime == "WA" else 1), (255 if case.regime == "WB" else 1)
        a_mats, b_mats = [], []
        for K in case.Ks:
            a = _ints(g, (K, M) if ak else (M, K), a_hi)
            b = _ints(g, (K, N) if bk else (N, K), b_hi)
            if thin:
                a = a * (torch.rand(a.shape, generator=g) >= thin)
            if case.overlap and case.mode == "fwd":
                a = _overlapping(g, M, case.overlap, K)
            elif case.overlap:
                b = _overlapping(g, K, case.overlap, N)
            a_mats.append(a)
            b_mats.append(b)
        bias, c0, add = _ints(g, (N,), 1), _ints(g, (M, N), 1), _ints(g, (M, N), 1)
        p = assemble(case, a_mats, b_mats, bias, c0, add, dev)
        if case.regime != "S":
            break
        eb = p.exact + bias.to(p.exact.device)
        p.unrepresentable = _s_violations(p.exact, eb, eb + c0.to(eb.device), eb + add.to(eb.device), p.colsum)
        if p.unrepresentable == 0:
            break
    # THE regime S condition: on the inputs (through the float64 reference), never on what a kernel returned
    assert case.regime != "S" or p.unrepresentable == 0, f"{case_id(case)}: regime S condition broken"
    return p


def build(case, dev="cpu"):
    """the Problem of `case` (cached: cases that differ in options and entry point only share their data)"""
    return _build(_data_key(case), dev)


def sentinel_buffer(M, N, dtype, pitch_mult=8):
    """(buffer [M + 2, pitch] of the sentinel bit pattern, row0, col0): the output is buffer[row0:row0 + M, col0:col0 + N]
    — pitch above N (a multiple of `pitch_mult` elements), 16-byte aligned start"""
    col0 = 8 if dtype == torch.bfloat16 else 4
    pitch = N + (12 if pitch_mult == 4 else 2 * col0)
    assert pitch % pitch_mult == 0 and pitch >= N + col0 and (pitch_mult != 4 or pitch % 8)
    ints = torch.int16 if dtype == torch.bfloat16 else torch.int32
    buf = torch.full((M + 2, pitch), SENT16 if dtype == torch.bfloat16 else SENT32, dtype=ints).view(dtype)
    return buf, 1, col0


# ---- the tile walk, restated from the comments of gemm_kernel.h -----------------------------------------------------------
def xcd_chunk(bid, total):
    """workgroups are dealt to the 8 XCDs round-robin: unit `bid` gets position bid >> 3 of XCD bid & 7's own contiguous
    eighth of the list"""
    xcd, local = bid & 7, bid >> 3
    q, r = total >> 3, total & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + local


def panel_group(vid, nbm, nbn):
    """a position inside a product -> its tile: 8-tall column-major groups, the last group possibly short"""
    per_group = 8 * nbn
    g, w = divmod(vid, per_group)
    gm = min(8, nbm - g * 8)
    return g * 8 + w % gm, w // gm


def tile_of_block(bid, nbm, nbn):
    return panel_group(xcd_chunk(bid, nbm * nbn), nbm, nbn)


def grouped_split(total, min_stages, ncu=NCU):
    """(parts, r): the grouped launch's last partial round of r tiles runs split in `parts` (1 = whole tiles)"""
    r = total % ncu
    if total <= ncu or r == 0 or r * 2 > ncu or min_stages < 16:
        return 1, r
    return min(ncu // r, min_stages // 8), r


def _units(units, ncu, persist):
    """(workgroup, unit) pairs of a launch: persistent = one workgroup per CU walks units b, b + G, ..."""
    G = ncu if persist and units > ncu else units
    for bid in range(G):
        for u in range(bid, units, G):
            yield bid, u


# ---- a plain-torch fp32 model of the kernel's structure: it carries the mutants, it never runs on the GPU -------------------
MUTANTS = {
    "a": "one whole stage skipped in tiles whose stage count is a multiple of 5",
    "b": "the contraction tail K % 64 of a contraction-major pair not zero-filled: the next row is read",
    "c": "the last contraction row k = K - 1 dropped",
    "d": "two 8-deep contraction slots swapped in B only",
    "e": "bias applied shifted by 4 columns in the last, ragged, 8-column group",
    "f": "one tile of a persistent walk visited twice under accumulate",
    "g": "the first stage of split part 1 also counted in part 0",
    "h": "the transposed copy taken from the other 64-row half of a wave's park",
    "i": "one term of magnitude 1 dropped in one single output element",
    "j": "the tail of an overlapping row read as zeros",
}


def _pad_operand(op, kmaj, rows_to, mutant):
    """fp32 [rows_to, stages * 64]: zero fill beyond the operand's rows and beyond K"""
    x = _logical(op.view().float(), kmaj)
    R, K = x.shape
    out = torch.zeros(rows_to, (K + STAGE - 1) // STAGE * STAGE)
    out[:R, :K] = x
    if mutant == "b" and kmaj and K % STAGE:
        # rows k >= K of the stage come from memory: whatever follows the operand in its buffer (its NaN padding)
        for k in range(K, out.shape[1]):
            lo = op.offset + k * op.pitch
            row = op.buf[lo:lo + R].float()
            out[:R, k] = float("nan")
            out[:row.numel(), k] = row
    if mutant == "c":
        out[:, K - 1] = 0
    if mutant == "j" and not kmaj and op.pitch < K:
        # the descriptor ends (R - 1) * pitch + pitch elements behind the first row: what lies behind reads as zeros
        for r in range(R):
            keep = max(0, min(K, R * op.pitch - r * op.pitch))
            out[r, keep:K] = 0
    return out


class _Prod:
    """one product inside the model: padded fp32 operands per segment, the output it fills, who visited which tile"""

    def __init__(self, p, case, mutant):
        ak, bk = MODES[case.mode]
        self.M, self.N = p.exact.shape
        self.nbm, self.nbn = -(-self.M // BM), -(-self.N // BN)
        self.A = [_pad_operand(a, ak, self.nbm * BM, mutant) for a in p.A]
        self.B = [_pad_operand(b, bk, self.nbn * BN, mutant if mutant == "b" else None) for b in p.B]
        self.stages = sum(a.shape[1] // STAGE for a in self.A)
        self.bias = torch.zeros(self.nbn * BN)
        if case.bias:
            self.bias[:self.N] = p.bias.float()
        self.other = p.add.view().float() if case.addend else p.c0.float() if case.accumulate else None
        dtype = torch.float32 if case.f32 else torch.bfloat16
        self.C = self.other.to(dtype).clone() if case.accumulate else torch.full((self.M, self.N), float("nan"), dtype=dtype)
        self.Ct = torch.full((self.N, self.M), float("nan"), dtype=torch.bfloat16) if case.out_t else None
        self.bg = torch.full((self.M,), float("nan"), dtype=torch.bfloat16) if case.bias_grad else None
        self.visits = {}
        self.case, self.mutant = case, mutant

    def acc(self, tm, tn, lo, hi):
        """the fp32 accumulators of tile (tm, tn) over the stages [lo, hi) of the concatenated segments"""
        acc = torch.zeros(BM, BN)
        t = 0
        for A, B in zip(self.A, self.B):
            for s in range(A.shape[1] // STAGE):
                if lo <= t < hi and not (self.mutant == "a" and self.stages % 5 == 0 and t == 2):
                    a = A[tm * BM:(tm + 1) * BM, s * STAGE:(s + 1) * STAGE]
                    b = B[tn * BN:(tn + 1) * BN, s * STAGE:(s + 1) * STAGE]
                    if self.mutant == "d":
                        b = torch.cat([b[:, 8:16], b[:, :8], b[:, 16:]], 1)
                    acc += a @ b.t()
                t += 1
        if self.mutant == "i" and tm == tn == 0 and lo == 0:
            terms = self.A[0][:min(self.M, BM), :STAGE] * self.B[0][0, :STAGE]
            m, k = (terms != 0).nonzero()[0].tolist()               # the first non-zero term of column 0 (regime S: +-1)
            acc[m, 0] -= terms[m, k]
        return acc

    def colsum(self, tm, lo, hi):
        cols = torch.cat(self.A, 1)[tm * BM:(tm + 1) * BM, lo * STAGE:hi * STAGE]
        return cols.sum(1)

    def visit(self, tm, tn, part=0):
        self.visits[(tm, tn, part)] = self.visits.get((tm, tn, part), 0) + 1

    def store(self, tm, tn, acc, bsum=None, reduce=False):
        """the epilogue: + bias, to bf16, then accumulate / addend (the split-K reduce kernel rounds once)"""
        case = self.case
        m0, n0 = tm * BM, tn * BN
        m1, n1 = min(self.M, m0 + BM), min(self.N, n0 + BN)
        bias = self.bias[n0:n0 + BN].clone()
        if self.mutant == "e" and self.N % BN and n1 == self.N:
            g0 = self.N - 8 - n0
            bias[g0:g0 + 8] = self.bias[[min(n + 4, self.N - 1) for n in range(self.N - 8, self.N)]]
        other = self.C[m0:m1, n0:n1].float() if case.accumulate else self.other[m0:m1, n0:n1] if case.addend else None
        v = acc + bias
        if case.f32:
            self.C[m0:m1, n0:n1] = v[:m1 - m0, :n1 - n0] + (other if other is not None else 0)
        elif reduce:
            self.C[m0:m1, n0:n1] = (v[:m1 - m0, :n1 - n0] + (other if other is not None else 0)).to(torch.bfloat16)
        else:
            v = v.to(torch.bfloat16)
            if self.Ct is not None:
                src = v[[m ^ 64 for m in range(BM)]] if self.mutant == "h" else v
                self.Ct[n0:n1, m0:m1] = src[:m1 - m0, :n1 - n0].t()
            out = v[:m1 - m0, :n1 - n0]
            if other is not None:
                out = (out.float() + other).to(torch.bfloat16)
            self.C[m0:m1, n0:n1] = out
        if bsum is not None and tn == 0:
            self.bg[m0:m1] = bsum[:m1 - m0].to(torch.bfloat16)


def _launch(prod, ncu, persist, tile0, ntiles, parts, with_bg=True):
    """one launch over the tiles [tile0, tile0 + ntiles) of one product, `parts` split-K parts"""
    kchunk = -(-prod.stages // parts)
    ws, bws = {}, {}
    for bid, u in _units(ntiles * parts, ncu, persist):
        part, t = divmod(u, ntiles)
        if prod.mutant == "f" and persist and u == ncu:
            part, t = 0, 0                        # workgroup 0 goes to its first tile again instead of to its second
        tm, tn = tile_of_block(t + tile0, prod.nbm, prod.nbn)
        prod.visit(tm, tn, part)
        lo, hi = (0, prod.stages) if parts == 1 else (part * kchunk, min((part + 1) * kchunk, prod.stages))
        if prod.mutant == "g" and parts > 1 and part == 0:
            hi = min(hi + 1, prod.stages)
        acc = prod.acc(tm, tn, lo, hi)
        bsum = prod.colsum(tm, lo, hi) if prod.bg is not None and with_bg else None
        if parts == 1:
            prod.store(tm, tn, acc, bsum)
        else:
            ws[(tm, tn)] = ws.get((tm, tn), 0) + acc
            if bsum is not None:
                bws[tm] = bws.get(tm, 0) + bsum if tn == 0 else bws.get(tm, 0)
    for (tm, tn), acc in ws.items():
        prod.store(tm, tn, acc, bws.get(tm) if prod.bg is not None else None, reduce=True)


def _sub_case(case, i):
    M, N, K = case.products[i]
    return dataclasses.replace(case, M=M, N=N, Ks=(K,), products=(), index=i)


def emulate(case, mutant=None, ncu=NCU, problem=None):
    """what the kernel's structure — 256 x 256 tiles, 64-deep stages, zero fill beyond M, N and K, split parts of `kchunk`
    stages, the tile-to-workgroup walk, the epilogue order bias -> bf16 -> accumulate — makes of `case`; `mutant`: one of
    MUTANTS.  Returns a list (one entry per product) of dicts C, Ct, bias_grad, visits."""
    if case.products:
        prods = [_Prod(p, s, mutant) for s, p in sub_problems(case)]
        starts, total = [], 0
        for pr in prods:
            starts.append(total)
            total += pr.nbm * pr.nbn
        which = lambda v: max(g for g, s in enumerate(starts) if s <= v)
        if case.group == "table":
            for bid, u in _units(total, ncu, case.persist):
                v = xcd_chunk(u, total)
                g = which(v)
                pr = prods[g]
                tm, tn = panel_group(v - starts[g], pr.nbm, pr.nbn)
                pr.visit(tm, tn)
                pr.store(tm, tn, pr.acc(tm, tn, 0, pr.stages), pr.colsum(tm, 0, pr.stages) if pr.bg is not None else None)
        else:
            S, r = grouped_split(total, min(pr.stages for pr in prods), ncu)
            main = total - r if S > 1 else total
            for bid, u in _units(main, ncu, case.persist):
                g = which(u)
                pr = prods[g]
                tm, tn = tile_of_block(u - starts[g], pr.nbm, pr.nbn)
                pr.visit(tm, tn)
                pr.store(tm, tn, pr.acc(tm, tn, 0, pr.stages))
            if S > 1:
                for g, pr in enumerate(prods):
                    lo, hi = max(main, starts[g]), starts[g] + pr.nbm * pr.nbn
                    if lo < hi:
                        _launch(pr, ncu, case.persist, lo - starts[g], hi - lo, S)
    else:
        pr = _Prod(problem if problem is not None else build(case), case, mutant)
        prods = [pr]
        tiles = pr.nbm * pr.nbn
        main = tiles // ncu * ncu if case.tail else 0
        if main:
            _launch(pr, ncu, True, 0, main, 1)                       # whole rounds first, unsplit, one workgroup per CU
        _launch(pr, ncu, case.persist, main, tiles - main, case.parts)
    return [dict(C=pr.C, Ct=pr.Ct, bias_grad=pr.bg, visits=pr.visits) for pr in prods]


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _plain_cases():
    out = []
    mns = [(1, 8), (7, 8), (8, 72), (33, 136), (129, 264), (248, 256), (256, 8), (264, 264)]
    opts = [dict(), dict(bias=True), dict(bias=True, accumulate=True)]
    for mode in MODES:
        w = mode == "wgrad"
        shapes = []
        for K in ([1, 7, 8, 63, 64, 65, 127, 129, 321, 449] if w else [64, 128, 192, 256, 320, 384, 448, 704]):
            shapes.append((136 if w else 129, 264, K))
        for M, N in mns:
            shapes.append(((M + 7) // 8 * 8 if w else M, N, 321 if w else 320))
        for M, N, K in dict.fromkeys(shapes):
            for o in opts:
                out.append(Case("plain", mode, M, N, (K,), **o))
        for regime in ("WA", "WB"):                                  # the starred case: one per kernel instantiation
            for o in opts:
                out.append(Case("plain", mode, 136 if w else 129, 264, (321 if w else 320,), regime, **o))
    return out


def _segment_cases():
    out = []
    for mode, depths in (("fwd", [(64, 64, 64), (64, 320, 128), (192, 64)]), ("dgrad", [(64, 64, 64), (64, 320, 128), (192, 64)]),
                         ("wgrad", [(1, 65, 130), (64, 63)])):
        for Ks in depths:
            out += [Case("seg", mode, 264, 136, Ks), Case("seg", mode, 264, 136, Ks, bias=True, accumulate=True)]
    return out


def _out_t_cases():
    return [Case("out_t", mode, M, N, (K,), bias=bias, out_t=True) for mode in MODES
            for M, N, K in [(8, 8, 64), (264, 72, 192), (520, 264, 320)] for bias in (False, True)]


def _addend_cases():
    return [Case("addend", mode, M, N, (K,), bias=bias, addend=True) for mode in ("fwd", "dgrad")
            for M, N, K in [(7, 8, 64), (264, 136, 320)] for bias in (False, True)]


_WGRAD_ENTRIES = [dict(entry="wgrad_f32", f32=True), dict(entry="wgrad_bias", bias_grad=True),
                  dict(entry="wgrad_bias", bias_grad=True, f32=True)]


def _wgrad_out_cases():
    out = []
    for M, N, K in [(8, 8, 1), (264, 72, 65), (520, 264, 321)]:
        for e in _WGRAD_ENTRIES:
            for acc in (False, True):
                out.append(Case("wgrad_out", "wgrad", M, N, (K,), accumulate=acc, **e))
    for regime in ("WA", "WB"):
        for e in _WGRAD_ENTRIES:
            for acc in (False, True):
                out.append(Case("wgrad_out", "wgrad", 264, 72, (65,), regime, accumulate=acc, **e))
    return out


def _splitk_cases():
    out = []
    for M, N, K, parts in [(8, 8, 1, 2), (264, 72, 65, 2), (264, 72, 129, 3), (256, 256, 321, 4), (520, 264, 1000, 5)]:
        out += [Case("splitk", "wgrad", M, N, (K,), entry="splitk", parts=parts),
                Case("splitk", "wgrad", M, N, (K,), entry="splitk", parts=parts, bias=True, accumulate=True)]
        for e in _WGRAD_ENTRIES:
            for acc in (False, True):
                out.append(Case("splitk", "wgrad", M, N, (K,), parts=parts, accumulate=acc, **e))
    for mode in ("fwd", "dgrad"):
        for M, N, K, parts in [(7, 8, 128, 2), (264, 264, 384, 3), (300, 264, 640, 5)]:
            out += [Case("splitk", mode, M, N, (K,), entry="splitk", parts=parts),
                    Case("splitk", mode, M, N, (K,), entry="splitk", parts=parts, bias=True, accumulate=True)]
    return out


def _persist_cases():
    shapes = [(mode, 4104, 4104, K) for K in (64, 128) for mode in MODES]            # 17 x 17 = 289 tiles
    shapes += [("fwd", 5640, 5640, 64), ("wgrad", 5640, 5640, 1), ("wgrad", 5640, 5640, 65)]   # 23 x 23 = 529: three per workgroup
    shapes += [("fwd", 16392, 776, 64), ("wgrad", 16392, 776, 64)]                   # 65 x 4: panel_group's short last group
    return [Case("persist", mode, M, N, (K,), accumulate=acc, persist=persist, device_ref=True)
            for mode, M, N, K in shapes for acc in (False, True) for persist in (True, False)]


def _tail_cases():
    return [Case("tail", mode, 4104, 4104, (K,), entry="splitk", parts=2, tail=True, device_ref=True, **o)
            for mode, K in (("wgrad", 130), ("fwd", 128)) for o in (dict(), dict(bias=True, accumulate=True))]


def _grouped_cases():
    small = ((8, 8, 1), (264, 72, 65), (256, 520, 64))
    out = [Case("grouped", "wgrad", 0, 0, (), f32=f32, accumulate=acc, products=small) for f32 in (False, True)
           for acc in (False, True)]
    # (D) 3 x (11 x 10) = 330 tiles = one round + 74, which run split in 2 parts
    out += [Case("grouped", "wgrad", 0, 0, (), f32=f32, products=((2568, 2560, 1000),) * 3, device_ref=True) for f32 in (False, True)]
    return out


def _table_cases():
    nine = ((8, 8, 1), (8, 264, 63), (264, 8, 64), (520, 264, 321), (256, 256, 65), (8, 8, 1), (264, 8, 64), (8, 264, 63),
            (256, 256, 65))
    return [Case("table", "wgrad", 0, 0, (), f32=f32, accumulate=acc, products=nine) for f32 in (False, True)
            for acc in (False, True)]


def _fused_cases():
    out = []
    three = [(1, 8, 64), (7, 136, 128), (264, 264, 320)]
    for M, I, K in three:
        out.append(Case("swiglu_fwd", "fwd", M, 2 * I, (K,)))         # B = the rows of gate_proj, then those of up_proj
        out.append(Case("swiglu_bwd", "dgrad", M, I, (K,)))
        out.append(Case("gelu_fwd", "fwd", M, I, (K,), bias=True))
        out.append(Case("gelu_bwd", "dgrad", M, I, (K,)))
    for M, heads, D, K in [(1, 1, 64, 64), (7, 3, 64, 128), (264, 2, 128, 64), (129, 4, 128, 320)]:
        for bias in (False, True):
            out.append(Case("rope", "fwd", M, heads * D, (K,), bias=bias, heads=heads, head_dim=D))
    return out


def _overlap_cases():
    out = []
    for ld in (64, 128):
        for R in (40, 264):
            out.append(Case("overlap", "fwd", R, 72, (192,), overlap=ld))        # A: R overlapping rows of length 192
            out.append(Case("overlap", "wgrad", 136, 192, (R,), overlap=ld))     # B [K = R, 192], pitch ld
    return out


CASES = (_plain_cases() + _segment_cases() + _out_t_cases() + _addend_cases() + _wgrad_out_cases() + _splitk_cases()
         + _persist_cases() + _tail_cases() + _grouped_cases() + _table_cases() + _fused_cases() + _overlap_cases())
IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def sub_problems(case, dev="cpu"):
    """[(sub case, Problem)] of a case: its products one by one for grouped / table launches, else the case itself"""
    if not case.products:
        return [(case, build(case, dev))]
    subs = [_sub_case(case, i) for i in range(len(case.products))]
    if case.group == "table":                                       # bias gradients on every second product
        subs = [dataclasses.replace(s, bias_grad=i % 2 == 0) for i, s in enumerate(subs)]
    return [(s, build(s, dev)) for s in subs]
