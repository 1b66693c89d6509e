"""csrc/optim.hip through the C ABI, against the float64 restatement of tests/row_kernel_reference.py: the multi-tensor
sum of squares, the device step state, the (bounded-grid) multi-tensor AdamW at tensor sizes around its chunk sizes,
on its aligned and its scalar path, and the single-tensor entries tn_sumsq / tn_adamw_step that nothing else calls.
The device tables are built the way FusedAdamW.step builds them."""
import math

import pytest
import torch

import row_kernel_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
f32 = lambda x: float(torch.tensor(x, dtype=F32))            # what a `float` argument of the C ABI holds
LR, B1, B2, EPS, WD, MAX_NORM = f32(3e-3), f32(0.9), f32(0.95), f32(1e-8), f32(0.1), f32(0.7)
HYPER = (LR, B1, B2, EPS, WD)
RTOL, ATOL = 3e-5, 3e-6          # the project's bounds for this kernel (test_fused_adamw_multi_tensor_mixed_shapes)
ARRAYS = ("p", "m", "v", "g", "shadow")


def _lib():
    from touchnet_amd import _C
    return _C, _C.lib()


def _chunks():
    _, lib = _lib()
    return int(lib.tn_adamw_multi_chunk()), int(lib.tn_sumsq_multi_chunk())


def _sizes():
    Cc, S = _chunks()
    return [1, 3, 4, Cc - 1, Cc, Cc + 1, 2 * Cc + 5, S - 1, S, S + 1, 3 * S + 7]


def _values(gdtype):
    """CPU values of the tensor set of one gradient dtype: bf16-gradient tensors (with a shadow) and fp32-gradient tensors
    (without) alternate through the size list; non-zero m, positive v, non-zero p; the tensor of C + 1 elements (fp32) /
    C elements (bf16) has all-zero g, m and v."""
    Cc, _ = _chunks()
    out = []
    for i, n in enumerate(_sizes()):
        if (BF16 if i % 2 == 0 else F32) != gdtype:
            continue
        g = torch.Generator().manual_seed(100 + i)
        t = dict(p=torch.randn(n, generator=g) + 0.05, m=0.02 * torch.randn(n, generator=g) + 0.003,
                 v=1e-3 * torch.rand(n, generator=g) + 1e-6, g=(0.1 * torch.randn(n, generator=g) - 0.004).to(gdtype))
        if n in (Cc, Cc + 1):
            t["m"], t["v"], t["g"] = torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=gdtype)
        t["p"] = torch.where(t["p"] == 0, torch.ones(n), t["p"])
        out.append(t)
    return out


def _place(t, off_bytes=0):
    """`t` on the device at `off_bytes` behind a 16-byte boundary (a view into a larger buffer)"""
    k = off_bytes // t.element_size()
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[k:k + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == off_bytes
    return view


class TensorSet:
    def __init__(self, gdtype, off=None):
        """device copies of _values(gdtype) and their tables; `off`: the array of ARRAYS placed 4 bytes off alignment"""
        _C, lib = _lib()
        self.gdtype, self.code = gdtype, _C.DTYPE_CODE[gdtype]
        self.cpu = _values(gdtype)
        self.t = []
        for c in self.cpu:
            e = {k: _place(c[k], 4 if off == k else 0) for k in ("p", "m", "v", "g")}
            e["shadow"] = _place(c["p"].to(BF16), 4 if off == "shadow" else 0) if gdtype == BF16 else None
            self.t.append(e)
        Cc, S = _chunks()
        self.sizes = [c["p"].numel() for c in self.cpu]

        def firsts(chunk):
            first, tot = [], 0
            for n in self.sizes:
                first.append(tot)
                tot += (n + chunk - 1) // chunk
            return first, tot
        fa, self.nchunks = firsts(Cc)
        fs, self.nchunks_sumsq = firsts(S)
        ptrs = lambda k: [(e[k].data_ptr() if e[k] is not None else 0) for e in self.t]
        self.table = torch.tensor([ptrs("p"), ptrs("m"), ptrs("v"), ptrs("g"), ptrs("shadow"), self.sizes, fa, fs],
                                  dtype=torch.int64).to(DEV)

    def sumsq(self, norm_sq):
        _C, lib = _lib()
        partial = torch.empty(self.nchunks_sumsq, dtype=F32, device=DEV)
        t = self.table
        _C.check(lib.tn_sumsq_multi(_C.ptr(t[3]), _C.ptr(t[5]), _C.ptr(t[7]), len(self.t), self.nchunks_sumsq,
                                    _C.ptr(partial), _C.ptr(norm_sq), self.code, _C.stream()), "tn_sumsq_multi")

    def adamw(self, state, max_workgroups=0, bounded=True):
        _C, lib = _lib()
        t = self.table
        args = [_C.ptr(t[i]) for i in (0, 1, 2, 3, 4, 5, 6)] + [len(self.t), self.nchunks, _C.ptr(state), *HYPER, self.code]
        if bounded:
            _C.check(lib.tn_adamw_multi_bounded(*args, max_workgroups, _C.stream()), "tn_adamw_multi_bounded")
        else:
            _C.check(lib.tn_adamw_multi(*args, _C.stream()), "tn_adamw_multi")

    def snapshot(self):
        torch.cuda.synchronize()
        return [{k: (e[k].clone() if e[k] is not None else None) for k in ARRAYS if k != "g"} for e in self.t]


def _bits_equal(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        for k in x:
            if x[k] is not None:
                assert torch.equal(x[k], y[k]), f"{what}: tensor {i} ({x[k].numel()} elements), {k} differs"


def _state(step=0):
    s = torch.zeros(8, dtype=F32, device=DEV)
    s[:1].view(torch.int32).fill_(step)
    return s


def _prepare(norm_sq, state, max_norm=MAX_NORM):
    _C, lib = _lib()
    _C.check(lib.tn_adamw_prepare(_C.ptr(norm_sq), _C.ptr(state), B1, B2, max_norm, _C.stream()), "tn_adamw_prepare")
    torch.cuda.synchronize()
    s = state.cpu()
    return int(s[:1].view(torch.int32)), float(s[1]), float(s[2]), float(s[3]), float(s[4])


def _against_restatement(ts, before, step, clip):
    """p, m, v of the set against adamw_step from the values `before`; the shadow is bf16 of the device p, bit for bit"""
    after = ts.snapshot()
    for c, b, a in zip(ts.cpu, before, after):
        p, m, v, _ = R.adamw_step(b["p"], b["m"], b["v"], c["g"], step, *HYPER, clip)
        for k, ref in (("p", p), ("m", m), ("v", v)):
            torch.testing.assert_close(a[k].cpu().double(), ref, rtol=RTOL, atol=ATOL,
                                       msg=lambda s, k=k, n=p.numel(): f"{k} of the tensor of {n} elements: {s}")
        if a["shadow"] is not None:
            assert torch.equal(a["shadow"], a["p"].to(BF16)), f"shadow of the tensor of {p.numel()} elements"
    return after


@pytest.fixture(scope="module")
def unbounded():
    """{gradient dtype: p / m / v / shadow after ONE step from step 6 with an unbounded grid, all arrays aligned}"""
    out = {}
    for gdtype in (BF16, F32):
        ts = TensorSet(gdtype)
        norm_sq = torch.full((1,), 900.0, dtype=F32, device=DEV)
        state = _state(6)
        _prepare(norm_sq, state)
        ts.adamw(state)
        out[gdtype] = ts.snapshot()
    return out


def _one_step(gdtype, max_workgroups=0, off=None, bounded=True):
    ts = TensorSet(gdtype, off)
    norm_sq = torch.full((1,), 900.0, dtype=F32, device=DEV)
    state = _state(6)
    _prepare(norm_sq, state)
    ts.adamw(state, max_workgroups, bounded)
    return ts.snapshot()


@pytest.mark.parametrize("gdtype", [BF16, F32], ids=["bf16", "fp32"])
def test_multi_tensor_norm_and_update_against_the_restatement(gdtype):
    ts = TensorSet(gdtype)
    Cc, S = _chunks()
    assert ts.nchunks == sum((n + Cc - 1) // Cc for n in ts.sizes) and ts.nchunks > len(ts.t)
    start = 0.25                                                      # tn_sumsq_multi ADDS to norm_sq
    norm_sq = torch.full((1,), start, dtype=F32, device=DEV)
    ts.sumsq(norm_sq)
    want = start + sum(float(R.sumsq(c["g"]).value) for c in ts.cpu)
    assert float(norm_sq) == pytest.approx(want, rel=1e-5)
    before = ts.snapshot()
    state = _state(6)
    step, bc1, bc2, clip, skip = _prepare(norm_sq, state)
    r_step, r_bc1, r_bc2, r_clip, r_skip = R.adamw_prepare(6, float(norm_sq), B1, B2, MAX_NORM)
    assert (step, skip) == (r_step, 0.0) == (7, float(r_skip))
    assert bc1 == pytest.approx(r_bc1, rel=1e-6) and bc2 == pytest.approx(r_bc2, rel=1e-6)
    assert clip == pytest.approx(r_clip, rel=1e-6) and clip < 0.1       # the clip is active
    ts.adamw(state, bounded=False)
    after = _against_restatement(ts, before, 7, r_clip)
    # the tensor without gradient and moments: the update is exactly the weight decay
    i = ts.sizes.index(Cc if gdtype == BF16 else Cc + 1)
    assert not ts.cpu[i]["g"].any()
    assert not after[i]["m"].any() and not after[i]["v"].any()
    p0 = before[i]["p"].cpu()
    lr, wd = torch.tensor(LR, dtype=F32), torch.tensor(WD, dtype=F32)
    decays = [1 - lr * wd, (1 - lr.double() * wd.double()).to(F32)]   # 1 - lr wd in two roundings or contracted to one
    assert any(torch.equal(after[i]["p"].cpu(), p0 * dk) for dk in decays)
    assert torch.equal(after[i]["p"], before[i]["p"]) is False


@pytest.mark.parametrize("gdtype", [BF16, F32], ids=["bf16", "fp32"])
def test_bounded_grid_strides_over_the_chunks_bit_identically(gdtype, unbounded):
    """max_workgroups < nchunks: a workgroup takes chunks c, c + grid, ... (the pipelined optimizer's side-stream launch).
    With `c += gridDim.x` replaced by `break`, max_workgroups = 1 updates the first chunk only: every later tensor keeps its
    old p / m / v and the bit comparison with the unbounded launch fails at the first of them."""
    nchunks = TensorSet(gdtype).nchunks
    assert nchunks > 5
    for mw in (1, 3, nchunks - 1, nchunks, nchunks + 5):
        _bits_equal(_one_step(gdtype, mw), unbounded[gdtype], f"max_workgroups = {mw} of {nchunks} chunks")
    _bits_equal(_one_step(gdtype, bounded=False), unbounded[gdtype], "tn_adamw_multi")


@pytest.mark.parametrize("gdtype,off", [(BF16, k) for k in ARRAYS] + [(F32, k) for k in ARRAYS[:4]],
                         ids=lambda v: {BF16: "bf16", F32: "fp32"}.get(v, v))
def test_scalar_path_of_a_misaligned_array_is_the_aligned_path_bit_for_bit(gdtype, off, unbounded):
    """any one of p / m / v / g / shadow 4 bytes off a 16-byte boundary sends every chunk down the scalar loop: same
    operations, same order, same bits.  (fp32-gradient tensors carry no shadow: nothing to misalign there.)"""
    _bits_equal(_one_step(gdtype, off=off), unbounded[gdtype], f"{off} misaligned")
    if off == "g":                                                    # the sum of squares has a scalar path of its own
        ts = TensorSet(gdtype, off)
        norm_sq = torch.full((1,), 0.25, dtype=F32, device=DEV)
        ts.sumsq(norm_sq)
        assert float(norm_sq) == pytest.approx(0.25 + sum(float(R.sumsq(c["g"]).value) for c in ts.cpu), rel=1e-5)


@pytest.mark.parametrize("old", [0, 1, 999])
def test_device_step_state(old):
    _C, lib = _lib()
    ts = TensorSet(BF16)
    state = _state(old)
    nsq = torch.full((1,), 0.04, dtype=F32, device=DEV)
    step, bc1, bc2, clip, skip = _prepare(nsq, state)
    assert (step, clip, skip) == (old + 1, 1.0, 0.0)
    assert bc1 == pytest.approx(1.0 - B1 ** (old + 1), rel=1e-6) and bc2 == pytest.approx(1.0 - B2 ** (old + 1), rel=1e-6)
    before = ts.snapshot()
    ts.adamw(state)
    before = _against_restatement(ts, before, old + 1, 1.0)
    for bad in (float("nan"), float("inf")):
        nsq.fill_(bad)
        step, _, _, clip, skip = _prepare(nsq, state)
        assert (step, clip, skip) == (old + 1, 1.0, 1.0), bad         # the step does not advance; the skip flag is set
        ts.adamw(state)
        _bits_equal(ts.snapshot(), before, f"update under a norm of {bad}")
    nsq.fill_(1.96)                                                   # the next finite step is old + 2, clipped
    step, bc1, bc2, clip, skip = _prepare(nsq, state)
    want_clip = MAX_NORM / (math.sqrt(f32(1.96)) + 1e-6)              # a norm of twice max_norm
    assert (step, skip) == (old + 2, 0.0) and clip == pytest.approx(want_clip, rel=1e-6)
    assert bc1 == pytest.approx(1.0 - B1 ** (old + 2), rel=1e-6) and bc2 == pytest.approx(1.0 - B2 ** (old + 2), rel=1e-6)
    ts.adamw(state)
    _against_restatement(ts, before, old + 2, want_clip)


def test_clip_coefficient_of_the_step_state():
    state = _state(3)
    nsq = torch.full((1,), f32(0.35) ** 2, dtype=F32, device=DEV)
    assert _prepare(nsq, state)[3:] == (1.0, 0.0)                     # a norm of half max_norm: exactly 1
    nsq.fill_(1.96)
    assert _prepare(nsq, state, max_norm=0.0)[3:] == (1.0, 0.0)       # max_norm = 0: no clip
    _C, lib = _lib()
    _C.check(lib.tn_adamw_prepare(None, _C.ptr(state), B1, B2, MAX_NORM, _C.stream()), "tn_adamw_prepare")
    torch.cuda.synchronize()
    s = state.cpu()
    assert int(s[:1].view(torch.int32)) == 6 and float(s[3]) == 1.0 and float(s[4]) == 0.0    # NULL norm: no clip, no skip


@pytest.mark.parametrize("shadow", [False, True], ids=["no shadow", "shadow"])
@pytest.mark.parametrize("gdtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [1, 7, 8, 1031, 300001])
def test_single_tensor_entries(n, gdtype, shadow):
    """tn_sumsq and tn_adamw_step (exported in include/touchnet_amd.h, called by nothing else) against the same restatement"""
    _C, lib = _lib()
    g_ = torch.Generator().manual_seed(n)
    c = dict(p=torch.randn(n, generator=g_) + 0.05, m=0.02 * torch.randn(n, generator=g_) + 0.003,
             v=1e-3 * torch.rand(n, generator=g_) + 1e-6, g=(0.1 * torch.randn(n, generator=g_) - 0.004).to(gdtype))
    t = {k: x.to(DEV) for k, x in c.items()}
    sh = c["p"].to(BF16).to(DEV) if shadow else None
    code, step = _C.DTYPE_CODE[gdtype], 4
    scratch = torch.empty(int(lib.tn_sumsq_scratch_floats()), dtype=F32, device=DEV)
    norm_sq = torch.full((1,), 0.25, dtype=F32, device=DEV)           # tn_sumsq ADDS to norm_sq
    _C.check(lib.tn_sumsq(_C.ptr(t["g"]), _C.ptr(scratch), _C.ptr(norm_sq), n, code, _C.stream()), "tn_sumsq")
    assert float(norm_sq) == pytest.approx(0.25 + float(R.sumsq(c["g"]).value), rel=1e-5)
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step

    def run(nsq):
        _C.check(lib.tn_adamw_step(_C.ptr(t["p"]), _C.ptr(t["m"]), _C.ptr(t["v"]), _C.ptr(t["g"]), _C.ptr(sh),
                                   _C.ptr(nsq), n, *HYPER, MAX_NORM, bc1, bc2, code, _C.stream()), "tn_adamw_step")
        torch.cuda.synchronize()

    before = {k: x.clone() for k, x in t.items()}
    run(torch.full((1,), float("nan"), dtype=F32, device=DEV))       # a NaN norm: nothing is written
    assert all(torch.equal(t[k], before[k]) for k in t) and (sh is None or torch.equal(sh, c["p"].to(BF16).to(DEV)))
    norm_sq.fill_(0.25 if n < 8 else 4.0)                             # clip 1 (norm 0.5) or 0.35 (norm 2)
    clip = min(1.0, MAX_NORM / (math.sqrt(float(norm_sq)) + 1e-6))
    run(norm_sq if n != 7 else None)                                  # NULL norm: no clip
    p, m, v, _ = R.adamw_step(c["p"], c["m"], c["v"], c["g"], step, *HYPER, clip if n != 7 else 1.0)
    for k, ref in (("p", p), ("m", m), ("v", v)):
        torch.testing.assert_close(t[k].cpu().double(), ref, rtol=RTOL, atol=ATOL, msg=lambda s, k=k: f"{k}: {s}")
    if shadow:
        assert torch.equal(sh, t["p"].to(BF16))


def test_pipelined_fused_adamw_with_a_bounded_side_stream_grid_is_the_plain_one():
    """one parameter of 128 chunks and a tail, updated from 5 workgroups on the side stream (the 7B run's form: each
    workgroup strides over 25 or 26 chunks), three steps == the un-pipelined optimizer, bit for bit"""
    from touchnet_amd.utils.optimizer import FusedAdamW
    Cc, _ = _chunks()
    n = 128 * Cc + 77
    g = torch.Generator().manual_seed(9)
    init = torch.randn(n, generator=g).to(BF16)
    pa, pb = torch.nn.Parameter(init.to(DEV)), torch.nn.Parameter(init.to(DEV))
    a, b = FusedAdamW([pa], lr=3e-3, max_norm=0.7), FusedAdamW([pb], lr=3e-3, max_norm=0.7)
    a.pipeline_updates([[0]])
    a.side_workgroups = 5
    for it in range(3):
        grad = ((0.01 if it == 1 else 1.0) * torch.randn(n, generator=g)).to(BF16).to(DEV)
        pa.grad, pb.grad = grad.clone(), grad.clone()
        na, nb = a.step(), b.step()
        a.wait_updates()
        torch.cuda.synchronize()
        assert torch.equal(na, nb)
        for k in ("master", "m", "v"):
            assert torch.equal(a.state[0][k], b.state[0][k]), (it, k)
        assert torch.equal(pa.data, pb.data) and torch.equal(pa.data, a.state[0]["master"].to(BF16))
    assert a.step_count == b.step_count == 3 and not torch.equal(pa.data, init.to(DEV))
