"""Every GEMM entry point (csrc/gemm.hip, gemm_table.hip: Kernel and Kernel16 of gemm_kernel.h in all their instantiations,
splitk_reduce_kernel) held to EXACT integer products at its edges: the cases of tests/gemm_reference.py — M from 1,
N from 8, K from 1, one to eleven stages, segments, the transposed copy in all three operand modes, the addend, fp32
outputs and the bias gradient, split-K with the number of parts chosen here (a part that begins behind K included), the
persistent tile walk with two and three tiles per workgroup and a short last panel group, the tail split, the grouped
and the table launch, the five fused epilogues and overlapping rows.  Every comparison is on bit patterns; there is no
tolerance in this file.  Each output is a pitched view inside a buffer of a sentinel bit pattern that must come back
unchanged, each operand a pitched view inside a buffer of NaNs (gemm_reference.py has the regimes and the guards;
tests/test_gemm_reference_cpu.py shows that ten kinds of one-term mistakes break these comparisons, two of which the
tolerance of the older GEMM tests lets through).

MEASURED on an MI355X: the file's 366 cases take 9.2 - 13.5 s (three runs), the slowest 1.4 - 1.6 s (swiglu_fwd 1x16x64, the
first case to load the row kernels; the largest product, persist 5640 x 5640, 0.45 - 0.7 s with its float64 reference on the
device).  On first contact 362 cases passed and no sentinel element was touched anywhere.  The four that failed were the
overlapping-row forward products, at exactly the rows read off the code beforehand: rows 38, 39 of 40 and 262, 263 of 264
at ld = 64, row 39 and row 263 at ld = 128 (K = 192) — the tails of the last ceil((K - ld) / ld) rows read as zeros,
because Stream::open ended a row-stored tile's descriptor (R - origin) ld behind its start.  It now ends with the last
row's last element, (R - origin - 1) ld + K; after that one change all 366 pass, and so does the rest of the GPU suite,
unchanged.  The overlapping contraction-major B of a weight gradient was right as it stood.  (One case also failed
through a mistake of this file's own, the shape of a seeded input; no expected value was touched after the first run.)"""
import ctypes

import pytest
import torch

import gemm_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _f():
    import touchnet_amd.functional as F
    return F


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class _Guarded:
    """an output: a pitched view inside a sentinel buffer; `check` compares the WHOLE buffer, bit for bit"""

    def __init__(self, M, N, dtype=BF16, init=None, pitch_mult=8):
        buf, r0, c0 = R.sentinel_buffer(M, N, dtype, pitch_mult)
        self.buf = buf.to(DEV)
        self.view = self.buf[r0:r0 + M, c0:c0 + N]
        if init is not None:
            self.view.copy_(init)
        self.want = self.buf.clone()
        self.want_view = self.want[r0:r0 + M, c0:c0 + N]
        assert self.view.data_ptr() % 16 == 0 and self.view.stride(0) > N

    def check(self, expected, what):
        self.want_view.copy_(expected.to(DEV))
        assert expected.dtype == self.view.dtype
        if torch.equal(_bits(self.buf), _bits(self.want)):
            return
        wrong = _bits(self.view) != _bits(self.want_view)
        rows = wrong.any(1).nonzero().flatten().tolist()
        guard = int((_bits(self.buf) != _bits(self.want)).sum()) - int(wrong.sum())
        raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.numel()} output elements differ (rows {rows[:6]}.."
                             f"{rows[-3:]}, {len(rows)} rows), {guard} sentinel elements changed")


class _GuardedVec(_Guarded):
    def __init__(self, M):
        self.buf = torch.full((M + 16,), R.SENT16, dtype=torch.int16).view(BF16).to(DEV)
        self.view = self.buf[8:8 + M]
        self.want = self.buf.clone()
        self.want_view = self.want[8:8 + M]

    def check(self, expected, what):
        self.want_view.copy_(expected.to(DEV))
        assert torch.equal(_bits(self.buf), _bits(self.want)), what


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _workspace(lib, M, N, parts, with_bg, tail):
    if parts <= 1:
        return None, 0
    need = int(lib.tn_gemm_splitk_workspace_bytes(M, N, parts, int(with_bg), int(tail)))
    assert need > 0
    return torch.empty(need // 4, dtype=F32, device=DEV), need


def _run_single(case, p, what):
    """one product through the entry `case.entry` names; returns nothing, asserts everything"""
    from touchnet_amd import _C
    F, lib = _f(), _C.lib()
    ak, bk = R.MODES[case.mode]
    M, N = case.M, case.N
    segs = [(a.view(DEV), b.view(DEV)) for a, b in zip(p.A, p.B)]
    expected = p.expected(case)
    out = _Guarded(M, N, F32 if case.f32 else BF16, init=p.c0.to(DEV).to(F32 if case.f32 else BF16) if case.accumulate else None)
    bias = p.bias.to(DEV) if case.bias else None
    out_t = _Guarded(N, M) if case.out_t else None
    bg = _GuardedVec(M) if case.bias_grad else None
    a0, b0 = segs[0]
    K = case.Ks[0]
    if case.entry == "gemm":
        got = F.gemm(segs, ak, bk, bias=bias, out=out.view, accumulate=case.accumulate,
                     out_t=out_t.view if out_t else None, addend=p.add.view(DEV) if case.addend else None)
        assert got.data_ptr() == out.view.data_ptr()
    else:
        ws, need = _workspace(lib, M, N, case.parts, case.bias_grad, case.tail)
        if case.entry == "splitk":
            rc = lib.tn_gemm_bf16_splitk(_ptr(a0), _ptr(b0), a0.stride(0), b0.stride(0), K, int(ak), int(bk), _ptr(out.view),
                                         _ptr(bias), M, N, out.view.stride(0), int(case.accumulate), case.parts,
                                         int(case.tail), _ptr(ws), need, _stream())
        elif case.entry == "wgrad_f32":
            rc = lib.tn_gemm_bf16_wgrad_f32(_ptr(a0), _ptr(b0), a0.stride(0), b0.stride(0), K, _ptr(out.view), M, N,
                                            out.view.stride(0), int(case.accumulate), case.parts, _ptr(ws), need, _stream())
        else:
            rc = lib.tn_gemm_bf16_wgrad_bias(_ptr(a0), _ptr(b0), a0.stride(0), b0.stride(0), K, _ptr(out.view), _ptr(bg.view),
                                             M, N, out.view.stride(0), int(case.accumulate), int(case.f32), case.parts,
                                             _ptr(ws), need, _stream())
        _C.check(rc, f"tn_gemm_bf16_{case.entry}")
    torch.cuda.synchronize()
    out.check(expected, what)
    if out_t:
        out_t.check(expected.t(), what + ": transposed copy")
    if bg:
        bg.check(p.expected_bias_grad(), what + ": bias gradient")


def _run_products(case, what):
    """the grouped and the table launch: several weight gradients, one launch"""
    from touchnet_amd import _C
    F = _f()
    subs = R.sub_problems(case, DEV if case.device_ref else "cpu")
    dtype = F32 if case.f32 else BF16
    pairs = [(p.A[0].view(DEV), p.B[0].view(DEV)) for _, p in subs]
    outs = [_Guarded(s.M, s.N, dtype, init=p.c0.to(DEV).to(dtype) if case.accumulate else None,
                     pitch_mult=4 if case.f32 else 8) for s, p in subs]
    if case.group == "grouped":
        arr = lambda v: (ctypes.c_int * len(v))(*v)
        need = int(_C.lib().tn_gemm_grouped_workspace_bytes(arr([s.M for s, _ in subs]), arr([s.N for s, _ in subs]),
                                                            arr([s.Ks[0] for s, _ in subs]), len(subs)))
        tiles = sum(-(-s.M // 256) * -(-s.N // 256) for s, _ in subs)
        if case.device_ref:      # the remainder of the tile list runs split: on a device of another size it would not
            assert tiles > _ncu() and need > 0, (tiles, _ncu(), need)
        F.gemm_grouped_wgrad(pairs, outs=[o.view for o in outs], accumulate=case.accumulate)
        bgs = [None] * len(subs)
    else:
        bgs = [_GuardedVec(s.M) if s.bias_grad else None for s, _ in subs]
        F.gemm_grouped_table_wgrad(pairs, outs=[o.view for o in outs], accumulate=case.accumulate,
                                   bias_grads=[b.view if b else None for b in bgs])
    torch.cuda.synchronize()
    for i, ((s, p), o, b) in enumerate(zip(subs, outs, bgs)):
        o.check(p.expected(s), f"{what}: product {i}")
        if b:
            b.check(p.expected_bias_grad(), f"{what}: bias gradient {i}")


def _uniform(case, *shape, salt=0):
    g = torch.Generator().manual_seed(R._seed("extra", case, salt))
    return ((torch.rand(*shape, generator=g) * 6 - 3).to(BF16)).to(DEV)


def _run_fused(case, p, what):
    """the product that reaches memory must be the exact one; the derived output must have the bits the row kernel makes of
    the EXACT product (the reference's, not the kernel's own)"""
    from touchnet_amd import _C
    from touchnet_amd import library as L
    F, lib = _f(), _C.lib()
    M, N, K = case.M, case.N, case.Ks[0]
    a, b = p.A[0].view(DEV), p.B[0].view(DEV)
    exact = p.expected(case).to(DEV)                       # bf16(product + bias): exact in regime S
    bias = p.bias.to(DEV) if case.bias else None
    if case.group == "swiglu_fwd":
        I = N // 2
        gate, up, act = _Guarded(M, I), _Guarded(M, I), _Guarded(M, I)
        wg, wu = b[:I], b[I:]
        rc = lib.tn_gemm_bf16_swiglu_fwd(_ptr(a), _ptr(wg), _ptr(wu), _ptr(gate.view), _ptr(up.view), _ptr(act.view), M, I, K,
                                         a.stride(0), wg.stride(0), gate.view.stride(0), _stream())
        _C.check(rc, "tn_gemm_bf16_swiglu_fwd")
        eg, eu = exact[:, :I].contiguous(), exact[:, I:].contiguous()
        checks = [(gate, eg, "gate"), (up, eu, "up"), (act, F.swiglu(eg, eu), "act")]
    elif case.group == "swiglu_bwd":
        gate_in, up_in = _Guarded(M, N, init=_uniform(case, M, N)), _Guarded(M, N, init=_uniform(case, M, N, salt=1))
        dgate, dup = _Guarded(M, N), _Guarded(M, N)
        rc = lib.tn_gemm_bf16_swiglu_bwd(_ptr(a), _ptr(b), _ptr(gate_in.view), _ptr(up_in.view), _ptr(dgate.view), _ptr(dup.view),
                                         M, N, K, a.stride(0), b.stride(0), dgate.view.stride(0), _stream())
        _C.check(rc, "tn_gemm_bf16_swiglu_bwd")
        dg, du = L.swiglu_bwd(exact, gate_in.view.contiguous(), up_in.view.contiguous())
        checks = [(dgate, dg, "d(gate)"), (dup, du, "d(up)"), (gate_in, gate_in.view.clone(), "gate (input)"),
                  (up_in, up_in.view.clone(), "up (input)")]
    elif case.group == "gelu_fwd":
        pre, act = _Guarded(M, N), _Guarded(M, N)
        rc = lib.tn_gemm_bf16_gelu_fwd(_ptr(a), _ptr(b), _ptr(bias), _ptr(pre.view), _ptr(act.view), M, N, K, a.stride(0),
                                       b.stride(0), pre.view.stride(0), _stream())
        _C.check(rc, "tn_gemm_bf16_gelu_fwd")
        checks = [(pre, exact, "pre"), (act, F.gelu(exact), "act")]
    elif case.group == "gelu_bwd":
        pre_in, dpre = _Guarded(M, N, init=_uniform(case, M, N)), _Guarded(M, N)
        rc = lib.tn_gemm_bf16_gelu_bwd(_ptr(a), _ptr(b), _ptr(pre_in.view), _ptr(dpre.view), M, N, K, a.stride(0), b.stride(0),
                                       dpre.view.stride(0), _stream())
        _C.check(rc, "tn_gemm_bf16_gelu_bwd")
        checks = [(dpre, L.gelu_bwd(exact, pre_in.view.contiguous()), "d(pre)"), (pre_in, pre_in.view.clone(), "pre (input)")]
    else:
        D = case.head_dim
        g = torch.Generator().manual_seed(R._seed("positions", case))
        pos = torch.randint(0, 4000, (1, M), generator=g).to(DEV)
        cos, sin = F.rope_tables(pos, F.rope_inv_freq(D, 1e6, device=DEV), BF16)
        out = _Guarded(M, N)
        rc = lib.tn_gemm_bf16_rope(_ptr(a), _ptr(b), _ptr(bias), _ptr(cos), _ptr(sin), _ptr(out.view), M, N, K, a.stride(0),
                                   b.stride(0), out.view.stride(0), D, _stream())
        _C.check(rc, "tn_gemm_bf16_rope")
        y = exact.view(1, M, case.heads, D)
        checks = [(out, F.apply_rope(y, y.new_empty(1, M, 0, D), cos, sin)[0].view(M, N), "rope")]
    torch.cuda.synchronize()
    for guarded, want, name in checks:
        guarded.check(want, f"{what}: {name}")


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_gemm_entry_point_returns_the_exact_product(case, monkeypatch):
    if case.persist:
        monkeypatch.delenv("TN_GEMM_PERSIST", raising=False)
    else:
        monkeypatch.setenv("TN_GEMM_PERSIST", "0")
    what = R.case_id(case)
    if case.group in ("persist", "tail"):
        # the tile counts are chosen against 256 CUs: a device of another size fails here instead of passing vacuously
        tiles = -(-case.M // 256) * -(-case.N // 256)
        assert tiles > (2 * _ncu() if case.M == 5640 else _ncu()), (tiles, _ncu())
    if case.products:
        return _run_products(case, what)
    p = R.build(case, DEV if case.device_ref else "cpu")
    if case.group in ("swiglu_fwd", "swiglu_bwd", "gelu_fwd", "gelu_bwd", "rope"):
        return _run_fused(case, p, what)
    _run_single(case, p, what)
