"""The prefill GEMM on weight codes (csrc/gemm_codes.hip: tn_gemm_prefill_fp8 / _mxfp4 and their _swiglu forms; any M >= 1,
128 x 64 and 128 x 128 tiles) against float64 on the dequantised weights, its SwiGLU form and its RoPE against the row kernels
on the plain products, and an extend of 300 rows that reaches it."""
import copy
import ctypes as C

import pytest
import torch

from test_gemm_midm_gpu import DEV, SENTINEL, _fp8, _ints, _pitched, _randn, _rope_case

pytestmark = pytest.mark.gpu
FMTS = ("fp8", "mxfp4")
BM, BN = 128, 64          # the tile of few-tile launches; from 256 tiles of 128 x 128 on the launch uses those


def _exact_weight(fmt, g, N, K):
    """exact codes: FP8 as the mid-M tests make them; MXFP4 every code (both zeros) under scale bytes 125 .. 129"""
    from touchnet_amd import functional as F
    if fmt == "fp8":
        return _fp8(g, N, K)
    codes = torch.randint(0, 256, (N, K // 2), generator=g).to(DEV, torch.uint8)
    return F.Mxfp4Weight(codes, (125 + torch.randint(0, 5, (N, K // 32), generator=g)).to(DEV, torch.uint8))


def _quantize(fmt, w):
    from touchnet_amd import functional as F
    return (F.quantize_weight_fp8 if fmt == "fp8" else F.quantize_weight_mxfp4)(w)


def _deq(w):
    from touchnet_amd import functional as F
    return (F.dequantize_weight_fp8 if isinstance(w, F.Fp8Weight) else F.dequantize_weight_mxfp4)(w)


def _linear(fmt):
    from touchnet_amd import functional as F
    return getattr(F, f"linear_prefill_{fmt}")


def _swiglu(fmt):
    from touchnet_amd import functional as F
    return getattr(F, f"swiglu_prefill_{fmt}")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,K,Ns", [(M, K, Ns) for M in (1, BM - 1, BM + 1, 257) for K in (128, 384)
                                    for Ns in ([16], [BN + 16], [BN + 16, 16, 48])] + [(BM + 1, 128, [16400])])
@pytest.mark.parametrize("fmt", FMTS)
def test_integer_products_are_exact_and_nothing_else_is_written(fmt, M, K, Ns, bias):
    """x in {-1, 0, 1} and exact codes: every partial sum is a small multiple of 2^-9 (2^-3), so any fp32 order is exact and
    the result is bf16(float64 product + bias) bit for bit.  x is a pitched view in NaN, the outputs pitched views in a
    sentinel, compared as whole buffers.  N = 16400 at 129 rows is 2 x 129 tiles of 128 x 128 (the last one 16 wide)."""
    g = torch.Generator().manual_seed(1000 * M + K)
    x = _pitched(_ints(g, -1, 1, M, K), rows_behind=3)
    layers = [(_exact_weight(fmt, g, N, K), _ints(g, -8, 8, N) if bias and i != 1 else None) for i, N in enumerate(Ns)]
    bufs = [torch.full((M + 2, N + 8), SENTINEL, dtype=torch.int16, device=DEV) for N in Ns]
    _linear(fmt)(x, layers, outs=[b.view(torch.bfloat16)[:M, :N] for b, N in zip(bufs, Ns)])
    for (w, b), buf, N in zip(layers, bufs, Ns):
        ref = x.double() @ _deq(w).double().t() + (b.double() if b is not None else 0)
        want = torch.full_like(buf, SENTINEL)
        want[:M, :N] = ref.to(torch.bfloat16).view(torch.int16)
        assert torch.equal(buf, want), (M, K, N, int((buf != want).sum()))


@pytest.mark.parametrize("K", [384, 1152])
@pytest.mark.parametrize("fmt", FMTS)
def test_real_products_within_one_rounding_of_float64(fmt, K):
    """|y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k| on the dequantised weights: one bf16 rounding + fp32 accumulation in
    any order, no term for the format"""
    g = torch.Generator().manual_seed(K)
    x, w, b = _randn(g, 300, K), _quantize(fmt, _randn(g, 48, K)), _randn(g, 48)
    y = _linear(fmt)(x, [(w, b)])[0].double()
    wd = _deq(w).double()
    ref = x.double() @ wd.t() + b.double()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (x.double().abs() @ wd.abs().t())
    ratio = float(((y - ref).abs() / bound).max())
    print(f"{fmt}, K = {K}: worst |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("fmt", FMTS)
def test_a_row_does_not_depend_on_its_batch(fmt):
    """rows of a 300-row call again in reversed, strided order inside a 130-row call, and alone at M = 1"""
    g = torch.Generator().manual_seed(4)
    x, layers, rope = _rope_case(g, 300, 64, 4, 1, K=1152)
    layers = [(_quantize(fmt, w), b) for w, b in layers]
    y300 = _linear(fmt)(x, layers, rope=rope)
    pick = torch.arange(299, 3, -2, device=DEV)[:130]
    y130 = _linear(fmt)(x[pick], layers, rope=(rope[0][pick], rope[1][pick], 64, (0, 1)))
    for a, b in zip(y130, y300):
        assert torch.equal(a, b[pick])
    for i in (0, 127, 128, 299):
        one = _linear(fmt)(x[i:i + 1], layers, rope=(rope[0][i:i + 1], rope[1][i:i + 1], 64, (0, 1)))
        for a, b in zip(one, y300):
            assert torch.equal(a[0], b[i]), i


@pytest.mark.parametrize("M,I", [(129, 16), (129, BN // 2 + 16), (300, 16), (300, BN // 2 + 16), (129, 8208)])
@pytest.mark.parametrize("fmt", FMTS)
def test_swiglu_form_is_swiglu_of_the_plain_products(fmt, M, I):
    """(I = 8208 at 129 rows: 2 x 129 tiles of 128 rows x 64 features, the 128-wide instantiation, the last tile 16 wide)"""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(I + M)
    x = _randn(g, M, 384)
    wg, wu = _quantize(fmt, _randn(g, I, 384) * 0.1), _quantize(fmt, _randn(g, I, 384) * 0.1)
    gate, up = _linear(fmt)(x, [(wg, None), (wu, None)])
    act = _swiglu(fmt)(x, wg, wu)
    assert torch.equal(act, F.swiglu(gate, up)) and bool(act.float().abs().sum() > 0)


@pytest.mark.parametrize("D,nq,nkv", [(64, 4, 1), (128, 2, 1)])
@pytest.mark.parametrize("fmt", FMTS)
def test_rope_is_apply_rope_of_the_plain_product(fmt, D, nq, nkv):
    from touchnet_amd import functional as F
    M = 300
    x, layers, rope = _rope_case(torch.Generator().manual_seed(D + M), M, D, nq, nkv, K=384)
    layers = [(_quantize(fmt, w), b) for w, b in layers]
    q, k, v = _linear(fmt)(x, layers)
    qr, kr = F.apply_rope(q.view(1, M, nq, D), k.view(1, M, nkv, D), rope[0], rope[1])
    got = _linear(fmt)(x, layers, rope=rope)
    assert torch.equal(got[0], qr.view(M, -1)) and torch.equal(got[1], kr.view(M, -1)) and torch.equal(got[2], v)
    assert not torch.equal(got[0], q)


@pytest.mark.parametrize("case", ["M=0", "K=192", "N=24", "fp32", "misaligned", "codes dtype"])
@pytest.mark.parametrize("fmt", FMTS)
def test_refusals_by_name_and_by_code_before_any_launch(fmt, case):
    """`functional` raises by name; the C entries return -22 and leave the output alone (they take no dtype: the fp32 and
    code-dtype cases are functional's alone)."""
    from touchnet_amd import _C, functional as F
    M, K, N = {"M=0": (0, 128, 16), "K=192": (300, 192, 16), "N=24": (300, 128, 24)}.get(case, (300, 128, 16))
    x = torch.ones(M * K + 8, dtype=torch.float32 if case == "fp32" else torch.bfloat16, device=DEV)
    x = x[1:M * K + 1].view(M, K) if case == "misaligned" else x[:M * K].view(M, K)
    cdt = torch.int8 if case == "codes dtype" else torch.uint8
    if fmt == "fp8":
        q = F.Fp8Weight(torch.zeros(N, K, dtype=cdt, device=DEV), torch.ones(N, device=DEV))
    else:
        q = F.Mxfp4Weight(torch.zeros(N, K // 2, dtype=cdt, device=DEV), torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV))
    with pytest.raises(_C.KernelError, match=f"linear_prefill_{fmt}"):
        _linear(fmt)(x, [(q, None)])
    with pytest.raises(_C.KernelError, match=f"swiglu_prefill_{fmt}"):
        _swiglu(fmt)(x, q, q)
    if case not in ("fp32", "codes dtype"):
        y = torch.full((max(M, 1), N), SENTINEL, dtype=torch.int16, device=DEV)
        one = lambda t, v: (t * 1)(v)
        lib, s = _C.lib(), F._scales_of(q)
        pitch = (one(C.c_longlong, s.stride(0)),) if fmt == "mxfp4" else ()
        rcs = [getattr(lib, f"tn_gemm_prefill_{fmt}")(
                   x.data_ptr(), K, M, K, 1, one(C.c_void_p, q.codes.data_ptr()), one(C.c_longlong, q.codes.stride(0)),
                   one(C.c_void_p, s.data_ptr()), *pitch, None, one(C.c_void_p, y.data_ptr()), one(C.c_longlong, N),
                   one(C.c_int, N), None),
               getattr(lib, f"tn_gemm_prefill_swiglu_{fmt}")(
                   x.data_ptr(), q.codes.data_ptr(), q.codes.data_ptr(), s.data_ptr(), s.data_ptr(), y.data_ptr(), M, N, K, K,
                   q.codes.stride(0), *((s.stride(0),) if fmt == "mxfp4" else ()), N, None)]
        torch.cuda.synchronize()
        assert all(rc == -22 for rc in rcs) and bool((y == SENTINEL).all())


@pytest.mark.parametrize("fmt", FMTS)
def test_an_extend_of_300_rows_runs_on_codes_without_dequantising(fmt, monkeypatch):
    """Two sequences of 170 and 130 new rows behind empty prefixes: every product of the 300 rows (and lm_head) runs on the
    prefill kernel — the dequantisers raise if asked — and the logits agree with a bf16 copy of the model on the dequantised
    weights within the decoders' summation-order bound 3e-2 max|logit|."""
    from test_gemm_smallm_gpu import _tiny
    from touchnet_amd import _C, functional as F, generation as G
    model, _ = _tiny("qwen2", seed=12)
    ref = copy.deepcopy(model)
    assert G.quantize_decoder_weights(model, "fp8_e4m3" if fmt == "fp8" else "mxfp4") > 0
    for name, m in model.named_modules():
        if isinstance(m, (G.Fp8Linear, G.Mxfp4Linear)):
            ref.get_submodule(name).weight = torch.nn.Parameter(_deq(m.weight))
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(4, 640, (n,), generator=g) for n in (170, 130)]
    logits = {}
    with torch.no_grad():
        for arm, m in (("bf16", ref), (fmt, model)):
            lm, _ = G._parts(m)
            c = lm.config
            cache = G.KVCache.allocate(len(lm.model.layers), 2, 180, c.num_key_value_heads, c.head_dim, DEV)
            if arm == fmt:
                def refuse(w):
                    raise _C.KernelError("a dequantiser was called")
                monkeypatch.setattr(F, "dequantize_weight_fp8", refuse)
                monkeypatch.setattr(F, "dequantize_weight_mxfp4", refuse)
            h = G.extend(m, cache, [0, 1], ids, keep_rows=range(300), prefix_len=[0, 0])
            logits[arm] = F.linear_group(h, [(lm.lm_head.weight, lm.lm_head.bias)])[0].float()
    diff, top = float((logits[fmt] - logits["bf16"]).abs().max()), float(logits["bf16"].abs().max())
    print(f"{fmt}: max|codes - bf16| = {diff:.4g}, max|bf16| = {top:.4g}")
    assert logits[fmt].shape == (300, 640) and diff <= 3e-2 * top
