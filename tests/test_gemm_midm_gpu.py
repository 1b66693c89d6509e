"""The mid-M weight-streaming GEMM (csrc/gemm_midm.hip: tn_gemm_midm, _swiglu, _fp8, _swiglu_fp8; 1..256 rows, X staged through
LDS) against float64, its epilogues against the row kernels, its FP8 form against itself on the dequantised weights, and an
FP8 extend of 130 rows that reaches it."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7B7B          # bit pattern the output buffers hold wherever nothing may be written
SMALL_CODES = torch.tensor(list(range(0x00, 0x51)) + list(range(0x80, 0xD1)), dtype=torch.uint8)    # finite, |value| <= 8


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(DEV, torch.bfloat16)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _pitched(t, rows_behind=0):
    """t as a view with a row pitch above its width inside a NaN-filled buffer (`rows_behind` NaN rows follow it)"""
    buf = torch.full((t.shape[0] + rows_behind, t.shape[1] + 8), float("nan"), dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf[:t.shape[0], :t.shape[1]]


def _fp8(g, N, K):
    """an Fp8Weight of exact codes (every finite code with |value| <= 8) with scales 2^(n % 5 - 2)"""
    from touchnet_amd import functional as F
    codes = SMALL_CODES[torch.randint(0, len(SMALL_CODES), (N, K), generator=g)].to(DEV)
    return F.Fp8Weight(codes, (2.0 ** (torch.arange(N) % 5 - 2)).to(DEV, torch.float32))


@pytest.mark.parametrize("Ns", [[16], [48], [256, 64, 64]])
@pytest.mark.parametrize("K", [64, 320, 1088])
@pytest.mark.parametrize("M", [1, 49, 64, 65, 127, 129, 255, 256])
def test_integer_products_are_exact_and_nothing_else_is_written(M, K, Ns):
    """|x| <= 1, |w| <= 255: every partial sum is an integer below 2^24, so any summation order is exact and the result is
    bf16(float64 product + bias) bit for bit.  Operands are pitched views in NaN, outputs pitched views in a sentinel."""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(1000 * M + K)
    x = _pitched(_ints(g, -1, 1, M, K), rows_behind=3)
    layers = [(_pitched(_ints(g, -255, 255, N, K)), _ints(g, -8, 8, N) if i != 1 else None) for i, N in enumerate(Ns)]
    bufs = [torch.full((M + 2, N + 8), SENTINEL, dtype=torch.int16, device=DEV) for N in Ns]
    F.linear_midm(x, layers, outs=[b.view(torch.bfloat16)[:M, :N] for b, N in zip(bufs, Ns)])
    for (w, b), buf, N in zip(layers, bufs, Ns):
        ref = x.double() @ w.double().t() + (b.double() if b is not None else 0)
        want = torch.full_like(buf, SENTINEL)
        want[:M, :N] = ref.to(torch.bfloat16).view(torch.int16)
        assert torch.equal(buf, want), (M, K, N, int((buf != want).sum()))


@pytest.mark.parametrize("M", [49, 256])
@pytest.mark.parametrize("N", [16400, 32784])
def test_integer_products_are_exact_in_ragged_last_workgroups(N, M):
    """1025 strips at one strip per wave (256 workgroups of 4 + one wave's strip) and 2049 at two (256 of 8 + one strip):
    several workgroups, a last one whose other waves and strips have nothing to store."""
    test_integer_products_are_exact_and_nothing_else_is_written(M, 64, [N])


@pytest.mark.parametrize("K", [320, 1088])
def test_real_products_within_one_rounding_of_float64(K):
    """|y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k|: one bf16 rounding + fp32 accumulation in any order"""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(K)
    x, w, b = _randn(g, 200, K), _randn(g, 48, K), _randn(g, 48)
    y = F.linear_midm(x, [(w, b)])[0].double()
    ref = x.double() @ w.double().t() + b.double()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t())
    ratio = float(((y - ref).abs() / bound).max())
    print(f"K = {K}: worst |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def _rope_case(g, M, D, nq, nkv, K=320, pos=None):
    from touchnet_amd import functional as F
    x = _randn(g, M, K)
    layers = [(_randn(g, n * D, K), _randn(g, n * D)) for n in (nq, nkv, nkv)]
    pos = ((torch.arange(M) * 37 + 5) % 101) if pos is None else pos                  # positions that differ per row
    cos, sin = F.rope_tables(pos[None].to(DEV), F.rope_inv_freq(D, 10000.0, device=DEV), torch.bfloat16)
    return x, layers, (cos, sin, D, (0, 1))


@pytest.mark.parametrize("M", [49, 130])
@pytest.mark.parametrize("D,nq,nkv", [(64, 4, 1), (128, 2, 1)])
def test_rope_epilogue_is_apply_rope_of_the_plain_product(D, nq, nkv, M):
    from touchnet_amd import functional as F
    x, layers, rope = _rope_case(torch.Generator().manual_seed(D + M), M, D, nq, nkv)
    q, k, v = F.linear_midm(x, layers)
    qr, kr = F.apply_rope(q.view(1, M, nq, D), k.view(1, M, nkv, D), rope[0], rope[1])
    got = F.linear_midm(x, layers, rope=rope)
    assert torch.equal(got[0], qr.view(M, -1)) and torch.equal(got[1], kr.view(M, -1)) and torch.equal(got[2], v)
    assert not torch.equal(got[0], q)


@pytest.mark.parametrize("M", [49, 130])
@pytest.mark.parametrize("I", [16, 80])
def test_swiglu_epilogue_is_swiglu_of_the_plain_products(I, M):
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(I + M)
    x, wg, wu = _randn(g, M, 320), _randn(g, I, 320) * 0.1, _randn(g, I, 320) * 0.1
    gate, up = F.linear_midm(x, [(wg, None), (wu, None)])
    assert torch.equal(F.swiglu_midm(x, wg, wu), F.swiglu(gate, up))


def test_a_row_does_not_depend_on_its_batch():
    """rows of a 200-row call, alone at M = 1, and at other indices of a 49-row call"""
    from touchnet_amd import functional as F
    x, layers, rope = _rope_case(torch.Generator().manual_seed(4), 200, 64, 4, 1, K=1088)
    y200 = F.linear_midm(x, layers, rope=rope)
    pick = torch.arange(199, 3, -4, device=DEV)[:49]                 # rows 199, 195, .. at indices 0, 1, ..
    y49 = F.linear_midm(x[pick], layers, rope=(rope[0][pick], rope[1][pick], 64, (0, 1)))
    for a, b in zip(y49, y200):
        assert torch.equal(a, b[pick])
    for i in (0, 16, 77, 199):
        one = F.linear_midm(x[i:i + 1], layers, rope=(rope[0][i:i + 1], rope[1][i:i + 1], 64, (0, 1)))
        for a, b in zip(one, y200):
            assert torch.equal(a[0], b[i]), i


@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("M", [49, 129, 256])
def test_fp8_is_the_bf16_kernel_on_the_dequantised_weights(M, K):
    """The FP8 chunk is 128 deep and the bf16 chunk 64, so the two forms group the K terms into different MFMAs: they are
    equal bit for bit where the fp32 sums are exact.  x in {-1, 0, 1}; weights: the exact codes (multiples of 2^-9 up to 8:
    sums below 2^14), and quantised randn weights (codes are multiples of 2^-9 up to 448, a row's sums stay some 2^12 —
    far below the 2^15 at which a multiple of 2^-9 stops being an fp32).  The row scale, a power of two, and the bias come
    behind the sum in both forms."""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(M + K)
    x = _ints(g, -1, 1, M, K)
    qs = [_fp8(g, 48, K), _fp8(g, 80, K), F.quantize_weight_fp8(_randn(g, 80, K))]
    bs = [_randn(g, 48), None, None]
    deq = [F.dequantize_weight_fp8(q) for q in qs]
    for a, b in zip(F.linear_midm_fp8(x, list(zip(qs, bs))), F.linear_midm(x, list(zip(deq, bs)))):
        assert torch.equal(a, b)
    assert torch.equal(F.swiglu_midm_fp8(x, qs[1], qs[2]), F.swiglu_midm(x, deq[1], deq[2]))


@pytest.mark.parametrize("case", ["M=0", "M=257", "K=96", "K=192 fp8", "N=24", "fp32", "misaligned"])
def test_refusals_by_name_and_by_code_before_any_launch(case):
    """`functional` raises by name; the C entries return -22 and leave the output alone (they take no dtype: the fp32 case is
    functional's alone).  K = 192 is a refusal of the FP8 entries only."""
    from touchnet_amd import _C, functional as F
    M, K, N = {"M=0": (0, 128, 16), "M=257": (257, 128, 16), "K=96": (16, 96, 16), "K=192 fp8": (16, 192, 16),
               "N=24": (16, 128, 24)}.get(case, (16, 128, 16))
    x = torch.ones(M * K + 8, dtype=torch.float32 if case == "fp32" else torch.bfloat16, device=DEV)
    x = x[1:M * K + 1].view(M, K) if case == "misaligned" else x[:M * K].view(M, K)
    w = torch.ones(N, K, dtype=torch.bfloat16, device=DEV)
    q = F.Fp8Weight(torch.zeros(N, K, dtype=torch.uint8, device=DEV), torch.ones(N, device=DEV))
    if case != "K=192 fp8":
        with pytest.raises(_C.KernelError, match="linear_midm"):
            F.linear_midm(x, [(w, None)])
        with pytest.raises(_C.KernelError, match="swiglu_midm"):
            F.swiglu_midm(x, w, w)
    with pytest.raises(_C.KernelError, match="linear_midm_fp8"):
        F.linear_midm_fp8(x, [(q, None)])
    with pytest.raises(_C.KernelError, match="swiglu_midm_fp8"):
        F.swiglu_midm_fp8(x, q, q)
    if case != "fp32":
        y = torch.full((max(M, 1), N), SENTINEL, dtype=torch.int16, device=DEV)
        one = lambda t, v: (t * 1)(v)
        lin = (x.data_ptr(), K, M, K, 1)
        out = (None, one(C.c_void_p, y.data_ptr()), one(C.c_longlong, N), one(C.c_int, N), None, None, 0, 0, None)
        lib, s = _C.lib(), q.scale.data_ptr()
        rcs = [lib.tn_gemm_midm_fp8(*lin, one(C.c_void_p, q.codes.data_ptr()), one(C.c_longlong, K), one(C.c_void_p, s), *out),
               lib.tn_gemm_midm_swiglu_fp8(x.data_ptr(), q.codes.data_ptr(), q.codes.data_ptr(), s, s, y.data_ptr(), M, N, K,
                                           K, K, N, None)]
        if case != "K=192 fp8":
            rcs += [lib.tn_gemm_midm(*lin, one(C.c_void_p, w.data_ptr()), one(C.c_longlong, K), *out),
                    lib.tn_gemm_midm_swiglu(x.data_ptr(), w.data_ptr(), w.data_ptr(), y.data_ptr(), M, N, K, K, K, N, None)]
        torch.cuda.synchronize()
        assert all(rc == -22 for rc in rcs) and bool((y == SENTINEL).all())


def test_an_fp8_extend_of_130_rows_runs_on_the_kernel_without_dequantising(monkeypatch):
    """Two sequences of 70 and 60 new rows behind empty prefixes, FP8 weights: every product (and lm_head on all 130 rows)
    runs on the mid-M kernel — `dequantize_weight_fp8` raises if asked — and the logits agree with the bf16 path on the
    dequantised weights within the decoders' summation-order bound 3e-2 max|logit|.  (The bf16 route of TN_DECODE_GEMM=own
    stays at 48 rows — DESIGN.md §9.14 —, so there is no 60-row decode step on this kernel to compare.)"""
    from test_gemm_smallm_gpu import _tiny
    from touchnet_amd import _C, functional as F, generation as G
    model, _ = _tiny("qwen2", seed=12)
    ref = copy.deepcopy(model)
    assert G.quantize_decoder_weights(model) > 0
    for name, m in model.named_modules():
        if isinstance(m, G.Fp8Linear):
            ref.get_submodule(name).weight = torch.nn.Parameter(F.dequantize_weight_fp8(m.weight))
    g = torch.Generator().manual_seed(7)
    ids = [torch.randint(4, 640, (n,), generator=g) for n in (70, 60)]
    logits = {}
    with torch.no_grad():
        for arm, m in (("bf16", ref), ("fp8", model)):
            lm, _ = G._parts(m)
            c = lm.config
            cache = G.KVCache.allocate(len(lm.model.layers), 2, 80, c.num_key_value_heads, c.head_dim, DEV)
            if arm == "fp8":
                def refuse(w):
                    raise _C.KernelError("dequantize_weight_fp8 called")
                monkeypatch.setattr(F, "dequantize_weight_fp8", refuse)
            h = G.extend(m, cache, [0, 1], ids, keep_rows=range(130), prefix_len=[0, 0])
            logits[arm] = F.linear_group(h, [(lm.lm_head.weight, lm.lm_head.bias)])[0].float()
    diff, top = float((logits["fp8"] - logits["bf16"]).abs().max()), float(logits["bf16"].abs().max())
    print(f"max|fp8 - bf16| = {diff:.4g}, max|bf16| = {top:.4g}")
    assert logits["fp8"].shape == (130, 640) and diff <= 3e-2 * top
