"""The table-driven grouped weight-gradient launch (csrc/gemm.hip EPI_TABLE, tn_gemm_bf16_grouped_table): any number of
products dW_g = dY_g^T x_g (+ the bias gradient dY_g.sum(0)) as ONE persistent launch over the concatenation of their tile
lists.  Held BIT FOR BIT to the unsplit single-product launches it replaces, to an fp64 product of the same bf16 inputs with
the bounds tests/test_gemm_fused_gpu.py uses for the weight-gradient mode, and to itself (a second launch)."""
import ctypes as C

import pytest
import torch

DEV = "cuda"

# (M, N, K, bias gradient?): one tile / ragged edges / more than one tile row and column; a depth below one 64-deep stage, one
# that is no multiple of 64 (the descriptor zero-fills the last stage), differing depths inside one launch; products with
# and without a bias gradient interleaved.  24 tiles: every workgroup has one.
SEVEN = [(8, 8, 8, True), (136, 264, 200, False), (520, 256, 1024, True), (264, 520, 1032, False), (256, 136, 200, True),
         (520, 520, 1032, True), (8, 264, 1024, False)]
# 40 products (more than one chunk of the table's upload) of 9 tiles each = 360 tiles on 256 CUs: persistent workgroups walk
# from one product into the next, across differing depths, and meet tiles with and without column sums
FORTY = [(520, 520, 72 if i % 2 else 200, i % 3 != 1) for i in range(40)]


def _f():
    import touchnet_amd.functional as F
    return F


def _r(g, *shape, scale=1.0):
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(torch.bfloat16).to(DEV)


def _pitched(t, pad=8):
    """the same values in a buffer whose rows are `pad` elements longer (a pitch larger than the row)"""
    big = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("products", [SEVEN, FORTY], ids=["seven_mixed", "forty_persistent"])
def test_table_launch_equals_the_unsplit_single_products(products, f32, accumulate, monkeypatch):
    F = _f()
    monkeypatch.setattr(F, "SPLIT_K", False)                  # the single-product reference: always the unsplit launch
    g = torch.Generator().manual_seed(len(products) + 2 * f32 + accumulate)
    odt = torch.float32 if f32 else torch.bfloat16
    pairs, init, biased = [], [], []
    for i, (M, N, K, bias) in enumerate(products):
        dy, x = _r(g, K, M), _r(g, K, N)
        dy[:, :8] += 0.5                                      # (a non-zero mean: the column sums are not just noise)
        if i % 2:                                             # every other product: pitches larger than the row
            dy, x = _pitched(dy), _pitched(x, 16)
        pairs.append((dy, x))
        c0 = (torch.rand(M, N, generator=g) - 0.5).to(odt).to(DEV)
        init.append(_pitched(c0, 8) if i % 2 else c0)
        biased.append(bias)

    def fresh():
        outs = []
        for c0 in init:
            if c0.stride(0) != c0.shape[1]:
                o = _pitched(c0.contiguous(), c0.stride(0) - c0.shape[1])
            else:
                o = c0.clone()
            outs.append(o if accumulate else o.fill_(float("nan")))
        return outs

    def nan_bias():
        return [torch.full((M,), float("nan"), dtype=torch.bfloat16, device=DEV) if b else None
                for (M, _, _, _), b in zip(products, biased)]

    outs, bgs = fresh(), nan_bias()
    F.gemm_grouped_table_wgrad(pairs, outs=outs, accumulate=accumulate, bias_grads=bgs)
    # bit equality with the existing unsplit single-product entries, product by product
    refs, rbgs = fresh(), nan_bias()
    for (dy, x), o, bg in zip(pairs, refs, rbgs):
        F.gemm([(dy, x)], True, True, out=o, accumulate=accumulate, bias_grad=bg)
    for i, (o, r, bg, rbg) in enumerate(zip(outs, refs, bgs, rbgs)):
        assert not torch.isnan(o).any(), i
        assert torch.equal(o, r), (i, products[i])
        if bg is not None:
            assert not torch.isnan(bg).any(), i
            assert torch.equal(bg, rbg), (i, products[i])
    # fp64 product of the same bf16 inputs, the bounds of tests/test_gemm_fused_gpu.py: 2^-7 of the largest value for bf16
    # outputs, 2e-5 for fp32 outputs written, 1e-3 for fp32 outputs added to; the column sums as its bias-gradient test
    for i, ((dy, x), o, c0, bg) in enumerate(zip(pairs, outs, init, bgs)):
        ref = dy.double().t() @ x.double() + (c0.double() if accumulate else 0.0)
        bound = float(ref.abs().max()) * ((1e-3 if accumulate else 2e-5) if f32 else 2 ** -7)
        err = float((o.double() - ref).abs().max())
        assert err <= bound, (i, products[i], err, bound)
        if bg is not None:
            rb = dy.double().sum(0)
            tol = 2.0 ** -8 * rb.abs().clamp_min(1.0) + 1e-3 * dy.shape[0] ** 0.5
            assert ((bg.double() - rb).abs() <= tol).all(), (i, float((bg.double() - rb).abs().max()))
    # a second identical launch: identical bits
    again, abgs = fresh(), nan_bias()
    F.gemm_grouped_table_wgrad(pairs, outs=again, accumulate=accumulate, bias_grads=abgs)
    assert all(torch.equal(a, b) for a, b in zip(again, outs))
    assert all(torch.equal(a, b) for a, b in zip(abgs, bgs) if a is not None)


def test_table_entry_refuses_malformed_arguments_before_any_launch():
    """Host only: the checks of tn_gemm_bf16_grouped_table answer TN_EINVAL (-22) without touching the device, so host
    addresses that are never dereferenced will do."""
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    EINVAL = -22
    raw = (C.c_char * 8192)()
    p = (C.addressof(raw) + 255) // 256 * 256
    M, N, K = 264, 520, 200
    limit = 1024
    assert lib.tn_gemm_grouped_table_bytes(limit) > 0 and lib.tn_gemm_grouped_table_bytes(limit + 1) == -1
    assert lib.tn_gemm_grouped_table_bytes(0) == -1

    def call(n=1, c=p, m=M, table=p, table_bytes=1 << 20, count=None):
        k = count if count is not None else max(n, 1)
        arr = lambda t, v: (t * k)(*([v] * k))
        return lib.tn_gemm_bf16_grouped_table(arr(C.c_void_p, p), arr(C.c_void_p, p), arr(C.c_longlong, M + 8), arr(C.c_longlong, N),
                                              arr(C.c_int, K), arr(C.c_void_p, c), arr(C.c_longlong, N), arr(C.c_int, m),
                                              arr(C.c_int, N), arr(C.c_void_p, None), n, 0, 0, table, table_bytes, None)
    assert call(n=0) == EINVAL
    assert call(n=limit + 1, count=limit + 1) == EINVAL                  # over the limit
    assert call(c=p + 2) == EINVAL                                       # a misaligned C
    assert call(m=M + 4) == EINVAL                                       # M % 8 != 0
    assert call(table=None) == EINVAL                                    # no table buffer
    assert call(table=p + 8) == EINVAL                                   # ... a misaligned one
    assert call(n=3, table_bytes=lib.tn_gemm_grouped_table_bytes(3) - 1) == EINVAL   # ... one a byte short
