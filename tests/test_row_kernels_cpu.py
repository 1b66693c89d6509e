"""What the row-kernel and optimizer entry points (csrc/norm_act.hip, csrc/optim.hip; contracts in
include/touchnet_amd.h) must refuse WITHOUT the device.  Their kernels trust the shapes they are launched with — a
negative element count becomes a vector count near 2^61, a width of zero a division by it — so a shape they cannot
serve must return -22 before anything is launched.

Only refused calls are made here.  The addresses are host memory, never dereferenced by a refused call."""
import ctypes as C

import pytest

EINVAL = -22
F32, BF16 = 0, 1
VEC = {F32: 4, BF16: 8}                 # elements of a 16-byte vector
WIDEST = {F32: 4096, BF16: 8192}        # widest row of the norm kernels


@pytest.fixture(scope="module")
def env():
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    raw = (C.c_char * 8192)()
    p = (C.addressof(raw) + 255) // 256 * 256
    return lib, p, raw                  # (`raw` is kept alive by the fixture)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_elementwise_entries_refuse_counts_they_cannot_serve(env, dtype):
    lib, p, _ = env
    N = VEC[dtype]
    for n in (-N, -1, -2 ** 40, 1, N - 1, N + 1, 3 * N + N // 2):
        assert lib.tn_swiglu_fwd(p, p, p, n, dtype, None) == EINVAL, n
        assert lib.tn_swiglu_bwd(p, p, p, p, p, n, dtype, None) == EINVAL, n
        assert lib.tn_gelu_fwd(p, p, n, dtype, None) == EINVAL, n
        assert lib.tn_gelu_bwd(p, p, p, n, dtype, None) == EINVAL, n


@pytest.mark.parametrize("code", [-1, 2, 7])
def test_unknown_dtype_codes_are_refused(env, code):
    lib, p, _ = env
    assert lib.tn_swiglu_fwd(p, p, p, 64, code, None) == EINVAL
    assert lib.tn_swiglu_bwd(p, p, p, p, p, 64, code, None) == EINVAL
    assert lib.tn_gelu_fwd(p, p, 64, code, None) == EINVAL
    assert lib.tn_gelu_bwd(p, p, p, 64, code, None) == EINVAL
    assert lib.tn_rmsnorm_fwd(p, p, p, p, p, p, 4, 64, 1e-5, code, None) == EINVAL
    assert lib.tn_rmsnorm_bwd(p, p, p, p, p, p, p, p, 4, 64, code, None) == EINVAL
    assert lib.tn_layernorm_fwd(p, p, p, p, p, p, p, p, 4, 64, 1e-5, code, None) == EINVAL
    assert lib.tn_layernorm_bwd(p, p, p, p, p, p, p, p, p, p, 4, 64, code, None) == EINVAL
    assert lib.tn_rope_table(p, p, p, p, 4, 8, 1.0, code, None) == EINVAL
    assert lib.tn_rope_apply(p, p, p, p, p, p, 4, 2, 2, 16, 0, code, None) == EINVAL
    assert lib.tn_sumsq(p, p, p, 64, code, None) == EINVAL
    assert lib.tn_adamw_step(p, p, p, p, p, p, 64, 1e-3, 0.9, 0.95, 1e-8, 0.1, 1.0, 0.1, 0.05, code, None) == EINVAL
    assert lib.tn_sumsq_multi(p, p, p, 1, 1, p, p, code, None) == EINVAL
    assert lib.tn_adamw_multi(p, p, p, p, p, p, p, 1, 1, p, 1e-3, 0.9, 0.95, 1e-8, 0.1, code, None) == EINVAL
    assert lib.tn_adamw_multi_bounded(p, p, p, p, p, p, p, 1, 1, p, 1e-3, 0.9, 0.95, 1e-8, 0.1, code, 0, None) == EINVAL


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_norm_entries_refuse_shapes_they_cannot_serve(env, dtype):
    """forward and backward separately: they pick their instantiation by different rules (a wave per row / a workgroup
    per row)"""
    lib, p, _ = env
    N, top = VEC[dtype], WIDEST[dtype]
    shapes = [(0, 64), (-1, 64), (-2 ** 31, 64),                               # rows <= 0
              (4, 0), (4, -N), (4, -64), (4, -2 ** 31),                         # H <= 0
              (4, N - 1), (4, N + 1), (4, 64 + N // 2), (4, top - 1),           # H no multiple of the vector
              (4, top + N), (4, 2 * top), (4, 2 ** 30)]                         # wider than the widest instantiation
    for rows, H in shapes:
        assert lib.tn_rmsnorm_fwd(p, p, p, p, p, p, rows, H, 1e-5, dtype, None) == EINVAL, (rows, H)
        assert lib.tn_rmsnorm_fwd(p, None, p, p, None, p, rows, H, 1e-5, dtype, None) == EINVAL, (rows, H)
        assert lib.tn_rmsnorm_bwd(p, p, p, p, p, p, p, p, rows, H, dtype, None) == EINVAL, (rows, H)
        assert lib.tn_layernorm_fwd(p, p, p, p, p, p, p, p, rows, H, 1e-5, dtype, None) == EINVAL, (rows, H)
        assert lib.tn_layernorm_bwd(p, p, p, p, p, p, p, p, p, p, rows, H, dtype, None) == EINVAL, (rows, H)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_rope_entries_refuse_shapes_they_cannot_serve(env, dtype):
    lib, p, _ = env
    for n, hq, hk, D in [(0, 4, 2, 64), (-5, 4, 2, 64), (5, 0, 2, 64), (5, -4, 2, 64), (5, 4, -1, 64), (5, 4, -6, 64),
                         (5, 4, 2, 0), (5, 4, 2, -64), (5, 4, 2, 63), (5, 4, 2, 1), (5, 4, 2, 17)]:
        for backward in (0, 1):
            assert lib.tn_rope_apply(p, p, p, p, p, p, n, hq, hk, D, backward, dtype, None) == EINVAL, (n, hq, hk, D)
    for n, half in [(0, 32), (-3, 32), (5, 0), (5, -32), (-2 ** 31, 4), (4, -2 ** 31)]:
        assert lib.tn_rope_table(p, p, p, p, n, half, 1.0, dtype, None) == EINVAL, (n, half)


def test_transposing_swiglu_entries_refuse_shapes_they_cannot_serve(env):
    lib, p, _ = env
    for rows, cols in [(0, 64), (64, 0), (-8, 64), (64, -8), (-64, -64), (4, 64), (64, 4), (12, 64), (64, 100),
                       (63, 64), (64, 65), (7, 7)]:
        assert lib.tn_swiglu_fwd_t(p, p, p, p, rows, cols, None) == EINVAL, (rows, cols)
        assert lib.tn_swiglu_bwd_t(p, p, p, p, p, p, rows, cols, None) == EINVAL, (rows, cols)


def test_column_sum_refuses_every_rule_of_its_guard(env):
    lib, p, _ = env
    bad = {"no rows": (p, 0, 64, 64), "negative rows": (p, -4, 64, 64), "no columns": (p, 4, 0, 64),
           "negative columns": (p, 4, -8, 64), "columns no multiple of 8": (p, 4, 60, 64),
           "pitch no multiple of 8": (p, 4, 64, 68), "pitch below the columns": (p, 4, 64, 56),
           "a negative pitch": (p, 4, 64, -64), "x off a 16-byte boundary": (p + 8, 4, 64, 64),
           "x two bytes off": (p + 2, 4, 64, 64)}
    for what, (x, rows, cols, ld) in bad.items():
        assert lib.tn_colsum_bf16(x, p, p, rows, cols, ld, None) == EINVAL, what


def test_optimizer_entries_refuse_what_they_cannot_serve(env):
    lib, p, _ = env
    hyper = (1e-3, 0.9, 0.95, 1e-8, 0.1)
    for dtype in (F32, BF16):
        for n in (0, -1, -8, -2 ** 40):
            assert lib.tn_sumsq(p, p, p, n, dtype, None) == EINVAL, n
            assert lib.tn_adamw_step(p, p, p, p, p, p, n, *hyper, 1.0, 0.1, 0.05, dtype, None) == EINVAL, n
            assert lib.tn_adamw_step(p, p, p, p, None, None, n, *hyper, 0.0, 0.1, 0.05, dtype, None) == EINVAL, n
        for ntensors, nchunks in [(0, 1), (-1, 1), (1, 0), (1, -1), (0, 0), (1, 2 ** 31)]:
            assert lib.tn_sumsq_multi(p, p, p, ntensors, nchunks, p, p, dtype, None) == EINVAL, (ntensors, nchunks)
            assert lib.tn_adamw_multi(p, p, p, p, p, p, p, ntensors, nchunks, p, *hyper, dtype, None) == EINVAL
            for bound in (0, 3):
                assert lib.tn_adamw_multi_bounded(p, p, p, p, p, p, p, ntensors, nchunks, p, *hyper, dtype, bound,
                                                  None) == EINVAL, (ntensors, nchunks, bound)
        assert lib.tn_adamw_multi(p, p, p, p, p, p, p, 1, 1, None, *hyper, dtype, None) == EINVAL, "NULL state"
        assert lib.tn_adamw_multi_bounded(p, p, p, p, p, p, p, 1, 1, None, *hyper, dtype, 0, None) == EINVAL
        for bound in (-1, -128, -2 ** 31):
            assert lib.tn_adamw_multi_bounded(p, p, p, p, p, p, p, 1, 1, p, *hyper, dtype, bound, None) == EINVAL, bound
    assert lib.tn_adamw_prepare(p, None, 0.9, 0.95, 1.0, None) == EINVAL, "NULL state"
    assert lib.tn_adamw_prepare(None, None, 0.9, 0.95, 1.0, None) == EINVAL
