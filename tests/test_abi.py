"""The C-ABI library builds for gfx950, loads on a host without a GPU, and exports every symbol that
include/touchnet_amd.h declares; the ctypes stub covers exactly that set (no compute calls here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "touchnet_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_header_symbols():
    from touchnet_amd import build
    lib_path = build.build()
    assert os.path.exists(lib_path)
    from touchnet_amd import _C
    lib = _C.lib()
    syms = _header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/touchnet_amd.h but not exported"
    assert set(_C.PROTOTYPES) == set(syms), set(_C.PROTOTYPES) ^ set(syms)
    assert "gfx950" in _C.version()


def test_every_entry_point_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "touchnet_amd.h")).read()
    for needle in ("touchnet/loss/cross_entropy.py", "touchnet/data/functions.py", "flex_attention.py",
                   "touchnet/utils/optimizer.py", "modeling_llama.py"):
        assert needle in text


def test_product_never_imports_oracle():
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, "touchnet_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
                    bad.append(os.path.join(d, f))
    assert not bad, bad


def test_gemm_tuning_replay_env(monkeypatch, tmp_path):
    """gemm_tuning.enable(): replay mode by default (tuning OFF, one results file per device ordinal), untouched when
    the user configured TunableOp, opt-in tuning of new shapes into a caller-chosen directory."""
    import os

    from touchnet_amd.utils import gemm_tuning
    for k in [k for k in os.environ if k.startswith("PYTORCH_TUNABLEOP") or k.startswith("TN_TUNE")]:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("TN_RECORD_UNTUNED", raising=False)
    assert os.path.exists(gemm_tuning.RESULTS)
    lines = open(gemm_tuning.RESULTS).read().splitlines()
    keys = [tuple(ln.split(",")[:2]) for ln in lines if not ln.startswith("Validator")]
    assert len(keys) == len(set(keys)), "duplicate GEMM entries in the replay table"
    assert gemm_tuning.enable() is True
    assert os.environ["PYTORCH_TUNABLEOP_ENABLED"] == "1" and os.environ["PYTORCH_TUNABLEOP_TUNING"] == "0"
    d = os.path.dirname(os.environ["PYTORCH_TUNABLEOP_FILENAME"])
    assert all(os.path.exists(os.path.join(d, f"results{i}.csv")) for i in range(8))
    assert gemm_tuning.enable() is False                       # already configured -> hands off
    for k in [k for k in os.environ if k.startswith("PYTORCH_TUNABLEOP")]:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TN_TUNE_NEW", "1")
    monkeypatch.setenv("TN_TUNE_DIR", str(tmp_path / "tune"))
    assert gemm_tuning.enable() is True and os.environ["PYTORCH_TUNABLEOP_TUNING"] == "1"
    assert os.environ["PYTORCH_TUNABLEOP_FILENAME"].startswith(str(tmp_path / "tune"))


def test_round5_gemm_entry_points_refuse_malformed_arguments_before_any_launch():
    """The fused-epilogue / grouped GEMM entry points (include/touchnet_amd.h) check shapes, strides and alignment on the host
    and return TN_EINVAL (-22) without touching the device — so the checks can be exercised on a box with no GPU.  (Valid calls
    are the `-m gpu` tests' business: tests/test_gemm_fused_gpu.py.)"""
    import ctypes as C
    from touchnet_amd import _C
    lib = _C.lib()
    EINVAL = -22
    raw = (C.c_char * 8192)()
    p = (C.addressof(raw) + 255) // 256 * 256            # a 256-byte-aligned host address: never dereferenced by a refused call
    odd = p + 2                                          # not 16-byte aligned
    H, I, M = 4096, 11008, 256
    # SwiGLU forward: K not a multiple of 64, an output stride shorter than a row, a misaligned operand
    ok = dict(M=M, I=I, K=H, ldx=H, ldw=H, ldc=I)
    def swiglu_fwd(x=p, **kw):
        a = {**ok, **kw}
        return lib.tn_gemm_bf16_swiglu_fwd(x, p, p, p, p, p, a["M"], a["I"], a["K"], a["ldx"], a["ldw"], a["ldc"], None)
    assert swiglu_fwd(K=H + 32) == EINVAL
    assert swiglu_fwd(ldc=I - 8) == EINVAL
    assert swiglu_fwd(M=0) == EINVAL
    assert swiglu_fwd(x=odd) == EINVAL
    assert swiglu_fwd(ldx=H - 64) == EINVAL and swiglu_fwd(ldw=H - 64) == EINVAL     # a row pitch below the contraction
    # SwiGLU backward
    assert lib.tn_gemm_bf16_swiglu_bwd(p, p, p, p, p, p, M, I, H + 8, I, I, I, None) == EINVAL
    assert lib.tn_gemm_bf16_swiglu_bwd(p, p, p, p, p, p, M, I, H, I, I, I - 8, None) == EINVAL
    assert lib.tn_gemm_bf16_swiglu_bwd(odd, p, p, p, p, p, M, I, H, I, I, I, None) == EINVAL
    assert lib.tn_gemm_bf16_swiglu_bwd(p, p, p, p, p, p, M, I, H, H - 64, I, I, None) == EINVAL      # dY pitch below H
    # RoPE epilogue: head_dim other than 64 / 128, N not a whole number of heads, no tables
    assert lib.tn_gemm_bf16_rope(p, p, None, p, p, p, M, 4096, H, H, H, 4096, 96, None) == EINVAL
    assert lib.tn_gemm_bf16_rope(p, p, None, p, p, p, M, 4096 + 128, H, H, H, 4096 + 128, 128, None) == EINVAL
    assert lib.tn_gemm_bf16_rope(p, p, None, None, None, p, M, 4096, H, H, H, 4096, 128, None) == EINVAL
    assert lib.tn_gemm_bf16_rope(p, p, None, p, p, p, M, 4096, H, H - 64, H, 4096, 128, None) == EINVAL
    assert lib.tn_gemm_bf16_rope(p, p, None, p, p, p, M, 4096, H, H, H - 64, 4096, 128, None) == EINVAL
    # weight gradient + bias gradient without a bias buffer
    assert lib.tn_gemm_bf16_wgrad_bias(p, p, I, H, M, p, None, I, H, H, 0, 0, 1, None, 0, None) == EINVAL
    # grouped launch: no group, too many groups, a mode other than the weight-gradient one
    arr_p, arr_ll, arr_i = (C.c_void_p * 1)(p), (C.c_longlong * 1)(I), (C.c_int * 1)(M)
    Ns, Ms, ldc = (C.c_int * 1)(H), (C.c_int * 1)(I), (C.c_longlong * 1)(H)
    def grouped(ngrp=1, a_kmaj=1, b_kmaj=1):
        return lib.tn_gemm_bf16_grouped(arr_p, arr_p, arr_ll, (C.c_longlong * 1)(H), arr_i, arr_p, ldc, Ms, Ns, ngrp, a_kmaj,
                                        b_kmaj, 0, 0, None, 0, None)
    assert grouped(ngrp=0) == EINVAL
    assert grouped(ngrp=1000) == EINVAL
    assert grouped(a_kmaj=0) == EINVAL
    arr_ll[0] = I - 8                                    # lda < M: the contraction-major A's rows would overlap
    assert grouped() == EINVAL
    arr_ll[0] = I
    # GELU forward / backward (the audio tower: 1280 -> 5120 -> 1280): a depth that is no multiple of 64, a pitch shorter than
    # the row, a misaligned base, one buffer for both outputs
    D, Fd = 1280, 5120
    ok = dict(x=p, pre=p, act=p + 4096, M=M, N=Fd, K=D, ldx=D, ldw=D, ldc=Fd)
    def gelu_fwd(**kw):
        a = {**ok, **kw}
        return lib.tn_gemm_bf16_gelu_fwd(a["x"], p, p, a["pre"], a["act"], a["M"], a["N"], a["K"], a["ldx"], a["ldw"], a["ldc"], None)
    assert gelu_fwd(K=D + 32) == EINVAL
    assert gelu_fwd(ldx=D - 64) == EINVAL and gelu_fwd(ldw=D - 64) == EINVAL and gelu_fwd(ldc=Fd - 8) == EINVAL
    assert gelu_fwd(x=odd) == EINVAL and gelu_fwd(act=odd) == EINVAL
    assert gelu_fwd(act=p) == EINVAL                                                  # pre == act
    ok = dict(dy=p, M=M, I=Fd, H=D, lddy=D, ldw=Fd, ld=Fd)
    def gelu_bwd(**kw):
        a = {**ok, **kw}
        return lib.tn_gemm_bf16_gelu_bwd(a["dy"], p, p, p, a["M"], a["I"], a["H"], a["lddy"], a["ldw"], a["ld"], None)
    assert gelu_bwd(H=D + 32) == EINVAL
    assert gelu_bwd(lddy=D - 64) == EINVAL and gelu_bwd(ldw=Fd - 8) == EINVAL and gelu_bwd(ld=Fd - 8) == EINVAL
    assert gelu_bwd(dy=odd) == EINVAL
    # the general entry: N not a multiple of 8, A contraction-major beside a row-stored B, a pitch that is no multiple of 8
    one = lambda t, v: (t * 1)(v)
    def general(N=H, a_kmaj=0, b_kmaj=0, lda=H):
        return lib.tn_gemm_bf16(one(C.c_void_p, p), one(C.c_void_p, p), one(C.c_longlong, lda), one(C.c_longlong, H),
                                one(C.c_int, H), 1, a_kmaj, b_kmaj, p, None, None, M, N, N, 0, 0, None)
    assert general(N=H + 4) == EINVAL
    assert general(a_kmaj=1, b_kmaj=0) == EINVAL
    assert general(lda=H + 4) == EINVAL
    # the residual addend may not be the output
    assert lib.tn_gemm_bf16_addend(p, p, H, H, H, 0, 0, p, None, p, H, M, H, H, None) == EINVAL
    # split-K: fewer than two parts, 64 stages of a row-stored operand cut in 3, a workspace one byte short of
    # tn_gemm_splitk_workspace_bytes
    need = lib.tn_gemm_splitk_workspace_bytes(M, H, 4, 0, 0)
    def splitk(parts=4, ws_bytes=need):
        return lib.tn_gemm_bf16_splitk(p, p, H, H, H, 0, 0, p, None, M, H, H, 0, parts, 0, p, ws_bytes, None)
    assert splitk(parts=1) == EINVAL
    assert splitk(parts=3, ws_bytes=need) == EINVAL
    assert splitk(ws_bytes=need - 1) == EINVAL
    # ... whose layout is the header's: parts x tiles x 256 x 256 floats of slabs (+ parts x ceil(M / 256) x 256 floats of
    # partial column sums with a bias gradient); tail_only: the tiles of the last partial round (256 CUs: an MI355X, and what
    # the library assumes where no device is visible)
    assert need == 4 * (1 * 16) * 65536 * 4
    assert lib.tn_gemm_splitk_workspace_bytes(1280, 520, 4, 0, 0) == 4 * (5 * 3) * 65536 * 4
    assert lib.tn_gemm_splitk_workspace_bytes(1280, 520, 4, 1, 0) == (4 * (5 * 3) * 65536 + 4 * 5 * 256) * 4
    assert lib.tn_gemm_splitk_workspace_bytes(1280, 520, 1, 1, 0) == 0
    assert lib.tn_gemm_splitk_workspace_bytes(11008, 4096, 4, 0, 1) == 4 * (43 * 16 % 256) * 65536 * 4      # 688 = 2 rounds + 176
    assert lib.tn_gemm_splitk_workspace_bytes(4096, 4096, 4, 0, 1) == -1       # 256 tiles: a whole round, no remainder
    assert lib.tn_gemm_splitk_workspace_bytes(1280, 520, 4, 0, 1) == -1        # 15 tiles: no whole round


def test_attn_bwd_rope_refuses_missing_or_misaligned_tables_before_any_launch():
    """tn_attn_bwd_rope (round 6: the rotary embedding's backward inside the attention backward) checks its tables and the head
    geometry on the host: TN_EINVAL without touching the device.  (Valid calls: tests/test_kernels_gpu.py, bit-identity with
    tn_attn_bwd + tn_rope_apply.)"""
    import ctypes as C
    from touchnet_amd import _C
    lib = _C.lib()
    EINVAL = -22
    raw = (C.c_char * 4096)()
    p = (C.addressof(raw) + 255) // 256 * 256
    call = lambda cos, sin, D=128, Nh=4, Nkv=4: lib.tn_attn_bwd_rope(p, p, p, p, p, p, p, p, p, p, p, p, 1, 256, Nh, Nkv, D, 0.1,
                                                                     cos, sin, None)
    assert call(None, p) == EINVAL and call(p, None) == EINVAL
    assert call(p + 2, p) == EINVAL and call(p, p + 8) == EINVAL          # 16-byte loads of the table rows
    assert call(p, p, D=96) == EINVAL
    assert call(p, p, Nh=6, Nkv=4) == EINVAL                              # query heads not a multiple of kv heads


def test_row_kernel_entry_points_refuse_by_rule_before_any_launch():
    """Every rule the host layer of csrc/norm_act.hip owns, by name, for every entry point it guards: one launcher checks the
    two norm forwards, one the two backwards, one the four element-wise entries; the transposing SwiGLU, RoPE and column-sum
    entries carry their own guards.  A refused call returns TN_EINVAL (-22) before any launch, so host addresses that are
    never dereferenced will do.  (tests/test_row_kernels_cpu.py sweeps more values per rule; valid calls are the `-m gpu`
    tests' business: tests/test_row_kernels_gpu.py.)  The workspace sizes are the header's layouts, restated here."""
    import ctypes as C
    from touchnet_amd import _C
    lib = _C.lib()
    EINVAL = -22
    raw = (C.c_char * 8192)()
    p = (C.addressof(raw) + 255) // 256 * 256
    F32, BF16 = 0, 1
    table = []                                            # (rule, entry point, return code)

    def norms(rule, rows, H, dtype):
        table.extend([(rule, "tn_rmsnorm_fwd", lib.tn_rmsnorm_fwd(p, p, p, p, p, p, rows, H, 1e-5, dtype, None)),
                      (rule, "tn_rmsnorm_bwd", lib.tn_rmsnorm_bwd(p, p, p, p, p, p, p, p, rows, H, dtype, None)),
                      (rule, "tn_layernorm_fwd", lib.tn_layernorm_fwd(p, p, p, p, p, p, p, p, rows, H, 1e-5, dtype, None)),
                      (rule, "tn_layernorm_bwd", lib.tn_layernorm_bwd(p, p, p, p, p, p, p, p, p, p, rows, H, dtype, None))])

    def elementwise(rule, n, dtype):
        table.extend([(rule, "tn_swiglu_fwd", lib.tn_swiglu_fwd(p, p, p, n, dtype, None)),
                      (rule, "tn_swiglu_bwd", lib.tn_swiglu_bwd(p, p, p, p, p, n, dtype, None)),
                      (rule, "tn_gelu_fwd", lib.tn_gelu_fwd(p, p, n, dtype, None)),
                      (rule, "tn_gelu_bwd", lib.tn_gelu_bwd(p, p, p, n, dtype, None))])

    def transposing(rule, rows, cols):
        table.extend([(rule, "tn_swiglu_fwd_t", lib.tn_swiglu_fwd_t(p, p, p, p, rows, cols, None)),
                      (rule, "tn_swiglu_bwd_t", lib.tn_swiglu_bwd_t(p, p, p, p, p, p, rows, cols, None))])

    for dtype, name, N, widest in ((F32, "fp32", 4, 4096), (BF16, "bf16", 8, 8192)):
        norms(f"rows <= 0 ({name})", 0, 64, dtype)
        norms(f"rows < 0 ({name})", -4, 64, dtype)
        norms(f"H <= 0 ({name})", 4, 0, dtype)
        norms(f"H < 0 ({name})", 4, -64, dtype)
        norms(f"H % {N} ({name})", 4, 64 + N // 2, dtype)
        norms(f"H one vector above the widest row ({name})", 4, widest + N, dtype)
        elementwise(f"n < 0 ({name})", -N, dtype)
        elementwise(f"n % {N} ({name})", 3 * N + N // 2, dtype)
        for rule, (n, hq, hk, D) in {"odd D": (5, 4, 2, 63), "D <= 0": (5, 4, 2, 0), "hq <= 0": (5, 0, 2, 64),
                                     "hk < 0": (5, 4, -1, 64), "n <= 0": (0, 4, 2, 64)}.items():
            table.append((f"{rule} ({name})", "tn_rope_apply", lib.tn_rope_apply(p, p, p, p, p, p, n, hq, hk, D, 0, dtype, None)))
        table.append((f"n <= 0 ({name})", "tn_rope_table", lib.tn_rope_table(p, p, p, p, 0, 32, 1.0, dtype, None)))
        table.append((f"half <= 0 ({name})", "tn_rope_table", lib.tn_rope_table(p, p, p, p, 5, 0, 1.0, dtype, None)))
    norms("an unknown dtype code", 4, 64, 2)
    elementwise("an unknown dtype code", 64, 2)
    table.append(("an unknown dtype code", "tn_rope_apply", lib.tn_rope_apply(p, p, p, p, p, p, 5, 4, 2, 64, 0, 2, None)))
    table.append(("an unknown dtype code", "tn_rope_table", lib.tn_rope_table(p, p, p, p, 5, 32, 1.0, 2, None)))
    transposing("rows % 8", 12, 64)
    transposing("cols % 8", 64, 100)
    transposing("rows <= 0", 0, 64)
    transposing("cols <= 0", 64, 0)
    for rule, (x, rows, cols, ld) in {"rows <= 0": (p, 0, 64, 64), "cols <= 0": (p, 4, 0, 64), "cols % 8": (p, 4, 60, 64),
                                      "ld % 8": (p, 4, 64, 68), "ld < cols": (p, 4, 64, 56),
                                      "x not 16-byte aligned": (p + 8, 4, 64, 64)}.items():
        table.append((rule, "tn_colsum_bf16", lib.tn_colsum_bf16(x, p, p, rows, cols, ld, None)))
    assert len(table) == 102
    accepted = [(rule, entry, rc) for rule, entry, rc in table if rc != EINVAL]
    assert not accepted, accepted

    # norm backward: dw partials, then db partials, one row of H floats per workgroup, a workgroup per row up to 1024;
    # column sum: one row of `cols` floats per slab, about 4096 workgroups of 256 columns, at most 1024 slabs of >= 16 rows
    for rows in (1, 5, 1023, 1024, 1025, 2051, 30000):
        for H in (8, 64, 520, 1280, 4096, 8192):
            assert lib.tn_norm_bwd_workspace_floats(rows, H) == 2 * min(rows, 1024) * H, (rows, H)
            slabs = max(1, min(-(-4096 // -(-H // 256)), 1024, max(rows // 16, 1)))
            assert lib.tn_colsum_workspace_floats(rows, H) == slabs * H, (rows, H)
