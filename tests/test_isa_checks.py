"""Compile-time (CPU, hipcc cross-compiles gfx950) checks on the generated ISA of kernels whose speed depends on a
compiler behaviour that the source cannot express."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_attention_stage_loops_are_not_serialised_by_alias_waits():
    """The LDS-DMA stage rings of the dK/dV, dQ and stream forward kernels rely on counted vmcnt waits.  hipcc inserts a
    full `s_waitcnt vmcnt(0)` in front of LDS reads without alias metadata while a DMA is pending (attn_common.h,
    i32x4_t): the check fails if such a wait appears in front of a row-operand read inside the stage
    loops, or if the set of stage-loop kernels it inspected is not exactly the attention's seven."""
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "check_dma_waits.sh")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    hits = {}                       # "kernel<template args>" -> alias waits found in its stage loop
    for line in r.stdout.splitlines():
        m = re.match(r"_ZN2tn\d+(attn_\w+?_kernel)I((?:Li\d+E)+)E\S*: (\d+) vmcnt", line)
        if m:
            hits[m.group(1) + "<" + ",".join(re.findall(r"Li(\d+)E", m.group(2))) + ">"] = int(m.group(3))
    # every stage-loop kernel of the attention, each with no hit
    assert hits == {"attn_bwd_kv_kernel<128,0>": 0, "attn_bwd_kv_kernel<128,1>": 0, "attn_bwd_kv_kernel<64,2>": 0,
                    "attn_bwd_dq_stream_kernel<128>": 0, "attn_bwd_dq_stream_kernel<64>": 0,
                    "attn_fwd_stream_kernel<128>": 0, "attn_fwd_stream_kernel<64>": 0}, r.stdout


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_gemm_library_holds_exactly_the_kernels_the_product_launches(tmp_path):
    """csrc/gemm.hip compiled with the library's own flags holds the 21 kernels `launch` and the fused entry points reach,
    no development variant beside them, and none of them spills a vector register or uses scratch.  (SGPR spills are not
    zero — up to 14 per kernel — and are not asserted.)"""
    import itertools

    from touchnet_amd import build
    out = tmp_path / "gemm.s"
    r = subprocess.run(["hipcc", *build.FLAGS, "-S", "--cuda-device-only",
                        os.path.join(ROOT, "touchnet_amd", "csrc", "gemm.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    text = out.read_text()
    PLAIN, GROUPED, SWIGLU_FWD, SWIGLU_BWD, BIASG, ROPE, GELU_FWD, GELU_BWD = range(8)      # csrc/gemm.hip EPI_*
    ROW, KMAJ = 0, 1
    b = lambda *flags: "".join(f"Lb{int(f)}E" for f in flags)
    # gemm16_kernel<AK, BK, EPI>: row-stored A, forward (B row-stored) and input-gradient (B contraction-major) products
    want = {f"_ZN2tn4gemm13gemm16_kernelI{b(ROW, bk)}Li{epi}EEEvNS0_6ParamsE"
            for bk, epi in [(ROW, PLAIN), (ROW, SWIGLU_FWD), (ROW, ROPE), (ROW, GELU_FWD),
                            (KMAJ, PLAIN), (KMAJ, SWIGLU_BWD), (KMAJ, GELU_BWD)]}
    # gemm_kernel<AK, BK, HAS_CT, SPLITK, OUT_F32, EPI>
    CT, SPLITK, NONE = (1, 0), (0, 1), (0, 0)
    modes = [(ROW, bk, *m, 0, PLAIN) for bk in (ROW, KMAJ) for m in (CT, SPLITK)]                       # 4
    modes += [(KMAJ, KMAJ, *NONE, f32, epi) for epi, f32 in itertools.product((PLAIN, GROUPED, BIASG), (0, 1))]   # 6
    modes += [(KMAJ, KMAJ, *SPLITK, 0, PLAIN), (KMAJ, KMAJ, *SPLITK, 0, BIASG), (KMAJ, KMAJ, *CT, 0, PLAIN)]      # 3
    want |= {f"_ZN2tn4gemm11gemm_kernelI{b(*m[:5])}Li{m[5]}EEEvNS0_6ParamsE" for m in modes}
    want.add("_ZN2tn4gemm20splitk_reduce_kernelEPKfiiiiiiiPtxPKtiiS2_S3_")
    assert len(want) == 21
    meta = text[text.find("amdhsa.kernels"):]
    found = {}
    for ent in meta.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", ent).group(1)
        found[name] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", ent).group(1)),
                       int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", ent).group(1)))
    assert set(found) == want, (sorted(set(found) - want), sorted(want - set(found)))
    assert all(v == (0, 0) for v in found.values()), {k: v for k, v in found.items() if v != (0, 0)}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_fused_dkdv_accumulators_and_stage_ring(tmp_path):
    """csrc/attn_bwd_fused.hip keeps dK^T / dV^T in the LITERAL registers a[0:127] at one wave per SIMD and runs every
    MFMA as inline asm.  Sound only while hipcc never touches the accumulator file (no spill, no scratch, every
    v_accvgpr_* and v_mfma inside an asm region, < 256 VGPRs of its own), and fast only while the stage loop keeps the
    counted vmcnt(5) wait of the four-slot LDS-DMA ring and no compiler-inserted vmcnt(0)."""
    import re
    out = tmp_path / "fused.s"
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result", "-S",
                        "--cuda-device-only", os.path.join(ROOT, "touchnet_amd", "csrc", "attn_bwd_fused.hip"),
                        "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    text = out.read_text()
    m = re.search(r"^(_ZN2tn24attn_bwd_kv_fused_kernel\S*):(.*?)s_endpgm", text, re.S | re.M)
    assert m
    body = m.group(2)
    in_asm, mine, theirs, mfma_in, mfma_out = False, 0, [], 0, 0
    for line in body.split("\n"):
        t = line.strip()
        if t.startswith(";;#ASMSTART") or t.startswith(";#ASMSTART"):
            in_asm = True
        elif t.startswith(";;#ASMEND") or t.startswith(";#ASMEND"):
            in_asm = False
        elif t.startswith("v_accvgpr"):
            if in_asm:
                mine += 1
            else:
                theirs.append(t)
        elif t.startswith("v_mfma"):
            mfma_in, mfma_out = mfma_in + in_asm, mfma_out + (not in_asm)
        assert not t.startswith("scratch_"), t
    # 128 zeroing writes + 128 epilogue reads; five loop-trip variants with MFMAs (32 + 32 + 16 + 16 + 16)
    assert mfma_out == 0 and mine == 256 and mfma_in == 112, (mine, mfma_in, mfma_out)
    # hipcc may park a few of its own values in accumulator registers ABOVE the literal block a[0:127] (outside the stage
    # loop: checked below), never inside it
    for t in theirs:
        idx = [int(x) for x in re.findall(r"\ba(\d+)\b", t)]
        assert idx and all(i >= 128 for i in idx), t
    meta = re.search(r"\.agpr_count:\s+(\d+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
                     r".*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    assert meta, "kernel metadata not found"
    agpr, priv, vgpr, spill = map(int, meta.groups())
    assert 128 <= agpr <= 136 and priv == 0 and spill == 0 and vgpr - agpr <= 256, (agpr, priv, vgpr, spill)
    # the stage loop = the innermost loop holding the barriers of the loop trips
    ins = [l.strip() for l in body.split("\n") if l.strip() and not l.strip().startswith(";")]
    labels = {mm.group(1): i for i, l in enumerate(ins) for mm in [re.match(r"(\.LBB\d+_\d+):", l)] if mm}
    loops = []
    for i, l in enumerate(ins):
        mm = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if mm and labels.get(mm.group(1), len(ins)) < i:
            seg = ins[labels[mm.group(1)]:i + 1]
            if sum(x.startswith("v_mfma") for x in seg) == 112:
                loops.append(seg)
    assert loops, "stage loop not found"
    seg = min(loops, key=len)
    vm = [x for x in seg if x.startswith("s_waitcnt") and "vmcnt" in x]
    assert vm == ["s_waitcnt vmcnt(5)"] * 6, vm          # one counted wait per trip variant, nothing else
    # no SGPR spill traffic and none of hipcc's parked accumulator values inside the loop
    assert not any(x.startswith(("v_readlane", "v_writelane")) for x in seg)
    assert sum(x.startswith("v_accvgpr") for x in seg) == 0
    assert sum(x.startswith("v_pk_") for x in seg) == 0, "packed f32 VALU beside the MFMAs (see the kernel's ds_elem)"


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_product_gemm_kernels_keep_their_stage_loops_clean(tmp_path):
    """Every instantiation of the product GEMM (csrc/gemm.hip: `gemm_kernel` with its epilogue modes — plain, grouped, bias
    gradient — and `gemm16_kernel`, the 16x16x32 kernel, plain and with the SwiGLU forward / backward, RoPE and GELU epilogues)
    compiled for gfx950: no scratch, no
    VGPR spill (a fused epilogue must not push the main loop out of the register file); each kernel issues ONE MFMA shape;
    and its stage loops hold no `s_waitcnt vmcnt` but the hand-counted `vmcnt(4)` of the five-slot LDS-DMA ring (a
    compiler-inserted one in front of an LDS access would drain the ring every stage)."""
    import re
    out = tmp_path / "gemm.s"
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result", "-S", "--cuda-device-only",
                        os.path.join(ROOT, "touchnet_amd", "csrc", "gemm.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    text = out.read_text()
    kernels = re.findall(r"^(_ZN2tn4gemm(?:11gemm_kernel|13gemm16_kernel)\S*):(.*?)s_endpgm", text, re.S | re.M)
    names = [n for n, _ in kernels]
    # (gemm16: plain x 2 operand modes, SwiGLU forward / backward, RoPE, GELU forward / backward)
    assert sum("gemm16_kernel" in n for n in names) == 7 and sum("11gemm_kernel" in n for n in names) == 13, names
    meta = text[text.find("amdhsa.kernels"):]
    for ent in meta.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", ent).group(1)
        if "gemm" not in name or "splitk_reduce" in name:
            continue
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", ent).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", ent).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", ent).group(1)) <= 256, name
    for name, body in kernels:
        ins = [l.strip() for l in body.split("\n") if l.strip() and not l.strip().startswith(";")]
        m16 = "gemm16_kernel" in name
        shapes = {l.split()[0] for l in ins if l.startswith("v_mfma")}
        assert shapes == ({"v_mfma_f32_16x16x32_bf16"} if m16 else {"v_mfma_f32_32x32x16_bf16"}), (name, shapes)
        per_trip = 64 if m16 else 32
        labels = {m.group(1): i for i, l in enumerate(ins) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
        found = 0
        for i, l in enumerate(ins):
            m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
            if m and labels.get(m.group(1), len(ins)) < i:
                seg = ins[labels[m.group(1)]:i + 1]
                if sum(x.startswith("v_mfma") for x in seg) == per_trip:          # the steady-state stage loop
                    found += 1
                    vm = [x for x in seg if x.startswith("s_waitcnt") and "vmcnt" in x]
                    assert vm == ["s_waitcnt vmcnt(4)"], (name, vm)
        assert found == 1, (name, found)
