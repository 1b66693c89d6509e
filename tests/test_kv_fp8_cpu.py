"""The FP8 KV cache without a device: config keys and refusals, cache shapes / dtypes / bytes, fake-tensor tracing of the
four ops, and a default path that allocates no scale tensors."""
import pytest
import torch

from touchnet_amd import generation as G


@pytest.mark.parametrize("cls", [G.GenerationConfig, G.KimiGenerationConfig])
def test_the_config_key_is_parsed_and_checked(cls):
    assert cls().kv_cache_dtype == "bf16" and cls(kv_cache_dtype="fp8_e4m3").kv_cache_dtype == "fp8_e4m3"
    with pytest.raises(ValueError, match="kv_cache_dtype = 'fp8'"):
        cls(kv_cache_dtype="fp8")


def test_from_hf_and_the_command_lines_pass_the_key_on():
    from touchnet_amd.bin import infer_asr, infer_kimi_audio, infer_qwen2_audio
    assert G.GenerationConfig.from_hf({}).kv_cache_dtype == "bf16"
    assert G.GenerationConfig.from_hf({}, kv_cache_dtype="fp8_e4m3").kv_cache_dtype == "fp8_e4m3"
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        G.GenerationConfig.from_hf({}, kv_cache_dtype="int8")
    base = ["--model_path", "m", "--data_list", "d", "--output_dir", "o"]
    for mod in (infer_asr, infer_qwen2_audio, infer_kimi_audio):
        ap = mod.build_parser()
        assert mod.generation_config(ap.parse_args(base)).kv_cache_dtype == "bf16"
        assert mod.generation_config(ap.parse_args(base + ["--kv_cache_dtype", "fp8_e4m3"])).kv_cache_dtype == "fp8_e4m3"
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--kv_cache_dtype", "fp8"])


@pytest.mark.parametrize("D", [64, 128])
def test_cache_shapes_dtypes_and_bytes(D):
    nbytes = lambda c: sum(t.numel() * t.element_size() for t in c.k + c.v + (c.k_scale or []) + (c.v_scale or []))
    bf = G.KVCache.allocate(2, 3, 10, 4, D, "cpu")
    assert bf.kv_dtype == "bf16" and bf.k_scale is None and bf.v_scale is None and bf.k[0].dtype == torch.bfloat16
    f8 = G.KVCache.allocate(2, 3, 10, 4, D, "cpu", kv_dtype="fp8_e4m3")
    assert f8.kv_dtype == "fp8_e4m3" and len(f8.k_scale) == len(f8.v_scale) == 2
    assert f8.k[1].dtype == f8.v[1].dtype == torch.uint8 and tuple(f8.v[1].shape) == (3, 10, 4, D)
    assert f8.k_scale[1].dtype == torch.float32 and tuple(f8.v_scale[1].shape) == (3, 10, 4)
    keys = 2 * 2 * 3 * 10 * 4
    assert nbytes(bf) == keys * 2 * D and nbytes(f8) == keys * (D + 4)
    f8.k_scale[0].fill_(3.0)
    f8.grow(16)
    assert tuple(f8.k[0].shape) == (3, 16, 4, D) and tuple(f8.v_scale[0].shape) == (3, 16, 4)
    assert float(f8.k_scale[0][:, :10].min()) == 3.0
    beams = G.BeamState.allocate(2, 3, 2, 10, 4, D, "cpu", kv_dtype="fp8_e4m3")
    assert beams.kv_dtype == "fp8_e4m3" and tuple(beams.k_scale[0].shape) == (6, 10, 4) and beams.k[0].dtype == torch.uint8
    beams.grow(12)
    assert tuple(beams.v_scale[1].shape) == (6, 12, 4) and tuple(beams.src.shape) == (6, 12)
    assert G.BeamState.allocate(2, 3, 2, 10, 4, D, "cpu").k_scale is None
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        G.KVCache.allocate(2, 3, 10, 4, D, "cpu", kv_dtype="fp8_e5m2")


def test_the_four_ops_trace_on_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import touchnet_amd.functional as F
    B, S, Nh, Nkv, D, T = 3, 20, 8, 2, 64, 7
    with FakeTensorMode():
        t = lambda *s, dtype=torch.bfloat16: torch.empty(*s, dtype=dtype, device="cuda")
        codes, scales = F.kv_quantize(t(T, Nkv, D))
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == (T, Nkv, D)
        assert scales.dtype == torch.float32 and tuple(scales.shape) == (T, Nkv)
        cache = (t(B, S, Nkv, D, dtype=torch.uint8), t(B, S, Nkv, D, dtype=torch.uint8),
                 t(B, S, Nkv, dtype=torch.float32), t(B, S, Nkv, dtype=torch.float32))
        lens = t(B, dtype=torch.int32)
        o = F.attn_decode_fp8(t(B, Nh, D), t(B, Nkv, D), t(B, Nkv, D), *cache, lens)
        assert tuple(o.shape) == (B, Nh, D) and o.dtype == torch.bfloat16
        o = F.attn_decode_beam_fp8(t(B, Nh, D), t(B, Nkv, D), t(B, Nkv, D), *cache, lens, t(B, S, dtype=torch.int32))
        assert tuple(o.shape) == (B, Nh, D)
        o = F.attn_extend_fp8(t(T, Nh, D), codes, codes, scales, scales, *cache, t(3, dtype=torch.int32),
                              t(2, dtype=torch.int32))
        assert tuple(o.shape) == (T, Nh, D) and o.dtype == torch.bfloat16
