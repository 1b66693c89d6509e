"""Kimi-Audio's speech tokenizer (WhisperVQEncoder, touchnet/models/kimi_audio/modeling_kimi_audio.py:140-319) — the
host side: config resolution and refusals, parameter names against the reference-run fixture, the ops' fake impls,
the exactness of trimming and the batcher's per-clip token counts.  No GPU."""
import ast
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speech_tokenizer.npz")

# the keys of examples/audio/sft/asr/wenetspeech/config/Kimi-Audio-7B.json `speech_tokenizer_config` this path reads
# (+ two it ignores)
KIMI_7B_TOKENIZER = {"d_model": 1280, "encoder_attention_heads": 20, "encoder_ffn_dim": 5120, "encoder_layers": 32,
                     "max_source_positions": 1500, "num_mel_bins": 128, "pooling_kernel_size": 4, "pooling_position": 16,
                     "pooling_type": "avg", "quantize_causal_block_size": 200, "quantize_ema_decay": 0.99,
                     "quantize_encoder_only": True, "quantize_position": 16, "quantize_vocab_size": 16384,
                     "encoder_causal_convolution": True, "activation_function": "gelu", "model_type": "whisper",
                     "architectures": ["WhisperVQEncoder"]}


def test_config_resolves_the_kimi_audio_7b_tokenizer():
    from touchnet_amd.models.kimi_audio.speech_tokenizer import WhisperVQConfig
    c = WhisperVQConfig.from_dict(KIMI_7B_TOKENIZER)
    assert (c.d_model, c.encoder_attention_heads, c.encoder_ffn_dim, c.num_mel_bins) == (1280, 20, 5120, 128)
    assert (c.quantize_position, c.pooling_position, c.pooling_kernel_size, c.pooling_type) == (16, 16, 4, "avg")
    assert (c.quantize_vocab_size, c.quantize_causal_block_size, c.quantize_ema_decay) == (16384, 200, 0.99)
    d = WhisperVQConfig.from_dict({"d_model": 128, "encoder_attention_heads": 2})    # the rest: WhisperVQConfig's defaults
    assert (d.quantize_vocab_size, d.quantize_causal_block_size, d.pooling_position) == (16384, 200, 16)


@pytest.mark.parametrize("key,value", [("encoder_causal_convolution", False), ("quantize_encoder_only", False),
                                       ("quantize_causal_block_size", None), ("quantize_vocab_size", None),
                                       ("pooling_type", "mean"), ("pooling_position", 15), ("encoder_attention_heads", 16)])
def test_config_refuses_what_the_reference_asserts_or_cannot_run(key, value):
    from touchnet_amd.models.kimi_audio.speech_tokenizer import WhisperVQConfig
    with pytest.raises(ValueError):
        WhisperVQConfig.from_dict({**KIMI_7B_TOKENIZER, key: value})


def test_state_dict_keys_are_the_references():
    from touchnet_amd.models.kimi_audio.speech_tokenizer import WhisperVQConfig, WhisperVQEncoder
    g = np.load(GOLD)
    m = WhisperVQEncoder(WhisperVQConfig.from_dict(ast.literal_eval(str(g["config_json"]))))
    assert sorted(m.state_dict()) == sorted(str(k) for k in g["keys"])
    assert not any(p.requires_grad for p in m.parameters())


def test_model_holds_a_frozen_tokenizer_only_when_configured():
    from touchnet_amd.models.kimi_audio import KimiAudioConfig, KimiAudioPackedForCausalLM, get_num_params
    kw = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
              num_key_value_heads=1, head_dim=64, kimia_mimo_layers=1, kimia_mimo_transformer_from_layer_index=0,
              use_whisper_feature=True, kimia_adaptor_input_dim=512,
              speech_encoder_config=dict(num_mel_bins=16, d_model=128, encoder_layers=1, encoder_attention_heads=2,
                                         encoder_ffn_dim=128, max_source_positions=150))
    plain = KimiAudioPackedForCausalLM(KimiAudioConfig(**kw))
    assert plain.speech_tokenizer is None and not any(k.startswith("speech_tokenizer.") for k in plain.state_dict())
    tok = dict(num_mel_bins=16, d_model=128, encoder_attention_heads=2, encoder_ffn_dim=128, max_source_positions=150,
               pooling_position=2, quantize_position=2, quantize_vocab_size=64, quantize_causal_block_size=50)
    m = KimiAudioPackedForCausalLM(KimiAudioConfig(**kw, speech_tokenizer_config=tok))
    m.post_init()
    st = m.speech_tokenizer
    assert not any(p.requires_grad for p in st.parameters())
    assert torch.equal(st.embed_positions2.weight, st.embed_positions.weight[:st.embed_positions2.weight.shape[0]])
    assert get_num_params(m) == get_num_params(plain) + sum(p.numel() for p in st.parameters())


def test_new_ops_have_fake_impls():
    import touchnet_amd.library as L
    q = torch.empty(2, 300, 4, 64, dtype=torch.bfloat16, device="meta")
    i32 = torch.empty(2, 300, dtype=torch.int32, device="meta")
    o = L.attn_block_causal_fwd(q, q, q, i32, i32, 50, 0.125)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    ids = L.vq_nearest(torch.empty(7, 128, dtype=torch.bfloat16, device="meta"),
                       torch.empty(64, 128, dtype=torch.bfloat16, device="meta"), torch.empty(64, device="meta"))
    assert ids.shape == (7,) and ids.dtype == torch.int64
    assert "attn_block_causal_fwd" in L.OPS and "vq_nearest" in L.OPS


def test_causal_stem_is_the_pad1_conv_of_the_shifted_input():
    """CausalConv1d (:101-137: pad 2 on the left) == the symmetric pad-1 conv of the input shifted right by one zero frame,
    for stride 1 and 2 — what lets the stem run on the tower's conv1d_k3 GEMM path."""
    g = torch.Generator().manual_seed(0)
    for stride in (1, 2):
        for Tm in (9, 10, 300):
            x = torch.randn(2, 5, Tm, generator=g, dtype=torch.float64)
            w, b = torch.randn(6, 5, 3, generator=g, dtype=torch.float64), torch.randn(6, generator=g, dtype=torch.float64)
            ref = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (2, 0)), w, b, stride=stride)
            got = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (1, 0)), w, b, stride=stride, padding=1)
            assert torch.equal(got[..., :ref.shape[-1]], ref)


@pytest.mark.parametrize("T,block,p", [(1500, 200, 4), (150, 50, 4), (150, 64, 4), (149, 7, 3)])
def test_trimming_drops_no_frame_a_needed_token_depends_on(T, block, p):
    """For every id count K a clip of T post-conv frames can be asked for (Kimi-Audio: T 1500, p 4, block 200; the fixture's
    T 150 is not a multiple of p): the frames the trimmed schedule keeps contain every frame the first K ids depend on —
    brute force from the reference's mask formula (:226-242, any number of layers: its reachability closes after one
    layer) and the causal stem — and in the packed layout (`packed_layout`) every pooling tap of those ids reads a kept
    frame of its own clip, or the zero row exactly where the reference zero-pads (tap >= T, :305-307)."""
    from touchnet_amd.models.kimi_audio.speech_tokenizer import needed_frames, packed_layout
    i = np.arange(T)
    S = -(-T // p)
    for K in range(1, S + 1):
        for Lk in {max(1, min(T, p * K - p + 1)), min(T, p * K), T}:     # valid-key counts a clip asking for K ids can have
            m = i < Lk
            allowed = m[None, :] & ((i[None, :] <= i[:, None]) | (i[None, :] // block == i[:, None] // block))
            reach = np.zeros(T, bool)
            reach[:min(T, p * K)] = True                                # the real frames pooled into ids 0..K-1
            for _ in range(3):
                reach = reach | allowed[reach].any(0)
            need = needed_frames(K, T, block, p)
            assert need <= T and not reach[need:].any(), (K, Lk, need, int(np.nonzero(reach)[0].max()))
        for ks in ([K], [K, 1, S], [S, K, 1]):                           # the full-length clip first, in the middle, last
            lay = packed_layout(ks, T, block, p)
            starts = sorted(set(lay.start))
            assert all(s0 % 64 == 0 for s0 in starts) and len(starts) == len(ks)
            tap = 0
            for c, (k, s0) in enumerate(zip(ks, starts)):
                f = needed_frames(k, T, block, p)
                for t in range(p * k):
                    r = lay.taps[tap]
                    tap += 1
                    if t < T:
                        assert s0 <= r < s0 + f and lay.src[r] == c * lay.frames + t, (ks, c, t, r)
                    else:
                        assert r == lay.rows, (ks, c, t, r)                 # the zero row behind the packed row
                assert lay.slots[tap // p - k:tap // p] == list(range(c * S, c * S + k))
                assert set(lay.cap[s0:s0 + f]) == {s0 + f} and set(lay.clip[s0:s0 + f]) == {c}
            assert tap == len(lay.taps) and lay.rows == starts[-1] + -(-needed_frames(ks[-1], T, block, p) // 64) * 64


def test_batcher_emits_host_token_counts():
    from touchnet_amd.models.kimi_audio.processing_kimi_audio import WHISPER_FRAMES, _emit, num_audio_tokens
    buf = []
    for n in (16000, 1, 123457, 480000, 600000):
        L = min(-(-n // 160), WHISPER_FRAMES)
        mask = (torch.arange(WHISPER_FRAMES) < L).to(torch.int32)
        buf.append({"text": [1, 2], "audio": [3, 4], "labels": [-100, 5], "slen": 1, "features": torch.zeros(128, 3000),
                    "mask": mask, "n_audio": num_audio_tokens(n)})
    out = _emit(buf, 0)
    assert out["clip_tokens"] == [-(-int(b["mask"].sum()) // 8) for b in buf]
    assert all(isinstance(k, int) for k in out["clip_tokens"])


@pytest.mark.skipif(__import__("shutil").which("hipcc") is None, reason="hipcc not on PATH")
def test_new_kernels_have_no_scratch_and_no_spills(tmp_path):
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for src, kernel in (("attn_block_causal.hip", "attn_block_causal_fwd_kernel"), ("vq.hip", "vq_nearest_kernel")):
        out = tmp_path / (src + ".s")
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result", "-S",
                            "--cuda-device-only", os.path.join(root, "touchnet_amd", "csrc", src), "-o", str(out)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        text = out.read_text()
        assert kernel in text and "scratch_" not in text
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            vals = [int(v) for v in re.findall(rf"\.{field}:\s+(\d+)", text)]
            assert vals and all(v == 0 for v in vals), (src, field, vals)
