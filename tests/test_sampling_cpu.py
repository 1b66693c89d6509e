"""Sampled decoding and Qwen2-Audio inference (csrc/sample.hip, generation.GenerationConfig.from_hf,
models/qwen2_audio/inference_qwen2_audio.py): everything that must hold WITHOUT the device — generation_config.json
parsing, the Philox generator, op registration, host-side argument refusal, the prompt contract and the valid-frame count."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- GenerationConfig
def test_generation_config_defaults_are_unchanged():
    from touchnet_amd.generation import GenerationConfig
    c = GenerationConfig()
    assert (c.max_new_tokens, c.repetition_penalty, c.no_repeat_ngram_size, c.eos_token_id, c.check_every) == \
        (256, 1.5, 2, None, 16)
    assert c.do_sample is False


def test_from_hf_reads_sampling_knobs_and_several_eos(tmp_path):
    from touchnet_amd.generation import GenerationConfig
    d = {"do_sample": True, "temperature": 0.7, "top_k": 20, "top_p": 0.5, "repetition_penalty": 1.1,
         "eos_token_id": [151643, 151645], "pad_token_id": 151643, "bos_token_id": 151643, "transformers_version": "4.51"}
    (tmp_path / "generation_config.json").write_text(json.dumps(d))
    for src in (tmp_path, tmp_path / "generation_config.json", d):
        c = GenerationConfig.from_hf(src)
        assert c.do_sample and c.temperature == 0.7 and c.top_k == 20 and c.top_p == 0.5
        assert c.repetition_penalty == pytest.approx(1.1) and c.no_repeat_ngram_size == 0
        assert c.eos_token_id == [151643, 151645] and c.pad_token_id == 151643
        assert c.max_new_tokens is None and c.max_length == 20                 # HF's default max_length
    c = GenerationConfig.from_hf(d, seed=7, top_k=0)
    assert c.seed == 7 and c.top_k == 0


def test_from_hf_warpers_are_inert_without_do_sample():
    from touchnet_amd.generation import GenerationConfig
    c = GenerationConfig.from_hf({"temperature": 0.3, "top_k": 5, "top_p": 0.2})
    assert not c.do_sample and (c.temperature, c.top_k, c.top_p) == (1.0, 0, 1.0)
    assert c.repetition_penalty == 1.0 and c.no_repeat_ngram_size == 0       # HF's defaults, not the reference recipe's
    c = GenerationConfig.from_hf({"do_sample": True})
    assert (c.temperature, c.top_k, c.top_p) == (1.0, 50, 1.0)               # HF's defaults when sampling


def test_from_hf_max_new_tokens_takes_precedence_over_max_length():
    from touchnet_amd.generation import GenerationConfig
    c = GenerationConfig.from_hf({"max_new_tokens": 64, "max_length": 100}, max_length=70000)
    assert c.new_tokens(500) == 64
    c = GenerationConfig.from_hf({"max_length": 100}, max_length=70000)
    assert c.max_new_tokens is None and c.new_tokens(500) == 69500
    assert GenerationConfig.from_hf({}).new_tokens(5) == 15


@pytest.mark.parametrize("key,value", [("num_beams", 2), ("typical_p", 0.9), ("min_p", 0.05), ("epsilon_cutoff", 3e-4),
                                       ("eta_cutoff", 1e-3), ("bad_words_ids", [[5]]), ("suppress_tokens", [1, 2]),
                                       ("penalty_alpha", 0.6), ("num_return_sequences", 2)])
def test_from_hf_refuses_knobs_it_does_not_implement(key, value):
    from touchnet_amd.generation import GenerationConfig
    with pytest.raises(ValueError, match=key):
        GenerationConfig.from_hf({"do_sample": True, key: value})
    GenerationConfig.from_hf({"do_sample": True, key: None if key != "num_beams" else 1})      # the inert value passes


def test_from_hf_refuses_bad_sampling_values():
    from touchnet_amd.generation import GenerationConfig
    for bad in ({"temperature": 0.0}, {"top_p": 0.0}, {"top_p": 1.5}, {"top_k": -1}):
        with pytest.raises(ValueError):
            GenerationConfig.from_hf({"do_sample": True, **bad})
    with pytest.raises(TypeError):
        GenerationConfig.from_hf({}, not_a_field=1)


# ---------------------------------------------------------------------------------------------------- kernel entry
def test_philox_matches_the_random123_known_answers():
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    for ctr, key, want in (((0, 0, 0, 0), 0, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, 0xffffffffffffffff, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), 0x299f31d0a4093822,
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        a = (C.c_uint * 4)(*ctr)
        lib.tn_philox4x32_10(a, key)
        assert tuple(a) == want


def test_sample_step_is_declared_in_the_header_and_the_stub():
    from touchnet_amd import _C
    text = open(os.path.join(ROOT, "include", "touchnet_amd.h")).read()
    assert "int tn_sample_step(" in text and "TopPLogitsWarper" in text and "inference_qwen2_audio.py" in text
    assert "tn_sample_step" in _C.PROTOTYPES and "tn_philox4x32_10" not in _C.PROTOTYPES


def test_sample_op_is_registered_with_declared_mutations_and_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import touchnet_amd.library as L
    assert "sample_step_" in L.OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mi355_touch::sample_step_", "Meta")
    s = str(torch.ops.mi355_touch.sample_step_.default._schema)
    for arg in ("hist", "hist_len", "cache_len", "finished", "n_unfinished"):
        assert f"!) {arg}" in s, (arg, s)
    assert "!) logits" not in s and "!) row_key" not in s and s.endswith("-> ()"), s
    with FakeTensorMode():
        B, S = 3, 50
        i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device="cuda")
        r = torch.ops.mi355_touch.sample_step_(torch.empty(B, 1000, device="cuda"), i32(B, S), i32(B), i32(B), i32(B),
                                               i32(1), torch.empty(B, dtype=torch.int64, device="cuda"), None, None, 1.1,
                                               True, 0.7, 20, 0.9, 5, [1, 2], 0)
        assert r is None


def test_sample_entry_point_refuses_malformed_arguments_before_any_launch():
    """tn_sample_step checks its arguments on the host and returns -22 without touching the device (the addresses are
    host memory, never dereferenced by a refused call)."""
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    raw = (C.c_char * 8192)()
    p = (C.addressof(raw) + 255) // 256 * 256
    eos = (C.c_int * 2)(5, 6)

    def ss(lg=p, hist=p, hl=p, rk=p, un=None, nk=None, B=2, V=156032, S=64, pen=1.0, smp=1, T=1.0, k=20, tp=0.9,
           ep=eos, ne=2, dtype=1):
        return lib.tn_sample_step(lg, hist, hl, p, p, p, rk, un, nk, B, V, S, pen, smp, T, k, tp, 1, ep, ne, 0, dtype,
                                  None)
    assert ss(lg=None) == EINVAL and ss(hist=None) == EINVAL and ss(hl=p + 2) == EINVAL and ss(rk=p + 4) == EINVAL
    assert ss(un=p + 2) == EINVAL and ss(nk=p + 1) == EINVAL and ss(lg=p + 1) == EINVAL and ss(lg=p + 2, dtype=0) == EINVAL
    assert ss(V=0) == EINVAL and ss(V=262145) == EINVAL and ss(S=0) == EINVAL and ss(B=0) == EINVAL
    assert ss(pen=0.0) == EINVAL and ss(dtype=2) == EINVAL
    assert ss(ne=9) == EINVAL and ss(ep=None) == EINVAL and ss(ne=-1) == EINVAL
    assert ss(T=0.0) == EINVAL and ss(k=-1) == EINVAL and ss(tp=0.0) == EINVAL and ss(tp=1.01) == EINVAL


def test_trim_at_eos_takes_several_ids():
    from touchnet_amd.generation import trim_at_eos
    ids = torch.tensor([[5, 6, 2, 0], [7, 4, 0, 0], [9, 9, 9, 9]])
    assert trim_at_eos(ids, [2, 4]) == [[5, 6], [7], [9, 9, 9, 9]]


# ---------------------------------------------------------------------------------------------------- Qwen2-Audio inputs
def _tiny_tokenizer(tmp_path):
    """A word-level tokenizer with Qwen2-Audio's special tokens, saved locally and loaded back with AutoTokenizer."""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import AutoTokenizer, PreTrainedTokenizerFast
    words = ["Generate", "the", "transcription:", "hello", "world", "a", "b", "c"]
    vocab = {w: i + 3 for i, w in enumerate(words)}
    vocab.update({"[UNK]": 0, "x": 1, "y": 2})
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="[UNK]", eos_token="<|endoftext|>",
                                   pad_token="<|endoftext|>",
                                   additional_special_tokens=["<|audio_bos|>", "<|AUDIO|>", "<|audio_eos|>", "<|im_end|>"])
    fast.save_pretrained(str(tmp_path / "tok"))
    return AutoTokenizer.from_pretrained(str(tmp_path / "tok"))


def test_prompts_follow_the_reference_formula(tmp_path):
    from touchnet_amd.models.qwen2_audio.inference_qwen2_audio import build_prompts, prompt_ids
    from touchnet_amd.models.qwen2_audio.processing_qwen2_audio import TEMPLATE_S2T, audio_token_count
    tok = _tiny_tokenizer(tmp_path)
    audio = tok.convert_tokens_to_ids("<|AUDIO|>")
    instruct = "Generate the transcription:"
    for L in (1, 2, 3, 4, 5, 99, 100, 101, 1500, 2999, 3000):
        # the reference, touchnet/models/qwen2_audio/inference_qwen2_audio.py:111-120
        input_length = (L - 1) // 2 + 1
        n = (input_length - 2) // 2 + 1
        assert audio_token_count(L) == n
        text = TEMPLATE_S2T.replace("<|INSTRUCT|>", instruct).replace("<|AUDIO|>", "<|AUDIO|>" * n, 1)
        want = tok(text, padding=False, return_tensors="pt")["input_ids"].squeeze(0).tolist()
        got = prompt_ids(tok, n, instruct)
        assert got == want and got.count(audio) == n
        assert got[0] == tok.convert_tokens_to_ids("<|audio_bos|>")
    pr = build_prompts(tok, [100, 3000, 7], instruct)
    assert [int((t == audio).sum()) for t in pr.input_ids] == [audio_token_count(L) for L in (100, 3000, 7)]


def test_valid_frames_equal_the_whisper_extractor_attention_mask():
    from transformers import WhisperFeatureExtractor
    from touchnet_amd.models.qwen2_audio.inference_qwen2_audio import valid_frames
    fe = WhisperFeatureExtractor(feature_size=128)
    rng = np.random.RandomState(0)
    for n in (1, 159, 160, 161, 16000, 48000 + 17, 479999, 480000, 480001, 560000):
        x = rng.randn(n).astype(np.float32) * 0.1
        out = fe(x, sampling_rate=16000, truncation=True, return_attention_mask=True, padding="max_length",
                 return_tensors="np")
        assert out["input_features"].shape[-1] == 3000
        assert valid_frames(n) == int(out["attention_mask"].sum()), n
