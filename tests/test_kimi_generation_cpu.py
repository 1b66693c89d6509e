"""Kimi-Audio decoding without a GPU: the plain-torch restatement (tests/kimi_generate_reference.py) against the run of the
reference's own generate() stored in tests/golden/kimi_generate.npz, the prompt builder against the reference script's
prompts, the config's refusals, the op's registration, the decoder's unchanged default path and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kimi_generate_reference as KR  # noqa: E402
import oracle.ops as oops  # noqa: E402
from touchnet_amd.models.backend import use_ops  # noqa: E402


fixture_model, cases = KR.fixture_model, KR.cases


def test_restatement_reproduces_the_reference_run(golden):
    g = golden("kimi_generate.npz")
    blank, eos, offset, max_new = (int(x) for x in g["special"])
    m = fixture_model(g)
    E = m.model.embed_tokens.weight.detach()
    crossed = finished_early = ran_out = 0
    with torch.no_grad(), use_ops(oops):
        fn = lambda x: m.lm_head(m.model(x)[0][:, -1])
        for c in cases(g):
            W = int(g[f"{c}/window"])
            text, audio = torch.tensor(g[f"{c}/text_ids"]), torch.tensor(g[f"{c}/audio_ids"])
            returned, raw, logits = KR.generate(fn, E, text, audio, max_new, window=W, eos=eos, blank=blank,
                                                token_offset=offset)
            want = torch.tensor(g[f"{c}/raw"]).long()
            err = float((logits - torch.tensor(g[f"{c}/logits"])).abs().max())
            print(f"{c}: {raw.shape[1]} steps, logits max |diff| {err:.2e}")
            assert torch.equal(raw, want), c
            assert err < 1e-4 * float(np.abs(g[f"{c}/logits"]).max())
            for b, r in enumerate(returned):
                assert r == g[f"{c}/returned{b}"].tolist(), (c, b)
            crossed += raw.shape[1] > W + 1
            finished_early += int(((want == eos).any(1)).sum())
            ran_out += int((~(want == eos).any(1)).sum())
    assert crossed == len(cases(g)) and finished_early >= 1 and ran_out >= 1


def test_build_prompts_equals_the_reference_scripts(golden):
    from touchnet_amd.models.kimi_audio.inference_kimi_audio import audio_token_count, build_prompts
    g = golden("kimi_generate.npz")

    class Tok:                                         # the stand-in tokenizer the fixture was made with
        SPECIAL = {"<|im_kimia_user_msg_start|>": 300, "<|im_kimia_text_blank|>": 301, "<|im_media_begin|>": 302,
                   "<|im_media_end|>": 303, "<|im_kimia_speech_ct_id|>": 304, "<|im_msg_end|>": 305,
                   "<|im_kimia_assistant_msg_start|>": 306, "<|im_kimia_text_eos|>": 307}

        def __call__(self, text, add_special_tokens=False):
            ids, i = [], 0
            while i < len(text):
                for sp, v in self.SPECIAL.items():
                    if text.startswith(sp, i):
                        ids.append(v)
                        i += len(sp)
                        break
                else:
                    ids.append(10 + ord(text[i]) % 200)
                    i += 1
            return {"input_ids": ids}
    counts = [int(n) for n in g["prompt/counts"]]
    p = build_prompts(Tok(), str(g["prompt/instruct"]), counts)
    for n, t, a in zip(counts, p.text_ids, p.audio_ids):
        assert t.tolist() == g[f"prompt/{n}/text"].tolist() and a.tolist() == g[f"prompt/{n}/audio"].tolist()
        assert int((a == 302).sum()) == 1 and int((a == 303).nonzero()) - int((a == 302).nonzero()) - 1 == n
    assert [audio_token_count(L) for L in (1, 8, 9, 3000)] == [1, 1, 2, 375]


def test_config_refuses_what_the_kernel_refuses():
    from touchnet_amd.generation import KimiGenerationConfig
    c = KimiGenerationConfig()
    assert (c.text_temperature, c.text_top_k, c.text_repetition_penalty, c.text_repetition_window_size) == (0.0, 5, 1.1, 16)
    assert c.new_tokens(300) == 2048 and KimiGenerationConfig(max_new_tokens=-1).new_tokens(300) == 7200
    KimiGenerationConfig(audio_temperature=0.3, audio_top_k=0, audio_repetition_window_size=1000)      # ignored knobs
    for bad in (dict(text_repetition_window_size=0), dict(text_repetition_window_size=65), dict(text_top_k=65),
                dict(text_top_k=-1), dict(text_repetition_penalty=0.0), dict(text_temperature=0.7, text_top_k=0),
                dict(seed=-1), dict(max_new_tokens=-2)):
        with pytest.raises(ValueError):
            KimiGenerationConfig(**bad)
    KimiGenerationConfig(text_temperature=0.0, text_top_k=0)                    # greedy: top_k is inert


def test_kimi_text_step_is_declared_registered_and_traces():
    import os
    from touchnet_amd import _C
    import touchnet_amd.library as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "touchnet_amd.h")).read()
    assert "int tn_kimi_text_step(" in text and "modeling_kimi_audio.py:797-844" in text and ":1153-1214" in text
    assert "tn_kimi_text_step" in _C.PROTOTYPES and "kimi_text_step_" in L.OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mi355_touch::kimi_text_step_", "Meta")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        B, V, H, S = 3, 1000, 64, 32
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
        x = torch.empty(B, H, dtype=torch.bfloat16, device="cuda")
        r = torch.ops.mi355_touch.kimi_text_step_(torch.empty(B, V, device="cuda"), i32(B, S), i32(B), i32(B), i32(B), i32(1),
                                                  i32(B), torch.empty(V, H, dtype=torch.bfloat16, device="cuda"), x, None,
                                                  None, 1.1, 16, 0.0, 5, 0, 7, 8, 8)
        assert r is None and tuple(x.shape) == (B, H)


def test_kimi_text_step_refuses_on_the_host():
    """tn_kimi_text_step checks its arguments before any launch and returns -22 without touching the device (the addresses
    are never dereferenced)."""
    from touchnet_amd import _C
    lib = _C.lib()
    P = 0x10000

    def call(logits=P, hist=P, hl=P, cl=P, fin=P, nu=P, pl=P, emb=P, xn=P, rk=None, un=None, B=2, V=1000, S=32, H=64,
             pen=1.1, W=16, T=0.0, k=5, eos=7, blank=8, audio=8, dtype=1):
        return lib.tn_kimi_text_step(logits, hist, hl, cl, fin, nu, pl, emb, xn, rk, un, B, V, S, H, pen, W, T, k, 1, eos,
                                     blank, audio, dtype, None)
    bad = [dict(logits=None), dict(hist=None), dict(pl=None), dict(emb=None), dict(xn=None), dict(hl=P + 2), dict(pl=P + 1),
           dict(emb=P + 8), dict(xn=P + 4), dict(rk=P + 4), dict(un=P + 2), dict(logits=P + 1), dict(logits=P + 2, dtype=0),
           dict(V=0), dict(V=262145), dict(S=0), dict(B=0), dict(W=0), dict(W=65), dict(k=-1), dict(k=65), dict(pen=0.0),
           dict(pen=-1.0), dict(H=60), dict(H=0), dict(T=0.7, k=0), dict(blank=1000), dict(audio=-1), dict(dtype=2)]
    for kw in bad:
        assert call(**kw) == -22, kw


def test_kimi_decoder_default_path_is_unchanged():
    from touchnet_amd.models.kimi_audio import KimiAudioConfig, KimiDecoderModel
    torch.manual_seed(3)
    cfg = KimiAudioConfig(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                          num_key_value_heads=1, head_dim=64, kimia_mimo_layers=1, kimia_mimo_transformer_from_layer_index=0)
    m = KimiDecoderModel(cfg).eval()
    x = torch.randn(2, 24, 128)
    doc = torch.cat([torch.ones(2, 10), 2 * torch.ones(2, 14)], 1).long()
    pos = torch.cat([torch.arange(10), torch.arange(14)]).repeat(2, 1)
    with torch.no_grad(), use_ops(oops):
        for mimo in (False, True):
            a = m(x, position_ids=pos, attention_mask=doc, with_mimo=mimo)
            b = m(x, position_ids=pos, attention_mask=doc, with_mimo=mimo, keep_rows=None, kv_out=None)
            assert torch.equal(a[0], b[0]) and (a[1] is None) == (not mimo)
            if mimo:
                assert torch.equal(a[1], b[1])
        # the new arguments: the kept rows are the full computation's, one key / value pair per layer
        kv = []
        rows = torch.tensor([9, 23, 24 + 9, 24 + 23])
        h, none = m(x, position_ids=pos, attention_mask=doc, keep_rows=rows, kv_out=kv)
        assert none is None and len(kv) == 2 and tuple(kv[0][0].shape) == (2, 24, 1, 64)
        torch.testing.assert_close(h[0], a[0].reshape(48, -1)[rows], rtol=1e-5, atol=1e-5)
        with pytest.raises(RuntimeError, match="mimo"):
            m(x, position_ids=pos, attention_mask=doc, with_mimo=True, keep_rows=rows)
        with pytest.raises(RuntimeError, match="mimo"):
            m(x, position_ids=pos, attention_mask=doc, with_mimo=True, kv_out=[])


def test_decode_logits_takes_the_step_input():
    import inspect
    from touchnet_amd.generation import decode_logits
    sig = inspect.signature(decode_logits)
    assert sig.parameters["inputs_embeds"].default is None and list(sig.parameters)[:3] == ["lm", "cache", "table"]


def test_command_line_help_runs():
    r = subprocess.run([sys.executable, "-m", "touchnet_amd.bin.infer_kimi_audio", "--help"], capture_output=True, text=True,
                       cwd=str(__import__("pathlib").Path(__file__).parent.parent))
    assert r.returncode == 0 and "--model_path" in r.stdout and "--max_new_tokens" in r.stdout
