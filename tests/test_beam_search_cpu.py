"""Beam search (touchnet_amd.generation, csrc/beam.hip, csrc/attn_decode.hip): everything that must hold without a GPU —
the oracle of the GPU tests (tests/beam_search_reference.py) against transformers' generate(), the generation config, the
op registrations and the argument checks of the two C entry points."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_search_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ (1) the oracle is HF's
def _tiny_llama(seed):
    import transformers
    cfg = transformers.LlamaConfig(vocab_size=48, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                   num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=64,
                                   eos_token_id=2, pad_token_id=0, bos_token_id=1)
    torch.manual_seed(seed)
    m = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0, 0.25)                  # peaked enough that eos is reached and beams part
    return m


@pytest.fixture(scope="module")
def tiny_models():
    return {seed: _tiny_llama(seed) for seed in range(6)}


@pytest.mark.parametrize("early_stopping", [False, True, "never"])
@pytest.mark.parametrize("length_penalty", [1.0, 0.6, 2.0])
@pytest.mark.parametrize("K", [2, 4])
def test_restatement_equals_transformers_generate(tiny_models, K, length_penalty, early_stopping):
    """Token-exact, sequences_scores within 1e-4: V 48, eos reachable, prompts of 5-10 ids, 12 new tokens, penalty / n-gram
    off and 1.5 / 2, six seeds (equal-length prompts: HF's left padding would put the pad id into the penalty set)."""
    n_new, eos, finished_early = 12, [2], 0
    for seed, model in tiny_models.items():
        g = torch.Generator().manual_seed(100 + seed)
        P = 5 + seed
        prompts = torch.randint(3, 48, (2, P), generator=g)
        for penalty, ngram in ((1.0, 0), (1.5, 2)):
            with torch.no_grad():
                out = model.generate(prompts, attention_mask=torch.ones_like(prompts), num_beams=K, do_sample=False,
                                     length_penalty=length_penalty, early_stopping=early_stopping,
                                     repetition_penalty=penalty, no_repeat_ngram_size=ngram, max_new_tokens=n_new,
                                     eos_token_id=eos[0], pad_token_id=0, return_dict_in_generate=True, output_scores=True)
            st = ref.new_state(prompts.tolist(), K, P + n_new)
            kw = dict(K=K, penalty=penalty, ngram=ngram, eos=eos, n_new=n_new, length_penalty=length_penalty,
                      early_stopping=early_stopping, dtype=torch.float32)
            for step in range(n_new):
                if int(st["n_unfinished"][0]) == 0:
                    break
                rows = [r for r in range(2 * K) if step > 0 or r % K == 0]
                L = P + step
                with torch.no_grad():
                    logits = model(st["hist"][rows, :L].to(torch.int64)).logits[:, -1].float().detach()
                ref.beam_step(st, logits, **kw)
            assert int(st["n_unfinished"][0]) == 0
            for b, (ids, score) in enumerate(ref.best_hypotheses(st, K, [P, P])):
                want = out.sequences[b, P:].tolist()
                # (behind a hypothesis HF pads; this version of transformers fills with the eos id, older ones with pad)
                assert want[:len(ids)] == ids and all(t in (0, eos[0]) for t in want[len(ids):]), (seed, penalty, b)
                assert len(ids) == n_new or ids[-1] == eos[0]
                assert abs(score - float(out.sequences_scores[b])) < 1e-4, (seed, penalty, b)
                finished_early += len(ids) < n_new
    # eos was reached somewhere, so the finished-set branches ran (a length penalty of 2 favours the full-length rows)
    assert finished_early > 0 or length_penalty > 1.0


# ------------------------------------------------------------------------------------------------ (2) generation config
def test_from_hf_resolves_beam_search_knobs():
    from touchnet_amd.generation import GenerationConfig
    cfg = GenerationConfig.from_hf({"num_beams": 4, "length_penalty": 0.6, "early_stopping": True})
    assert (cfg.num_beams, cfg.length_penalty, cfg.early_stopping, cfg.do_sample) == (4, 0.6, True, False)
    assert GenerationConfig.from_hf({"num_beams": 2, "early_stopping": "never"}).early_stopping == "never"
    d = GenerationConfig.from_hf({})
    assert (d.num_beams, d.length_penalty, d.early_stopping) == (1, 1.0, False)
    assert GenerationConfig().num_beams == 1
    assert GenerationConfig.from_hf({}, num_beams=3).num_beams == 3


def test_from_hf_refuses_what_beam_search_does_not_cover():
    from touchnet_amd.generation import GenerationConfig
    with pytest.raises(ValueError, match="num_beams"):
        GenerationConfig.from_hf({"num_beams": 4, "do_sample": True})
    with pytest.raises(ValueError, match="num_beams"):
        GenerationConfig.from_hf({"num_beams": 9})
    with pytest.raises(ValueError, match="eos"):
        GenerationConfig.from_hf({"num_beams": 2, "eos_token_id": [1, 2, 3, 4]})
    GenerationConfig.from_hf({"num_beams": 8, "eos_token_id": [1, 2, 3]})
    with pytest.raises(ValueError, match="early_stopping"):
        GenerationConfig.from_hf({"num_beams": 2, "early_stopping": "sometimes"})
    for key, value in (("num_beam_groups", 2), ("num_return_sequences", 2), ("diversity_penalty", 0.5)):
        with pytest.raises(ValueError, match=key):
            GenerationConfig.from_hf({"num_beams": 4, key: value})


# ------------------------------------------------------------------------------------------------ (3) ops and C ABI
def test_beam_ops_are_registered_with_meta_kernels():
    from touchnet_amd import library as L
    for name in ("attn_decode_beam_", "beam_step_"):
        assert name in L.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"mi355_touch::{name}", "Meta")
    s = str(torch.ops.mi355_touch.attn_decode_beam_.default._schema)
    assert "Tensor(a3!) k_cache" in s and "Tensor(a4!) v_cache" in s and "Tensor src" in s
    s = str(torch.ops.mi355_touch.beam_step_.default._schema)
    for name in ("hist", "src", "run_score", "fin_ids", "fin_score", "done", "n_unfinished", "out_parent"):
        assert f"!) {name}" in s, (name, s)
    R, S, Nh, Nkv, D = 6, 40, 4, 1, 64
    m = lambda *shape, dt=torch.bfloat16: torch.empty(*shape, dtype=dt, device="meta")
    o = torch.ops.mi355_touch.attn_decode_beam_(m(R, Nh, D), m(R, Nkv, D), m(R, Nkv, D), m(R, S, Nkv, D), m(R, S, Nkv, D),
                                                m(R, dt=torch.int32), m(R, S, dt=torch.int32), 0.125)
    assert o.shape == (R, Nh, D) and o.dtype == torch.bfloat16


def test_header_and_stub_declare_the_beam_entries():
    from touchnet_amd import _C
    text = open(os.path.join(ROOT, "include", "touchnet_amd.h")).read()
    assert "int tn_attn_decode_beam(" in text and "int tn_beam_step(" in text
    assert "inference_touch_audio.py:177-192" in text and "_beam_search" in text
    assert "tn_attn_decode_beam" in _C.PROTOTYPES and "tn_beam_step" in _C.PROTOTYPES


def test_c_entries_return_einval_before_any_launch():
    """Host addresses only: a launch would fault, -22 must come first."""
    from touchnet_amd import _C
    lib = _C.lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    a = ctypes.c_void_p((base + 63) // 64 * 64)
    odd = ctypes.c_void_p(a.value + 2)

    def attn(q=a, kn=a, vn=a, kc=a, vc=a, cl=a, src=a, o=a, ws=a, R=6, Nh=4, Nkv=1, D=64, S=200):
        return lib.tn_attn_decode_beam(q, kn, vn, kc, vc, cl, src, o, ws, R, Nh, Nkv, D, S, 0.125, None)
    assert attn(src=None) == -22 and attn(src=odd) == -22 and attn(q=None) == -22 and attn(kc=odd) == -22
    assert attn(D=96) == -22 and attn(Nh=5, Nkv=2) == -22 and attn(Nh=17) == -22 and attn(ws=None) == -22
    assert attn(R=0) == -22 and attn(S=0) == -22 and attn(cl=None) == -22

    eos = (ctypes.c_int * 4)(1, 2, 3, 4)

    def step(ptrs=None, B=2, K=3, K_in=3, V=128, S=32, pen=1.5, ngram=2, n_eos=1, n_new=8, lp=1.0, early=0, dtype=0,
             eos_p=eos):
        p = [a] * 17
        for i, v in (ptrs or {}).items():
            p[i] = v
        return lib.tn_beam_step(*p, B, K, K_in, V, S, pen, ngram, eos_p, n_eos, n_new, lp, early, dtype, None)
    for i in range(17):
        assert step({i: None}) == -22, i
    for i in range(1, 17):
        assert step({i: odd}) == -22, i
    assert step({0: ctypes.c_void_p(a.value + 1)}, dtype=1) == -22 and step({0: odd}) == -22
    assert step(K=1, K_in=1) == -22 and step(K=9, K_in=9) == -22 and step(K_in=2) == -22
    assert step(n_eos=4) == -22 and step(n_eos=-1) == -22 and step(n_eos=1, eos_p=None) == -22
    assert step(V=63) == -22 and step(V=262145) == -22 and step(pen=0.0) == -22 and step(pen=-1.0) == -22
    assert step(ngram=-1) == -22 and step(n_new=0) == -22 and step(early=3) == -22 and step(dtype=2) == -22
    assert step(B=0) == -22 and step(S=0) == -22
    assert lib.tn_beam_step_workspace_bytes(12, 4) == 12 * 4 * 32 * 8
