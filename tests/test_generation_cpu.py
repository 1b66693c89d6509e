"""KV-cache greedy decoding (touchnet_amd.generation, csrc/attn_decode.hip, csrc/generate.hip): everything that must hold
WITHOUT the device — the ASR prompt contract, op registration, host-side argument checks of the C entries, and the refusal
of CPU models."""
import ctypes as C

import pytest
import torch
from torch.nn.utils.rnn import pad_sequence

EINVAL = -22


def _reference_feature_extraction(feats, pad_id, bos_id):
    """The batch of touchnet/models/touch_audio/inference_touch_audio.py:51-100 (restated; the frontend stages left out):
    per utterance the n stacked rows + one zero row, ids pad x n + bos, positions 0..n, all LEFT-padded."""
    ids, fs, masks, positions = [], [], [], []
    for f in feats:
        feat = torch.cat([f, torch.zeros([1, f.size(1)], dtype=f.dtype)], dim=0)
        fs.append(feat)
        masks.append(torch.ones(feat.size(0), dtype=torch.int64))
        positions.append(torch.arange(0, feat.size(0), dtype=torch.int64))
        ids.append(torch.tensor([pad_id] * (feat.size(0) - 1) + [bos_id], dtype=torch.int64))
    return {"input_ids": pad_sequence(ids, batch_first=True, padding_side="left", padding_value=pad_id),
            "input_features": pad_sequence(fs, batch_first=True, padding_side="left", padding_value=0),
            "attention_mask": pad_sequence(masks, batch_first=True, padding_side="left", padding_value=0),
            "position_ids": pad_sequence(positions, batch_first=True, padding_side="left", padding_value=0)}


def test_prompt_builder_is_the_reference_batch_without_its_left_padding():
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts, prompt_positions
    g = torch.Generator().manual_seed(0)
    lens = [7, 1, 30, 12]
    feats = [torch.randn(n, 40, generator=g) for n in lens]
    pad_id, bos_id = 128004, 128000
    ref = _reference_feature_extraction(feats, pad_id, bos_id)
    pr = build_prompts(feats, pad_id, bos_id)
    pos = prompt_positions(pr)
    assert len(pr) == len(lens)
    for b, n in enumerate(lens):
        keep = ref["attention_mask"][b] == 1
        assert int(keep.sum()) == n + 1
        assert torch.equal(pr.input_ids[b], ref["input_ids"][b][keep])
        assert torch.equal(pr.input_features[b], ref["input_features"][b][keep])
        assert torch.equal(pos[b], ref["position_ids"][b][keep])
        assert pr.input_ids[b][-1] == bos_id and (pr.input_ids[b][:-1] == pad_id).all()
        assert (pr.input_features[b][-1] == 0).all()


def test_decode_ops_are_registered_with_declared_mutations_and_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import touchnet_amd.library as L
    for name in ("attn_decode_", "greedy_step_"):
        assert name in L.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"mi355_touch::{name}", "Meta"), name
    s = str(torch.ops.mi355_touch.attn_decode_.default._schema)
    assert "Tensor(a3!) k_cache" in s and "Tensor(a4!) v_cache" in s and s.endswith("-> Tensor"), s
    s = str(torch.ops.mi355_touch.greedy_step_.default._schema)
    for arg in ("hist", "hist_len", "cache_len", "finished", "n_unfinished"):
        assert f"!) {arg}" in s, (arg, s)
    assert "!) logits" not in s and s.endswith("-> ()"), s
    with FakeTensorMode():
        B, Nh, Nkv, D, S = 3, 28, 4, 128, 100
        q = torch.empty(B, Nh, D, dtype=torch.bfloat16, device="cuda")
        kn = torch.empty(B, Nkv, D, dtype=torch.bfloat16, device="cuda")
        kc = torch.empty(B, S, Nkv, D, dtype=torch.bfloat16, device="cuda")
        cl = torch.empty(B, dtype=torch.int32, device="cuda")
        o = torch.ops.mi355_touch.attn_decode_(q, kn, kn, kc, kc.clone(), cl, 0.088)
        assert o.shape == (B, Nh, D) and o.dtype == torch.bfloat16
        hist = torch.empty(B, S, dtype=torch.int32, device="cuda")
        r = torch.ops.mi355_touch.greedy_step_(torch.empty(B, 512, device="cuda"), hist, cl, cl.clone(), cl.clone(),
                                               torch.empty(1, dtype=torch.int32, device="cuda"), 1.5, 2, 2, 0)
        assert r is None


def test_decode_entry_points_refuse_malformed_arguments_before_any_launch():
    """tn_attn_decode / tn_greedy_step check their arguments on the host and return -22 without touching the device (the
    addresses below are host memory, never dereferenced by a refused call)."""
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    raw = (C.c_char * 8192)()
    p = (C.addressof(raw) + 255) // 256 * 256
    odd = p + 2

    def dec(q=p, kn=p, vn=p, kc=p, vc=p, cl=p, o=p, ws=p, B=2, Nh=32, Nkv=8, D=64, S=100):
        return lib.tn_attn_decode(q, kn, vn, kc, vc, cl, o, ws, B, Nh, Nkv, D, S, 0.125, None)
    assert dec(q=None) == EINVAL and dec(kc=None) == EINVAL and dec(cl=None) == EINVAL and dec(o=None) == EINVAL
    assert dec(q=odd) == EINVAL and dec(vc=odd) == EINVAL and dec(o=odd) == EINVAL and dec(cl=p + 2) == EINVAL
    assert dec(D=96) == EINVAL and dec(D=256) == EINVAL
    assert dec(Nh=30) == EINVAL                      # Nh % Nkv
    assert dec(Nh=136, Nkv=8) == EINVAL              # group 17
    assert dec(B=0) == EINVAL and dec(S=0) == EINVAL
    assert dec(ws=None, B=1, Nkv=1, Nh=16, S=4096) == EINVAL            # split launch without its workspace
    assert lib.tn_attn_decode_workspace_bytes(1, 16, 1, 64, 4096) > 0
    assert lib.tn_attn_decode_workspace_bytes(64, 32, 8, 64, 8192) == 0  # 512 workgroups already: no split

    def gs(lg=p, hist=p, hl=p, cl=p, fin=p, nu=p, B=2, V=128256, S=64, pen=1.5, n=2, dtype=1):
        return lib.tn_greedy_step(lg, hist, hl, cl, fin, nu, B, V, S, pen, n, 2, 0, dtype, None)
    assert gs(lg=None) == EINVAL and gs(hist=None) == EINVAL and gs(nu=None) == EINVAL
    assert gs(hl=p + 2) == EINVAL and gs(lg=p + 1) == EINVAL and gs(lg=p + 2, dtype=0) == EINVAL
    assert gs(V=0) == EINVAL and gs(V=262145) == EINVAL and gs(S=0) == EINVAL and gs(B=0) == EINVAL
    assert gs(n=-1) == EINVAL and gs(pen=0.0) == EINVAL and gs(dtype=2) == EINVAL


def test_generate_refuses_cpu_models():
    from touchnet_amd import _C
    from touchnet_amd.generation import GenerationConfig, Prompts, generate
    from touchnet_amd.models.llama import DecoderConfig, PackedCausalLM
    cfg = DecoderConfig(vocab_size=128, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                        num_key_value_heads=1, head_dim=64, eos_token_id=2)
    model = PackedCausalLM(cfg).to(torch.bfloat16)
    with pytest.raises(_C.KernelError, match="device"):
        generate(model, Prompts([torch.tensor([1, 5, 7])]), GenerationConfig(max_new_tokens=4))


def test_trim_at_eos():
    from touchnet_amd.generation import trim_at_eos
    ids = torch.tensor([[5, 6, 2, 0, 0], [7, 2, 0, 0, 0], [9, 9, 9, 9, 9]])
    assert trim_at_eos(ids, 2) == [[5, 6], [7], [9, 9, 9, 9, 9]]
