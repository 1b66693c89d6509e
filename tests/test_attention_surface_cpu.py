"""The Python surface of the attention kernels (touchnet_amd/library.py "attention", touchnet_amd/functional.py) WITHOUT the
device: every public entry point forward and backward on meta tensors (the fakes and the registered autograd formulas
decide shapes, dtypes and layouts there), the one restatement of a C header rule that Python holds, and the autograd
registration of the bidirectional op."""
import pytest
import torch

import touchnet_amd.functional as F
import touchnet_amd.library as L

BF = torch.bfloat16


@pytest.mark.parametrize("B", [1, 2, 3])
def test_metadata_size_formula_is_the_headers(B):
    """library.attn_meta_ints (what the fake of attn_build_meta allocates) == tn_attn_meta_ints (csrc/attn_common.h)."""
    from touchnet_amd import _C, build
    build.build()
    lib = _C.lib()
    for T in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 700, 8192):
        assert L.attn_meta_ints(B, T) == lib.tn_attn_meta_ints(B, T), (B, T)
        doc = torch.empty(B, T, dtype=torch.int32, device="meta")
        assert torch.ops.mi355_touch.attn_build_meta(doc).shape == (lib.tn_attn_meta_ints(B, T),)


SHARD = F.SeqShard(((0, 128, 0), (128, 128, 384)), 256)
ENTRY_POINTS = {
    "packed_attention": (None, lambda q, k, v, m, rope: F.packed_attention(q, k, v, m)),
    "packed_attention_rope_grad": (None, lambda q, k, v, m, rope: F.packed_attention(q, k, v, m, rope_grad=rope)),
    "bidirectional_attention": (None, lambda q, k, v, m, rope: F.bidirectional_attention(q, k, v, m)),
    "packed_attention_sharded": (SHARD, lambda q, k, v, m, rope: F.packed_attention_sharded(q, k, v, m, SHARD)),
    "packed_attention_sharded_split": (SHARD, lambda q, k, v, m, rope: F.packed_attention_sharded_split(
        q, k, v, m, SHARD, 128, (0, 3), (1, 2))),
}


@pytest.mark.parametrize("Nh,Nkv", [(4, 2), (2, 2)])
@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_every_entry_point_forward_and_backward_on_the_meta_device(entry, Nh, Nkv):
    """q arrives as a non-contiguous view ([B, Nh, R, D] transposed); the output is q-shaped, bf16 and contiguous, and
    every gradient has its input's shape — whichever layout (three tensors, stacked, flat) the backward op returns."""
    B, T, D = 2, 512, 64
    shard, call = ENTRY_POINTS[entry]
    R = T if shard is None else shard.rows_per_batch
    e = lambda *s: torch.empty(*s, device="meta", dtype=BF)
    q = e(B, Nh, R, D).transpose(1, 2).requires_grad_()
    k, v = e(B, T, Nkv, D).requires_grad_(), e(B, T, Nkv, D).requires_grad_()
    assert not q.is_contiguous()
    mask = F.build_packed_mask(torch.empty(B, T, dtype=torch.int64, device="meta"))
    out = call(q, k, v, mask, (e(B * T, D // 2), e(B * T, D // 2)))
    assert out.shape == q.shape and out.dtype == BF and out.is_contiguous()
    grads = torch.autograd.grad(out, [q, k, v], torch.empty_like(out))
    for g, x in zip(grads, (q, k, v)):
        assert g.shape == x.shape and g.dtype == BF


def test_bidirectional_forward_op_has_an_autograd_formula():
    """torch.ops.mi355_touch.attn_fwd_bidir differentiates by its registration (no autograd.Function around it)."""
    B, T, Nh, D = 1, 128, 2, 64
    q, k, v = (torch.empty(B, T, Nh, D, device="meta", dtype=BF, requires_grad=True) for _ in range(3))
    doc = torch.empty(B, T, dtype=torch.int32, device="meta")
    meta = torch.ops.mi355_touch.attn_build_meta(doc)
    o, lse2 = torch.ops.mi355_touch.attn_fwd_bidir(q, k, v, doc, meta, 0.125)
    assert o.requires_grad and o.grad_fn is not None
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], torch.empty_like(o))
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    assert not hasattr(F, "_BidirectionalAttention")
