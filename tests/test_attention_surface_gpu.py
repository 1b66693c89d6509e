"""The Python surface of the attention kernels on the device (touchnet_amd/library.py "attention"): torch.library.opcheck
of the forward ops that gained a shared registration, the three gradient layouts against each other bit for bit, and the
forward prologue's refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16


def _rand(*shape, seed, dtype=BF, grad=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g).to(dtype).requires_grad_(grad)


def test_opcheck_of_the_bidirectional_forward_op():
    """schema, fake-vs-real agreement, autograd registration and AOT dispatch of attn_fwd_bidir, as attn_fwd gets them in
    test_library.test_opcheck_on_device"""
    from torch.library import opcheck
    B, T, Nh, Nkv, D = 2, 256, 4, 2, 64
    q, k, v = (_rand(B, T, n, D, seed=s, grad=True) for s, n in ((1, Nh), (2, Nkv), (3, Nkv)))
    doc = torch.ones(B, T, dtype=torch.int32, device=DEV)
    doc[1, 200:] = 0
    meta = torch.ops.mi355_touch.attn_build_meta(doc)
    opcheck(torch.ops.mi355_touch.attn_fwd_bidir.default, (q, k, v, doc, meta, 0.125),
            test_utils=("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic"))


def test_opcheck_of_the_sharded_forward_op():
    from torch.library import opcheck
    B, T, R, Nh, Nkv, D = 2, 512, 256, 4, 2, 64
    q = _rand(B, R, Nh, D, seed=4, grad=True)
    k, v = _rand(B, T, Nkv, D, seed=5, grad=True), _rand(B, T, Nkv, D, seed=6, grad=True)
    doc = torch.ones(B, T, dtype=torch.int32, device=DEV)
    meta = torch.ops.mi355_touch.attn_build_meta(doc)
    opcheck(torch.ops.mi355_touch.attn_fwd_seg.default, (q, k, v, doc, meta, 0.125, [0, 128, 0, 128, 128, 384], R),
            test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


@pytest.mark.parametrize("D", [64, 128])
def test_gradient_layouts_agree_bit_for_bit(D):
    """Ragged T, two documents and a padded tail, Nh == Nkv: the stacked buffer holds the bits of the three tensors, the
    rope backward's stacked and flat buffers hold the same bits, and the bidirectional backward's three gradients are
    tensors of their own (back-to-back gradients would re-route the audio tower's q/k/v weight gradient,
    functional._stacked_view)."""
    import touchnet_amd.functional as F
    import touchnet_amd.library as L
    B, T, Nh = 2, 200, 2
    doc = torch.tensor([1] * 90 + [2] * 70 + [0] * 40, dtype=torch.int32).repeat(B, 1).to(DEV)
    q, k, v, do = (_rand(B, T, Nh, D, seed=10 * D + i) for i in range(4))
    mask = F.build_packed_mask(doc)
    scale = D ** -0.5
    o, lse2 = L.attn_fwd(q, k, v, mask.doc, mask.meta, scale)
    args = (q, k, v, o, do, lse2, mask.doc, mask.meta, scale)
    three = L.attn_bwd(*args)
    stacked = L.attn_bwd_stacked(*args)
    assert stacked.shape == (3, B, T, Nh, D)
    for name, a, b in zip(("dq", "dk", "dv"), three, stacked.unbind(0)):
        assert torch.equal(a, b), name
    pos = torch.arange(T, device=DEV).repeat(B, 1)
    cos, sin = F.rope_tables(pos, F.rope_inv_freq(D, 1000000.0, device=DEV), BF)
    rs, rf = L.attn_bwd_rope(*args, cos, sin, True), L.attn_bwd_rope(*args, cos, sin, False)
    assert rs.shape == (3, B, T, Nh, D) and rf.shape == (3 * B * T * Nh * D,)
    for name, a, b in zip(("dq", "dk", "dv"), L.attn_grads(q, k, "stacked", rs)[1], L.attn_grads(q, k, "flat", rf)[1]):
        assert a.shape == b.shape == q.shape and torch.equal(a, b), name
    ob, lb = L.attn_fwd_bidir(q, k, v, mask.doc, mask.meta, scale)
    grads = L.attn_bwd_bidir(q, k, v, ob, do, lb, mask.doc, mask.meta, scale)
    assert len({g.untyped_storage().data_ptr() for g in grads}) == 3
    assert all(g.untyped_storage().nbytes() == g.numel() * 2 for g in grads)


def test_forward_ops_refuse_other_dtypes_and_masks_of_another_shape():
    """Each of the four forward ops raises from the shared prologue, before anything is launched."""
    import touchnet_amd.library as L
    from touchnet_amd import _C
    B, T, R, Nh, Nkv, D = 2, 256, 128, 4, 2, 64
    k, v = _rand(B, T, Nkv, D, seed=7), _rand(B, T, Nkv, D, seed=8)
    doc = torch.ones(B, T, dtype=torch.int32, device=DEV)
    meta = L.attn_build_meta(doc)
    segs = [0, R, 128]
    ops = {"attn_fwd": (L.attn_fwd, T, ()), "attn_fwd_bidir": (L.attn_fwd_bidir, T, ()),
           "attn_fwd_seg": (L.attn_fwd_seg, R, (segs, R)), "attn_fwd_seg_chunks": (L.attn_fwd_seg_chunks, R, (segs, R, 128, 3))}
    for name, (op, rows, tail) in ops.items():
        q = _rand(B, rows, Nh, D, seed=9)
        op(q, k, v, doc, meta, 0.125, *tail)                                     # (the well-formed call is served)
        with pytest.raises(_C.KernelError, match="bf16"):
            op(q.to(torch.float16), k.to(torch.float16), v.to(torch.float16), doc, meta, 0.125, *tail)
        for bad in (doc[:, :T - 64].contiguous(), doc[:1]):
            with pytest.raises(_C.KernelError, match="mask built for"):
                op(q, k, v, bad, meta, 0.125, *tail)
    torch.cuda.synchronize()
