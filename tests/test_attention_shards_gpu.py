"""The sequence-sharded attention entry points (tn_attn_fwd_seg, tn_attn_fwd_seg_chunks, tn_attn_merge, tn_attn_bwd_seg)
at every KIND of shard the segment contract admits (include/touchnet_amd.h), each at the smallest shape that reaches it:
one segment, one segment at an offset, a ragged end inside the row, unequal segments with a gap, segments in descending
global order, the whole row, a ragged T.  The suite's other shard tests only ever build two equal 128-aligned head/tail
segments.

Reference: oracle.nn.attention with doc_causal_allow in fp32 on the CPU, on the bf16-rounded inputs, as
test_packed_attention_fwd_bwd uses it.  Forward = its rows at the shard's global positions.  Backward = ONE oracle backward
with dO zero everywhere but at the shard's rows: its dQ rows are the local dQ, its dK / dV are the shard's PARTIAL dK / dV.
Tolerances are that test's: O 2e-2 / 2e-2; dQ, dK, dV 4e-2 / 3e-2 (a few bf16 ulps of O(1) values; P rounded to bf16)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nn as onn
from test_kernels_gpu import DEV, _close, _docs, _f, _ref

# case -> (T, B, Nh, Nkv, segments (row0, rows, off), rows_per_batch, what it reaches)
CASES = {
    "A": (512, 2, 4, 2, ((0, 256, 0),), 256),                    # one segment, offset 0, rows < T
    "B": (512, 2, 4, 2, ((0, 256, 256),), 256),                  # one segment at an offset (contiguous split, last rank)
    "C": (512, 2, 4, 2, ((0, 200, 128),), 200),                  # ragged end inside the row: a partial 128-row tile
    "D": (512, 2, 4, 2, ((0, 256, 0), (256, 128, 384)), 384),    # unequal segments, a gap in the global positions
    "E": (512, 2, 4, 2, ((0, 128, 384), (128, 128, 0)), 256),    # descending global order
    "F": (512, 2, 4, 2, ((0, 512, 0),), 512),                    # the whole row through the seg entry
    "G": (700, 1, 4, 2, ((0, 128, 128), (128, 188, 512)), 316),  # ragged T, second segment ends at T; B * nt = 11
    "H": (700, 1, 4, 2, ((0, 444, 256),), 444),                  # one segment running to a ragged T
    # kv tile 0 meets 68 > kListPre (64) query tiles of the row, later kv tiles <= 64; one document only
    "I": (4352, 1, 2, 2, ((0, 1024, 0),), 1024),
}
# every segment ends at a multiple of 128 or at T: the kernel's tiles are the full-sequence kernel's, bit for bit
SAME_TILES = "ABDEFGH"
LAYOUTS = ["one_document", "short_documents"]
PARAMS = [(c, D, lay) for c in CASES for D in (64, 128) for lay in LAYOUTS if not (c == "I" and lay != "one_document")]


def _layout(B, T, layout):
    if layout == "one_document":
        return torch.ones(B, T, dtype=torch.int64)
    return _docs(B, T, T + B, 90, 40)        # many short documents, a padded tail


@functools.lru_cache(maxsize=None)
def _problem(T, B, Nh, Nkv, D, layout):
    """Inputs, the oracle's forward (graph kept: every shard differentiates it with its own dO) and the full-sequence
    kernel's forward / backward — computed once per shape, read by every case of that shape, never written."""
    F = _f()
    doc = _layout(B, T, layout)
    g = torch.Generator().manual_seed(1000 * T + D + len(layout))
    q, k, v, do = [torch.randn(B, T, n, D, generator=g).bfloat16() for n in (Nh, Nkv, Nkv, Nh)]
    qr, kr, vr = [_ref(t) for t in (q, k, v)]
    allow = onn.doc_causal_allow(doc)
    ref = onn.attention(qr.transpose(1, 2), kr.transpose(1, 2), vr.transpose(1, 2), allow, D ** -0.5)
    mask = F.build_packed_mask(doc.to(DEV))
    qd, kd, vd, dod = [t.to(DEV) for t in (q, k, v, do)]
    qf, kf, vf = [t.clone().requires_grad_() for t in (qd, kd, vd)]
    of = F.packed_attention(qf, kf, vf, mask)
    of.backward(dod)
    torch.cuda.synchronize()
    return dict(doc=doc, allow=allow, q=qd, k=kd, v=vd, do=dod, do_cpu=do.float(), leaves=(qr, kr, vr), ref=ref,
                mask=mask, of=of.detach(), dq_full=qf.grad, dk_full=kf.grad, dv_full=vf.grad)


def _positions(segs, rpb):
    """Global position of every local row (every case covers all of its local rows)."""
    pos = torch.full((rpb,), -1, dtype=torch.int64)
    for row0, rows, off in segs:
        pos[row0:row0 + rows] = torch.arange(off, off + rows)
    assert int(pos.min()) >= 0
    return pos


def _oracle_backward(p, pos):
    """dO zero everywhere but at the shard's rows -> (dQ, partial dK, partial dV) of the oracle, [B, T, heads, D]."""
    do = torch.zeros_like(p["do_cpu"])
    do[:, pos] = p["do_cpu"][:, pos]
    return torch.autograd.grad(p["ref"], p["leaves"], do, retain_graph=True)


def _unseen_keys(doc, pos):
    """[B, T] bool: key positions no query of the shard may see (no local q >= kv in the same document)."""
    B, T = doc.shape
    local = torch.zeros(T, dtype=torch.bool)
    local[pos] = True
    seen = (onn.doc_causal_allow(doc) & local[None, :, None]).any(1)
    return ~seen


def _exact_zero(t, where, what):
    if where.any():
        assert float(t.detach().float().cpu()[where].abs().max()) == 0.0, f"{what} must be exactly 0"


@pytest.mark.parametrize("case,D,layout", PARAMS)
def test_sharded_attention_against_the_oracle(case, D, layout):
    F = _f()
    T, B, Nh, Nkv, segs, rpb = CASES[case]
    p = _problem(T, B, Nh, Nkv, D, layout)
    pos = _positions(segs, rpb)
    shard = F.SeqShard(segs, rpb)
    ql = p["q"][:, pos].clone().requires_grad_()
    kl, vl = p["k"].clone().requires_grad_(), p["v"].clone().requires_grad_()
    ol = F.packed_attention_sharded(ql, kl, vl, p["mask"], shard)
    ol.backward(p["do"][:, pos].contiguous())
    torch.cuda.synchronize()
    dq_ref, dk_ref, dv_ref = _oracle_backward(p, pos)

    _close(ol, p["ref"][:, pos], 2e-2, 2e-2, f"case {case}: O")
    _close(ql.grad, dq_ref[:, pos], 4e-2, 3e-2, f"case {case}: dQ")
    _close(kl.grad, dk_ref, 4e-2, 3e-2, f"case {case}: partial dK")
    _close(vl.grad, dv_ref, 4e-2, 3e-2, f"case {case}: partial dV")
    pad = p["doc"][:, pos] == 0
    _exact_zero(ol, pad, "O of pad rows")
    _exact_zero(ql.grad, pad, "dQ of pad rows")
    # key rows no local query may see: the oracle's partial gradient is exactly 0 over the whole head row there (masked
    # probabilities are exact zeros, so are the products with a zero dO row), and it is so nowhere else
    zero = (dk_ref == 0).all(-1) & (dv_ref == 0).all(-1)                       # [B, T, Nkv]
    assert torch.equal(zero, _unseen_keys(p["doc"], pos)[:, :, None].expand_as(zero))
    _exact_zero(kl.grad, zero, "dK of key rows no local query sees")
    _exact_zero(vl.grad, zero, "dV of key rows no local query sees")

    if case in SAME_TILES:
        idx = pos.to(DEV)
        assert torch.equal(ol, p["of"][:, idx]), f"case {case}: forward differs from the full-sequence kernel's rows"
        _close(ql.grad, p["dq_full"][:, idx], 1e-6, 0, f"case {case}: dQ vs the full-sequence kernel")
    if case == "F":
        assert torch.equal(kl.grad, p["dk_full"]) and torch.equal(vl.grad, p["dv_full"])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_chunk_restricted_forward_and_merge_at_a_ragged_length(D, layout):
    """tn_attn_fwd_seg_chunks + tn_attn_merge away from T = 65536: T = 700, the segments of case G, four key chunks of 192
    positions (the last one 124 long), part a = chunks {0, 2}, part b = chunks {1, 3}.  2 ** -7 is the project's figure for
    a merge of bf16-rounded partial results (test_config_d_local_remote_split_with_lse_merge_equals_the_single_kernel)."""
    F = _f()
    from touchnet_amd import library as Lb
    T, B, Nh, Nkv, segs, rpb = CASES["G"]
    chunk = 192
    p = _problem(T, B, Nh, Nkv, D, layout)
    pos = _positions(segs, rpb)
    shard = F.SeqShard(segs, rpb)
    flat, scale = shard.flat(), D ** -0.5
    mask = p["mask"]
    ql = p["q"][:, pos].contiguous()
    qr, kr, vr = [t.detach() for t in p["leaves"]]
    parts = {}
    for name, chunks in (("a", (0, 2)), ("b", (1, 3))):
        o, lse = Lb.attn_fwd_seg_chunks(ql, p["k"], p["v"], mask.doc, mask.meta, scale, flat, rpb, chunk,
                                        sum(1 << c for c in chunks))
        torch.cuda.synchronize()
        in_set = torch.zeros(T, dtype=torch.bool)
        for c in chunks:
            in_set[c * chunk:(c + 1) * chunk] = True
        allow = p["allow"] & in_set[None, None, :]
        want = onn.attention(qr.transpose(1, 2), kr.transpose(1, 2), vr.transpose(1, 2), allow, scale)[:, pos]
        _close(o, want, 2e-2, 2e-2, f"part {name}: O")
        empty = ~allow.any(-1)[:, pos]                                          # [B, rpb]: no allowed key in the set
        got_empty = torch.isinf(lse).cpu()                                      # [B, Nh, rpb]
        assert torch.equal(got_empty, empty[:, None, :].expand_as(got_empty)), f"part {name}: rows without a key"
        assert bool((lse[torch.isinf(lse)] > 0).all())
        _exact_zero(o, empty, f"part {name}: O of rows without a key")
        parts[name] = (o, lse, int(empty.sum()))
    assert parts["a"][2] + parts["b"][2] > 0, "the case is meant to hold rows that see no key of a part"
    merged, _ = Lb.attn_merge(*parts["a"][:2], *parts["b"][:2])
    single, _ = Lb.attn_fwd_seg(ql, p["k"], p["v"], mask.doc, mask.meta, scale, flat, rpb)
    _close(merged, single, 2 ** -7, 2 ** -7, "merged parts vs the single kernel over all keys")
    _close(merged, p["ref"][:, pos], 2 ** -7 + 2e-2, 2 ** -7 + 2e-2, "merged parts vs the oracle")

    qs = ql.clone().requires_grad_()
    ks, vs = p["k"].clone().requires_grad_(), p["v"].clone().requires_grad_()
    out = F.packed_attention_sharded_split(qs, ks, vs, mask, shard, chunk, (0, 2), (1, 3))
    out.backward(p["do"][:, pos].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(out, merged)
    dq_ref, dk_ref, dv_ref = _oracle_backward(p, pos)
    _close(qs.grad, dq_ref[:, pos], 4e-2, 3e-2, "split node: dQ")
    _close(ks.grad, dk_ref, 4e-2, 3e-2, "split node: partial dK")
    _close(vs.grad, dv_ref, 4e-2, 3e-2, "split node: partial dV")
