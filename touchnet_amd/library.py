"""PyTorch-ROCm custom ops `torch.ops.mi355_touch.*` over the C ABI of libtouchnet_amd.so (SURVEY §8b "C-ABI realisation").

Each op has a schema (inferred from the annotations), a device implementation that only ENQUEUES the HIP kernel on the
current stream (outputs come from the caching allocator; no sync), a `register_fake` meta kernel (shapes / dtypes only:
meta-device construction, FakeTensor tracing, `torch.compile` of the surrounding module, activation-checkpoint
policies that list ops — touchnet/models/helper_func.py:39-96 — all see the ops without executing them) and a
`register_autograd` formula whose backward is again an op of this namespace.  `touchnet_amd.functional` is the
user-facing layer on top (it adds argument normalisation and the multi-op autograd nodes of the linear layers).

Conventions: activations are [..., H] dense; "rows" = product of the leading dims.  No op returns an alias of an input
(the dispatcher forbids it): where the kernel would pass an input through (the residual stream without an add), the op
returns an EMPTY placeholder and the autograd formula keeps the input itself.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.library import custom_op

from . import _C

NS = "mi355_touch"
_p, _cur = _C.ptr, _C.stream


def _lib():
    return _C.lib()


def _c(t: Tensor) -> Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _empty0(like: Tensor) -> Tensor:
    return like.new_empty(0)


# ===================================================================================================== norms
# RMSNorm and LayerNorm are two ops each way that differ by one tensor (the bias in, the mean out, db back); the reshapes,
# allocations, meta results and the autograd formula are stated once for both.
def _norm_fwd_buffers(x: Tensor, residual: Optional[Tensor]):
    """-> (x2, r2, y, h): x and the residual as [rows, H]; y and, with a residual, h = x + residual for the kernel to fill"""
    H = x.shape[-1]
    x2 = _c(x).view(-1, H)
    r2 = _c(residual).view(-1, H) if residual is not None else None
    return x2, r2, torch.empty_like(x2), (torch.empty_like(x2) if r2 is not None else None)


def _norm_fwd_fake(x, residual, nstats):
    e = lambda: torch.empty_like(x, memory_format=torch.contiguous_format)
    rows = x.numel() // x.shape[-1]
    return (e(), e() if residual is not None else x.new_empty(0),
            *(x.new_empty(rows, dtype=torch.float32) for _ in range(nstats)))


def _norm_bwd_buffers(dy: Tensor, h: Tensor, dres: Optional[Tensor]):
    """-> (dy2, h2, dr2, dh, ws): the operands as [rows, H], dh for the kernel to fill, the partial sums' workspace"""
    H = h.shape[-1]
    h2 = _c(h).view(-1, H)
    rows = h2.shape[0]
    dy2 = _c(dy).view(rows, H)
    dr2 = _c(dres).view(rows, H) if dres is not None else None
    ws = torch.empty(_lib().tn_norm_bwd_workspace_floats(rows, H), dtype=torch.float32, device=h.device)
    return dy2, h2, dr2, torch.empty_like(h2), ws


def _norm_setup(ctx, inputs, output):
    """inputs = (x, residual, weight, ...), output = (y, h, *statistics)"""
    x, residual, weight = inputs[:3]
    ctx.has_res = residual is not None
    ctx.wdtype = weight.dtype
    ctx.set_materialize_grads(False)     # (no zero tensors for the statistics outputs' gradients: 2-3 tiny fills per norm)
    ctx.save_for_backward(output[1] if ctx.has_res else x, weight, *output[2:])


def _norm_backward(bwd_op):
    """the autograd formula over `bwd_op(dy, h, weight, *statistics, dres) -> (dh, *parameter gradients)`"""
    def backward(ctx, dy, dh_new, *_dstats):
        h, weight, *stats = ctx.saved_tensors
        dres = dh_new if (ctx.has_res and dh_new is not None) else None
        if dy is None:
            dy = torch.zeros_like(h)
        dh, *dparams = bwd_op(dy, h, weight, *stats, dres)
        return (dh, dh if ctx.has_res else None, *[d.to(ctx.wdtype) for d in dparams], None)
    return backward


@custom_op(f"{NS}::rmsnorm_fwd", mutates_args=(), device_types="cuda")
def rmsnorm_fwd(x: Tensor, residual: Optional[Tensor], weight: Tensor, eps: float) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (y, h, rstd): h = x + residual (EMPTY when residual is None: then h == x), y = w * T(h * rstd)."""
    x2, r2, y, h = _norm_fwd_buffers(x, residual)
    rows, H = x2.shape
    w = _c(weight).to(x.dtype)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _C.check(_lib().tn_rmsnorm_fwd(_p(x2), _p(r2), _p(w), _p(y), _p(h), _p(rstd), rows, H, float(eps), _C.dcode(x2),
                                   _cur()), "tn_rmsnorm_fwd")
    return y.view(x.shape), (h.view(x.shape) if h is not None else _empty0(x)), rstd


@rmsnorm_fwd.register_fake
def _(x, residual, weight, eps):
    return _norm_fwd_fake(x, residual, 1)


@custom_op(f"{NS}::rmsnorm_bwd", mutates_args=(), device_types="cuda")
def rmsnorm_bwd(dy: Tensor, h: Tensor, weight: Tensor, rstd: Tensor, dres: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """-> (dh, dw): dh includes the incoming residual-stream gradient `dres`."""
    dy2, h2, dr2, dh, ws = _norm_bwd_buffers(dy, h, dres)
    rows, H = h2.shape
    w = _c(weight).to(h.dtype)
    dw = torch.empty(H, dtype=h.dtype, device=h.device)
    _C.check(_lib().tn_rmsnorm_bwd(_p(dy2), _p(h2), _p(w), _p(rstd), _p(dr2), _p(dh), _p(dw), _p(ws), rows, H,
                                   _C.dcode(h2), _cur()), "tn_rmsnorm_bwd")
    return dh.view(h.shape), dw


@rmsnorm_bwd.register_fake
def _(dy, h, weight, rstd, dres):
    return torch.empty_like(h, memory_format=torch.contiguous_format), h.new_empty(h.shape[-1])


rmsnorm_fwd.register_autograd(_norm_backward(rmsnorm_bwd), setup_context=_norm_setup)


@custom_op(f"{NS}::layernorm_fwd", mutates_args=(), device_types="cuda")
def layernorm_fwd(x: Tensor, residual: Optional[Tensor], weight: Tensor, bias: Tensor,
                  eps: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (y, h, mean, rstd); h EMPTY when residual is None."""
    x2, r2, y, h = _norm_fwd_buffers(x, residual)
    rows, H = x2.shape
    w, b = _c(weight).to(x.dtype), _c(bias).to(x.dtype)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    _C.check(_lib().tn_layernorm_fwd(_p(x2), _p(r2), _p(w), _p(b), _p(y), _p(h), _p(mean), _p(rstd), rows, H,
                                     float(eps), _C.dcode(x2), _cur()), "tn_layernorm_fwd")
    return y.view(x.shape), (h.view(x.shape) if h is not None else _empty0(x)), mean, rstd


@layernorm_fwd.register_fake
def _(x, residual, weight, bias, eps):
    return _norm_fwd_fake(x, residual, 2)


@custom_op(f"{NS}::layernorm_bwd", mutates_args=(), device_types="cuda")
def layernorm_bwd(dy: Tensor, h: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor,
                  dres: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (dh, dw, db): dh includes the incoming residual-stream gradient `dres`."""
    dy2, h2, dr2, dh, ws = _norm_bwd_buffers(dy, h, dres)
    rows, H = h2.shape
    w = _c(weight).to(h.dtype)
    dw = torch.empty(H, dtype=h.dtype, device=h.device)
    db = torch.empty_like(dw)
    _C.check(_lib().tn_layernorm_bwd(_p(dy2), _p(h2), _p(w), _p(mean), _p(rstd), _p(dr2), _p(dh), _p(dw), _p(db),
                                     _p(ws), rows, H, _C.dcode(h2), _cur()), "tn_layernorm_bwd")
    return dh.view(h.shape), dw, db


@layernorm_bwd.register_fake
def _(dy, h, weight, mean, rstd, dres):
    return (torch.empty_like(h, memory_format=torch.contiguous_format), h.new_empty(h.shape[-1]),
            h.new_empty(h.shape[-1]))


layernorm_fwd.register_autograd(_norm_backward(layernorm_bwd), setup_context=_norm_setup)


# ===================================================================================================== activations
@custom_op(f"{NS}::swiglu_fwd", mutates_args=(), device_types="cuda")
def swiglu_fwd(gate: Tensor, up: Tensor) -> Tensor:
    g, u = _c(gate), _c(up)
    out = torch.empty_like(g)
    _C.check(_lib().tn_swiglu_fwd(_p(g), _p(u), _p(out), g.numel(), _C.dcode(g), _cur()), "tn_swiglu_fwd")
    return out


@swiglu_fwd.register_fake
def _(gate, up):
    return torch.empty_like(gate, memory_format=torch.contiguous_format)


@custom_op(f"{NS}::swiglu_bwd", mutates_args=(), device_types="cuda")
def swiglu_bwd(dout: Tensor, gate: Tensor, up: Tensor) -> Tuple[Tensor, Tensor]:
    d, g, u = _c(dout), _c(gate), _c(up)
    dg, du = torch.empty_like(g), torch.empty_like(u)
    _C.check(_lib().tn_swiglu_bwd(_p(d), _p(g), _p(u), _p(dg), _p(du), g.numel(), _C.dcode(g), _cur()),
             "tn_swiglu_bwd")
    return dg, du


@swiglu_bwd.register_fake
def _(dout, gate, up):
    e = lambda t: torch.empty_like(t, memory_format=torch.contiguous_format)
    return e(gate), e(up)


swiglu_fwd.register_autograd(lambda ctx, d: swiglu_bwd(d, *ctx.saved_tensors),
                             setup_context=lambda ctx, inputs, output: ctx.save_for_backward(*inputs))


@custom_op(f"{NS}::gelu_fwd", mutates_args=(), device_types="cuda")
def gelu_fwd(x: Tensor) -> Tensor:
    x = _c(x)
    out = torch.empty_like(x)
    _C.check(_lib().tn_gelu_fwd(_p(x), _p(out), x.numel(), _C.dcode(x), _cur()), "tn_gelu_fwd")
    return out


@gelu_fwd.register_fake
def _(x):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@custom_op(f"{NS}::gelu_bwd", mutates_args=(), device_types="cuda")
def gelu_bwd(dout: Tensor, x: Tensor) -> Tensor:
    d, x = _c(dout), _c(x)
    dx = torch.empty_like(x)
    _C.check(_lib().tn_gelu_bwd(_p(d), _p(x), _p(dx), x.numel(), _C.dcode(x), _cur()), "tn_gelu_bwd")
    return dx


@gelu_bwd.register_fake
def _(dout, x):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


gelu_fwd.register_autograd(lambda ctx, d: gelu_bwd(d, *ctx.saved_tensors),
                           setup_context=lambda ctx, inputs, output: ctx.save_for_backward(*inputs))


# ===================================================================================================== RoPE
@custom_op(f"{NS}::rope_apply", mutates_args=(), device_types="cuda")
def rope_apply(q: Tensor, k: Tensor, cos: Tensor, sin: Tensor, backward: bool) -> Tuple[Tensor, Tensor]:
    """q [B,T,Nh,D], k [B,T,Nkv,D]; cos/sin [B*T, D/2].  `backward` applies the transposed rotation (gradients)."""
    q, k = _c(q), _c(k)
    B, T, hq, D = q.shape
    hk = k.shape[2]
    qo, ko = torch.empty_like(q), torch.empty_like(k)
    _C.check(_lib().tn_rope_apply(_p(q), _p(k), _p(qo), _p(ko), _p(cos), _p(sin), B * T, hq, hk, D, int(backward),
                                  _C.dcode(q), _cur()), "tn_rope_apply")
    return qo, ko


@rope_apply.register_fake
def _(q, k, cos, sin, backward):
    e = lambda t: torch.empty_like(t, memory_format=torch.contiguous_format)
    return e(q), e(k)


def _rope_setup(ctx, inputs, output):
    _, _, cos, sin, backward = inputs
    ctx.save_for_backward(cos, sin)
    ctx.backward_flag = backward


def _rope_backward(ctx, dq, dk):
    cos, sin = ctx.saved_tensors
    gq, gk = rope_apply(dq, dk, cos, sin, not ctx.backward_flag)
    return gq, gk, None, None, None


rope_apply.register_autograd(_rope_backward, setup_context=_rope_setup)


# ===================================================================================================== attention
# The ops differ in their C entry and its trailing arguments; every rule they share is stated once:
#   _attn_forward / _attn_forward_fake   the forward prologue (checks, o and lse2 [B, Nh, rows]) of the four forward ops
#   attn_grads                           the three layouts of (dq, dk, dv): real ops, fakes and functional read it
#   _attn_backward                       the backward prologue (do, the delta scratch, the gradients) of the five backward ops
#   _attn_autograd                       setup_context / backward of the forward ops that have a backward op
def _attn_forward(name: str, entry: str, q: Tensor, k: Tensor, v: Tensor, doc: Tensor, meta: Tensor, scale: float,
                  tail=(), rows_per_batch: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """q [B, rows, Nh, D], k / v [B, T, Nkv, D] bf16, doc int32 [B, T], meta from `attn_build_meta` ->
    (o [B, rows, Nh, D], lse2 fp32 [B, Nh, rows]) by the C entry `entry(.., scale, *tail, stream)`.  rows = T, or the
    `rows_per_batch` of a sequence-sharded query side; `name` is the public function the messages speak of."""
    q, k, v = _c(q), _c(k), _c(v)
    B, R, Nh, D = q.shape
    T, Nkv = k.shape[1], k.shape[2]
    if q.dtype != torch.bfloat16:
        raise _C.KernelError(f"{name}: bf16 only (MFMA 32x32x16 bf16 kernels), got q {q.dtype}")
    rows = T if rows_per_batch is None else rows_per_batch
    if tuple(doc.shape) != (B, T) or R != rows:
        raise _C.KernelError(f"{name}: mask built for {tuple(doc.shape)}, {rows} query rows per batch; "
                             f"got q {(B, R)}, k {(B, T)}")
    o = torch.empty_like(q)
    lse2 = torch.empty(B, Nh, R, dtype=torch.float32, device=q.device)
    _C.check(getattr(_lib(), entry)(_p(q), _p(k), _p(v), _p(o), _p(lse2), _p(doc), _p(meta), B, T, Nh, Nkv, D,
                                    float(scale), *tail, _cur()), entry)
    return o, lse2


def _attn_forward_fake(q, k, v, doc, meta, scale, *tail):
    B, R, Nh, D = q.shape
    return torch.empty_like(q, memory_format=torch.contiguous_format), q.new_empty(B, Nh, R, dtype=torch.float32)


def attn_grads(q: Tensor, k: Tensor, layout: str, out=None):
    """-> (out, (dq, dk, dv)): what a backward op of `layout` returns, and its three gradients as q- / k- / v-shaped views.
         "tuple"    three tensors of their own
         "stacked"  ONE buffer [3, B, T, Nh, D] (Nh == Nkv), dq, dk, dv = its slices: a consumer that wants them side by
                    side — the fused q/k/v weight gradient of the audio tower — runs a batched GEMM over the buffer instead
                    of concatenating three tensors first (functional._LinearGroup, wgrad="nt_fused")
         "flat"     ONE buffer [B * T * (Nh + 2 Nkv) * D] = dq | dk | dv
    `out` = None allocates (works on fake tensors too); otherwise the views are taken of that result of a backward op."""
    if layout == "tuple":
        out = out if out is not None else (q.new_empty(q.shape), k.new_empty(k.shape), k.new_empty(k.shape))
        return out, tuple(out)
    if layout == "stacked":
        if q.shape != k.shape:
            raise _C.KernelError(f"stacked attention gradients need Nh == Nkv: q {tuple(q.shape)}, k {tuple(k.shape)}")
        out = out if out is not None else q.new_empty(3, *q.shape)
        return out, tuple(out.unbind(0))
    if layout == "flat":
        out = out if out is not None else q.new_empty(q.numel() + 2 * k.numel())
        dq, dk, dv = out.split([q.numel(), k.numel(), k.numel()])
        return out, (dq.view(q.shape), dk.view(k.shape), dv.view(k.shape))
    raise ValueError(f"unknown attention gradient layout {layout!r}")


def _attn_backward(entry: str, layout: str, q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse2: Tensor,
                   doc: Tensor, meta: Tensor, scale: float, tail=()):
    """dq / dk / dv in `layout` by the C entry `entry(.., scale, *tail, stream)`; q, k, v, o as the forward saved them
    (contiguous).  delta fp32 [B, Nh, rows] is the call's scratch: the dQ pass fills it for the dK / dV pass behind it."""
    do = _c(do)
    B, R, Nh, D = q.shape
    T, Nkv = k.shape[1], k.shape[2]
    out, (dq, dk, dv) = attn_grads(q, k, layout)
    delta = torch.empty_like(lse2)
    _C.check(getattr(_lib(), entry)(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse2), _p(delta), _p(dq), _p(dk), _p(dv),
                                    _p(doc), _p(meta), B, T, Nh, Nkv, D, float(scale), *tail, _cur()), entry)
    return out


def _attn_autograd(fwd_op, grads):
    """The autograd formula of `fwd_op(q, k, v, doc, meta, scale, *tail) -> (o, lse2)` over
    `grads(q, k, v, o, do, lse2, doc, meta, scale, *tail) -> (dq, dk, dv)`."""
    def setup(ctx, inputs, output):
        q, k, v, doc, meta, scale, *tail = inputs
        o, lse2 = output
        ctx.save_for_backward(_c(q), _c(k), _c(v), o, lse2, doc, meta)
        ctx.scale, ctx.tail = scale, tuple(tail)
        ctx.set_materialize_grads(False)     # (the LSE output has no gradient: no [B, Nh, T] zero fill per layer)

    def backward(ctx, do, _dlse):
        q, k, v, o, lse2, doc, meta = ctx.saved_tensors
        if do is None:
            do = torch.zeros_like(o)
        dq, dk, dv = grads(q, k, v, o, do, lse2, doc, meta, ctx.scale, *ctx.tail)
        return (dq, dk, dv, None, None, None, *(None for _ in ctx.tail))

    fwd_op.register_autograd(backward, setup_context=setup)


def _segs_tail(segs: List[int], rows_per_batch: int):
    """(nseg, int[6], rows_per_batch) of the sequence-sharded C entries; `segs` = up to two flattened triples"""
    return len(segs) // 3, (ctypes.c_int * 6)(*segs, *([0] * (6 - len(segs)))), rows_per_batch


@custom_op(f"{NS}::attn_fwd", mutates_args=(), device_types="cuda")
def attn_fwd(q: Tensor, k: Tensor, v: Tensor, doc: Tensor, meta: Tensor, scale: float) -> Tuple[Tensor, Tensor]:
    """Packed (document-masked causal) attention: q [B,T,Nh,D], k/v [B,T,Nkv,D] bf16, doc int32 [B,T], meta from
    `attn_build_meta` -> (o [B,T,Nh,D], lse2 fp32 [B,Nh,T])."""
    return _attn_forward("packed_attention", "tn_attn_fwd", q, k, v, doc, meta, scale)


@custom_op(f"{NS}::attn_fwd_bidir", mutates_args=(), device_types="cuda")
def attn_fwd_bidir(q: Tensor, k: Tensor, v: Tensor, doc: Tensor, meta: Tensor, scale: float) -> Tuple[Tensor, Tensor]:
    """`attn_fwd` with the mask bidirectional inside a document: softmax over ALL keys of the query's document (no causal
    restriction).  `tn_attn_fwd_bidir` / `tn_attn_bwd_bidir` are the packed-attention kernels with the causal term of the
    predicate switched off and the key range of a query tile extended to the last tile that shares a document with it
    (csrc/attn_common.h QView::bidir).  Used by the Whisper speech encoder of Kimi-Audio
    (touchnet/models/kimi_audio/modeling_kimi_audio.py:337-339, 942-947: transformers' WhisperEncoder, bidirectional
    self-attention over the 1500 frames of a clip)."""
    return _attn_forward("bidirectional_attention", "tn_attn_fwd_bidir", q, k, v, doc, meta, scale)


@custom_op(f"{NS}::attn_fwd_seg", mutates_args=(), device_types="cuda")
def attn_fwd_seg(q: Tensor, k: Tensor, v: Tensor, doc: Tensor, meta: Tensor, scale: float, segs: List[int],
                 rows_per_batch: int) -> Tuple[Tensor, Tensor]:
    """Sequence-sharded query side (context parallelism): q [B, R, Nh, D] local rows, k/v [B, T, Nkv, D] global;
    `segs` = up to two (row0, rows, global_offset) triples, flattened."""
    return _attn_forward("packed_attention_sharded", "tn_attn_fwd_seg", q, k, v, doc, meta, scale,
                         _segs_tail(segs, rows_per_batch), rows_per_batch)


@custom_op(f"{NS}::attn_fwd_seg_chunks", mutates_args=(), device_types="cuda")
def attn_fwd_seg_chunks(q: Tensor, k: Tensor, v: Tensor, doc: Tensor, meta: Tensor, scale: float, segs: List[int],
                        rows_per_batch: int, chunk_len: int, chunk_mask: int) -> Tuple[Tensor, Tensor]:
    """attn_fwd_seg with the KEY side restricted to the sequence chunks whose bit is set in `chunk_mask` (chunk c =
    positions [c * chunk_len, (c + 1) * chunk_len)).  Rows without a key there: O = 0, LSE2 = +inf.  One half of the
    local / remote split of context-parallel attention (no autograd formula of its own: functional._SplitAttention
    differentiates the MERGED result with one attn_bwd_seg)."""
    return _attn_forward("packed_attention_sharded_split", "tn_attn_fwd_seg_chunks", q, k, v, doc, meta, scale,
                         (*_segs_tail(segs, rows_per_batch), int(chunk_len), int(chunk_mask)), rows_per_batch)


for _op in (attn_fwd, attn_fwd_bidir, attn_fwd_seg, attn_fwd_seg_chunks):
    _op.register_fake(_attn_forward_fake)


@custom_op(f"{NS}::attn_bwd", mutates_args=(), device_types="cuda")
def attn_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse2: Tensor, doc: Tensor, meta: Tensor,
             scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    return _attn_backward("tn_attn_bwd", "tuple", q, k, v, o, do, lse2, doc, meta, scale)


@custom_op(f"{NS}::attn_bwd_bidir", mutates_args=(), device_types="cuda")
def attn_bwd_bidir(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse2: Tensor, doc: Tensor, meta: Tensor,
                   scale: float) -> Tuple[Tensor, Tensor, Tensor]:
    """Three tensors of their own also for Nh == Nkv: back-to-back gradients would send the audio tower's q/k/v weight
    gradient down another launch (functional._stacked_view)."""
    return _attn_backward("tn_attn_bwd_bidir", "tuple", q, k, v, o, do, lse2, doc, meta, scale)


@custom_op(f"{NS}::attn_bwd_stacked", mutates_args=(), device_types="cuda")
def attn_bwd_stacked(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse2: Tensor, doc: Tensor, meta: Tensor,
                     scale: float) -> Tensor:
    """attn_bwd for Nh == Nkv with the three gradients in ONE buffer [3, B, T, Nh, D] (`attn_grads`, "stacked")."""
    return _attn_backward("tn_attn_bwd", "stacked", q, k, v, o, do, lse2, doc, meta, scale)


@custom_op(f"{NS}::attn_bwd_rope", mutates_args=(), device_types="cuda")
def attn_bwd_rope(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse2: Tensor, doc: Tensor, meta: Tensor,
                  scale: float, cos: Tensor, sin: Tensor, stacked: bool) -> Tensor:
    """attn_bwd for ROTATED q / k whose gradients are wanted for the un-rotated projections (tn_attn_bwd_rope: the rotary
    embedding's backward in the attention kernels' epilogues; bit-identical to attn_bwd followed by rope_apply(backward)).
    One buffer (`attn_grads`): "stacked" (Nh == Nkv) or "flat"."""
    B, T, Nh, D = q.shape
    if not (cos.dtype == torch.bfloat16 and sin.dtype == torch.bfloat16 and cos.is_contiguous() and sin.is_contiguous()
            and cos.numel() == B * T * (D // 2) and sin.numel() == cos.numel()):
        raise _C.KernelError("attn_bwd_rope: cos / sin are the bf16 [B * T, head_dim / 2] tables of rope_tables")
    return _attn_backward("tn_attn_bwd_rope", "stacked" if stacked else "flat", q, k, v, o, do, lse2, doc, meta, scale,
                          (_p(cos), _p(sin)))


@custom_op(f"{NS}::attn_bwd_seg", mutates_args=(), device_types="cuda")
def attn_bwd_seg(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse2: Tensor, doc: Tensor, meta: Tensor,
                 scale: float, segs: List[int], rows_per_batch: int) -> Tuple[Tensor, Tensor, Tensor]:
    """dk / dv are this rank's PARTIAL sums over the global [B, T, Nkv, D]."""
    return _attn_backward("tn_attn_bwd_seg", "tuple", q, k, v, o, do, lse2, doc, meta, scale,
                          _segs_tail(segs, q.shape[1]))


for _op, _layout in ((attn_bwd, "tuple"), (attn_bwd_bidir, "tuple"), (attn_bwd_stacked, "stacked"), (attn_bwd_seg, "tuple")):
    _op.register_fake(lambda q, k, *rest, _layout=_layout: attn_grads(q, k, _layout)[0])
attn_bwd_rope.register_fake(lambda q, k, *rest: attn_grads(q, k, "stacked" if rest[-1] else "flat")[0])


def _attn_causal_grads(q, k, *rest):
    """multi-head attention (Nh == Nkv): one buffer, three slices; grouped-query attention: three tensors"""
    if q.shape == k.shape:
        return attn_bwd_stacked(q, k, *rest).unbind(0)
    return attn_bwd(q, k, *rest)


_attn_autograd(attn_fwd, _attn_causal_grads)
_attn_autograd(attn_fwd_bidir, attn_bwd_bidir)
_attn_autograd(attn_fwd_seg, attn_bwd_seg)


def attn_meta_ints(B: int, T: int) -> int:
    """tn_attn_meta_ints restated for shapes without the library (csrc/attn_common.h attn_meta_ints is the owner; the
    test suite holds the two together): 5 statistics per 64-position tile, 4 per 32 positions (qstat), and the two
    stored tile lists (klist, qlist) of 4 + 4 * kListPre ints per 128 positions, kListPre = 64."""
    nt, nq32, nq128 = (T + 63) // 64, (T + 31) // 32, (T + 127) // 128
    return B * (5 * nt + 4 * nq32 + 2 * (4 + 4 * 64) * nq128)


@custom_op(f"{NS}::attn_build_meta", mutates_args=(), device_types="cuda")
def attn_build_meta(doc: Tensor) -> Tensor:
    """doc int32 [B, T] -> per-64-tile range metadata (int32 [tn_attn_meta_ints(B, T)]); once per batch."""
    B, T = doc.shape
    meta = torch.empty(_lib().tn_attn_meta_ints(B, T), dtype=torch.int32, device=doc.device)
    _C.check(_lib().tn_attn_build_meta(_p(doc), _p(meta), B, T, _cur()), "tn_attn_build_meta")
    return meta


@attn_build_meta.register_fake
def _(doc):
    return doc.new_empty(attn_meta_ints(*doc.shape), dtype=torch.int32)


@custom_op(f"{NS}::attn_merge", mutates_args=(), device_types="cuda")
def attn_merge(o_a: Tensor, lse2_a: Tensor, o_b: Tensor, lse2_b: Tensor) -> Tuple[Tensor, Tensor]:
    """Two partial attention results over disjoint key sets -> (O, LSE2) of their union (log2-domain LSE, +inf = empty)."""
    o_a, o_b, la, lb = _c(o_a), _c(o_b), _c(lse2_a), _c(lse2_b)
    B, R, Nh, D = o_a.shape
    o, lse2 = torch.empty_like(o_a), torch.empty_like(la)
    _C.check(_lib().tn_attn_merge(_p(o_a), _p(la), _p(o_b), _p(lb), _p(o), _p(lse2), B, R, Nh, D, _cur()),
             "tn_attn_merge")
    return o, lse2


@attn_merge.register_fake
def _(o_a, lse2_a, o_b, lse2_b):
    return (torch.empty_like(o_a, memory_format=torch.contiguous_format),
            torch.empty_like(lse2_a, memory_format=torch.contiguous_format))


# ===================================================================================================== cross-entropy
@custom_op(f"{NS}::ce_fwd", mutates_args=(), device_types="cuda")
def ce_fwd(logits: Tensor, labels: Tensor, sentence_lens: Tensor, num_sentence: Tensor,
           ignore_index: int) -> Tuple[Tensor, Tensor, Tensor]:
    """logits [n, V]; labels / sentence_lens int64 [n]; num_sentence fp32 [1] ->
    (loss_per_sample 0-d [differentiable], stats fp32 [4] = {per_sample, per_token, accuracy, n_valid}, lse fp32 [n])."""
    n, V = logits.shape
    nll = torch.empty(n, dtype=torch.float32, device=logits.device)
    lse = torch.empty_like(nll)
    hit = torch.empty(n, dtype=torch.int32, device=logits.device)
    out = torch.empty(4, dtype=torch.float32, device=logits.device)
    _C.check(_lib().tn_ce_forward(_p(logits), _p(labels), _p(sentence_lens), _p(num_sentence), _p(nll), _p(lse),
                                  _p(hit), _p(out), n, V, int(ignore_index), _C.dcode(logits), _cur()),
             "tn_ce_forward")
    return out[0].clone(), out, lse


@ce_fwd.register_fake
def _(logits, labels, sentence_lens, num_sentence, ignore_index):
    f32 = dict(dtype=torch.float32)
    return logits.new_empty((), **f32), logits.new_empty(4, **f32), logits.new_empty(logits.shape[0], **f32)


@custom_op(f"{NS}::ce_bwd", mutates_args=(), device_types="cuda")
def ce_bwd(logits: Tensor, labels: Tensor, sentence_lens: Tensor, lse: Tensor, num_sentence: Tensor, grad_out: Tensor,
           ignore_index: int) -> Tensor:
    n, V = logits.shape
    dlog = torch.empty_like(logits)
    _C.check(_lib().tn_ce_backward(_p(logits), _p(dlog), _p(labels), _p(sentence_lens), _p(lse), _p(num_sentence),
                                   _p(grad_out), n, V, int(ignore_index), _C.dcode(logits), _cur()), "tn_ce_backward")
    return dlog


@ce_bwd.register_fake
def _(logits, labels, sentence_lens, lse, num_sentence, grad_out, ignore_index):
    return torch.empty_like(logits)


@custom_op(f"{NS}::ce_bwd_", mutates_args=("logits",), device_types="cuda")
def ce_bwd_(logits: Tensor, labels: Tensor, sentence_lens: Tensor, lse: Tensor, num_sentence: Tensor,
            grad_out: Tensor, ignore_index: int) -> None:
    """In-place form: dlogits overwrite the logits (they are dead after the loss: saves n x V x 2 bytes)."""
    n, V = logits.shape
    _C.check(_lib().tn_ce_backward(_p(logits), _p(logits), _p(labels), _p(sentence_lens), _p(lse), _p(num_sentence),
                                   _p(grad_out), n, V, int(ignore_index), _C.dcode(logits), _cur()), "tn_ce_backward")


def _ce_setup(ctx, inputs, output):
    logits, labels, sentence_lens, num_sentence, ignore_index = inputs
    _, _, lse = output
    ctx.save_for_backward(logits, labels, sentence_lens, lse, num_sentence)
    ctx.ignore_index = ignore_index


def _ce_backward(ctx, g_loss, _g_stats, _g_lse):
    logits, labels, sentence_lens, lse, ns = ctx.saved_tensors
    g = _c(g_loss).to(torch.float32).reshape(1)
    return ce_bwd(logits, labels, sentence_lens, lse, ns, g, ctx.ignore_index), None, None, None, None


ce_fwd.register_autograd(_ce_backward, setup_context=_ce_setup)


# ===================================================================================================== GEMM
@custom_op(f"{NS}::gemm_tn", mutates_args=(), device_types="cuda")
def gemm_tn(a: Tensor, b: Tensor, bias: Optional[Tensor]) -> Tensor:
    """a [M, K] · b [N, K]^T (+ bias [N]) -> [M, N]; bf16, fp32 accumulation — the hand-written MFMA kernel
    (csrc/gemm.hip).  Differentiable: both gradients are GEMMs of the same kernel on transposed operands."""
    if a.dim() != 2 or b.dim() != 2 or a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise _C.KernelError("gemm_tn: 2-D bf16 operands only")
    a, b = (a if a.stride(1) == 1 else a.contiguous()), (b if b.stride(1) == 1 else b.contiguous())
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    bias_c = _c(bias).to(a.dtype) if bias is not None else None
    _C.check(_lib().tn_gemm_bf16_tn(_p(a), _p(b), _p(out), None, _p(bias_c), M, N, K, a.stride(0), b.stride(0), N, 0,
                                    0, _cur()), "tn_gemm_bf16_tn")
    return out


@gemm_tn.register_fake
def _(a, b, bias):
    return a.new_empty(a.shape[0], b.shape[0])


def _gemm_setup(ctx, inputs, output):
    a, b, bias = inputs
    ctx.save_for_backward(a, b)
    ctx.has_bias = bias is not None


def _gemm_backward(ctx, dy):
    a, b = ctx.saved_tensors
    dy = _c(dy)
    da = db = dbias = None
    if ctx.needs_input_grad[0]:
        da = gemm_tn(dy, b.t().contiguous(), None)          # dA[M,K] = dY[M,N] · (B^T)[K,N]^T
    if ctx.needs_input_grad[1]:
        db = gemm_tn(dy.t().contiguous(), a.t().contiguous(), None)   # dB[N,K] = (dY^T)[N,M] · (A^T)[K,M]^T
    if ctx.has_bias and ctx.needs_input_grad[2]:
        dbias = dy.sum(0)
    return da, db, dbias


gemm_tn.register_autograd(_gemm_backward, setup_context=_gemm_setup)


# ===================================================================================================== helpers of the linear layers
@custom_op(f"{NS}::rope_table", mutates_args=(), device_types="cuda")
def rope_table(position_ids: Tensor, inv_freq: Tensor, attention_scaling: float, dtype: torch.dtype) -> Tuple[Tensor, Tensor]:
    """int64 positions [n] x fp32 inv_freq [half] -> cos / sin [n, half] in `dtype` (once per forward)."""
    n, half = position_ids.numel(), inv_freq.numel()
    cos = torch.empty(n, half, dtype=dtype, device=position_ids.device)
    sin = torch.empty_like(cos)
    _C.check(_lib().tn_rope_table(_p(position_ids), _p(inv_freq), _p(cos), _p(sin), n, half, float(attention_scaling),
                                  _C.dcode(cos), _cur()), "tn_rope_table")
    return cos, sin


@rope_table.register_fake
def _(position_ids, inv_freq, attention_scaling, dtype):
    e = lambda: position_ids.new_empty(position_ids.numel(), inv_freq.numel(), dtype=dtype)
    return e(), e()


@custom_op(f"{NS}::transpose_bf16_", mutates_args=("dst",), device_types="cuda")
def transpose_bf16_(src: Tensor, dst: Tensor) -> None:
    """dst[c, r] = src[r, c]; both 2-D bf16 with contiguous rows (row strides are passed to the kernel)."""
    R, Cn = src.shape
    _C.check(_lib().tn_transpose_bf16(_p(src), _p(dst), R, Cn, src.stride(0), dst.stride(0), _cur()),
             "tn_transpose_bf16")


@custom_op(f"{NS}::colsum_bf16", mutates_args=(), device_types="cuda")
def colsum_bf16(x: Tensor) -> Tensor:
    """x.sum(0) of a bf16 [rows, cols] matrix (fp32 accumulation, deterministic two-stage): the bias gradient."""
    R, Cn = x.shape
    ws = torch.empty(int(_lib().tn_colsum_workspace_floats(R, Cn)), dtype=torch.float32, device=x.device)
    out = torch.empty(Cn, dtype=x.dtype, device=x.device)
    _C.check(_lib().tn_colsum_bf16(_p(x), _p(out), _p(ws), R, Cn, x.stride(0), _cur()), "tn_colsum_bf16")
    return out


@colsum_bf16.register_fake
def _(x):
    return x.new_empty(x.shape[1])


@custom_op(f"{NS}::swiglu_fwd_t", mutates_args=(), device_types="cuda")
def swiglu_fwd_t(gate: Tensor, up: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (act [M, I], act^T [I, M]): the transposed copy feeds the weight-gradient GEMM of down_proj."""
    M, I = gate.shape
    act = torch.empty_like(gate)
    act_t = torch.empty(I, M, dtype=gate.dtype, device=gate.device)
    _C.check(_lib().tn_swiglu_fwd_t(_p(gate), _p(up), _p(act), _p(act_t), M, I, _cur()), "tn_swiglu_fwd_t")
    return act, act_t


@swiglu_fwd_t.register_fake
def _(gate, up):
    return torch.empty_like(gate), gate.new_empty(gate.shape[1], gate.shape[0])


@custom_op(f"{NS}::swiglu_bwd_t", mutates_args=(), device_types="cuda")
def swiglu_bwd_t(dact: Tensor, gate: Tensor, up: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (dgate, dup, [dgate^T ; dup^T] as [2 I, M])."""
    M, I = gate.shape
    dgate, dup = torch.empty_like(gate), torch.empty_like(up)
    dgu_t = torch.empty(2 * I, M, dtype=gate.dtype, device=gate.device)
    _C.check(_lib().tn_swiglu_bwd_t(_p(dact), _p(gate), _p(up), _p(dgate), _p(dup), _p(dgu_t), M, I, _cur()),
             "tn_swiglu_bwd_t")
    return dgate, dup, dgu_t


@swiglu_bwd_t.register_fake
def _(dact, gate, up):
    return torch.empty_like(gate), torch.empty_like(up), gate.new_empty(2 * gate.shape[1], gate.shape[0])


@custom_op(f"{NS}::ce_fwd_rows", mutates_args=(), device_types="cuda")
def ce_fwd_rows(logits: Tensor, labels: Tensor, sentence_lens: Tensor, num_sentence: Tensor,
                ignore_index: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Per-row part of the CE (the chunks of the fused lm_head + CE): -> (nll, lse fp32 [n], hit int32 [n])."""
    n, V = logits.shape
    nll = torch.empty(n, dtype=torch.float32, device=logits.device)
    lse = torch.empty_like(nll)
    hit = torch.empty(n, dtype=torch.int32, device=logits.device)
    _C.check(_lib().tn_ce_forward(_p(logits), _p(labels), _p(sentence_lens), _p(num_sentence), _p(nll), _p(lse),
                                  _p(hit), None, n, V, int(ignore_index), _C.dcode(logits), _cur()), "tn_ce_forward")
    return nll, lse, hit


@ce_fwd_rows.register_fake
def _(logits, labels, sentence_lens, num_sentence, ignore_index):
    n = logits.shape[0]
    return (logits.new_empty(n, dtype=torch.float32), logits.new_empty(n, dtype=torch.float32),
            logits.new_empty(n, dtype=torch.int32))


@custom_op(f"{NS}::ce_reduce", mutates_args=(), device_types="cuda")
def ce_reduce(nll: Tensor, hit: Tensor, labels: Tensor, sentence_lens: Tensor, num_sentence: Tensor,
              ignore_index: int) -> Tensor:
    """-> stats fp32 [4] = {loss_per_sample, loss_per_token, accuracy, n_valid} from the per-row parts."""
    out = torch.empty(4, dtype=torch.float32, device=nll.device)
    _C.check(_lib().tn_ce_reduce(_p(nll), _p(hit), _p(labels), _p(sentence_lens), _p(num_sentence), _p(out),
                                 nll.numel(), int(ignore_index), _cur()), "tn_ce_reduce")
    return out


@ce_reduce.register_fake
def _(nll, hit, labels, sentence_lens, num_sentence, ignore_index):
    return nll.new_empty(4)


# ===================================================================================================== audio frontend
@custom_op(f"{NS}::log_mel", mutates_args=(), device_types="cuda")
def log_mel(wav: Tensor, mel_fb: Tensor, num_mel_bins: int) -> Tensor:
    feat = torch.empty(wav.numel() // 160, num_mel_bins, dtype=torch.float32, device=wav.device)
    gmax = torch.empty(1, dtype=torch.float32, device=wav.device)
    _C.check(_lib().tn_log_mel(_p(wav), _p(mel_fb), _p(feat), _p(gmax), wav.numel(), num_mel_bins, _cur()),
             "tn_log_mel")
    return feat


@log_mel.register_fake
def _(wav, mel_fb, num_mel_bins):
    return wav.new_empty(wav.numel() // 160, num_mel_bins)


@custom_op(f"{NS}::audiofeat_stack", mutates_args=(), device_types="cuda")
def audiofeat_stack(feat: Tensor, stack: int, stride: int, normalize: bool) -> Tensor:
    T, F = feat.shape
    out = torch.empty((T + stride - 1) // stride, F * stack, dtype=torch.float32, device=feat.device)
    _C.check(_lib().tn_audiofeat_stack(_p(feat), _p(out), T, F, stack, stride, int(normalize), _cur()),
             "tn_audiofeat_stack")
    return out


@audiofeat_stack.register_fake
def _(feat, stack, stride, normalize):
    return feat.new_empty((feat.shape[0] + stride - 1) // stride, feat.shape[1] * stack)


def resample_sinc(wave: Tensor, tab: Tensor, orig: int, new: int, n_out: int) -> Tensor:
    """tn_resample_sinc on a 1-D fp32 or int16 device waveform"""
    out = torch.empty(n_out, dtype=torch.float32, device=wave.device)
    _C.check(_lib().tn_resample_sinc(_p(wave), int(wave.dtype == torch.int16), _p(out), _p(tab), wave.numel(), int(n_out),
                                     int(orig), int(new), int(tab.shape[1]), _cur()), "tn_resample_sinc")
    return out


def _kaldi_frames(n_samples: int, win: int, shift: int) -> int:
    """Kaldi's snip_edges frame count"""
    return 0 if n_samples < win or shift < 1 else 1 + (n_samples - win) // shift


def _kaldi_feats(wav, window, bank_idx, bank_w, dct, sample_rate, shift, low_freq, high_freq) -> Tensor:
    """tn_kaldi_feats on a 1-D fp32 device waveform and the tables of functional.kaldi_feature_tables: fbank rows when
    dct is None, MFCC rows otherwise.  The geometry comes from the tables' shapes; the entry point refuses what does not
    fit (-22) before it launches anything."""
    win, bins = int(window.shape[0]), int(bank_idx.shape[0])
    ceps = 0 if dct is None else int(dct.shape[0])
    for t, dt in ((wav, torch.float32), (window, torch.float32), (bank_idx, torch.int32), (bank_w, torch.float32),
                  (dct, torch.float32)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise _C.KernelError("tn_kaldi_feats: contiguous fp32 waveform / window / weights / dct and int32 bank indices")
    if wav.dim() != 1 or bank_idx.dim() != 2 or bank_idx.shape[1] != 3 or (dct is not None and (
            dct.dim() != 2 or dct.shape[1] != bins or ceps < 1)):
        raise _C.KernelError("tn_kaldi_feats: wav [N], bank_idx [bins, 3], dct [num_ceps >= 1, bins]")
    out = torch.empty(_kaldi_frames(wav.numel(), win, int(shift)), ceps or bins, dtype=torch.float32, device=wav.device)
    _C.check(_lib().tn_kaldi_feats(_p(wav), _p(out), wav.numel(), int(sample_rate), win, int(shift),
                                   1 << max(win - 1, 0).bit_length(), bins, ceps, float(low_freq), float(high_freq),
                                   _p(window), _p(bank_idx), _p(bank_w), bank_w.numel(), _p(dct), _cur()),
             "tn_kaldi_feats")
    return out


@custom_op(f"{NS}::kaldi_feats", mutates_args=(), device_types="cuda")
def kaldi_feats(wav: Tensor, window: Tensor, bank_idx: Tensor, bank_w: Tensor, sample_rate: int, shift: int,
                low_freq: float, high_freq: float) -> Tensor:
    """-> log-fbank fp32 [frames, num_mel_bins] at the geometry of the tables (csrc/kaldi_feats.hip)"""
    return _kaldi_feats(wav, window, bank_idx, bank_w, None, sample_rate, shift, low_freq, high_freq)


@kaldi_feats.register_fake
def _(wav, window, bank_idx, bank_w, sample_rate, shift, low_freq, high_freq):
    return wav.new_empty(_kaldi_frames(wav.numel(), window.shape[0], shift), bank_idx.shape[0])


@custom_op(f"{NS}::kaldi_mfcc", mutates_args=(), device_types="cuda")
def kaldi_mfcc(wav: Tensor, window: Tensor, bank_idx: Tensor, bank_w: Tensor, dct: Tensor, sample_rate: int, shift: int,
               low_freq: float, high_freq: float) -> Tensor:
    """-> MFCC fp32 [frames, num_ceps]: dct [num_ceps, num_mel_bins] applied to the log-fbank row inside the kernel"""
    return _kaldi_feats(wav, window, bank_idx, bank_w, dct, sample_rate, shift, low_freq, high_freq)


@kaldi_mfcc.register_fake
def _(wav, window, bank_idx, bank_w, dct, sample_rate, shift, low_freq, high_freq):
    return wav.new_empty(_kaldi_frames(wav.numel(), window.shape[0], shift), dct.shape[0])


VAD_MAX_WIN, VAD_MAX_CTX = 4096, 64                # tn_vad_log_energy's and tn_vad_runs' limits


def vad_frames_per_block(win: int, shift: int) -> int:
    """frames one workgroup of tn_vad_log_energy owns (partials holds one double per workgroup); -1 for a geometry the
    kernel does not take"""
    return int(_lib().tn_vad_frames_per_block(int(win), int(shift)))


def _vad_partials(frames: int, win: int, shift: int) -> int:
    fpb = vad_frames_per_block(win, shift)
    if fpb < 1:
        raise _C.KernelError(f"vad_log_energy: win = {win} must be in [1, {VAD_MAX_WIN}] and shift = {shift} >= 1")
    return -(-frames // fpb)


@custom_op(f"{NS}::vad_log_energy", mutates_args=(), device_types="cuda")
def vad_log_energy(wave: Tensor, win: int, shift: int) -> Tuple[Tensor, Tensor]:
    """Kaldi's raw log-energy per frame (tn_vad_log_energy, csrc/vad.hip): wave 1-D fp32 in [-1, 1) or int16 PCM ->
    loge fp32 [T] with Kaldi's snip_edges frame count and partials fp64 [workgroups], each workgroup's sum of its frames'
    loge.  No frame: two empty tensors, nothing launched."""
    if wave.dim() != 1 or wave.dtype not in (torch.float32, torch.int16):
        raise _C.KernelError("vad_log_energy: a 1-D fp32 or int16 device waveform")
    wave = _c(wave)
    T = _kaldi_frames(wave.numel(), win, shift)
    loge = torch.empty(T, dtype=torch.float32, device=wave.device)
    partials = torch.empty(_vad_partials(T, win, shift), dtype=torch.float64, device=wave.device)
    if T:
        _C.check(_lib().tn_vad_log_energy(_p(wave), int(wave.dtype == torch.int16), _p(loge), _p(partials), wave.numel(),
                                          int(win), int(shift), _cur()), "tn_vad_log_energy")
    return loge, partials


@vad_log_energy.register_fake
def _(wave, win, shift):
    T = _kaldi_frames(wave.numel(), win, shift)
    return wave.new_empty(T, dtype=torch.float32), wave.new_empty(_vad_partials(T, win, shift), dtype=torch.float64)


@custom_op(f"{NS}::vad_runs", mutates_args=(), device_types="cuda")
def vad_runs(loge: Tensor, partials: Tensor, energy_threshold: float, mean_scale: float, ctx: int,
             proportion: float) -> Tuple[Tensor, Tensor]:
    """Threshold, vote and runs of the energy VAD (tn_vad_runs): loge fp32 [T], partials fp64 [>= 1] whose sum is loge's
    -> voiced uint8 [T] and runs int32 [1 + 2 (T // 2 + 1)]: element 0 is the number of runs R, elements 1 + 2 r and
    2 + 2 r the first frame of run r and the frame behind its last; what lies behind the R-th pair is not written.  One
    buffer, so that one host read fetches the count and the runs."""
    if loge.dim() != 1 or loge.dtype != torch.float32 or partials.dim() != 1 or partials.dtype != torch.float64:
        raise _C.KernelError("vad_runs: loge fp32 [T] and partials fp64 [n]")
    if not 0 <= ctx <= VAD_MAX_CTX:
        raise _C.KernelError(f"vad_runs: frames_context = {ctx} must be in [0, {VAD_MAX_CTX}]")
    if not 0.0 < proportion <= 1.0:
        raise _C.KernelError(f"vad_runs: proportion_threshold = {proportion} must be in (0, 1]")
    loge, partials = _c(loge), _c(partials)
    T, dev = loge.numel(), loge.device
    capacity = T // 2 + 1
    voiced = torch.empty(T, dtype=torch.uint8, device=dev)
    if T == 0:
        return voiced, torch.zeros(1 + 2 * capacity, dtype=torch.int32, device=dev)
    if partials.numel() < 1:
        raise _C.KernelError("vad_runs: partials needs at least one element")
    buf = torch.empty(1 + 2 * capacity, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib().tn_vad_runs_workspace_bytes(T)) // 8, dtype=torch.float64, device=dev)
    _C.check(_lib().tn_vad_runs(_p(loge), T, _p(partials), partials.numel(), float(energy_threshold), float(mean_scale),
                                int(ctx), float(proportion), _p(voiced), _p(buf[1:]), _p(buf), capacity, _p(ws), _cur()),
             "tn_vad_runs")
    return voiced, buf


@vad_runs.register_fake
def _(loge, partials, energy_threshold, mean_scale, ctx, proportion):
    T = loge.numel()
    return loge.new_empty(T, dtype=torch.uint8), loge.new_empty(1 + 2 * (T // 2 + 1), dtype=torch.int32)


def feat_augment(feat: Tensor, t_masks, f_masks, subs, out_rows: int) -> Tensor:
    """tn_feat_augment: the draws travel as kernel arguments (host int arrays), so this is a plain function, not a
    registered op (no tensor carries them)."""
    import ctypes as C
    T, F = feat.shape
    out = torch.empty(out_rows, F, dtype=torch.float32, device=feat.device)

    def arr(rows, width):
        flat = [int(v) for r in rows for v in r]
        assert len(flat) == width * len(rows)
        return (C.c_int * max(1, len(flat)))(*flat), len(rows)
    tm, nt = arr(t_masks, 2)
    fm, nf = arr(f_masks, 2)
    sb, ns = arr(subs, 3)
    _C.check(_lib().tn_feat_augment(_p(feat), _p(out), T, F, int(out_rows), C.cast(tm, C.c_void_p), nt,
                                    C.cast(fm, C.c_void_p), nf, C.cast(sb, C.c_void_p), ns, _cur()), "tn_feat_augment")
    return out


@custom_op(f"{NS}::pcm16_to_f32", mutates_args=(), device_types="cuda")
def pcm16_to_f32(pcm: Tensor) -> Tensor:
    out = torch.empty(pcm.shape, dtype=torch.float32, device=pcm.device)
    _C.check(_lib().tn_pcm16_to_f32(_p(pcm), _p(out), pcm.numel(), _cur()), "tn_pcm16_to_f32")
    return out


@pcm16_to_f32.register_fake
def _(pcm):
    return pcm.new_empty(pcm.shape, dtype=torch.float32)


@custom_op(f"{NS}::bestrq_tokenize", mutates_args=(), device_types="cuda")
def bestrq_tokenize(feat: Tensor, quantizer: Tensor, codebook: Tensor) -> Tensor:
    T, Fdim = feat.shape
    E, V = quantizer.shape[1], codebook.shape[0]
    codes = torch.empty(T, dtype=torch.int64, device=feat.device)
    _C.check(_lib().tn_bestrq_tokenize(_p(feat), _p(quantizer), _p(codebook), _p(codes), T, Fdim, E, V, _cur()),
             "tn_bestrq_tokenize")
    return codes


@bestrq_tokenize.register_fake
def _(feat, quantizer, codebook):
    return feat.new_empty(feat.shape[0], dtype=torch.int64)


# ===================================================================================================== KV-cache decoding
def _no_grad_inputs(what, *ts):
    if any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"{what}: inference only (no autograd formula); call it under torch.no_grad() on detached tensors")


@custom_op(f"{NS}::attn_decode_", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def attn_decode_(q: Tensor, k_new: Tensor, v_new: Tensor, k_cache: Tensor, v_cache: Tensor, cache_len: Tensor,
                 scale: float) -> Tensor:
    """One new token per row over a KV cache (tn_attn_decode): q [B, Nh, D], k_new / v_new [B, Nkv, D] (q, k rotated), caches
    [B, S_max, Nkv, D] bf16, cache_len int32 [B].  Stores k_new / v_new at slot cache_len[b] of the caches and returns
    o [B, Nh, D]; cache_len is not advanced."""
    _no_grad_inputs("attn_decode_", q, k_new, v_new, k_cache, v_cache)
    B, Nh, D = q.shape
    S_max, Nkv = k_cache.shape[1], k_cache.shape[2]
    if (q.dtype != torch.bfloat16 or k_new.dtype != torch.bfloat16 or v_new.dtype != torch.bfloat16
            or k_cache.dtype != torch.bfloat16 or v_cache.dtype != torch.bfloat16 or cache_len.dtype != torch.int32
            or tuple(k_new.shape) != (B, Nkv, D) or tuple(v_new.shape) != (B, Nkv, D)
            or tuple(k_cache.shape) != (B, S_max, Nkv, D) or tuple(v_cache.shape) != (B, S_max, Nkv, D)
            or tuple(cache_len.shape) != (B,) or not k_cache.is_contiguous() or not v_cache.is_contiguous()):
        raise _C.KernelError("attn_decode_: bf16 q [B, Nh, D], k_new / v_new [B, Nkv, D], contiguous caches "
                             "[B, S_max, Nkv, D], int32 cache_len [B]")
    q, k_new, v_new, cache_len = _c(q), _c(k_new), _c(v_new), _c(cache_len)
    o = torch.empty_like(q)
    nbytes = int(_lib().tn_attn_decode_workspace_bytes(B, Nh, Nkv, D, S_max))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device) if nbytes else None
    _C.check(_lib().tn_attn_decode(_p(q), _p(k_new), _p(v_new), _p(k_cache), _p(v_cache), _p(cache_len), _p(o), _p(ws),
                                   B, Nh, Nkv, D, S_max, float(scale), _cur()), "tn_attn_decode")
    return o


@attn_decode_.register_fake
def _(q, k_new, v_new, k_cache, v_cache, cache_len, scale):
    return torch.empty_like(q, memory_format=torch.contiguous_format)


@custom_op(f"{NS}::greedy_step_", mutates_args=("hist", "hist_len", "cache_len", "finished", "n_unfinished"),
           device_types="cuda")
def greedy_step_(logits: Tensor, hist: Tensor, hist_len: Tensor, cache_len: Tensor, finished: Tensor, n_unfinished: Tensor,
                 penalty: float, ngram: int, eos: int, pad: int) -> None:
    """One greedy step of HF generate() (tn_greedy_step): logits [B, V] fp32 / bf16; hist int32 [B, S_hist], hist_len /
    cache_len / finished int32 [B], n_unfinished int32 [1] — all advanced on the device."""
    _no_grad_inputs("greedy_step_", logits)
    B, V = logits.shape
    for t, shape in ((hist_len, (B,)), (cache_len, (B,)), (finished, (B,)), (n_unfinished, (1,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _C.KernelError("greedy_step_: int32 hist_len / cache_len / finished [B], n_unfinished [1]")
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] != B or not hist.is_contiguous():
        raise _C.KernelError("greedy_step_: int32 contiguous hist [B, S_hist]")
    logits = _c(logits)
    _C.check(_lib().tn_greedy_step(_p(logits), _p(hist), _p(hist_len), _p(cache_len), _p(finished), _p(n_unfinished), B, V,
                                   hist.shape[1], float(penalty), int(ngram), int(eos), int(pad), _C.dcode(logits), _cur()),
             "tn_greedy_step")


@greedy_step_.register_fake
def _(logits, hist, hist_len, cache_len, finished, n_unfinished, penalty, ngram, eos, pad):
    return None


MAX_EOS = 8


@custom_op(f"{NS}::sample_step_", mutates_args=("hist", "hist_len", "cache_len", "finished", "n_unfinished"),
           device_types="cuda")
def sample_step_(logits: Tensor, hist: Tensor, hist_len: Tensor, cache_len: Tensor, finished: Tensor, n_unfinished: Tensor,
                 row_key: Optional[Tensor], uniforms: Optional[Tensor], n_kept: Optional[Tensor], penalty: float,
                 do_sample: bool, temperature: float, top_k: int, top_p: float, seed: int, eos: List[int],
                 pad: int) -> None:
    """One decoding step of HF generate() with the sampling warpers (tn_sample_step): logits [B, V] fp32 / bf16; hist int32
    [B, S_hist], hist_len / cache_len / finished int32 [B], n_unfinished int32 [1] — all advanced on the device.  row_key
    int64 [B] keys the draws (None: the row index); uniforms fp32 [B] replaces the generator; n_kept int32 [B] receives the
    number of tokens top-k / top-p kept (None: not written)."""
    _no_grad_inputs("sample_step_", logits)
    B, V = logits.shape
    for t, shape in ((hist_len, (B,)), (cache_len, (B,)), (finished, (B,)), (n_unfinished, (1,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _C.KernelError("sample_step_: int32 hist_len / cache_len / finished [B], n_unfinished [1]")
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] != B or not hist.is_contiguous():
        raise _C.KernelError("sample_step_: int32 contiguous hist [B, S_hist]")
    for name, t, dt in (("row_key", row_key, torch.int64), ("uniforms", uniforms, torch.float32),
                        ("n_kept", n_kept, torch.int32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (B,) or not t.is_contiguous()):
            raise _C.KernelError(f"sample_step_: {name} must be a contiguous {dt} [B] tensor")
    if len(eos) > MAX_EOS:
        raise _C.KernelError(f"sample_step_: at most {MAX_EOS} eos ids")
    if do_sample and not (temperature > 0.0 and top_k >= 0 and 0.0 < top_p <= 1.0):
        raise _C.KernelError("sample_step_: temperature > 0, top_k >= 0 and 0 < top_p <= 1 when sampling")
    if not 0 <= int(seed) < 2 ** 64:
        raise _C.KernelError("sample_step_: seed must fit in 64 unsigned bits")
    logits = _c(logits)
    eos_arr = (ctypes.c_int * max(1, len(eos)))(*[int(e) for e in eos])
    _C.check(_lib().tn_sample_step(_p(logits), _p(hist), _p(hist_len), _p(cache_len), _p(finished), _p(n_unfinished),
                                   _p(row_key), _p(uniforms), _p(n_kept), B, V, hist.shape[1], float(penalty),
                                   int(bool(do_sample)), float(temperature), int(top_k), float(top_p), int(seed), eos_arr,
                                   len(eos), int(pad), _C.dcode(logits), _cur()), "tn_sample_step")


@sample_step_.register_fake
def _(logits, hist, hist_len, cache_len, finished, n_unfinished, row_key, uniforms, n_kept, penalty, do_sample, temperature,
      top_k, top_p, seed, eos, pad):
    return None


KIMI_MAX_WINDOW, KIMI_MAX_TOP_K = 64, 64


@custom_op(f"{NS}::kimi_text_step_", mutates_args=("hist", "hist_len", "cache_len", "finished", "n_unfinished", "x_next"),
           device_types="cuda")
def kimi_text_step_(logits: Tensor, hist: Tensor, hist_len: Tensor, cache_len: Tensor, finished: Tensor,
                    n_unfinished: Tensor, prompt_len: Tensor, embed: Tensor, x_next: Tensor, row_key: Optional[Tensor],
                    uniforms: Optional[Tensor], penalty: float, window: int, temperature: float, top_k: int, seed: int,
                    eos: int, blank: int, audio_token: int) -> None:
    """One text-stream step of Kimi-Audio's decoding loop (tn_kimi_text_step): logits [B, V] fp32 / bf16; hist int32
    [B, S_hist], hist_len / cache_len / finished / prompt_len int32 [B], n_unfinished int32 [1]; embed bf16 [V, H]; x_next
    bf16 [B, H] receives embed[token] + embed[audio_token].  row_key int64 [B] / uniforms fp32 [B] as for sample_step_."""
    _no_grad_inputs("kimi_text_step_", logits, embed)
    B, V = logits.shape
    for t, shape in ((hist_len, (B,)), (cache_len, (B,)), (finished, (B,)), (prompt_len, (B,)), (n_unfinished, (1,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _C.KernelError("kimi_text_step_: int32 hist_len / cache_len / finished / prompt_len [B], n_unfinished [1]")
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] != B or not hist.is_contiguous():
        raise _C.KernelError("kimi_text_step_: int32 contiguous hist [B, S_hist]")
    if (embed.dtype != torch.bfloat16 or embed.dim() != 2 or embed.shape[0] != V or not embed.is_contiguous()
            or x_next.dtype != torch.bfloat16 or tuple(x_next.shape) != (B, embed.shape[1]) or not x_next.is_contiguous()):
        raise _C.KernelError("kimi_text_step_: contiguous bf16 embed [V, H] and x_next [B, H]")
    for name, t, dt in (("row_key", row_key, torch.int64), ("uniforms", uniforms, torch.float32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (B,) or not t.is_contiguous()):
            raise _C.KernelError(f"kimi_text_step_: {name} must be a contiguous {dt} [B] tensor")
    if not 0 <= int(seed) < 2 ** 64:
        raise _C.KernelError("kimi_text_step_: seed must fit in 64 unsigned bits")
    logits = _c(logits)
    _C.check(_lib().tn_kimi_text_step(_p(logits), _p(hist), _p(hist_len), _p(cache_len), _p(finished), _p(n_unfinished),
                                      _p(prompt_len), _p(embed), _p(x_next), _p(row_key), _p(uniforms), B, V,
                                      hist.shape[1], embed.shape[1], float(penalty), int(window), float(temperature),
                                      int(top_k), int(seed), int(eos), int(blank), int(audio_token), _C.dcode(logits),
                                      _cur()), "tn_kimi_text_step")


@kimi_text_step_.register_fake
def _(logits, hist, hist_len, cache_len, finished, n_unfinished, prompt_len, embed, x_next, row_key, uniforms, penalty,
      window, temperature, top_k, seed, eos, blank, audio_token):
    return None


# ===================================================================================================== beam search
@custom_op(f"{NS}::attn_decode_beam_", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def attn_decode_beam_(q: Tensor, k_new: Tensor, v_new: Tensor, k_cache: Tensor, v_cache: Tensor, cache_len: Tensor,
                      src: Tensor, scale: float) -> Tensor:
    """attn_decode_ on R = B * K beam rows that share their ancestors' cache rows (tn_attn_decode_beam): key / value s of
    row r is read at cache[src[r, s], s], src int32 [R, S_max]; k_new / v_new are stored at cache[r, cache_len[r]]."""
    _no_grad_inputs("attn_decode_beam_", q, k_new, v_new, k_cache, v_cache)
    B, Nh, D = q.shape
    S_max, Nkv = k_cache.shape[1], k_cache.shape[2]
    if (q.dtype != torch.bfloat16 or k_new.dtype != torch.bfloat16 or v_new.dtype != torch.bfloat16
            or k_cache.dtype != torch.bfloat16 or v_cache.dtype != torch.bfloat16 or cache_len.dtype != torch.int32
            or src.dtype != torch.int32 or tuple(k_new.shape) != (B, Nkv, D) or tuple(v_new.shape) != (B, Nkv, D)
            or tuple(k_cache.shape) != (B, S_max, Nkv, D) or tuple(v_cache.shape) != (B, S_max, Nkv, D)
            or tuple(cache_len.shape) != (B,) or tuple(src.shape) != (B, S_max) or not k_cache.is_contiguous()
            or not v_cache.is_contiguous() or not src.is_contiguous()):
        raise _C.KernelError("attn_decode_beam_: bf16 q [R, Nh, D], k_new / v_new [R, Nkv, D], contiguous caches "
                             "[R, S_max, Nkv, D], int32 cache_len [R], contiguous int32 src [R, S_max]")
    q, k_new, v_new, cache_len = _c(q), _c(k_new), _c(v_new), _c(cache_len)
    o = torch.empty_like(q)
    nbytes = int(_lib().tn_attn_decode_workspace_bytes(B, Nh, Nkv, D, S_max))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device) if nbytes else None
    _C.check(_lib().tn_attn_decode_beam(_p(q), _p(k_new), _p(v_new), _p(k_cache), _p(v_cache), _p(cache_len), _p(src),
                                        _p(o), _p(ws), B, Nh, Nkv, D, S_max, float(scale), _cur()), "tn_attn_decode_beam")
    return o


@attn_decode_beam_.register_fake
def _(q, k_new, v_new, k_cache, v_cache, cache_len, src, scale):
    return torch.empty_like(q, memory_format=torch.contiguous_format)


BEAM_MAX_K, BEAM_MAX_EOS = 8, 3
_BEAM_STATE = ("hist", "hist_len", "cache_len", "src", "run_score", "fin_ids", "fin_len", "fin_score", "fin_flag", "gen",
               "unsat", "done", "n_unfinished", "out_ids", "out_parent")


@custom_op(f"{NS}::beam_step_", mutates_args=_BEAM_STATE, device_types="cuda")
def beam_step_(logits: Tensor, hist: Tensor, hist_len: Tensor, cache_len: Tensor, src: Tensor, run_score: Tensor,
               fin_ids: Tensor, fin_len: Tensor, fin_score: Tensor, fin_flag: Tensor, gen: Tensor, unsat: Tensor,
               done: Tensor, n_unfinished: Tensor, out_ids: Tensor, out_parent: Tensor, num_beams: int, penalty: float,
               ngram: int, eos: List[int], n_new: int, length_penalty: float, early_stopping: int) -> None:
    """One step of HF's beam search (tn_beam_step) on R = B * num_beams rows: logits [B, V] (right after the prefill: one
    live row per utterance) or [R, V], fp32 / bf16; hist / fin_ids / src int32 [R, S_hist]; hist_len / cache_len / fin_len /
    fin_flag / out_ids / out_parent int32 [R]; run_score / fin_score fp32 [R]; gen / unsat / done int32 [B]; n_unfinished
    int32 [1] — all advanced on the device.  early_stopping: 0 False, 1 True, 2 "never"."""
    _beam_step("beam_step_", logits, hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen,
               unsat, done, n_unfinished, out_ids, out_parent, num_beams, penalty, ngram, eos, n_new, length_penalty,
               early_stopping, None)


def _beam_step(what, logits, hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen, unsat,
               done, n_unfinished, out_ids, out_parent, num_beams, penalty, ngram, eos, n_new, length_penalty,
               early_stopping, edits):
    """The checks and the launch of beam_step_ (edits None: tn_beam_step) and beam_step_edits_ (edits = (ids, val, cnt):
    tn_beam_step_edits)."""
    _no_grad_inputs(what, logits)
    K = int(num_beams)
    if not 2 <= K <= BEAM_MAX_K:
        raise _C.KernelError(f"{what}: num_beams must be in [2, {BEAM_MAX_K}]")
    if len(eos) > BEAM_MAX_EOS:
        raise _C.KernelError(f"{what}: at most {BEAM_MAX_EOS} eos ids")
    if hist.dim() != 2 or hist.shape[0] % K or logits.dim() != 2:
        raise _C.KernelError(f"{what}: hist [B * num_beams, S_hist], logits [B or B * num_beams, V]")
    R, S_hist = hist.shape
    B, V = R // K, logits.shape[1]
    if logits.shape[0] not in (B, R):
        raise _C.KernelError(f"{what}: logits must have B (first step) or B * num_beams rows")
    if edits is not None:
        e_ids, e_val, e_cnt = edits
        n_edit = e_ids.shape[1] if e_ids.dim() == 2 else 0
        for name, t, dt, ok in (("edit_ids", e_ids, torch.int32, e_ids.dim() == 2 and e_ids.shape[0] >= logits.shape[0]),
                                ("edit_val", e_val, torch.float32, tuple(e_val.shape) == tuple(e_ids.shape)),
                                ("edit_cnt", e_cnt, torch.int32, tuple(e_cnt.shape) == (e_ids.shape[0],))):
            if t.dtype != dt or not ok or not t.is_contiguous() or n_edit < 1:
                raise _C.KernelError(f"{what}: {name} must be a contiguous {dt} tensor: edit_ids / edit_val [rows >= the "
                                     "logits' rows, n_edit >= 1], edit_cnt [rows]")
    for name, t, dt, shape in (("hist", hist, torch.int32, (R, S_hist)), ("fin_ids", fin_ids, torch.int32, (R, S_hist)),
                               ("src", src, torch.int32, (R, S_hist)), ("hist_len", hist_len, torch.int32, (R,)),
                               ("cache_len", cache_len, torch.int32, (R,)), ("fin_len", fin_len, torch.int32, (R,)),
                               ("fin_flag", fin_flag, torch.int32, (R,)), ("out_ids", out_ids, torch.int32, (R,)),
                               ("out_parent", out_parent, torch.int32, (R,)), ("run_score", run_score, torch.float32, (R,)),
                               ("fin_score", fin_score, torch.float32, (R,)), ("gen", gen, torch.int32, (B,)),
                               ("unsat", unsat, torch.int32, (B,)), ("done", done, torch.int32, (B,)),
                               ("n_unfinished", n_unfinished, torch.int32, (1,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _C.KernelError(f"{what}: {name} must be a contiguous {dt} tensor of shape {list(shape)}")
    logits = _c(logits)
    eos_arr = (ctypes.c_int * max(1, len(eos)))(*[int(e) for e in eos])
    ws = torch.empty(int(_lib().tn_beam_step_workspace_bytes(B, K)) // 4, dtype=torch.float32, device=logits.device)
    args = (_p(logits), _p(hist), _p(hist_len), _p(cache_len), _p(src), _p(run_score), _p(fin_ids), _p(fin_len),
            _p(fin_score), _p(fin_flag), _p(gen), _p(unsat), _p(done), _p(n_unfinished), _p(out_ids), _p(out_parent), _p(ws),
            B, K, logits.shape[0] // B, V, S_hist, float(penalty), int(ngram), eos_arr, len(eos), int(n_new),
            float(length_penalty), int(early_stopping), _C.dcode(logits))
    if edits is None:
        _C.check(_lib().tn_beam_step(*args, _cur()), "tn_beam_step")
    else:
        _C.check(_lib().tn_beam_step_edits(*args, _p(e_ids), _p(e_val), _p(e_cnt), int(n_edit), _cur()),
                 "tn_beam_step_edits")


@beam_step_.register_fake
def _(logits, hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen, unsat, done,
      n_unfinished, out_ids, out_parent, num_beams, penalty, ngram, eos, n_new, length_penalty, early_stopping):
    return None


@custom_op(f"{NS}::beam_step_edits_", mutates_args=_BEAM_STATE, device_types="cuda")
def beam_step_edits_(logits: Tensor, hist: Tensor, hist_len: Tensor, cache_len: Tensor, src: Tensor, run_score: Tensor,
                     fin_ids: Tensor, fin_len: Tensor, fin_score: Tensor, fin_flag: Tensor, gen: Tensor, unsat: Tensor,
                     done: Tensor, n_unfinished: Tensor, out_ids: Tensor, out_parent: Tensor, edit_ids: Tensor,
                     edit_val: Tensor, edit_cnt: Tensor, num_beams: int, penalty: float, ngram: int, eos: List[int],
                     n_new: int, length_penalty: float, early_stopping: int) -> None:
    """beam_step_ with the edit list that constrain_logits_ emitted for the same logits rows (tn_beam_step_edits): edit_ids
    int32 / edit_val fp32 [rows, n_edit], edit_cnt int32 [rows]; edit_val is added to the log-probability of every id with
    edit_ids >= 0, before the repetition penalty."""
    _beam_step("beam_step_edits_", logits, hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag,
               gen, unsat, done, n_unfinished, out_ids, out_parent, num_beams, penalty, ngram, eos, n_new, length_penalty,
               early_stopping, (edit_ids, edit_val, edit_cnt))


@beam_step_edits_.register_fake
def _(logits, hist, hist_len, cache_len, src, run_score, fin_ids, fin_len, fin_score, fin_flag, gen, unsat, done,
      n_unfinished, out_ids, out_parent, edit_ids, edit_val, edit_cnt, num_beams, penalty, ngram, eos, n_new,
      length_penalty, early_stopping):
    return None


CONSTRAIN_MAX_SEQS, CONSTRAIN_MAX_LEN = 16384, 64          # tn_logits_constrain's limits


@custom_op(f"{NS}::constrain_logits_", mutates_args=("logits", "edit_ids", "edit_val", "edit_cnt"), device_types="cuda")
def constrain_logits_(logits: Tensor, hist: Tensor, hist_len: Tensor, prompt_len: Optional[Tensor], seq_off: Tensor,
                      seq_ids: Tensor, seq_bias: Tensor, grp_off: Tensor, grp_tok: Tensor, grp_eos: Tensor,
                      edit_ids: Optional[Tensor], edit_val: Optional[Tensor], edit_cnt: Optional[Tensor], num_beams: int,
                      min_new: int) -> None:
    """`sequence_bias` and `min_new_tokens` of HF generate() on the device (tn_logits_constrain): logits [R_in, V] fp32 /
    bf16, contiguous; hist int32 [R, S_hist], hist_len / prompt_len int32 [R]; R_in == R, or R_in == R / num_beams right
    after a beam search's prefill.  The table of `generation.ConstraintPlan`: seq_off int32 [n_seq + 1], seq_ids int32,
    seq_bias fp32 [n_seq], grp_off int32 [n_grp + 1], grp_tok / grp_eos int32 [n_grp]; at most 16384 sequences of at most
    64 ids.  Without edit tensors the logits are edited in place (logits[t] = T(fp32(logits[t]) + total)); with edit_ids
    int32 / edit_val fp32 [>= R_in, n_grp] and edit_cnt int32 [rows] the logits are left alone and the edit list of
    beam_step_edits_ is written."""
    _no_grad_inputs("constrain_logits_", logits)
    K = int(num_beams)
    if logits.dim() != 2 or hist.dim() != 2 or K < 1 or hist.shape[0] % K:
        raise _C.KernelError("constrain_logits_: logits [R_in, V], hist [R, S_hist] with R a multiple of num_beams")
    R_in, V = logits.shape
    R, S_hist = hist.shape
    if R_in not in (R, R // K):
        raise _C.KernelError("constrain_logits_: logits must have R or R / num_beams rows")
    if not logits.is_contiguous():
        raise _C.KernelError("constrain_logits_: the logits are edited in place and must be contiguous")
    n_seq, n_grp = seq_bias.shape[0], grp_tok.shape[0]
    if n_seq > CONSTRAIN_MAX_SEQS:
        raise _C.KernelError(f"constrain_logits_: at most {CONSTRAIN_MAX_SEQS} sequences")
    for name, t, dt, shape in (("hist", hist, torch.int32, (R, S_hist)), ("hist_len", hist_len, torch.int32, (R,)),
                               ("prompt_len", prompt_len, torch.int32, (R,)),
                               ("seq_off", seq_off, torch.int32, (n_seq + 1,)),
                               ("seq_ids", seq_ids, torch.int32, (seq_ids.numel(),)),
                               ("seq_bias", seq_bias, torch.float32, (n_seq,)),
                               ("grp_off", grp_off, torch.int32, (n_grp + 1,)), ("grp_tok", grp_tok, torch.int32, (n_grp,)),
                               ("grp_eos", grp_eos, torch.int32, (n_grp,))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise _C.KernelError(f"constrain_logits_: {name} must be a contiguous {dt} tensor of shape {list(shape)}")
    emit = edit_ids is not None
    if emit:
        if edit_val is None or edit_cnt is None:
            raise _C.KernelError("constrain_logits_: edit_ids, edit_val and edit_cnt go together")
        rows = edit_ids.shape[0]
        for name, t, dt, shape in (("edit_ids", edit_ids, torch.int32, (rows, n_grp)),
                                   ("edit_val", edit_val, torch.float32, (rows, n_grp)),
                                   ("edit_cnt", edit_cnt, torch.int32, (rows,))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or rows < R_in:
                raise _C.KernelError(f"constrain_logits_: {name} must be a contiguous {dt} tensor of shape "
                                     f"{list(shape)} with at least {R_in} rows")
    _C.check(_lib().tn_logits_constrain(_p(logits), _p(hist), _p(hist_len), _p(prompt_len), _p(seq_off),
                                        _p(seq_ids) if n_seq else None, _p(seq_bias) if n_seq else None, _p(grp_off),
                                        _p(grp_tok), _p(grp_eos), _p(edit_ids), _p(edit_val), _p(edit_cnt), R_in, K,
                                        K if R_in == R and K > 1 else 1, V, S_hist, n_seq, int(seq_ids.numel()), n_grp,
                                        int(min_new), int(emit), _C.dcode(logits), _cur()), "tn_logits_constrain")


@constrain_logits_.register_fake
def _(logits, hist, hist_len, prompt_len, seq_off, seq_ids, seq_bias, grp_off, grp_tok, grp_eos, edit_ids, edit_val,
      edit_cnt, num_beams, min_new):
    return None


# ===================================================================================================== speech tokenizer (frozen)
@custom_op(f"{NS}::attn_block_causal_fwd", mutates_args=(), device_types="cuda")
def attn_block_causal_fwd(q: Tensor, k: Tensor, v: Tensor, seg_start: Tensor, key_end: Tensor, block: int,
                          scale: float) -> Tensor:
    """Block-causal attention of the Kimi-Audio speech tokenizer (tn_attn_block_causal_fwd): q / k / v bf16 [B, T, Nh, 64];
    seg_start / key_end int32 [B, T]: query i attends to keys [s, min(key_end, s + ((i - s) // block + 1) * block)),
    s = seg_start[i].  Forward only (no autograd formula: the tokenizer is frozen)."""
    _no_grad_inputs("attn_block_causal_fwd", q, k, v)
    B, T, Nh, D = q.shape
    if (q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16 or D != 64
            or tuple(k.shape) != (B, T, Nh, D) or tuple(v.shape) != (B, T, Nh, D)
            or seg_start.dtype != torch.int32 or key_end.dtype != torch.int32
            or tuple(seg_start.shape) != (B, T) or tuple(key_end.shape) != (B, T) or block < 1):
        raise _C.KernelError("attn_block_causal_fwd: bf16 q / k / v [B, T, Nh, 64] (Nh == Nkv), int32 seg_start / key_end "
                             "[B, T], block >= 1")
    q, k, v, s, e = _c(q), _c(k), _c(v), _c(seg_start), _c(key_end)
    o = torch.empty_like(q)
    _C.check(_lib().tn_attn_block_causal_fwd(_p(q), _p(k), _p(v), _p(o), _p(s), _p(e), B, T, Nh, D, int(block),
                                             float(scale), _cur()), "tn_attn_block_causal_fwd")
    return o


@attn_block_causal_fwd.register_fake
def _(q, k, v, seg_start, key_end, block, scale):
    return torch.empty_like(q, memory_format=torch.contiguous_format)


@custom_op(f"{NS}::vq_nearest", mutates_args=(), device_types="cuda")
def vq_nearest(x: Tensor, codebook: Tensor, cnorm: Tensor) -> Tensor:
    """ids int64 [M] = argmin_c (cnorm[c] - 2 x[r] . c), first index on ties (tn_vq_nearest): x bf16 [M, d], codebook bf16
    [V, d], cnorm fp32 [V] = |c|^2, d % 64 == 0.  Forward only."""
    _no_grad_inputs("vq_nearest", x, codebook)
    if (x.dim() != 2 or codebook.dim() != 2 or x.dtype != torch.bfloat16 or codebook.dtype != torch.bfloat16
            or x.shape[1] != codebook.shape[1] or x.shape[1] % 64 != 0 or codebook.shape[0] < 1
            or cnorm.dtype != torch.float32 or tuple(cnorm.shape) != (codebook.shape[0],)):
        raise _C.KernelError("vq_nearest: bf16 x [M, d] and codebook [V, d] with d % 64 == 0, fp32 cnorm [V]")
    x, cb, cn = _c(x), _c(codebook), _c(cnorm)
    M, d = x.shape
    ids = torch.empty(M, dtype=torch.int64, device=x.device)
    _C.check(_lib().tn_vq_nearest(_p(x), _p(cb), _p(cn), _p(ids), M, cb.shape[0], d, _cur()), "tn_vq_nearest")
    return ids


@vq_nearest.register_fake
def _(x, codebook, cnorm):
    return x.new_empty(x.shape[0], dtype=torch.int64)


# ===================================================================================================== scoring
def edit_align_ws_words(R: int, H: int) -> int:
    """words of tn_edit_align's workspace that one (R, H) pair needs; -1 for lengths the kernel does not take"""
    return int(_lib().tn_edit_align_ws_words(int(R), int(H)))


@custom_op(f"{NS}::edit_align", mutates_args=(), device_types="cuda")
def edit_align(ref_tok: Tensor, hyp_tok: Tensor, desc: Tensor) -> Tuple[Tensor, Tensor]:
    """Edit-distance alignment with the reference scorer's tie rule (tn_edit_align, csrc/edit_align.hip): ref_tok / hyp_tok
    packed int32 device tokens, desc a CPU int32 [P, 6] table {ref_start, R, hyp_start, H, ws_base, ops_base} whose
    workspace ranges ascend.  -> counts int32 [P, 5] (C, S, I, D, arcs) and ops uint8 [n_ref + n_hyp] (0 C, 1 S, 2 I, 3 D,
    each pair's arcs right-aligned in its R + H bytes; the bytes to their left are zero).  The entry point checks the whole
    table on the host and refuses (-22) before it launches anything."""
    if (ref_tok.dtype != torch.int32 or hyp_tok.dtype != torch.int32 or ref_tok.dim() != 1 or hyp_tok.dim() != 1
            or desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 6 or desc.is_cuda):
        raise _C.KernelError("edit_align: int32 device tokens ref_tok [n_ref] / hyp_tok [n_hyp], int32 CPU desc [P, 6]")
    ref_tok, hyp_tok, desc = _c(ref_tok), _c(hyp_tok), _c(desc)
    P, dev = desc.shape[0], ref_tok.device
    n_ops = ref_tok.numel() + hyp_tok.numel()
    counts = torch.empty(P, 5, dtype=torch.int32, device=dev)
    ops = torch.zeros(n_ops, dtype=torch.uint8, device=dev)
    if P == 0:
        return counts, ops
    last = desc[-1].tolist()                            # the ranges ascend, so the last pair's end is the workspace's
    if last[4] < 0 or edit_align_ws_words(last[1], last[3]) < 0:
        raise _C.KernelError("edit_align: 1 <= R <= 16383, 0 <= H <= 16383 and ws_base >= 0 for every pair")
    ws_words = last[4] + edit_align_ws_words(last[1], last[3])
    ws = torch.empty(ws_words, dtype=torch.int32, device=dev)
    desc_dev = torch.empty(P, 6, dtype=torch.int32, device=dev)
    _C.check(_lib().tn_edit_align(_p(ref_tok), ref_tok.numel(), _p(hyp_tok), hyp_tok.numel(),
                                  ctypes.c_void_p(desc.data_ptr()), _p(desc_dev), P, _p(ws), ws_words, _p(ops), n_ops,
                                  _p(counts), _cur()), "tn_edit_align")
    return counts, ops


@edit_align.register_fake
def _(ref_tok, hyp_tok, desc):
    return (ref_tok.new_empty(desc.shape[0], 5, dtype=torch.int32),
            ref_tok.new_empty(ref_tok.numel() + hyp_tok.numel(), dtype=torch.uint8))


TOKEN_SCORES_MAX_ALT, TOKEN_SCORES_MAX_VOCAB = 8, 262144          # tn_token_scores' limits


def _token_scores_logits(what: str, logits: Tensor, k: int) -> Tensor:
    _no_grad_inputs(what, logits)
    if logits.dim() != 2 or not 1 <= logits.shape[1] <= TOKEN_SCORES_MAX_VOCAB:
        raise _C.KernelError(f"{what}: logits [R, V] with 1 <= V <= {TOKEN_SCORES_MAX_VOCAB}")
    if not 0 <= k <= TOKEN_SCORES_MAX_ALT:
        raise _C.KernelError(f"{what}: k = {k} must be in [0, {TOKEN_SCORES_MAX_ALT}]")
    return _c(logits)


@custom_op(f"{NS}::token_scores", mutates_args=(), device_types="cuda")
def token_scores(logits: Tensor, tok: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Per-token confidences in token mode (tn_token_scores): logits [R, V] fp32 / bf16, tok int32 [R] -> logp fp32 [R] =
    log_softmax(logits)[r, tok[r]] (NaN for an id outside [0, V)), entropy fp32 [R], alt_id int32 [R, k] (the k most
    likely ids, ties to the lower id; -1 behind the V-th) and alt_logp fp32 [R, k].  A row with a NaN or +inf, or with
    nothing but -inf: NaN and ids -1."""
    logits = _token_scores_logits("token_scores", logits, k)
    R, V = logits.shape
    if tok.dtype != torch.int32 or tuple(tok.shape) != (R,):
        raise _C.KernelError("token_scores: int32 tok [R]")
    tok, dev = _c(tok), logits.device
    logp = torch.empty(R, dtype=torch.float32, device=dev)
    entropy = torch.empty(R, dtype=torch.float32, device=dev)
    alt_id = torch.empty(R, k, dtype=torch.int32, device=dev)
    alt_logp = torch.empty(R, k, dtype=torch.float32, device=dev)
    if R:
        _C.check(_lib().tn_token_scores(_p(logits), _p(tok), None, None, _p(logp), _p(entropy), _p(alt_id) if k else None,
                                        _p(alt_logp) if k else None, R, V, 0, int(k), _C.dcode(logits), _cur()),
                 "tn_token_scores")
    return logp, entropy, alt_id, alt_logp


@token_scores.register_fake
def _(logits, tok, k):
    R = logits.shape[0]
    return (logits.new_empty(R, dtype=torch.float32), logits.new_empty(R, dtype=torch.float32),
            logits.new_empty(R, k, dtype=torch.int32), logits.new_empty(R, k, dtype=torch.float32))


@custom_op(f"{NS}::token_scores_", mutates_args=("logp", "entropy", "alt_id", "alt_logp"), device_types="cuda")
def token_scores_(logits: Tensor, hist: Tensor, hist_len: Tensor, logp: Tensor, entropy: Tensor, alt_id: Optional[Tensor],
                  alt_logp: Optional[Tensor], k: int) -> None:
    """Per-token confidences in history mode (tn_token_scores), one launch behind a step kernel: logits [R, V], hist int32
    [R, S_hist], hist_len int32 [R]; the token is hist[r, hist_len[r] - 1] and its scores are written to column
    hist_len[r] - 1 of logp / entropy fp32 [R, S_hist] and alt_id int32 / alt_logp fp32 [R, S_hist, k] (None with k == 0).
    A row whose hist_len is outside [1, S_hist] writes nothing."""
    logits = _token_scores_logits("token_scores_", logits, k)
    R, V = logits.shape
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] != R or hist.shape[1] < 1 or not hist.is_contiguous():
        raise _C.KernelError("token_scores_: int32 contiguous hist [R, S_hist]")
    S = hist.shape[1]
    if hist_len.dtype != torch.int32 or tuple(hist_len.shape) != (R,) or not hist_len.is_contiguous():
        raise _C.KernelError("token_scores_: int32 hist_len [R]")
    for name, t, dt, shape in (("logp", logp, torch.float32, (R, S)), ("entropy", entropy, torch.float32, (R, S)),
                               ("alt_id", alt_id, torch.int32, (R, S, k)), ("alt_logp", alt_logp, torch.float32, (R, S, k))):
        if t is None and k == 0 and name.startswith("alt_"):
            continue
        if t is None or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != logits.device:
            raise _C.KernelError(f"token_scores_: {name} must be a contiguous {dt} tensor of shape {list(shape)}")
    if R:
        _C.check(_lib().tn_token_scores(_p(logits), None, _p(hist), _p(hist_len), _p(logp), _p(entropy),
                                        _p(alt_id) if k else None, _p(alt_logp) if k else None, R, V, S, int(k),
                                        _C.dcode(logits), _cur()), "tn_token_scores")


@token_scores_.register_fake
def _(logits, hist, hist_len, logp, entropy, alt_id, alt_logp, k):
    return None


OPS = ("rmsnorm_fwd","rmsnorm_bwd", "layernorm_fwd", "layernorm_bwd", "swiglu_fwd", "swiglu_bwd", "gelu_fwd",
       "gelu_bwd", "rope_apply", "attn_fwd", "attn_bwd", "attn_fwd_bidir", "attn_bwd_bidir", "attn_bwd_stacked",
       "attn_bwd_rope", "attn_build_meta", "attn_fwd_seg", "attn_fwd_seg_chunks", "attn_merge", "attn_bwd_seg", "ce_fwd",
       "ce_bwd", "ce_bwd_", "gemm_tn", "rope_table", "transpose_bf16_", "colsum_bf16", "swiglu_fwd_t", "swiglu_bwd_t",
       "ce_fwd_rows", "ce_reduce", "log_mel", "audiofeat_stack", "pcm16_to_f32", "bestrq_tokenize",
       "attn_decode_", "greedy_step_", "sample_step_", "attn_block_causal_fwd", "vq_nearest", "attn_decode_beam_",
       "beam_step_", "kimi_text_step_", "kaldi_feats", "kaldi_mfcc", "edit_align", "beam_step_edits_",
       "constrain_logits_", "token_scores", "token_scores_", "vad_log_energy", "vad_runs")
