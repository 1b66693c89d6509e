"""PyTorch-ROCm custom ops over the HIP kernels (autograd.Function wrappers around the C ABI).

Every function here runs on the device through libtouchnet_amd.so and raises if that is impossible
(CPU tensor, unsupported dtype/shape, missing library).  There is no eager fallback anywhere.

Signatures mirror the modules the reference swaps (the liger precedent at
touchnet/models/llama/__init__.py:11-15): RMSNorm, rotary embedding, SwiGLU MLP activation, the
attention interface (transformers attention-function contract, SURVEY.md §8b hook 2) and the
TrainSpec loss / acc functions (hook 3).
"""
from __future__ import annotations

import ctypes
import math
import os
import weakref
from dataclasses import dataclass
from typing import Optional

import torch

from . import _C
from . import library as L

_cur = _C.stream
_p = _C.ptr


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------ norms
def rms_norm(x, weight, eps, residual=None):
    """y = RMSNorm(x (+ residual)) * weight.  With ``residual`` returns ``(y, x + residual)``: the
    residual add of the decoder layer (modeling_llama.py:306-324) is fused into the norm that follows it."""
    y, h, _ = L.rmsnorm_fwd(x, residual, weight, float(eps))
    return (y, h) if residual is not None else y


def layer_norm(x, weight, bias, eps=1e-5, residual=None):
    y, h, _, _ = L.layernorm_fwd(x, residual, weight, bias, float(eps))
    return (y, h) if residual is not None else y


# ------------------------------------------------------------------------------------ activations
def swiglu(gate, up):
    """silu(gate) * up (modeling_llama.py:174-176)."""
    return L.swiglu_fwd(gate, up)


def gelu(x):
    return L.gelu_fwd(x)


# ------------------------------------------------------------------------------------ RoPE
def rope_inv_freq(head_dim: int, theta: float, scaling: Optional[dict] = None, device=None) -> torch.Tensor:
    """fp32 [head_dim/2] inverse frequencies, default or llama3-scaled
    (the table `post_init` re-derives at touchnet/models/llama/__init__.py:23-27)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    kind = (scaling or {}).get("rope_type", (scaling or {}).get("type", "default"))
    if kind == "llama3":
        factor, lo, hi = scaling["factor"], scaling["low_freq_factor"], scaling["high_freq_factor"]
        old = scaling["original_max_position_embeddings"]
        wavelen = 2 * math.pi / inv
        inv_l = torch.where(wavelen > old / lo, inv / factor, inv)
        smooth = (old / wavelen - lo) / (hi - lo)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        medium = ~(wavelen < old / hi) & ~(wavelen > old / lo)
        inv = torch.where(medium, smoothed, inv_l)
    elif kind != "default":
        raise _C.KernelError(f"unsupported rope_type {kind!r}")
    return inv.to(device) if device is not None else inv


def rope_tables(position_ids: torch.Tensor, inv_freq: torch.Tensor, dtype, attention_scaling: float = 1.0):
    """cos/sin [B*T, D/2] in ``dtype`` from packed int64 position_ids [B, T] (once per forward)."""
    pos = _c(position_ids).to(torch.int64).view(-1)
    inv = _c(inv_freq).float()
    if dtype not in _C.DTYPE_CODE:
        raise _C.KernelError(f"unsupported dtype {dtype} (float32 / bfloat16 only)")
    return L.rope_table(pos, inv, float(attention_scaling), dtype)


def apply_rope(q, k, cos, sin):
    """q [B,T,Nh,D], k [B,T,Nkv,D] (the GEMM output layout — no head transpose), tables from rope_tables."""
    return L.rope_apply(q, k, cos, sin, False)


# ------------------------------------------------------------------------------------ attention
@dataclass
class PackedMask:
    """Device-side form of the packers' document-id `attention_mask`
    (touchnet/models/llama/processing_llama.py:38-40): int32 ids + the range metadata of `library.attn_build_meta`
    (statistics per 64 and per 32 positions, stored tile lists per 128: csrc/attn_common.h).
    Built once per batch and shared by all layers (the reference builds its BlockMask once per forward)."""
    doc: torch.Tensor     # int32 [B, T], 0 = pad
    meta: torch.Tensor    # int32 [library.attn_meta_ints(B, T)]
    B: int
    T: int


def build_packed_mask(doc_ids: torch.Tensor) -> PackedMask:
    B, T = doc_ids.shape
    doc = _c(doc_ids).to(torch.int32)
    return PackedMask(doc, L.attn_build_meta(doc), B, T)


def causal_mask(B: int, T: int, device) -> PackedMask:
    """Plain causal attention (the Qwen2-Audio training path, qwen2_audio/__init__.py:231-236) =
    one document per row."""
    return build_packed_mask(torch.ones(B, T, dtype=torch.int32, device=device))


# False: the rotary embedding's backward as its own pass over dq / dk (same bits; the tests' reference)
ROPE_GRAD_IN_ATTENTION = True


class _AttentionRopeGrad(torch.autograd.Function):
    """`packed_attention` of q / k that carry a rotary embedding put there by `linear_group(rope=..)`: the backward hands
    dq / dk over as gradients of the UN-rotated projections (tn_attn_bwd_rope — the transposed rotation in the attention
    kernels' epilogues instead of a pass over dq / dk), and the projection node is told not to rotate them back again
    (`linear_group(.., rope_grad_in_attention=True)`; the pair is set up in one place, models/llama Attention.forward)."""

    @staticmethod
    def forward(ctx, q, k, v, doc, meta, scale, cos, sin):
        o, lse2 = L.attn_fwd(q, k, v, doc, meta, scale)
        ctx.save_for_backward(_c(q), _c(k), _c(v), o, lse2, doc, meta, cos, sin)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse2, doc, meta, cos, sin = ctx.saved_tensors
        stacked = q.shape == k.shape                       # (multi-head: one buffer, three slices; grouped-query: flat)
        out = L.attn_bwd_rope(q, k, v, o, do, lse2, doc, meta, ctx.scale, cos, sin, stacked)
        _, (dq, dk, dv) = L.attn_grads(q, k, "stacked" if stacked else "flat", out)
        return dq, dk, dv, None, None, None, None, None


def _attention_scale(name: str, q, mask: PackedMask, scale: Optional[float], rows: Optional[int] = None) -> float:
    """The check and the default that the attention entry points share: q is [B, rows, Nh, D] for a mask built for [B, T]
    (rows = T, or the `rows_per_batch` of a sequence-sharded query side) -> scale, head_dim ** -0.5 unless given."""
    rows = mask.T if rows is None else int(rows)
    if tuple(q.shape[:2]) != (mask.B, rows):
        raise _C.KernelError(f"{name}: mask built for {(mask.B, mask.T)}, {rows} query rows per batch; "
                             f"got q {tuple(q.shape[:2])}")
    return float(q.shape[-1] ** -0.5 if scale is None else scale)


def packed_attention(q, k, v, mask: PackedMask, scale: Optional[float] = None, rope_grad=None):
    """softmax(scale * Q K^T + doc-causal mask) V with q [B,T,Nh,D], k/v [B,T,Nkv,D] -> [B,T,Nh,D].
    ``rope_grad = (cos, sin)``: q and k are ROTATED outputs of `linear_group(.., rope=(cos, sin, ..),
    rope_grad_in_attention=True)`; their gradients leave this node already rotated back (`_AttentionRopeGrad`)."""
    scale = _attention_scale("packed_attention", q, mask, scale)
    if rope_grad is not None:
        cos, sin = rope_grad
        return _AttentionRopeGrad.apply(q, k, v, mask.doc, mask.meta, scale, _c(cos.detach()), _c(sin.detach()))
    return L.attn_fwd(q, k, v, mask.doc, mask.meta, scale)[0]


def bidirectional_attention(q, k, v, mask: PackedMask, scale: Optional[float] = None):
    """softmax(scale * Q K^T + same-document mask) V — every key of the query's document, before AND after it — with
    q [B,T,Nh,D], k/v [B,T,Nkv,D] -> [B,T,Nh,D]; pad rows (document 0) give 0 (`library.attn_fwd_bidir`)."""
    scale = _attention_scale("bidirectional_attention", q, mask, scale)
    return L.attn_fwd_bidir(q, k, v, mask.doc, mask.meta, scale)[0]


@dataclass(frozen=True)
class SeqShard:
    """Which global positions of the packed row the local query-side rows hold (context parallelism).
    `segs` = up to two (row0, rows, global_offset) triples; buffers are [B, rows_per_batch, ...]."""
    segs: tuple
    rows_per_batch: int

    def flat(self):
        return [int(v) for seg in self.segs for v in seg]


def packed_attention_sharded(q_local, k_full, v_full, mask: PackedMask, shard: SeqShard,
                             scale: Optional[float] = None):
    """Context-parallel building block: local query rows (per `shard`) against the full, all-gathered K/V.
    The gradient w.r.t. k_full / v_full is this rank's PARTIAL sum (to be reduce-scattered by the caller)."""
    scale = _attention_scale("packed_attention_sharded", q_local, mask, scale, shard.rows_per_batch)
    return L.attn_fwd_seg(q_local, k_full, v_full, mask.doc, mask.meta, scale, shard.flat(),
                          int(shard.rows_per_batch))[0]


class _SplitAttention(torch.autograd.Function):
    """Context-parallel attention with the exchange hidden under the LOCAL part: the rank's query rows first attend to
    the keys of its OWN chunks (in the global K/V buffers from the start), then the compute stream waits for the halo
    (`wait`), the rows attend to the RECEIVED chunks, and the two partial results are merged by their log-sum-exp
    (tn_attn_merge).  The backward is ONE tn_attn_bwd_seg over all chunks with the merged O / LSE — the gradient of a
    softmax over the union of the key sets does not care how the forward was split."""

    @staticmethod
    def forward(ctx, q, k_full, v_full, doc, meta, scale, segs, rpb, chunk_len, own_mask, remote_mask, wait):
        o, lse = L.attn_fwd_seg_chunks(q, k_full, v_full, doc, meta, scale, segs, rpb, chunk_len, own_mask)
        if wait is not None:
            wait()
        if remote_mask:
            o_b, lse_b = L.attn_fwd_seg_chunks(q, k_full, v_full, doc, meta, scale, segs, rpb, chunk_len, remote_mask)
            o, lse = L.attn_merge(o, lse, o_b, lse_b)
        ctx.save_for_backward(_c(q), _c(k_full), _c(v_full), o, lse, doc, meta)
        ctx.scale, ctx.segs, ctx.rpb = scale, list(segs), rpb
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, doc, meta = ctx.saved_tensors
        dq, dk, dv = L.attn_bwd_seg(q, k, v, o, do, lse, doc, meta, ctx.scale, ctx.segs, ctx.rpb)
        return dq, dk, dv, None, None, None, None, None, None, None, None, None


def packed_attention_sharded_split(q_local, k_full, v_full, mask: PackedMask, shard: SeqShard, chunk_len: int,
                                   own_chunks, remote_chunks, wait=None, scale: Optional[float] = None):
    """`packed_attention_sharded` as two key-side parts + an LSE merge: `own_chunks` / `remote_chunks` = indices of the
    sequence chunks (of `chunk_len` positions) the first / second part covers; `wait()` is called between the two (the
    halo exchange's completion: the remote chunks of k_full / v_full may still be in flight before it)."""
    scale = _attention_scale("packed_attention_sharded_split", q_local, mask, scale, shard.rows_per_batch)
    bits = lambda cs: sum(1 << int(c) for c in cs)
    return _SplitAttention.apply(q_local, k_full, v_full, mask.doc, mask.meta, scale, shard.flat(),
                                 int(shard.rows_per_batch), int(chunk_len), bits(own_chunks), bits(remote_chunks), wait)


# ------------------------------------------------------------------------------------ loss
def _num_sentence_dev(num_sentence, device):
    if isinstance(num_sentence, torch.Tensor):
        return num_sentence.to(device=device, dtype=torch.float32).reshape(1)
    return torch.tensor([float(num_sentence)], dtype=torch.float32, device=device)


class _PackedCEInplace(torch.autograd.Function):
    """`inplace_grad=True`: the backward writes dlogits over the logits (dead after the loss): mi355_touch::ce_bwd_."""

    @staticmethod
    def forward(ctx, logits, lab, sl, ns, ignore_index):
        with torch.no_grad():
            loss, out, lse = L.ce_fwd(logits, lab, sl, ns, ignore_index)
        ctx.save_for_backward(logits, lab, sl, lse, ns)
        ctx.ignore_index = ignore_index
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, g_loss, _g_out):
        logits, lab, sl, lse, ns = ctx.saved_tensors
        L.ce_bwd_(logits, lab, sl, lse, ns, _c(g_loss).to(torch.float32).reshape(1), ctx.ignore_index)
        return logits, None, None, None, None


def packed_cross_entropy(pred, labels, sentence_lens, num_sentence, ignore_index=-100, inplace_grad=False):
    """Returns ``(loss_per_sample [differentiable], stats)`` with
    ``stats = [loss_per_sample, loss_per_token, accuracy, n_valid]`` (fp32 device tensor, no host sync)."""
    V = pred.shape[-1]
    logits = _c(pred).view(-1, V)
    lab = _c(labels).to(torch.int64).view(-1)
    sl = _c(sentence_lens).to(torch.int64).view(-1)
    ns = _num_sentence_dev(num_sentence, pred.device)
    if inplace_grad:
        return _PackedCEInplace.apply(logits, lab, sl, ns, int(ignore_index))
    loss, stats, _ = L.ce_fwd(logits, lab, sl, ns, int(ignore_index))
    return loss, stats.detach()


class _FusedLinearCE(torch.autograd.Function):
    """lm_head GEMM + packed CE, chunked over tokens so the [B*T, V] logits never exist at once
    (the liger fused-linear-CE idea, touchnet/bin/train.py:443-445 — but keeping the reference's
    per-sentence normalisation, which liger's mean-over-tokens drops, SURVEY.md §2.3 K10').
    Gradients w.r.t. hidden and weight are produced in the forward pass and scaled by the upstream
    gradient in backward.
    Roundings: the logits and the dlogits of a chunk are stored in bf16; d(hidden) and d(weight) are fp32 sums rounded to
    bf16 once (d(weight) over ALL chunks: fp32 buffer, one rounding); the upstream gradient is cast to bf16 in backward."""

    @staticmethod
    def forward(ctx, hidden, weight, labels, sentence_lens, num_sentence, ignore_index, chunk, compact=False, tp=None):
        """`tp = (group, rank, size)` — loss parallel (models/tensor_parallel.py): `weight` holds rows
        [rank V/size, (rank+1) V/size) of the vocabulary.  Every chunk computes the LOCAL logits and row statistics with the
        unchanged CE kernels (a label outside the shard is passed as V_local = "no local target": the forward kernel then
        returns nll = lse_local, the backward kernel a pure softmax), combines max / sum-exp / target logit over the group
        (three [rows] all-reduces) and back-propagates with the GLOBAL log-sum-exp.  d(hidden) is this rank's PARTIAL sum
        over its vocabulary shard: the sequence gather in front of the head (`SequenceParallel.gather`, partial=True)
        reduce-scatters it."""
        H = hidden.shape[-1]
        h2 = hidden.reshape(-1, H)
        lab = labels.reshape(-1).to(torch.int64).contiguous()
        sl = sentence_lens.reshape(-1).to(torch.int64).contiguous()
        rows = None
        overflow = None
        if compact is not False and compact is not None:
            # Positions whose label is ignore_index contribute exactly 0 to the loss, to d(hidden) and to d(weight) —
            # the CE kernels already never read their logits; here the lm_head GEMMs skip them too (ASR-SFT batches:
            # > 90 % of the positions are audio / prompt).  Same loss and gradients up to GEMM summation order.
            #   compact = int   upper bound of the labelled positions, known to the data loader (the packers emit
            #                   `labelled_rows_max`): static shapes, NO host synchronisation — rows beyond the real count
            #                   are given the label ignore_index; a bound that is too small poisons the loss with NaN
            #                   (decided on the device) instead of silently dropping labels
            #   compact = True  exact count read back from the device (one host sync per step)
            n_all = h2.shape[0]
            labelled = lab != ignore_index
            if compact is True:
                rows = torch.nonzero(labelled).squeeze(1)
            else:
                n_max = min(int(compact), n_all)
                rows = torch.nonzero_static(labelled, size=max(n_max, 1), fill_value=0).squeeze(1)
                count = labelled.sum()
                valid = torch.arange(rows.numel(), device=lab.device) < count
                overflow = count > n_max
            if rows.numel() == 0:                              # nothing labelled: zero loss, zero gradients
                rows = None
            else:
                h2, lab, sl = h2.index_select(0, rows), lab.index_select(0, rows), sl.index_select(0, rows)
                if compact is not True:
                    lab = torch.where(valid, lab, torch.full_like(lab, ignore_index))
        n, V = h2.shape[0], weight.shape[0]
        ns = _num_sentence_dev(num_sentence, hidden.device)
        one = torch.ones(1, dtype=torch.float32, device=hidden.device)
        dh = torch.empty_like(h2)
        dw = None
        parts = []
        lab_k = lab                                        # the labels the kernels see
        if tp is not None:
            from touchnet_amd.models.tensor_parallel import tp_all_reduce
            group, tp_rank, _ = tp
            v0 = tp_rank * V
            mine = (lab >= v0) & (lab < v0 + V)
            lab_k = torch.where(lab == ignore_index, lab, torch.where(mine, lab - v0, torch.full_like(lab, V)))
        for s in range(0, n, chunk):
            e = min(s + chunk, n)
            logits = _mm_tn(h2[s:e], weight)                                  # [c, V]: the only logits alive
            nll_c, lse_c, hit_c = L.ce_fwd_rows(logits, lab_k[s:e], sl[s:e], ns, int(ignore_index))
            if tp is not None:
                valid = lab[s:e] != ignore_index
                target = lse_c - nll_c                                        # the target's logit where it is local, else 0
                top_v, top_i = logits.float().max(dim=1)
                mx = torch.where(valid, lse_c, torch.full_like(lse_c, float("-inf")))
                tp_all_reduce(mx, group, torch.distributed.ReduceOp.MAX)
                se = torch.where(valid, torch.exp(lse_c - mx), torch.zeros_like(lse_c))
                tp_all_reduce(se, group)
                tp_all_reduce(target, group)
                lse_c = torch.where(valid, mx + torch.log(se), torch.zeros_like(lse_c))
                nll_c = torch.where(valid, lse_c - target, torch.zeros_like(lse_c))
                # accuracy: the argmax over ALL shards (first index on ties: lowest shard, then lowest index inside it)
                best = torch.stack([top_v, (top_i + v0).float()], dim=1)                      # indices < 2^24: exact
                if not getattr(group, "emulated", False):
                    size = torch.distributed.get_world_size(group)
                    every = torch.empty((size * best.shape[0], 2), dtype=best.dtype, device=best.device)
                    torch.distributed.all_gather_into_tensor(every, best.contiguous(), group=group)
                    every = every.view(size, best.shape[0], 2)                                # rank-major
                    win = every[..., 0].argmax(dim=0)
                    best = every.gather(0, win[None, :, None].expand(1, -1, 2))[0]
                hit_c = ((best[:, 1].to(torch.int64) == lab[s:e]) & valid).to(hit_c.dtype)
            L.ce_bwd_(logits, lab_k[s:e], sl[s:e], lse_c, ns, one, int(ignore_index))     # logits := dlogits
            parts.append((nll_c, hit_c))
            _dgrad([logits], [weight], out=dh[s:e], dgrad_tn=False)           # dh = dlogits @ W
            if dw is None and n > chunk and logits.dtype == torch.bfloat16:
                # several chunks: the sum over the chunks is kept in fp32 and rounded to bf16 ONCE behind the loop (a bf16
                # buffer would round the partial sum once per chunk).  Costs V x H x 4 bytes while the loop runs and one
                # cast pass; the step's usual shape (labelled rows <= chunk) does not come here.
                dw = torch.zeros(V, H, dtype=torch.float32, device=h2.device)
            dw = _wgrad_unowned(logits, h2[s:e], out=dw, accumulate=dw is not None)      # dW (+)= dlogits^T @ h
            del logits
        if dw.dtype != h2.dtype:
            dw = dw.to(h2.dtype)
        nll = torch.cat([a for a, _ in parts]) if len(parts) > 1 else parts[0][0]
        hit = torch.cat([b for _, b in parts]) if len(parts) > 1 else parts[0][1]
        out = L.ce_reduce(nll, hit, lab, sl, ns, int(ignore_index))
        if rows is not None:                                   # scatter d(hidden) back; ignored rows stay 0
            # (index_add: the filler rows of the static form repeat index 0 and carry exact zeros)
            dh = torch.zeros(n_all, H, dtype=dh.dtype, device=dh.device).index_add_(0, rows, dh)
        if overflow is not None:
            # a bound that is too small poisons the statistics AND both gradients (they were computed from the truncated
            # label set): the optimizer's non-finite check then skips the step instead of applying it
            poison = torch.where(overflow, float("nan"), 1.0)
            out = out * poison.to(out.dtype)
            dh = dh * poison.to(dh.dtype)
            dw = dw * poison.to(dw.dtype) if dw is not None else dw
        ctx.save_for_backward(dh, dw)
        ctx.hshape, ctx.wdtype = hidden.shape, weight.dtype
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g_loss, _g):
        dh, dw = ctx.saved_tensors
        g = g_loss.to(torch.float32)
        # (same-dtype operands: a bf16 tensor times an fp32 0-dim DEVICE tensor takes TensorIterator's casting kernel,
        #  1.4 TB/s on the [V, H] weight gradient — 1.8 ms/step at V = 156 k; the upstream gradient is 1 or a power of two)
        return ((dh * g.to(dh.dtype)).view(ctx.hshape), (dw * g.to(dw.dtype)).to(ctx.wdtype), None, None, None, None, None,
                None, None)


def fused_linear_cross_entropy(hidden, weight, labels, sentence_lens, num_sentence, ignore_index=-100,
                               chunk_tokens=4096, compact=False, tp=None):
    """Returns ``(loss_per_sample [differentiable], stats)`` like packed_cross_entropy, from hidden states.
    ``compact``: run lm_head only on the labelled positions — an int upper bound from the data loader (no host sync)
    or True (exact, one sync); ``tp``: vocabulary-parallel head (loss parallel); see _FusedLinearCE.forward."""
    return _FusedLinearCE.apply(hidden, weight, labels, sentence_lens, num_sentence, ignore_index, chunk_tokens,
                                compact, tp)


# ------------------------------------------------------------------------------------ linear layers
def transpose_2d(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[c, r] = x[r, c]`` for a bf16 matrix whose rows are contiguous (row stride >= cols), HIP kernel."""
    if x.dim() != 2 or x.dtype != torch.bfloat16 or not (x.is_cuda or x.is_meta) or x.stride(1) != 1:
        raise RuntimeError("transpose_2d: expects a 2-D bf16 device tensor with contiguous rows")
    R, Cn = x.shape
    if out is None:
        out = torch.empty(Cn, R, dtype=x.dtype, device=x.device)
    L.transpose_bf16_(x, out)
    return out


def column_sum(x: torch.Tensor) -> torch.Tensor:
    """``x.sum(0)`` of a bf16 [rows, cols] device matrix (fp32 accumulation, bf16 result): the bias gradient."""
    R, Cn = x.shape
    if x.dtype != torch.bfloat16 or not (x.is_cuda or x.is_meta) or x.stride(1) != 1 or Cn % 8 or x.stride(0) % 8:
        return x.sum(0)                                    # (fp32 / odd widths: torch's reduction, still on the device)
    return L.colsum_bf16(x)


def _out_or_new(name, out, accumulate, M, N, device):
    """The output of a GEMM entry point: ``out`` or, by default, a new bf16 [M, N] matrix — which nothing can be added to."""
    if out is not None:
        return out
    if accumulate:
        raise _C.KernelError(f"{name}: accumulate needs an output to add to")
    return torch.empty(M, N, dtype=torch.bfloat16, device=device)


def gemm_tn(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            accumulate: bool = False, out_t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = a @ b.T (+ bias) (+ out)`` with the hand-written MFMA kernel (csrc/gemm.hip): a [M, K], b [N, K] bf16
    device matrices with contiguous rows.  ``out_t`` [N, M] additionally receives the transposed result."""
    if a.dim() != 2 or b.dim() != 2 or a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise _C.KernelError("gemm_tn: 2-D bf16 operands only")
    if a.stride(1) != 1 or b.stride(1) != 1 or a.shape[1] != b.shape[1]:
        raise _C.KernelError("gemm_tn: operands must be contraction-contiguous [M, K] / [N, K]")
    M, K = a.shape
    N = b.shape[0]
    out = _out_or_new("gemm_tn", out, accumulate, M, N, a.device)
    if out.stride(1) != 1 or tuple(out.shape) != (M, N):
        raise _C.KernelError("gemm_tn: bad `out`")
    if bias is not None:
        bias = _c(bias).to(a.dtype)
    _C.check(_C.lib().tn_gemm_bf16_tn(_p(a), _p(b), _p(out), _p(out_t), _p(bias), M, N, K, a.stride(0), b.stride(0),
                                      out.stride(0), out_t.stride(0) if out_t is not None else 0, int(accumulate),
                                      _cur()), "tn_gemm_bf16_tn")
    return out


def gemm(segs, a_kmaj: bool = False, b_kmaj: bool = False, bias: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None, accumulate: bool = False,
         out_t: Optional[torch.Tensor] = None, bias_grad: Optional[torch.Tensor] = None,
         addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[M, N] = sum_s opA_s @ opB_s^T (+ bias) (+ out)`` on the hand-written MFMA kernel (csrc/gemm.hip), fp32
    accumulation over all segments, one rounding.  ``segs`` = 1..3 pairs ``(a, b)`` of bf16 device matrices with
    contiguous rows AS STORED: ``a`` is [M, K] (``a_kmaj=False``) or [K, M] (``a_kmaj=True``: the contraction index is the
    slow one), ``b`` is [N, K] or [K, N] likewise.  The three products of a linear layer y = x W^T:
        forward          gemm([(x, W)])                          x [M, K], W [N, K]
        input gradient   gemm([(dy, W)], b_kmaj=True)            dy [M, N] · W [N, K]      (contraction over N)
        weight gradient  gemm([(dy, x)], True, True)             dy [M, N]^T · x [M, K]    (contraction over tokens)
    — none of them needs a transposed copy of an operand.
    ``bias_grad`` (weight-gradient mode, one segment): a bf16 [M] vector that receives the column sums of ``a`` — the bias
    gradient dY.sum(0) — from the same launch (tn_gemm_bf16_wgrad_bias): no separate pass over dY.
    ``addend`` (one segment, bf16 [M, N], contiguous rows): ``out = bf16(product + bias) + addend`` in the epilogue
    (tn_gemm_bf16_addend: the residual stream added where the projection is produced)."""
    if not 1 <= len(segs) <= 3:
        raise _C.KernelError("gemm: 1..3 segments")
    for a, b in segs:
        if a.dim() != 2 or b.dim() != 2 or a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
            raise _C.KernelError("gemm: 2-D bf16 operands only")
        if a.stride(1) != 1 or b.stride(1) != 1:
            raise _C.KernelError("gemm: operands need contiguous rows")
    a0, b0 = segs[0]
    M = a0.shape[1] if a_kmaj else a0.shape[0]
    N = b0.shape[1] if b_kmaj else b0.shape[0]
    Ks = []
    for a, b in segs:
        Ka, Ma = (a.shape[0], a.shape[1]) if a_kmaj else (a.shape[1], a.shape[0])
        Kb, Nb = (b.shape[0], b.shape[1]) if b_kmaj else (b.shape[1], b.shape[0])
        if Ka != Kb or Ma != M or Nb != N:
            raise _C.KernelError(f"gemm: segment shapes disagree: a {tuple(a.shape)} b {tuple(b.shape)}")
        Ks.append(Ka)
    out = _out_or_new("gemm", out, accumulate, M, N, a0.device)
    n = len(segs)
    f32 = out.dtype == torch.float32
    wgrad_mode = a_kmaj and b_kmaj and n == 1 and bias is None and out_t is None
    if f32:
        # weight gradient straight into an fp32 buffer (the data-parallel engine's reduce-scatter input)
        if not wgrad_mode:
            raise _C.KernelError("gemm: fp32 output exists for the single-segment weight-gradient mode only")
        if out.stride(1) != 1 or tuple(out.shape) != (M, N) or not a0.is_cuda:
            raise _C.KernelError("gemm: bad fp32 `out`")
    else:
        if out.stride(1) != 1 or tuple(out.shape) != (M, N) or out.dtype != torch.bfloat16:
            raise _C.KernelError("gemm: bad `out`")
        if bias is not None:
            bias = _c(bias).to(torch.bfloat16)
        if not a0.is_cuda:
            raise _C.KernelError("touchnet_amd kernels need device (HIP) tensors; got a CPU tensor")
        if addend is not None:
            if (n != 1 or accumulate or out_t is not None or bias_grad is not None or addend.dtype != torch.bfloat16
                    or tuple(addend.shape) != (M, N) or addend.stride(1) != 1 or addend.data_ptr() == out.data_ptr()):
                raise _C.KernelError("gemm: addend needs one segment, a bf16 [M, N] matrix with contiguous rows that is not `out`")
            _C.check(_C.lib().tn_gemm_bf16_addend(_p(a0), _p(b0), a0.stride(0), b0.stride(0), Ks[0], int(a_kmaj), int(b_kmaj),
                                                  _p(out), _p(bias), _p(addend), addend.stride(0), M, N, out.stride(0), _cur()),
                     "tn_gemm_bf16_addend")
            return out
    lib = _C.lib()
    if f32 or bias_grad is not None:
        # the weight gradient's own entry points: fp32 or bf16 output, with or without the bias gradient
        if not wgrad_mode:
            raise _C.KernelError("gemm: bias_grad exists for the single-segment weight-gradient mode only")
        split = split_k(M, N, Ks[0], True, True) if SPLIT_K else 1
        ws, ws_bytes = _splitk_workspace(M, N, split, bias_grad is not None, a0.device)
        if bias_grad is None:
            _C.check(lib.tn_gemm_bf16_wgrad_f32(_p(a0), _p(b0), a0.stride(0), b0.stride(0), Ks[0], _p(out), M, N, out.stride(0),
                                                int(accumulate), split, _p(ws), ws_bytes, _cur()), "tn_gemm_bf16_wgrad_f32")
        else:
            _check_bias_grad(bias_grad, M, a0)
            _C.check(lib.tn_gemm_bf16_wgrad_bias(_p(a0), _p(b0), a0.stride(0), b0.stride(0), Ks[0], _p(out), _p(bias_grad), M, N,
                                                 out.stride(0), int(accumulate), int(f32), split, _p(ws), ws_bytes, _cur()),
                     "tn_gemm_bf16_wgrad_bias")
        return out
    split = split_k(M, N, Ks[0], a_kmaj, b_kmaj) if n == 1 and out_t is None and SPLIT_K else 1
    if split > 1:
        ws, ws_bytes = _splitk_workspace(M, N, split, False, a0.device)
        _C.check(lib.tn_gemm_bf16_splitk(_p(a0), _p(b0), a0.stride(0), b0.stride(0), Ks[0], int(a_kmaj), int(b_kmaj), _p(out),
                                         _p(bias), M, N, out.stride(0), int(accumulate), split, 0, _p(ws), ws_bytes, _cur()),
                 "tn_gemm_bf16_splitk")
        return out
    _C.check(lib.tn_gemm_bf16(*_operand_arrays(segs), _carr(ctypes.c_int, Ks), n, int(a_kmaj), int(b_kmaj), _p(out), _p(out_t),
                              _p(bias), M, N, out.stride(0), out_t.stride(0) if out_t is not None else 0, int(accumulate),
                              _cur()), "tn_gemm_bf16")
    return out


def _splitk_workspace(M, N, split, with_bias_grad, device):
    """``(workspace, its size in bytes)`` of a product cut into ``split`` parts — ``(None, 0)`` when it is not split; the
    library owns the layout (tn_gemm_splitk_workspace_bytes)."""
    if split <= 1:
        return None, 0
    need = int(_C.lib().tn_gemm_splitk_workspace_bytes(M, N, split, int(with_bias_grad), 0))
    return torch.empty(need // 4, dtype=torch.float32, device=device), need


def _carr(ctype, values):
    return (ctype * len(values))(*values)


def _operand_arrays(pairs):
    """The ctypes arrays ``A, B, lda, ldb`` of tn_gemm_bf16 / tn_gemm_bf16_grouped: base addresses and row pitches."""
    return (_carr(ctypes.c_void_p, [a.data_ptr() for a, _ in pairs]), _carr(ctypes.c_void_p, [b.data_ptr() for _, b in pairs]),
            _carr(ctypes.c_longlong, [a.stride(0) for a, _ in pairs]), _carr(ctypes.c_longlong, [b.stride(0) for _, b in pairs]))


def _check_bias_grad(bias_grad, M, like):
    if (bias_grad.dtype != torch.bfloat16 or bias_grad.dim() != 1 or bias_grad.numel() != M or not bias_grad.is_contiguous()
            or bias_grad.device != like.device):
        raise _C.KernelError("gemm: bias_grad must be a contiguous bf16 [M] device vector")


def _check_grouped(name, pairs, outs, accumulate):
    """The operand and output checks of `gemm_grouped_wgrad` and `gemm_grouped_table_wgrad` (``name``: the caller, for the
    message); returns ``outs`` or, by default, new bf16 tensors."""
    for a, b in pairs:
        if (a.dim() != 2 or b.dim() != 2 or a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or a.stride(1) != 1
                or b.stride(1) != 1 or a.shape[0] != b.shape[0] or not a.is_cuda):
            raise _C.KernelError(f"{name}: pairs of 2-D bf16 device matrices [K, M] / [K, N] with contiguous rows")
    if outs is None:
        outs = [_out_or_new(name, None, accumulate, a.shape[1], b.shape[1], a.device) for a, b in pairs]
    for o, (a, b) in zip(outs, pairs):
        if (o.dtype != outs[0].dtype or o.dtype not in (torch.float32, torch.bfloat16) or o.stride(1) != 1
                or tuple(o.shape) != (a.shape[1], b.shape[1])):
            raise _C.KernelError(f"{name}: bad `outs`")
    return outs


def gemm_grouped_wgrad(pairs, outs=None, accumulate: bool = False):
    """``out_g[M_g, N_g] (+)= a_g^T @ b_g`` for 1..3 independent pairs of bf16 device matrices stored [K_g, M_g] / [K_g, N_g]
    (contraction-major: the weight gradients dY^T x of linear layers) as ONE persistent launch of the hand-written kernel
    (tn_gemm_bf16_grouped): the tile lists of the products are concatenated, so that only the remainder of the WHOLE list
    — not of every product — is left for a partial last round, and that remainder runs split-K.  ``outs``: bf16 or fp32
    [M_g, N_g] matrices (all of one dtype) to write (or, ``accumulate``, to add to); default new bf16 tensors."""
    n = len(pairs)
    if not 1 <= n <= 3:
        raise _C.KernelError("gemm_grouped_wgrad: 1..3 products")
    outs = _check_grouped("gemm_grouped_wgrad", pairs, outs, accumulate)
    f32 = outs[0].dtype == torch.float32
    Ms = _carr(ctypes.c_int, [a.shape[1] for a, _ in pairs])
    Ns = _carr(ctypes.c_int, [b.shape[1] for _, b in pairs])
    Ks = _carr(ctypes.c_int, [a.shape[0] for a, _ in pairs])
    need = int(_C.lib().tn_gemm_grouped_workspace_bytes(Ms, Ns, Ks, n))
    ws = torch.empty(need // 4, dtype=torch.float32, device=outs[0].device) if need > 0 else None
    Ap, Bp, la, lb = _operand_arrays(pairs)
    _C.check(_C.lib().tn_gemm_bf16_grouped(Ap, Bp, la, lb, Ks, _carr(ctypes.c_void_p, [o.data_ptr() for o in outs]),
                                           _carr(ctypes.c_longlong, [o.stride(0) for o in outs]), Ms, Ns, n, 1, 1,
                                           int(accumulate), int(f32), _p(ws), need, _cur()), "tn_gemm_bf16_grouped")
    return list(outs)


GROUPED_TABLE_MAX = 1024          # products per tn_gemm_bf16_grouped_table launch


def gemm_grouped_table_wgrad(pairs, outs=None, accumulate: bool = False, bias_grads=None):
    """``out_g[M_g, N_g] (+)= a_g^T @ b_g`` for ANY number (1..1024) of independent pairs of bf16 device matrices stored
    [K_g, M_g] / [K_g, N_g] as ONE persistent launch over the concatenation of their tile lists (tn_gemm_bf16_grouped_table):
    whole tiles only, every output has the bits of the unsplit single-product launch.  ``outs``: bf16 or fp32 matrices (all
    of one dtype; they may have a row pitch) to write or, ``accumulate``, to add to; default new bf16 tensors.
    ``bias_grads``: per product None or a contiguous bf16 [M_g] vector that receives the column sums of ``a_g``."""
    n = len(pairs)
    if not 1 <= n <= GROUPED_TABLE_MAX:
        raise _C.KernelError(f"gemm_grouped_table_wgrad: 1..{GROUPED_TABLE_MAX} products")
    outs = _check_grouped("gemm_grouped_table_wgrad", pairs, outs, accumulate)
    if bias_grads is None:
        bias_grads = [None] * n
    for bg, (a, _) in zip(bias_grads, pairs):
        if bg is not None:
            _check_bias_grad(bg, a.shape[1], a)
    lib = _C.lib()
    need = int(lib.tn_gemm_grouped_table_bytes(n))
    table = torch.empty(need, dtype=torch.uint8, device=outs[0].device)       # (stream-ordered: free to go after the call)
    Ap, Bp, la, lb = _operand_arrays(pairs)
    _C.check(lib.tn_gemm_bf16_grouped_table(
        Ap, Bp, la, lb, _carr(ctypes.c_int, [a.shape[0] for a, _ in pairs]),
        _carr(ctypes.c_void_p, [o.data_ptr() for o in outs]), _carr(ctypes.c_longlong, [o.stride(0) for o in outs]),
        _carr(ctypes.c_int, [a.shape[1] for a, _ in pairs]), _carr(ctypes.c_int, [b.shape[1] for _, b in pairs]),
        _carr(ctypes.c_void_p, [bg.data_ptr() if bg is not None else None for bg in bias_grads]), n, int(accumulate),
        int(outs[0].dtype == torch.float32), _p(table), need, _cur()), "tn_gemm_bf16_grouped_table")
    return list(outs)


def gemm_swiglu_fwd(x2: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor):
    """``(gate, up, act)`` with gate = x2 @ w_gate^T, up = x2 @ w_up^T, act = silu(gate) * up from ONE launch of the
    hand-written kernel whose epilogue applies the SwiGLU (tn_gemm_bf16_swiglu_fwd; bit-identical to the two products
    followed by `swiglu`)."""
    M, K = x2.shape
    I = w_gate.shape[0]
    if not _bf16_rows(x2, w_gate, w_up) or w_up.shape != w_gate.shape or w_gate.shape[1] != K or w_gate.stride(0) != w_up.stride(0):
        raise _C.KernelError("gemm_swiglu_fwd: bf16 device matrices x [M, K], w_gate / w_up [I, K] of one row pitch")
    gate, up, act = (torch.empty(M, I, dtype=torch.bfloat16, device=x2.device) for _ in range(3))
    _C.check(_C.lib().tn_gemm_bf16_swiglu_fwd(_p(x2), _p(w_gate), _p(w_up), _p(gate), _p(up), _p(act), M, I, K, x2.stride(0),
                                              w_gate.stride(0), I, _cur()), "tn_gemm_bf16_swiglu_fwd")
    return gate, up, act


def gemm_gelu_fwd(x2: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]):
    """``(pre, act)`` with pre = x2 @ w^T + bias and act = gelu(pre) (exact erf) from ONE launch (tn_gemm_bf16_gelu_fwd;
    bit-identical to the product followed by `gelu`)."""
    M, K = x2.shape
    N = w.shape[0]
    if not _bf16_rows(x2, w) or w.shape[1] != K or (bias is not None and (bias.dtype != torch.bfloat16 or bias.numel() != N)):
        raise _C.KernelError("gemm_gelu_fwd: bf16 device matrices x [M, K], w [N, K], bias [N]")
    pre, act = (torch.empty(M, N, dtype=torch.bfloat16, device=x2.device) for _ in range(2))
    _C.check(_C.lib().tn_gemm_bf16_gelu_fwd(_p(x2), _p(w), _p(_c(bias)) if bias is not None else None, _p(pre), _p(act), M, N,
                                            K, x2.stride(0), w.stride(0), N, _cur()), "tn_gemm_bf16_gelu_fwd")
    return pre, act


def gemm_gelu_bwd(dy2: torch.Tensor, w2: torch.Tensor, pre: torch.Tensor):
    """``d(pre) = (dy2 @ w2) o gelu'(pre)`` (w2 [H, I] read contraction-major): one launch, d(act) never reaches HBM
    (tn_gemm_bf16_gelu_bwd; bit-identical to the product followed by `gelu_bwd`)."""
    M, H = dy2.shape
    I = w2.shape[1]
    if not _bf16_rows(dy2, w2, pre) or w2.shape[0] != H or tuple(pre.shape) != (M, I) or pre.stride(0) != I:
        raise _C.KernelError("gemm_gelu_bwd: bf16 device matrices dy [M, H], w2 [H, I], dense pre [M, I]")
    dpre = torch.empty(M, I, dtype=torch.bfloat16, device=dy2.device)
    _C.check(_C.lib().tn_gemm_bf16_gelu_bwd(_p(dy2), _p(w2), _p(pre), _p(dpre), M, I, H, dy2.stride(0), w2.stride(0), I,
                                            _cur()), "tn_gemm_bf16_gelu_bwd")
    return dpre


def gemm_swiglu_bwd(dy2: torch.Tensor, w_down: torch.Tensor, gate: torch.Tensor, up: torch.Tensor):
    """``(d_gate, d_up)`` of act = silu(gate) * up for d(act) = dy2 @ w_down (w_down [H, I] read contraction-major): one
    launch, d(act) never reaches HBM (tn_gemm_bf16_swiglu_bwd; bit-identical to the product followed by `swiglu_bwd`)."""
    M, H = dy2.shape
    I = w_down.shape[1]
    if (not _bf16_rows(dy2, w_down, gate, up) or w_down.shape[0] != H or tuple(gate.shape) != (M, I) or gate.shape != up.shape
            or gate.stride(0) != up.stride(0)):
        raise _C.KernelError("gemm_swiglu_bwd: bf16 device matrices dy [M, H], w_down [H, I], gate / up [M, I]")
    dgate = torch.empty(M, I, dtype=torch.bfloat16, device=dy2.device)
    dup = torch.empty(M, I, dtype=torch.bfloat16, device=dy2.device)
    if gate.stride(0) != I:
        raise _C.KernelError("gemm_swiglu_bwd: gate / up must be dense [M, I]")
    _C.check(_C.lib().tn_gemm_bf16_swiglu_bwd(_p(dy2), _p(w_down), _p(gate), _p(up), _p(dgate), _p(dup), M, I, H,
                                              dy2.stride(0), w_down.stride(0), I, _cur()), "tn_gemm_bf16_swiglu_bwd")
    return dgate, dup


def gemm_rope(x2: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor,
              head_dim: int) -> torch.Tensor:
    """``rope(x2 @ weight^T + bias)`` [M, heads * head_dim] from ONE launch (tn_gemm_bf16_rope): the rotary embedding of a
    q / k projection in the GEMM's epilogue, bit-identical to the projection followed by `apply_rope`.  cos / sin: the
    bf16 [M, head_dim / 2] tables of `rope_tables`."""
    M, K = x2.shape
    N = weight.shape[0]
    if (not _bf16_rows(x2, weight) or weight.shape[1] != K or cos.dtype != torch.bfloat16 or sin.dtype != torch.bfloat16
            or tuple(cos.shape) != (M, head_dim // 2) or tuple(sin.shape) != (M, head_dim // 2)
            or not cos.is_contiguous() or not sin.is_contiguous()):
        raise _C.KernelError("gemm_rope: bf16 x [M, K], weight [N, K], cos / sin [M, head_dim / 2]")
    if bias is not None:
        bias = _c(bias).to(torch.bfloat16)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=x2.device)
    _C.check(_C.lib().tn_gemm_bf16_rope(_p(x2), _p(weight), _p(bias), _p(cos), _p(sin), _p(out), M, N, K, x2.stride(0),
                                        weight.stride(0), N, int(head_dim), _cur()), "tn_gemm_bf16_rope")
    return out


def rope_epilogue_ok(M: int, N: int, K: int, head_dim: int) -> bool:
    """shapes tn_gemm_bf16_rope takes (and the hand-written kernel is the configured GEMM for)"""
    return (ROPE_EPILOGUE and _own(M, N, (K,)) and _whole_unsplit(M, N, K)
            and ((head_dim == 128 and N % 256 == 0) or (head_dim == 64 and N % 64 == 0)))


def _rope_epilogue_own(x2, w, rope) -> bool:
    """`gemm_rope` runs ``rope(x2 w^T (+ b))`` for ``rope = (cos, sin, head_dim, ..)`` of `linear_group`"""
    (M, K), cos, D = x2.shape, rope[0], rope[2]
    return (rope_epilogue_ok(M, w.shape[0], K, D) and _bf16_rows(x2, w) and cos.dtype == torch.bfloat16
            and tuple(cos.shape) == (M, D // 2))


def _rotated(y2, rope):
    """the rotary embedding ``rope = (cos, sin, head_dim, ..)`` of y2 [M, heads * head_dim], behind its product"""
    cos, sin, D = rope[:3]
    M = y2.shape[0]
    y4 = y2.view(1, M, -1, D)
    return L.rope_apply(y4, y4.new_empty(1, M, 0, D), cos, sin, False)[0].view(M, -1)


def _whole_unsplit(M: int, N: int, K: int) -> bool:
    """x W^T runs as whole 64-deep stages in ONE pass over the contraction (a split-K product sums in another order): the
    product a fused epilogue stands in for.  (The SwiGLU and GELU epilogues never asked for the unsplit half: DESIGN.md.)"""
    return K % 64 == 0 and (not SPLIT_K or split_k(M, N, K, False, False) == 1)


# Flags of the fusions: read at call time, set by the tests alone — the off side is the unfused reference of each.
ROPE_EPILOGUE = True          # rotary embedding in the q / k projection's epilogue (off: rotated behind the product)
MLP_EPILOGUE = True           # SwiGLU inside the gate/up and down-dgrad epilogues
GROUPED_WGRAD = True          # the MLP's three weight gradients as one grouped launch
SPLIT_K = True                # few-tile products cut along their contraction (`split_k`)
_NUM_CU = 256


def split_k(M: int, N: int, K: int, a_kmaj: bool, b_kmaj: bool) -> int:
    """Parts the contraction of a single-segment product is cut into (1 = no split): outputs of fewer 256 x 256 tiles than
    half the CUs, at least 8 stages (512 deep) per part, tiles x parts <= CUs; with a contraction-contiguous operand the
    number of 64-deep stages has to divide evenly."""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    stages = (K + 63) // 64
    if tiles * 2 > _NUM_CU or stages < 16:
        return 1
    s = min(_NUM_CU // tiles, stages // 8)
    if not (a_kmaj and b_kmaj):
        while s > 1 and stages % s:
            s -= 1
    return max(s, 1)


def gemm_supported(M: int, N: int, Ks, a_kmaj: bool = False, b_kmaj: bool = False) -> bool:
    """Shapes tn_gemm_bf16 takes (two contraction-major operands: any depth, the tail is zero-filled)."""
    k_ok = all(k > 0 and (k % 64 == 0 or (a_kmaj and b_kmaj)) for k in Ks)
    return k_ok and N % 8 == 0 and M > 0 and (not a_kmaj or M % 8 == 0)


# Which GEMM runs the products of the linear layers below:
#   "own"  the hand-written MFMA kernel of csrc/gemm.hip in its three operand modes — forward x W^T, input gradient
#          dY W (W contraction-major) and weight gradient dY^T x (both contraction-major): every product reads nn.Linear's
#          own tensors, no transposed copy of W, dY or x is made, and the input gradient of a group (q/k/v, gate/up) is ONE
#          multi-segment launch.  Shapes the kernel does not take (K % 64, fewer output tiles than half the CUs) go to the
#          library.
#   "lib"  hipBLASLt through torch, every product brought into the forward layout by transposed copies
#          (tn_transpose_bf16).  Kept for A/B runs: on one box the Qwen2-Audio-7B step takes 742 ms
#          on "own" and 717 ms on "lib" (profiles/r03f_*): the library's kernel runs 12 % faster (same cycles within
#          4 %, higher clock: 2/3 of our LDS read traffic), "own" saves the transposes and their extra stores.
# TN_LINEAR_GEMM / `bench.py --linear-gemm` select; tests/test_kernels_gpu.py holds the two to each other.
# WHO ANSWERS: per product kind one predicate, asked with the tensors (the integer rule `_own` + `_bf16_rows`), and one
# function that runs the product on the kernel or in the library's form — forward `_fwd_own` / `_mm_tn`, input gradient
# `_dgrad_own` / `_dgrad`, weight gradient `_wgrad_own` / `_wgrads` and `_wgrad_unowned` (DESIGN.md §5.4 has the table).
LINEAR_GEMM = os.environ.get("TN_LINEAR_GEMM", "own")
_OWN_MIN_TILES = 96          # below this many 256 x 256 output tiles most CUs would idle: the library's split-K wins


def _own_configured() -> bool:
    return LINEAR_GEMM == "own"


def _own(M: int, N: int, Ks, a_kmaj: bool = False, b_kmaj: bool = False) -> bool:
    """The hand-written kernel takes this product (and is the configured choice)."""
    if not (_own_configured() and gemm_supported(M, N, Ks, a_kmaj, b_kmaj)):
        return False
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if tiles >= _OWN_MIN_TILES:
        return True
    # few tiles: taken when the contraction can be split over enough units to fill the chip
    return SPLIT_K and len(Ks) == 1 and tiles * split_k(M, N, Ks[0], a_kmaj, b_kmaj) >= _OWN_MIN_TILES


def _bf16_rows(*ts, meta_ok: bool = False) -> bool:
    """Operands the hand-written kernel takes: bf16 device matrices with contiguous rows, 16-byte aligned.  ``meta_ok``:
    meta tensors pass too (the bookkeeping of `DeferredWgrad` runs without a device)."""
    return all((t.is_cuda or (meta_ok and t.is_meta)) and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1
               and t.stride(0) % 8 == 0 and (t.is_meta or t.data_ptr() % 16 == 0) for t in ts)


def _transposable(*ts) -> bool:
    """`transpose_2d`, which brings the library forms' operands into the forward layout, applies: bf16, extents % 8 == 0"""
    return all(t.dtype == torch.bfloat16 and (t.is_cuda or t.is_meta) and t.shape[0] % 8 == 0 and t.shape[1] % 8 == 0
               for t in ts)


def _fwd_own(a, b, bias=None) -> bool:
    """The hand-written kernel runs the forward product a [M, K] b [N, K]^T (+ bias)."""
    return (_own(a.shape[0], b.shape[0], (a.shape[1],)) and _bf16_rows(a, b)
            and (bias is None or bias.dtype == torch.bfloat16))


def _mm_tn(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           accumulate: bool = False) -> torch.Tensor:
    """``a @ b.T (+ bias)`` (``out += ...`` if accumulate) for contraction-contiguous a [M, K], b [N, K]."""
    if _fwd_own(a, b, bias):
        return gemm([(a, b)], bias=bias, out=out, accumulate=accumulate)
    if accumulate:
        return out.addmm_(a, b.t())
    if out is not None:
        return torch.mm(a, b.t(), out=out) if bias is None else torch.addmm(bias, a, b.t(), out=out)
    return torch.nn.functional.linear(a, b, bias)


def _dgrad_own(dys, ws, out=None) -> bool:
    """The hand-written kernel runs the input gradient sum_i dY_i [M, N_i] W_i [N_i, K] (into ``out``, if given)."""
    return (_own(dys[0].shape[0], ws[0].shape[1], [w.shape[0] for w in ws])
            and _bf16_rows(*dys, *ws, *(() if out is None else (out,))))


def _dgrad(dys, ws, out: Optional[torch.Tensor] = None, dgrad_tn: bool = True) -> torch.Tensor:
    """``sum_i dY_i W_i`` [M, K] (written to ``out``, if given).  The hand-written kernel reads W_i [N_i, K] contraction-major,
    one launch for up to three layers.  The library form sums in the GEMM epilogue (addmm, beta = 1), ``dgrad_tn`` on W_i^T
    in the forward layout where the transposes apply, else on W_i as stored."""
    if _dgrad_own(dys, ws, out):
        for i in range(0, len(ws), 3):
            out = gemm(list(zip(dys[i:i + 3], ws[i:i + 3])), b_kmaj=True, out=out, accumulate=i > 0)
        return out
    if dgrad_tn and _transposable(*dys, *ws):
        wts = [transpose_2d(w) for w in ws]                                    # W^T [K, N]: forward layout
        out = _mm_tn(dys[0], wts[0], out=out)
        for d, wt in zip(dys[1:], wts[1:]):
            _mm_tn(d, wt, out=out, accumulate=True)
        return out
    out = torch.mm(dys[0], ws[0]) if out is None else torch.mm(dys[0], ws[0], out=out)
    for d, w in zip(dys[1:], ws[1:]):
        out.addmm_(d, w)
    return out


BIAS_IN_WGRAD = True          # bias gradients dY.sum(0) from the weight-gradient launch itself (EPI_BIASG, csrc/gemm.hip)


def _wgrad_own(dy, x2, queued: bool = False) -> bool:
    """The hand-written kernel runs the weight gradient dy [M, N]^T x2 [M, K] (both operands contraction-major: the
    contraction runs over tokens).  ``queued``: as one product of the deferred queue's table launch, which fills the chip
    with the tiles of many layers — the tile-count rule is not asked, and meta tensors pass (the queue's bookkeeping runs
    without a device)."""
    shape = (dy.shape[1], x2.shape[1], (dy.shape[0],), True, True)
    return (dy.shape[0] == x2.shape[0] and _bf16_rows(dy, x2, meta_ok=queued)
            and (_own_configured() and gemm_supported(*shape) if queued else _own(*shape)))


# Weight-gradient GEMMs on a side stream.  Nothing in the backward consumes a weight gradient, so these products can
# run beside the input-gradient chain: with one workgroup per tile (TN_GEMM_PERSIST=0) the tiles of two launches interleave
# and the last, partly filled round of one kernel (the MLP weight gradients are 688 tiles for 256 CUs: 2.69 rounds) is
# filled by the other's.  `enable_wgrad_stream()` switches it on (bench.py --wgrad-stream / TN_WGRAD_STREAM=1);
# `sync_wgrad_stream()` makes the current stream wait for everything issued there (before the optimizer, before a
# reduce-scatter).  Inputs are `record_stream`ed so the caching allocator does not recycle them under the side stream.
WGRAD_STREAM = None
WGRAD_MAIN = None             # the stream the backward itself runs on (noted by `_beside`)
# A sharding engine (utils/zero_dp.py, FSDP2) reads a returned weight gradient on the backward's own stream right away
# (cast-copy into the reduce-scatter input); it sets this and `_beside` then lets that stream wait for the product.
WGRAD_RETURNS_NEED_SYNC = False


def enable_wgrad_stream(on: bool = True) -> None:
    global WGRAD_STREAM
    # (a stream of another priority than the main one: streams of equal priority may share a hardware queue, and kernels
    #  of one queue never overlap — profiles/r05q_comm_stream_hw_queue_probe.log)
    WGRAD_STREAM = torch.cuda.Stream(priority=int(os.environ.get("TN_WGRAD_STREAM_PRIORITY", "-1"))) if on else None


def wgrad_streams():
    """Streams that may hold unfinished writes of gradients during a backward: the current one, and with the side stream
    on also that one and the backward's own."""
    out = [torch.cuda.current_stream()]
    for st in (WGRAD_STREAM, WGRAD_MAIN if WGRAD_STREAM is not None else None):
        if st is not None and all(st != o for o in out):
            out.append(st)
    return out


def sync_wgrad_stream() -> None:
    if WGRAD_STREAM is not None:
        torch.cuda.current_stream().wait_stream(WGRAD_STREAM)


def _beside(inputs, fn, written=()):
    """run `fn` (a weight-gradient product over `inputs`) on the side stream, if there is one.

    `written`: tensors ALLOCATED ON THE MAIN STREAM that `fn` fills on the side stream and that the caller hands to
    autograd next (the bias gradient that rides on a weight-gradient launch): the main stream waits for the side stream
    before it returns, and the allocator is told about the second stream.  A tensor (or list / tuple of tensors) RETURNED
    by `fn` was allocated on the side stream: it is recorded on the main stream, and — when the consumer reads it on the
    main stream right away (`WGRAD_RETURNS_NEED_SYNC`: FSDP2 and every engine without gradient sinks) — waited for."""
    side = WGRAD_STREAM
    if side is None:
        return fn()
    global WGRAD_MAIN
    main = torch.cuda.current_stream()
    WGRAD_MAIN = main
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    for t in inputs:
        t.record_stream(side)
    wait = False
    for t in written:
        if t is not None:
            t.record_stream(side)
            wait = True                           # (read by autograd / the engine's hook on the main stream)
    outs = out if isinstance(out, (list, tuple)) else (out,)
    for t in outs:
        if isinstance(t, torch.Tensor):
            t.record_stream(main)
            wait = wait or WGRAD_RETURNS_NEED_SYNC   # (record_stream only protects the allocator, not the reader)
    if wait:
        main.wait_stream(side)
    return out


# Gradient sinks: a data-parallel engine (utils/zero_dp.py) registers, per weight (by id), an object with
#   take(w) -> (view [N, K] in its reduce-scatter input — fp32 or bf16 —, accumulate?)   and   done(w)
# and the weight-gradient GEMM of that weight writes straight into the view instead of returning a tensor that would have
# to be cast-copied there (autograd then sees no gradient for the weight: the engine counts the arrival itself).  Who asks
# them: `_route_wgrad` (one product) and `_wgrad_group` (the MLP's three), through `_sink_of`.
GRAD_SINKS = {}          # id(weight) -> weakref to the engine (a dead engine's entries are ignored)


def _live(table, w):
    """the live object `table` (GRAD_SINKS, WGRAD_QUEUES) holds for ``w``, or None"""
    ref = table.get(id(w))
    return ref() if ref is not None else None


def _sink_of(w):
    """the live gradient sink that owns ``w``, or None"""
    sink = _live(GRAD_SINKS, w)
    return sink if sink is not None and sink.owns(w) else None


# Deferred weight gradients (the audio tower's linear layers).  Nothing reads a weight gradient before the gradient norm,
# so a product dY^T x does not have to run where the backward forms dY.  Per tower layer the six products (q, k, v, out,
# fc1, fc2 at 1280 / 5120 wide) are 4 x 25 + 2 x 100 = 300 output tiles of 256 x 256 — 1.17 rounds on 256 CUs, which no
# per-layer launch fills: whole tiles pay two rounds for 1.17, so `split_k` cut the contraction (fp32 workspace, a reduce
# kernel, 56 idle CUs at 100 tiles x 2).  A queue takes ``(weight, dY, x)`` instead, and ONE table-driven launch
# (gemm_grouped_table_wgrad) runs the products of many layers as a single unsplit tile list.  It follows the gradient-sink
# protocol above: autograd sees no gradient for a queued weight (nor for its bias), the queue writes ``.grad`` itself.
#   flush threshold  11 layers = 3300 tiles = 12.89 rounds -> 13 rounds at 99.2 % occupancy; the 32 layers of the tower flush
#                    as 11 + 11 + 10 (3000 tiles = 11.72 -> 12 rounds): 38 rounds in all, the same as ONE flush of 9600 tiles
#                    (37.5 -> 38), at a third of the memory
#   memory           a queued layer keeps its dY (691 MB at 30000 frames) and x (538 MB, saved activations that would have
#                    been freed by then) alive: at most 11 x 1.23 GB = 13.5 GB, while the tower's backward runs — after the
#                    decoder's activations are freed, so the step's peak (end of the decoder's forward) does not move
# Kept on the per-layer path: weights a data-parallel engine's sink owns, the side stream (`enable_wgrad_stream`), operands
# the kernel does not take, an existing ``.grad`` that is not a bf16 matrix; tensor / context parallelism and activation
# checkpointing never install a queue (bin/train.py).
DEFERRED_WGRAD = True         # (False: the per-layer path everywhere — the tests' reference)
DEFERRED_WGRAD_FLUSH_LAYERS = 11
WGRAD_QUEUES = {}        # id(weight) -> weakref to its queue (a dead queue's entries are ignored)


def _queue_of(w):
    """the live queue registered for ``w``, or None (`DeferredWgrad.push` checks that the weight is still the one it owns)"""
    return _live(WGRAD_QUEUES, w)


class DeferredWgrad:
    """The queue.  ``layers``: per layer a list of ``(weight, bias or None)`` parameters, the only ones it takes.  `push`
    during the backward, `flush` behind it (and by itself once ``flush_layers`` layers are waiting and another one
    arrives).  ``launch``: `gemm_grouped_table_wgrad`, replaceable (tests of the bookkeeping)."""

    def __init__(self, layers, flush_layers: int = DEFERRED_WGRAD_FLUSH_LAYERS):
        if flush_layers < 1:
            raise ValueError("DeferredWgrad: flush_layers >= 1")
        self.flush_layers = flush_layers
        self.launch = gemm_grouped_table_wgrad
        self.enabled = True              # False: `push` takes nothing (an owner that flushes only behind its own backward)
        self._owned = {}                 # id(weight) -> (weight, bias, layer)
        self._items = []                 # (weight, dy, x2, bias or None, stream) in queue order
        self._waiting = set()            # ids of the queued weights
        self._layers = set()             # layers with a queued weight
        self.flushes = 0
        for li, layer in enumerate(layers):
            for w, b in layer:
                self._owned[id(w)] = (w, b, li)
                WGRAD_QUEUES[id(w)] = weakref.ref(self)

    def __len__(self):
        return len(self._items)

    def close(self):
        """give the weights back to the per-layer path (the queue must be empty)"""
        if self._items:
            raise _C.KernelError("DeferredWgrad.close: the queue is not empty")
        for k in self._owned:
            ref = WGRAD_QUEUES.get(k)
            if ref is not None and ref() is self:
                del WGRAD_QUEUES[k]
        self._owned = {}

    def push(self, w, dy, x2, with_bias: bool) -> bool:
        """Take ``dW = dy^T x2`` (and, ``with_bias``, the bias gradient ``dy.sum(0)``) of an owned weight.  False: not this
        queue's business — the caller forms the gradient itself."""
        own = self._owned.get(id(w))
        if not self.enabled or own is None or own[0] is not w:
            return False
        _, bias, layer = own
        if id(w) in self._waiting:
            raise _C.KernelError("DeferredWgrad: a weight was queued twice without a flush in between "
                                 "(two backward passes through one layer: flush between them)")
        ok = (_wgrad_own(dy, x2, queued=True) and w.dtype == torch.bfloat16 and tuple(w.shape) == (dy.shape[1], x2.shape[1])
              and (not with_bias or (bias is not None and bias.dtype == torch.bfloat16))
              and (w.grad is None or (w.grad.dtype == torch.bfloat16 and w.grad.is_contiguous()
                                      and (w.grad.is_meta or w.grad.data_ptr() % 16 == 0))))
        if not ok:
            return False
        if layer not in self._layers and len(self._layers) >= self.flush_layers:
            self.flush()
        self._items.append((w, dy, x2, bias if with_bias else None, torch.cuda.current_stream() if dy.is_cuda else None))
        self._waiting.add(id(w))
        self._layers.add(layer)
        return True

    def flush(self) -> None:
        """Run everything queued, in queue order, and write the ``.grad`` of the weights and biases (added to an existing
        one).  One launch — two when some of the weights already have a gradient and others do not."""
        items, self._items = self._items, []
        self._waiting.clear()
        self._layers.clear()
        if not items:
            return
        self.flushes += 1
        cur = torch.cuda.current_stream() if items[0][1].is_cuda else None
        for w, dy, x2, _, st in items:
            if st is not None and st != cur:       # formed on another stream than the one the products run on
                cur.wait_stream(st)
                dy.record_stream(cur)
                x2.record_stream(cur)
        parts = {acc: [it for it in items if (it[0].grad is not None) == acc] for acc in (False, True)}
        for acc, part in parts.items():
            for i in range(0, len(part), GROUPED_TABLE_MAX):
                chunk = part[i:i + GROUPED_TABLE_MAX]
                outs = [w.grad if acc else torch.empty(w.shape, dtype=torch.bfloat16, device=dy.device)
                        for w, dy, _, _, _ in chunk]
                bgs = [torch.empty(dy.shape[1], dtype=torch.bfloat16, device=dy.device) if b is not None else None
                       for _, dy, _, b, _ in chunk]
                self.launch([(dy, x2) for _, dy, x2, _, _ in chunk], outs=outs, accumulate=acc, bias_grads=bgs)
                for (w, _, _, b, _), o, bg in zip(chunk, outs, bgs):
                    if not acc:
                        w.grad = o
                    if b is not None:
                        if b.grad is None:
                            b.grad = bg
                        else:
                            b.grad.add_(bg)


def _queue_wgrad(w, dy, x2, with_bias: bool) -> bool:
    """Step 1 of `_route_wgrad`: hand ``dW = dy^T x2`` to the deferred-weight-gradient queue that owns ``w``, if there is one
    and nothing else claims the product (a data-parallel engine's sink, the side stream)."""
    if not DEFERRED_WGRAD or WGRAD_STREAM is not None:
        return False
    q = _queue_of(w)
    return q is not None and _sink_of(w) is None and q.push(w, dy, x2, with_bias)


# WHERE A WEIGHT GRADIENT GOES.  `_route_wgrad` is the one owner of that decision for a single product dW = dY^T x of a
# linear layer: `_LinearGroup`, `_GeluMLP` and `_SwiGLUMLP` (and the per-product fallback of `_wgrad_group`) ask it, through
# `_wgrads`, and nothing else.  The rule, first match wins:
#   1. queue       DEFERRED_WGRAD is on, no side stream is enabled, a live queue owns the weight, no live sink owns it, and
#                  `DeferredWgrad.push` accepts the product (`_queue_wgrad`).  The queue is asked for the bias gradient exactly
#                  when it is wanted and BIAS_IN_WGRAD is on; it writes ``.grad`` itself, autograd gets no gradient.
#   2. sink        the kernel takes the product (`_wgrad_own`) and a live sink owns the weight (`_sink_of`): the launch
#                  writes the view the sink hands out (`take` ... `done`), autograd gets no gradient for the weight.
#   3. own kernel  the kernel takes the product: the same launch returns a new bf16 tensor.
#   4. not taken   `_wgrads` runs the library form (`_wgrad_lib`).
# In 2 and 3 a wanted bias gradient rides on the launch when BIAS_IN_WGRAD is on (column sums of the dY fragments it reads
# anyway): a bf16 [N] vector allocated on the current stream, that `_beside` is told about as `written`.  Everywhere else
# a wanted bias gradient is left to `column_sum(dy)` — `_bias_left` says when; `_wgrads` runs that pass behind all the weight
# gradients of its call.
def _route_wgrad(w, dy, x2, want_bias: bool = False):
    """``(dw, db, taken)`` for ``dW = dy^T x2`` of the weight ``w``; see the rule above.  ``dw``: the new gradient, None where
    a queue or a sink received it or nothing took it; ``db``: the bias gradient that rode on the launch, else None."""
    ride = bool(want_bias and BIAS_IN_WGRAD)
    if _queue_wgrad(w, dy, x2, ride):
        return None, None, True
    if not _wgrad_own(dy, x2):
        return None, None, False
    sink = _sink_of(w)
    db = torch.empty(dy.shape[1], dtype=torch.bfloat16, device=dy.device) if ride else None

    def launch():
        if sink is None:
            return gemm([(dy, x2)], True, True, bias_grad=db)
        view, acc = sink.take(w)
        gemm([(dy, x2)], True, True, out=view, accumulate=acc, bias_grad=db)
        sink.done(w)
    return _beside((dy, x2), launch, written=(db,)), db, True


def _bias_left(want_bias, taken) -> bool:
    """a wanted bias gradient that `_route_wgrad` did not settle: the caller owes `column_sum(dy)`"""
    return bool(want_bias and not (taken and BIAS_IN_WGRAD))


def _wgrad_lib(dys, x2, layout: str = "nt", out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """The library's weight gradients ``dW_i = dY_i^T x2`` of layers that share x2 [M, K], as a list.  ``layout``:
        "nt"        one product per layer in autograd's layout, dY_i^T read as a view (``out (+)= ..`` for a single layer;
                    an fp32 ``out`` takes the operands as fp32: the loss path's sum over chunks)
        "nt_fused"  ONE product over the column-concatenated dY (three 1280 x 1280 outputs of the audio tower are 25 tiles
                    each) — a batched one without the concatenation where the dY_i already lie back to back in one
                    storage (library.attn_bwd_stacked)
        "tn"        dY_i and x2 transposed by a HIP kernel and ONE product over the whole group [sum N_i, M] x [M, K] in the
                    forward layout: hipBLASLt contracts over the slow dimension of both operands at ~1.0 PFLOP/s only."""
    n, (M, K), Ns = len(dys), x2.shape, [d.shape[1] for d in dys]
    if layout == "nt_fused" and n > 1:
        st = _stacked_view(dys)
        if st is not None:
            return list(torch.bmm(st.transpose(1, 2), x2.unsqueeze(0).expand(n, M, K)).unbind(0))
        return list(torch.split(torch.mm(torch.cat(dys, dim=1).t(), x2), Ns, dim=0))
    if layout == "tn" and _transposable(x2, *dys):
        xt = transpose_2d(_c(x2))                                          # [K, M]
        dyt = torch.empty(sum(Ns), M, dtype=x2.dtype, device=x2.device)    # [sum N, M]
        o = 0
        for d, N in zip(dys, Ns):
            transpose_2d(d, out=dyt[o:o + N])
            o += N
        return list(torch.split(_mm_tn(dyt, xt), Ns, dim=0))               # TN: both contraction-contiguous
    if out is None:
        return [torch.mm(d.t(), x2) for d in dys]
    (d,) = dys
    if out.dtype != d.dtype:
        d, x2 = d.float(), x2.float()
    return [out.addmm_(d.t(), x2) if accumulate else torch.mm(d.t(), x2, out=out)]


def _wgrad_unowned(dy, x2, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """``dW = dy^T x2`` (``out (+)= ..``) of a weight whose gradient the caller keeps to itself — no queue, no sink, no side
    stream: the lm_head inside the loss, which sums its chunks."""
    if _wgrad_own(dy, x2):
        return gemm([(dy, x2)], True, True, out=out, accumulate=accumulate)
    return _wgrad_lib([dy], x2, out=out, accumulate=accumulate)[0]


def _wgrads(ws, dys, x2, want_w, want_b, layout: str = "nt"):
    """``(dws, dbs)`` of the layers ``ws`` that share the input x2 [M, K]: each wanted ``dW_i = dY_i^T x2`` where
    `_route_wgrad` puts it (None: a queue or a sink has it), what nothing takes by the library (`_wgrad_lib` — its group
    layouts only for a whole group), and behind all of them the wanted bias gradients no launch carried (`column_sum`)."""
    n = len(ws)
    dws, dbs, want_b = [None] * n, [None] * n, list(want_b)
    left = [i for i in range(n) if want_w[i]]
    for i in [i for i in left if dys[i].is_cuda]:         # (meta tensors: the library form; a queue would take them)
        dws[i], dbs[i], taken = _route_wgrad(ws[i], dys[i], x2, want_b[i])
        want_b[i] = _bias_left(want_b[i], taken)
        if taken:
            left.remove(i)
    if left:
        for i, dw in zip(left, _wgrad_lib([dys[i] for i in left], x2, layout if len(left) == n else "nt")):
            dws[i] = dw
    return dws, [column_sum(d) if nb else b for b, nb, d in zip(dbs, want_b, dys)]


def _wgrad_one(w, dy, x2):
    """dW of a bias-free layer"""
    return _wgrads([w], [dy], x2, [True], [False])[0][0]


def _wgrad_group(items):
    """Weight gradients dY_i^T x_i of up to three layers ``items = [(w, dy, x2), ...]`` as ONE grouped launch
    (gemm_grouped_wgrad), beside the backward's own stream like every weight gradient (`_beside`).  With a data-parallel
    engine's gradient sinks registered for ALL of them (one dtype, one accumulate state) the launch writes the engine's
    staging views and the result is [None, ...]; with none it returns new bf16 tensors; a mixed state, or operands the
    kernel does not take, fall back to one routed product per layer."""
    sinks = [_sink_of(w) for w, _, _ in items]
    owned = sum(sk is not None for sk in sinks)
    if not all(_wgrad_own(dy, x2) for _, dy, x2 in items) or 0 < owned < len(items):
        return [_wgrad_one(*it) for it in items]
    pairs = [(dy, x2) for _, dy, x2 in items]

    def launch():
        if not owned:
            return gemm_grouped_wgrad(pairs)
        taken = [sk.take(w) for sk, (w, _, _) in zip(sinks, items)]
        if len({(v.dtype, bool(acc)) for v, acc in taken}) == 1:
            gemm_grouped_wgrad(pairs, outs=[v for v, _ in taken], accumulate=bool(taken[0][1]))
        else:                                                 # (already taken: write each view by itself)
            for (view, acc), pair in zip(taken, pairs):
                gemm([pair], True, True, out=view, accumulate=acc)
        for sk, (w, _, _) in zip(sinks, items):
            sk.done(w)
        return [None] * len(items)
    return _beside([t for pair in pairs for t in pair], launch)


def _stacked_view(ts):
    """[n, M, N] view over `ts` if they are equally shaped contiguous [M, N] matrices lying back to back in one storage
    (in order), else None."""
    t0 = ts[0]
    if t0.dim() != 2 or not all(t.shape == t0.shape and t.dtype == t0.dtype and t.is_contiguous() for t in ts):
        return None
    step = t0.numel()
    try:
        base = t0.untyped_storage().data_ptr()
        if not all(t.untyped_storage().data_ptr() == base and t.storage_offset() == t0.storage_offset() + i * step
                   for i, t in enumerate(ts)):
            return None
    except (RuntimeError, NotImplementedError):          # (fake / meta tensors without storage)
        return None
    return t0.as_strided((len(ts), t0.shape[0], t0.shape[1]), (step, t0.shape[1], 1))


class _LinearGroup(torch.autograd.Function):
    """``y_i = x W_i^T + b_i`` for a group of linear layers that share their input (q/k/v, gate/up, or one layer).

    Forward is what nn.Linear does.  Each product runs where its kind's function puts it (`_mm_tn`, `_dgrad`, `_wgrads`):
    on the hand-written kernel in its native layout, or in the library's form — ``wgrad`` names the layout of the library's
    weight gradient ("tn" | "nt" | "nt_fused": `_wgrad_lib`), ``dgrad_tn=False`` keeps W as stored for the library's input
    gradient (no gain at 1280 x 1280).  ``extra = (norm_src, rope)``: op-level selective recomputation (`norm_source`) and
    the rotary embedding of some outputs (`linear_group`), either may be None."""

    @staticmethod
    def forward(ctx, x, n, wgrad, dgrad_tn, extra, *wb):
        ws, bs = wb[:n], wb[n:]
        src, rope = extra
        ctx.rope = rope
        if src is not None:
            # x = RMSNorm(h) * w_norm is a ROW kernel's output: keep its input (which the norm's own backward saves
            # anyway) and recompute x in the backward — bit-identical, the kernel norms the stored h
            ctx.save_for_backward(src[0], *ws, src[1])
            ctx.src_eps, ctx.xshape = float(src[2]), x.shape
        else:
            ctx.save_for_backward(x, *ws)
            ctx.src_eps = None
        ctx.has_bias = [b is not None for b in bs]
        ctx.wgrad, ctx.dgrad_tn = wgrad, dgrad_tn
        x2 = _c(x.reshape(-1, x.shape[-1]))
        # (launch order, kept as it has always been: the library configuration rotates behind ALL its products)
        at_once = _own_configured() and x.is_cuda
        outs = []
        for i, (w, b) in enumerate(zip(ws, bs)):
            w = _c(w)
            if rope is None or i not in rope[3]:
                y = _mm_tn(x2, w, b)
            elif _rope_epilogue_own(x2, w, rope):          # the rotary embedding in the product's epilogue
                y = gemm_rope(x2, w, b, *rope[:3])
            else:                                          # ... or behind it: same bits
                y = _mm_tn(x2, w, b)
                if at_once:
                    y = _rotated(y, rope)
            outs.append(y)
        if rope is not None and not at_once:
            for i in rope[3]:
                outs[i] = _rotated(outs[i], rope)
        return tuple(y.view(*x.shape[:-1], y.shape[-1]) for y in outs)

    @staticmethod
    def backward(ctx, *dys):
        x, *ws = ctx.saved_tensors
        if ctx.src_eps is not None:
            norm_w = ws.pop()
            x = L.rmsnorm_fwd(x, None, norm_w, ctx.src_eps)[0].view(ctx.xshape)
        n = len(ws)
        x2 = _c(x.reshape(-1, x.shape[-1]))
        M = x2.shape[0]
        dys = [torch.zeros(M, w.shape[0], dtype=x.dtype, device=x.device) if d is None else _c(d).reshape(M, -1)
               for d, w in zip(dys, ws)]
        if ctx.rope is not None and not ctx.rope[4]:
            # the outputs were rotated: their gradients are rotated back (the transposed rotation) before the products
            # (rope[4]: the consumer did that already — `_AttentionRopeGrad`)
            cos, sin, D, which = ctx.rope[:4]
            which = sorted(which)
            for a in range(0, len(which), 2):
                i, j = which[a], which[a + 1] if a + 1 < len(which) else None
                gi = dys[i].view(1, M, -1, D)
                gj = dys[j].view(1, M, -1, D) if j is not None else gi.new_empty(1, M, 0, D)
                ri, rj = L.rope_apply(gi, gj, cos, sin, True)
                dys[i] = ri.view(M, -1)
                if j is not None:
                    dys[j] = rj.view(M, -1)
        need = ctx.needs_input_grad
        dx = _dgrad(dys, [_c(w) for w in ws], dgrad_tn=ctx.dgrad_tn).view(x.shape) if need[0] else None
        dws, dbs = _wgrads(ws, dys, x2, need[5:5 + n], [hb and nb for hb, nb in zip(ctx.has_bias, need[5 + n:])], ctx.wgrad)
        return (dx, None, None, None, None, *dws, *dbs)


def norm_source(h, norm_weight, eps):
    """`norm_src` argument of `linear_group` / `swiglu_mlp`: says that their input x IS ``rms_norm(h, norm_weight, eps)`` (h =
    the residual stream the norm saw, i.e. its second output), so that the node may keep h instead of x and recompute x
    in its backward.  This is the op-level selective activation checkpointing of the reference
    (touchnet/models/helper_func.py:39-96: save the outputs of the compute ops — matmuls, attention — and recompute the
    rest) on this path's own autograd nodes: GEMM and attention outputs stay, the ROW kernels' outputs (norm outputs,
    the SwiGLU product) are recomputed."""
    return (h.detach(), norm_weight.detach(), float(eps))


def _norm_src_describes(norm_src, x) -> bool:
    """`norm_src` may stand in for x only if its residual stream has x's rows and dtype; anything else (a sequence-parallel
    wrapper that gathered x to the full sequence behind the norm) silently keeps x itself: a memory optimisation must
    never change or break a step."""
    return (norm_src is not None and tuple(norm_src[0].shape) == tuple(x.shape) and norm_src[0].dtype == x.dtype
            and norm_src[1].shape[-1] == x.shape[-1])


def linear_group(x, layers, wgrad: str = "tn", dgrad_tn: bool = True, norm_src=None, rope=None,
                 rope_grad_in_attention: bool = False):
    """``layers``: list of (weight [N_i, K], bias [N_i] | None) sharing the input ``x`` -> list of outputs.
    ``norm_src``: see `norm_source`.  ``rope = (cos, sin, head_dim, (i, j, ..))``: outputs i, j, .. ([.., heads * head_dim])
    are returned ROTATED — the rotary embedding `apply_rope` would apply to them, computed in the projection's epilogue
    (`gemm_rope`); cos / sin as from `rope_tables`, one row per row of x.  ``rope_grad_in_attention``: the rotated outputs
    go to `packed_attention(.., rope_grad=(cos, sin))` and nowhere else, which returns their gradients rotated back."""
    if wgrad not in ("tn", "nt", "nt_fused"):
        raise ValueError(f"linear_group: wgrad={wgrad!r}")
    if not (x.is_cuda or x.is_meta):
        raise _C.KernelError("linear_group: device tensors only (the product path has no CPU fallback)")
    ws = [w for w, _ in layers]
    bs = [b for _, b in layers]
    if not _norm_src_describes(norm_src, x):
        norm_src = None           # (e.g. under tensor-parallel sequence parallelism x is the gathered sequence): keep x itself
    if rope is not None:
        rope = (rope[0].detach(), rope[1].detach(), int(rope[2]), tuple(int(i) for i in rope[3]),
                bool(rope_grad_in_attention))
    return list(_LinearGroup.apply(x, len(ws), wgrad, dgrad_tn, (norm_src, rope), *ws, *bs))


class _SwiGLUMLP(torch.autograd.Function):
    """``down(silu(gate(x)) * up(x))`` as ONE autograd node (modeling_llama.py:174-176, three bias-free nn.Linear).

    ``ctx.own`` (the kernel takes all four product shapes, decided once in the forward): seven launches of the hand-written
    kernel (gate, up, down; dW_down, d(act), dX over the (gate, up) pair as one two-segment launch, dW_gate, dW_up) + the two
    SwiGLU kernels, which ``ctx.fused`` folds into epilogues; nothing is transposed.  Otherwise the library body
    (`_backward_lib`): same GEMMs in the forward layout, the transposed operands they need — act^T for dW_down,
    [d_gate^T; d_up^T] for the grouped dW_gate/up — written by the SwiGLU kernels themselves (tn_swiglu_fwd_t /
    tn_swiglu_bwd_t: one extra store each) instead of by separate transpose passes."""

    @staticmethod
    def forward(ctx, x, wg, wu, wd, src=None):
        K, I = x.shape[-1], wg.shape[0]
        x2 = _c(x.reshape(-1, K))
        M = x2.shape[0]
        own = _own(M, I, (K,)) and _own(M, K, (I,)) and _own(I, K, (M,), True, True) and _own(K, I, (M,), True, True)
        fused = own and MLP_EPILOGUE and _bf16_rows(x2, wg, wu, wd) and wg.stride(0) == wu.stride(0)
        if fused:
            gate, up, act = gemm_swiglu_fwd(x2, wg, wu)       # SwiGLU in the epilogue of ONE gate + up launch
            kept = act
        else:
            gate, up = _mm_tn(x2, _c(wg)), _mm_tn(x2, _c(wu))
            if own:
                act = L.swiglu_fwd(gate, up)
                kept = act
            else:
                act, kept = L.swiglu_fwd_t(gate, up)                   # kept = act^T
        y = _mm_tn(act, _c(wd))
        if src is not None and own:
            # op-level selective recomputation (`norm_source`): neither the norm output x nor act = silu(gate) * up is
            # kept — both are row kernels' outputs, recomputed bit-identically in the backward from h and (gate, up)
            ctx.save_for_backward(src[0].reshape(-1, K), gate, up, src[1], wg, wu, wd)
            ctx.src_eps = float(src[2])
        else:
            ctx.save_for_backward(x2, gate, up, kept, wg, wu, wd)
            ctx.src_eps = None
        ctx.xshape, ctx.own, ctx.fused = x.shape, own, fused
        return y.view(*x.shape[:-1], wd.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, gate, up, kept, wg, wu, wd = ctx.saved_tensors
        if ctx.src_eps is not None:
            x2 = L.rmsnorm_fwd(x2, None, kept, ctx.src_eps)[0]           # (x2 held h, `kept` the norm weight)
            kept = L.swiglu_fwd(gate, up)
        M, K = x2.shape
        I, H = wg.shape[0], wd.shape[0]
        dy2 = _c(dy).reshape(M, H)
        nx, ng, nu, nd = ctx.needs_input_grad[:4]
        if not ctx.own:
            return (*_SwiGLUMLP._backward_lib(x2, gate, up, kept, wg, wu, wd, dy2, nx, ng, nu, nd, ctx.xshape), None)
        grouped = GROUPED_WGRAD and ng and nu and nd
        if not grouped:                                   # one routed product each (`_route_wgrad`)
            dwd = _wgrad_one(wd, dy2, kept) if nd else None                        # dY^T act  [H, I]
        if ctx.fused and H % 64 == 0 and _bf16_rows(dy2, wd):
            dgate, dup = gemm_swiglu_bwd(dy2, wd, gate, up)     # d(act) = dY W_down lives in the accumulators only
        else:
            dact = gemm([(dy2, _c(wd))], b_kmaj=True)                              # dY W_down [M, I]
            dgate, dup = L.swiglu_bwd(dact, gate, up)
            del dact
        dx = gemm([(dgate, _c(wg)), (dup, _c(wu))], b_kmaj=True).view(ctx.xshape) if nx else None
        if grouped:
            # ONE launch for the three weight gradients (3 x 688 tiles = 8 whole rounds + 16 tiles split-K)
            dwg, dwu, dwd = _wgrad_group([(wg, dgate, x2), (wu, dup, x2), (wd, dy2, kept)])
        else:
            dwg = _wgrad_one(wg, dgate, x2) if ng else None
            dwu = _wgrad_one(wu, dup, x2) if nu else None
        return dx, dwg, dwu, dwd, None

    @staticmethod
    def _backward_lib(x2, gate, up, act_t, wg, wu, wd, dy2, nx, ng, nu, nd, xshape):
        """``(dx, dW_gate, dW_up, dW_down)`` of the library body: every product in the forward layout (`_mm_tn`), act^T kept
        by the forward's SwiGLU kernel, [d_gate^T; d_up^T] written by the backward's."""
        I = wg.shape[0]
        dwd = _mm_tn(transpose_2d(dy2), act_t) if nd else None                      # [H, I]
        dact = _mm_tn(dy2, transpose_2d(_c(wd)))                                    # [M, I]
        dgate, dup, dgu_t = L.swiglu_bwd_t(dact, gate, up)
        del dact
        dx = None
        if nx:
            dx = _mm_tn(dgate, transpose_2d(_c(wg)))
            _mm_tn(dup, transpose_2d(_c(wu)), out=dx, accumulate=True)
            dx = dx.view(xshape)
        dwg = dwu = None
        if ng or nu:
            dwg, dwu = torch.split(_mm_tn(dgu_t, transpose_2d(x2)), [I, I], dim=0)
        return dx, dwg if ng else None, dwu if nu else None, dwd


class _Conv1dK3(torch.autograd.Function):
    """``conv1d(kernel 3, padding 1, stride s)`` over channels-last sequences as GEMMs of the hand-written kernel — the
    Whisper / Qwen2-Audio conv stem (transformers' WhisperEncoder.conv1 / conv2 behind touchnet/models/qwen2_audio/
    __init__.py:52-73), which the reference runs through cuDNN/MIOpen.

    x [n, T, C] is copied once into zero-separated slots of P = T + 2 rows ([0, x_0 .. x_{T-1}, 0]; P a multiple of s) of
    ONE long [n P + s, C] sequence.  The im2col matrix then needs no copy: row r = the 3 C contiguous elements from row
    r s on — a strided VIEW with overlapping rows (pitch s C < 3 C), which the GEMM's DMA descriptors read as they are:
        forward      Y [n P / s, O] = A W2^T + b          W2[o, k C + c] = w[o, c, k]
        dW2          = dY^T A        (both contraction-major: the contraction runs over the output rows)
        dX           = overlap-add of dA = dY W2 over the three taps (fp32 accumulation, one rounding)
    Of the P / s output rows of a slot the first T_out are the convolution, the last one(s) mix two clips: the result is
    returned WHOLE ([n, P / s, O]; the caller slices behind its activation) so that nothing is copied here."""

    @staticmethod
    def forward(ctx, x, w, b, stride, need_dx):
        n, T, C0 = x.shape
        O, s = w.shape[0], int(stride)
        C = (C0 + 63) // 64 * 64                 # channels padded with zeros: 3 C is then a multiple of the 64-deep stage
        P = (T + 2 + s - 1) // s * s
        R = n * P // s
        xp = x.new_zeros(n * P + s + 2, C)                                 # (+ tail rows: the last window stays inside)
        xp[:n * P].view(n, P, C)[:, 1:T + 1, :C0] = x
        A = xp.as_strided((R, 3 * C), (s * C, 1))
        w2 = w.new_zeros(O, 3, C)
        w2[:, :, :C0] = w.permute(0, 2, 1)
        w2 = w2.view(O, 3 * C)
        y = gemm([(A, w2)], bias=b)
        ctx.save_for_backward(xp, w2)
        ctx.geom = (n, T, C0, C, O, s, P, R, bool(need_dx), b is not None, w.dtype)
        return y.view(n, P // s, O)

    @staticmethod
    def backward(ctx, dy):
        xp, w2 = ctx.saved_tensors
        n, T, C0, C, O, s, P, R, need_dx, has_b, wdtype = ctx.geom
        dyf = _c(dy).reshape(R, O)
        A = xp.as_strided((R, 3 * C), (s * C, 1))
        dw2 = gemm([(dyf, A)], True, True)                                 # [O, 3 C]
        dw = dw2.view(O, 3, C)[:, :, :C0].permute(0, 2, 1).contiguous().to(wdtype)
        db = column_sum(dyf) if has_b else None
        dx = None
        if need_dx:
            dA = gemm([(dyf, w2)], b_kmaj=True)                            # [R, 3 C]
            acc = torch.zeros(n * P + s + 2, C, dtype=torch.float32, device=dy.device)
            for k in range(3):                                             # tap k of output row r lands on row r s + k
                acc[k:k + R * s:s] += dA[:, k * C:(k + 1) * C]
            dx = acc[:n * P].view(n, P, C)[:, 1:T + 1, :C0].to(dy.dtype)
        return dx, dw, db, None, None


def conv1d_k3(x, weight, bias, stride: int = 1, need_dx: bool = True):
    """x [n, T, C] (channels last) -> (y [n, P / stride, O] with the convolution in rows [0, T_out), T_out); see
    _Conv1dK3.  bf16 device tensors, output channels a multiple of 8."""
    n, T, C = x.shape
    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and weight.shape[2] == 3 and weight.shape[1] == C and weight.shape[0] % (64 if need_dx else 8) == 0):
        raise _C.KernelError("conv1d_k3: bf16 device tensors, kernel size 3, output channels a multiple of 8 (of 64 when the "
                             "input gradient is wanted: it contracts over them)")
    return _Conv1dK3.apply(_c(x), weight, bias, stride, need_dx), (T + 2 - 3) // stride + 1


_MLP_FUSED = True             # `swiglu_mlp` as the one node `_SwiGLUMLP` (off: composed of `linear_group` and `swiglu`)
GELU_EPILOGUE = True          # `gelu_mlp` as the one node `_GeluMLP` (off: composed of `linear_group` and `gelu`; same bits)


class _GeluMLP(torch.autograd.Function):
    """``fc2(gelu(fc1(x)))`` of the Whisper-style encoder layer as ONE autograd node: GELU in fc1's epilogue (pre and act
    from one launch), its backward in the epilogue of fc2's input-gradient product (d(act) stays in the accumulators);
    weight and bias gradients by `_wgrads`, as in `_LinearGroup` (bias gradients ride on the weight-gradient launches).
    Every launch is bit-identical to the kernels it replaces.  Same box, interleaved: 707.5 -> 705.5 ms per headline step
    (profiles/r06g_*: the two GELU passes, 9.3 ms, against 4.9 ms of epilogue time inside the GEMMs).  `gelu_mlp` enters
    only where the hand-written kernel takes all four products (`_gelu_mlp_own`): the node launches them itself."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        K, I, H = x.shape[-1], w1.shape[0], w2.shape[0]
        x2 = _c(x.reshape(-1, K))
        pre, act = gemm_gelu_fwd(x2, _c(w1), b1)
        y = _mm_tn(act, _c(w2), b2)
        ctx.save_for_backward(x2, pre, act, w1, w2)
        ctx.xshape, ctx.has_b = x.shape, (b1 is not None, b2 is not None)
        return y.view(*x.shape[:-1], H)

    @staticmethod
    def backward(ctx, dy):
        x2, pre, act, w1, w2 = ctx.saved_tensors
        M, K = x2.shape
        I, H = w1.shape[0], w2.shape[0]
        dy2 = _c(dy).reshape(M, H)
        nx, n1, nb1, n2, nb2 = ctx.needs_input_grad[:5]
        dpre = gemm_gelu_bwd(dy2, _c(w2), pre)                                   # (dY W2) o gelu'(pre)   [M, I]
        dx = gemm([(dpre, _c(w1))], b_kmaj=True).view(ctx.xshape) if nx else None

        (dw2,), (db2,) = _wgrads([w2], [dy2], act, [n2], [nb2 and ctx.has_b[1]])
        (dw1,), (db1,) = _wgrads([w1], [dpre], x2, [n1], [nb1 and ctx.has_b[0]])
        return dx, dw1, db1, dw2, db2


def _gelu_mlp_own(x, w1, b1, w2, b2) -> bool:
    """The hand-written kernel takes fc1, fc2 and both input gradients of `_GeluMLP` (their extents; the weight gradients
    ask for themselves), on bf16 device operands."""
    M, K = x.numel() // x.shape[-1], x.shape[-1]
    I, H = w1.shape[0], w2.shape[0]
    return (x.is_cuda and x.dtype == torch.bfloat16
            and _own(M, I, (K,)) and _own(M, H, (I,)) and _own(M, I, (H,), False, True) and _own(M, K, (I,), False, True)
            and _bf16_rows(w1, w2) and all(b is None or b.dtype == torch.bfloat16 for b in (b1, b2)))


def gelu_mlp(x, w1, b1, w2, b2):
    """The Whisper / Qwen2-Audio encoder layer's MLP ``fc2(gelu(fc1(x)))``: bf16 device tensors of shapes the GELU
    epilogues take go through the fused node above, anything else composes the individual ops (same bits)."""
    if not (x.is_cuda or x.is_meta):
        raise _C.KernelError("gelu_mlp: device tensors only (the product path has no CPU fallback)")
    if GELU_EPILOGUE and _gelu_mlp_own(x, w1, b1, w2, b2):
        return _GeluMLP.apply(x, w1, b1, w2, b2)
    h = linear_group(x, [(w1, b1)], wgrad="nt", dgrad_tn=False)[0]
    return linear_group(gelu(h), [(w2, b2)], wgrad="nt", dgrad_tn=False)[0]


def swiglu_mlp(x, w_gate, w_up, w_down, norm_src=None):
    """Llama/Qwen2 MLP ``down(silu(gate(x)) * up(x))`` (bias-free).  bf16 device tensors with 8-aligned shapes take the
    fused node above; anything else composes the individual ops (same maths).  ``norm_src``: see `norm_source`."""
    if not (x.is_cuda or x.is_meta):
        raise _C.KernelError("swiglu_mlp: device tensors only (the product path has no CPU fallback)")
    M = x.numel() // x.shape[-1]
    if not _norm_src_describes(norm_src, x):
        norm_src = None
    # (the node's library body transposes x, the weights and dY: `_transposable`)
    if _MLP_FUSED and x.dtype == torch.bfloat16 and M % 8 == 0 and _transposable(w_gate, w_up, w_down):
        return _SwiGLUMLP.apply(x, w_gate, w_up, w_down, norm_src)
    gate, up = linear_group(x, [(w_gate, None), (w_up, None)], norm_src=norm_src)
    return linear_group(swiglu(gate, up), [(w_down, None)])[0]

# ------------------------------------------------------------------------------------ frontend
_MEL_CACHE = {}


def slaney_mel_filters(n_mels: int, device) -> torch.Tensor:
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels) (touchnet/data/functions.py:179-182): slaney scale
    and norm.  A constant table, built on the host once per (n_mels, device)."""
    key = (n_mels, str(device))
    if key not in _MEL_CACHE:
        import numpy as np
        sr, n_fft = 16000.0, 400
        f_sp, min_log_hz = 200.0 / 3, 1000.0
        min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
        to_mel = lambda f: np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep,
                                    f / f_sp)
        to_hz = lambda m: np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
        fftfreqs = np.linspace(0.0, sr / 2, 1 + n_fft // 2)
        mel_f = to_hz(np.linspace(to_mel(np.float64(0.0)), to_mel(np.float64(sr / 2)), n_mels + 2))
        fdiff = np.diff(mel_f)
        ramps = mel_f[:, None] - fftfreqs[None, :]
        lower = -ramps[:-2] / fdiff[:-1, None]
        upper = ramps[2:] / fdiff[1:, None]
        w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
        _MEL_CACHE[key] = torch.from_numpy(w.astype(np.float32)).to(device).contiguous()
    return _MEL_CACHE[key]


KALDI_MIN_PADDED, KALDI_MAX_PADDED = 32, 2048     # FFT sizes of csrc/kaldi_feats.hip (8 .. 48 kHz at 25 ms, 16 kHz to 128 ms)
KALDI_MIN_BINS, KALDI_MAX_BINS = 4, 256           # torchaudio asks for more than 3 bins; one thread per bin
KALDI_LIFTER = 22.0                               # torchaudio's / Kaldi's cepstral_lifter
_KALDI_TABLES = {}


def kaldi_feature_geometry(sample_rate, frame_length, frame_shift, num_mel_bins, low_freq=20.0, high_freq=0.0,
                           num_ceps=None):
    """(win, shift, padded, high) of a Kaldi feature configuration in samples and Hz — `win = int(sr frame_length / 1000)`,
    `padded` the next power of two, `high` after Kaldi's rule (high_freq <= 0: offset from Nyquist) — or a ValueError that
    names the field csrc/kaldi_feats.hip cannot take.  Pure host arithmetic: callers check a config with it before any
    sample is read."""
    sr = int(sample_rate)
    if sr < 1 or sr != sample_rate:
        raise ValueError(f"sample_rate = {sample_rate}: a positive integer number of Hz")
    win, shift = int(sr * frame_length * 0.001), int(sr * frame_shift * 0.001)
    if shift < 1:
        raise ValueError(f"audiofeat_frame_shift = {frame_shift} ms is less than one sample at {sr} Hz")
    padded = 1 << max(win - 1, 0).bit_length()
    if not KALDI_MIN_PADDED <= padded <= KALDI_MAX_PADDED:
        raise ValueError(f"audiofeat_frame_length = {frame_length} ms at {sr} Hz is a window of {win} samples, FFT size "
                         f"{padded}: the MI355X feature kernel takes FFT sizes {KALDI_MIN_PADDED} .. {KALDI_MAX_PADDED}")
    bins = int(num_mel_bins)
    if not KALDI_MIN_BINS <= bins <= KALDI_MAX_BINS:
        raise ValueError(f"audiofeat_num_mel_bins = {num_mel_bins}: the feature kernel takes {KALDI_MIN_BINS} .. "
                         f"{KALDI_MAX_BINS} mel bins (torchaudio needs more than 3)")
    if num_ceps is not None and not 1 <= int(num_ceps) <= bins:
        raise ValueError(f"audiofeat_num_ceps = {num_ceps} must lie in 1 .. audiofeat_num_mel_bins = {bins} "
                         f"(torchaudio asserts the same; the reference's own defaults, 40 over 23, do not pass it)")
    nyquist = 0.5 * sr
    high = float(high_freq) if high_freq > 0.0 else nyquist + float(high_freq)
    if not 0.0 <= float(low_freq) < high <= nyquist:
        raise ValueError(f"audiofeat_low_freq = {low_freq} / audiofeat_high_freq = {high_freq} (= {high} Hz): need "
                         f"0 <= low < high <= Nyquist = {nyquist} Hz")
    return win, shift, padded, high


def kaldi_feature_tables(sample_rate, frame_length, frame_shift, num_mel_bins, low_freq=20.0, high_freq=0.0,
                         num_ceps=None):
    """The host tables of csrc/kaldi_feats.hip in float64 (numpy; no GPU needed), as torchaudio.compliance.kaldi builds
    them:
        window    [win]         Povey: (0.5 - 0.5 cos(2 pi n / (win - 1)))^0.85
        bank_idx  [bins, 3]     int32 (first FFT bin, count, offset into bank_w) of the weights of each mel triangle
                                max(0, min(up, down)) over the padded / 2 FFT bins that are non-zero AS FLOAT32 — what
                                is left out is exactly 0.0f; a triangle no FFT bin falls into has count 0
        bank_w    [sum count]   those weights, packed in bin order
        dct       [num_ceps, bins]   lifter[k] DCT[k][n] with torchaudio's orthonormal DCT-II (row 0 = sqrt(1 / N)) and
                                lifter 1 + 0.5 Q sin(pi k / Q), Q = 22; None without num_ceps
    plus win, shift, padded.  The kernel reads the float32 cast of each."""
    import numpy as np
    win, shift, padded, high = kaldi_feature_geometry(sample_rate, frame_length, frame_shift, num_mel_bins, low_freq,
                                                      high_freq, num_ceps)
    sr, bins = int(sample_rate), int(num_mel_bins)
    n = np.arange(win, dtype=np.float64)
    window = (0.5 - 0.5 * np.cos(2.0 * math.pi * n / (win - 1))) ** 0.85
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    mel_lo, mel_hi = mel(float(low_freq)), mel(high)
    delta = (mel_hi - mel_lo) / (bins + 1)
    b = np.arange(bins, dtype=np.float64)[:, None]
    left, center, right = mel_lo + b * delta, mel_lo + (b + 1.0) * delta, mel_lo + (b + 2.0) * delta
    m = mel((sr / padded) * np.arange(padded // 2, dtype=np.float64))[None, :]
    dense = np.maximum(0.0, np.minimum((m - left) / (center - left), (right - m) / (right - center)))
    idx = np.zeros((bins, 3), dtype=np.int32)
    packed = []
    for r in range(bins):
        nz = np.flatnonzero(dense[r].astype(np.float32))
        if nz.size:
            idx[r] = (nz[0], nz[-1] - nz[0] + 1, sum(p.size for p in packed))
            packed.append(dense[r, nz[0]:nz[-1] + 1])
        else:
            idx[r] = (0, 0, sum(p.size for p in packed))
    tables = dict(win=win, shift=shift, padded=padded, window=window, bank_idx=idx,
                  bank_w=np.concatenate(packed) if packed else np.zeros(0), dct=None)
    if num_ceps is not None:
        k = np.arange(int(num_ceps), dtype=np.float64)[:, None]
        dct = np.cos(math.pi / bins * (np.arange(bins, dtype=np.float64)[None, :] + 0.5) * k) * math.sqrt(2.0 / bins)
        dct[0] = math.sqrt(1.0 / bins)
        tables["dct"] = (1.0 + 0.5 * KALDI_LIFTER * np.sin(math.pi * k / KALDI_LIFTER)) * dct
    return tables


def _kaldi_device_tables(device, *key):
    if (key, device) not in _KALDI_TABLES:
        t = kaldi_feature_tables(*key)
        dev = lambda a, dt: None if a is None else torch.from_numpy(a).to(dt).to(device).contiguous()
        _KALDI_TABLES[(key, device)] = (t["shift"], dev(t["window"], torch.float32), dev(t["bank_idx"], torch.int32),
                                        dev(t["bank_w"], torch.float32), dev(t["dct"], torch.float32))
    return _KALDI_TABLES[(key, device)]


def _kaldi_wave(wav, what):
    if not wav.is_cuda:
        raise RuntimeError(f"{what}: expects a device waveform (there is no CPU path)")
    return _c(wav).float().view(-1)


def kaldi_fbank(wav: torch.Tensor, num_mel_bins: int = 80, sample_rate: int = 16000, frame_length=25.0, frame_shift=10.0,
                low_freq: float = 20.0, high_freq: float = 0.0) -> torch.Tensor:
    """wav fp32 [N] in [-1, 1) at `sample_rate` Hz -> Kaldi log-fbank fp32 [frames, num_mel_bins] with windows of
    `frame_length` ms every `frame_shift` ms (functions.py:117-134 at any rate and geometry; the defaults are the
    recipes' 16 kHz 25 / 10, 20 Hz .. Nyquist)."""
    key = (int(sample_rate), frame_length, frame_shift, int(num_mel_bins), float(low_freq), float(high_freq), None)
    wav = _kaldi_wave(wav, "kaldi_fbank")
    shift, window, idx, w, _ = _kaldi_device_tables(wav.device, *key)
    return L.kaldi_feats(wav, window, idx, w, key[0], shift, key[4], key[5])


def kaldi_mfcc(wav: torch.Tensor, sample_rate: int, num_mel_bins: int, num_ceps: int, frame_length, frame_shift,
               low_freq: float = 20.0, high_freq: float = 0.0) -> torch.Tensor:
    """wav fp32 [N] in [-1, 1) at `sample_rate` Hz -> Kaldi MFCC fp32 [frames, num_ceps] (functions.py:137-156:
    torchaudio.compliance.kaldi.mfcc, use_energy false, cepstral lifter 22): the liftered orthonormal DCT-II of the
    log-fbank row, computed in the same launch."""
    key = (int(sample_rate), frame_length, frame_shift, int(num_mel_bins), float(low_freq), float(high_freq),
           int(num_ceps))
    wav = _kaldi_wave(wav, "kaldi_mfcc")
    shift, window, idx, w, dct = _kaldi_device_tables(wav.device, *key)
    return L.kaldi_mfcc(wav, window, idx, w, dct, key[0], shift, key[4], key[5])


VAD_MAX_WIN, VAD_MAX_CTX = L.VAD_MAX_WIN, L.VAD_MAX_CTX       # limits of csrc/vad.hip


@dataclass
class VadConfig:
    """The options of Kaldi's `compute-vad-energy` with that program's defaults, and the frame geometry of its features.
    Nobody has tuned these values for cutting long recordings into segments for the decoders here: they are Kaldi's
    defaults for its own use (dropping silence frames before speaker recognition), a starting point and no more."""
    frame_length: float = 25.0               # ms
    frame_shift: float = 10.0                # ms
    energy_threshold: float = 5.0            # constant term of the threshold on the log-energy
    energy_mean_scale: float = 0.5           # the threshold rises by this times the recording's mean log-energy
    frames_context: int = 0                  # frames on each side that vote on a frame
    proportion_threshold: float = 0.6        # share of the voting frames above the threshold that makes a frame voiced


def vad_geometry(sample_rate, cfg: VadConfig):
    """(win, shift) of a VAD configuration in samples at `sample_rate` Hz — `win = int(sr frame_length / 1000)` as
    kaldi_feature_geometry — or a ValueError that names the field csrc/vad.hip cannot take.  Pure host arithmetic."""
    sr = int(sample_rate)
    if sr < 1 or sr != sample_rate:
        raise ValueError(f"sample_rate = {sample_rate}: a positive integer number of Hz")
    win, shift = int(sr * cfg.frame_length * 0.001), int(sr * cfg.frame_shift * 0.001)
    if not 1 <= win <= VAD_MAX_WIN:
        raise ValueError(f"frame_length = {cfg.frame_length} ms at {sr} Hz is a window of {win} samples: the MI355X VAD "
                         f"kernel takes 1 .. {VAD_MAX_WIN}")
    if shift < 1:
        raise ValueError(f"frame_shift = {cfg.frame_shift} ms is less than one sample at {sr} Hz")
    ctx = cfg.frames_context
    if isinstance(ctx, bool) or ctx != int(ctx) or not 0 <= ctx <= VAD_MAX_CTX:
        raise ValueError(f"frames_context = {ctx!r} must be an integer in [0, {VAD_MAX_CTX}]")
    if not 0.0 < cfg.proportion_threshold <= 1.0:
        raise ValueError(f"proportion_threshold = {cfg.proportion_threshold} must be in (0, 1]")
    if not (math.isfinite(cfg.energy_threshold) and math.isfinite(cfg.energy_mean_scale)):
        raise ValueError(f"energy_threshold = {cfg.energy_threshold} / energy_mean_scale = {cfg.energy_mean_scale} must be "
                         "finite")
    return win, shift


def vad_energy(wave: torch.Tensor, sample_rate: int, cfg: Optional[VadConfig] = None):
    """Kaldi's energy VAD of one recording on the device (csrc/vad.hip): wave fp32 in [-1, 1) or int16 PCM, [N] or
    [1, N], at `sample_rate` Hz -> (runs int64 [R, 2] on the HOST: the maximal intervals [start, end) of voiced frames in
    order; voiced uint8 [T] and loge fp32 [T] on the device).  Frame t covers the samples [t shift, t shift + win) of
    vad_geometry.  One host read per recording: the run count and the runs, in one buffer.  A recording shorter than one
    window has no frame: empty results, nothing launched."""
    cfg = cfg or VadConfig()
    win, shift = vad_geometry(sample_rate, cfg)
    if not wave.is_cuda:
        raise RuntimeError("vad_energy: expects a device waveform (there is no CPU path)")
    if wave.dtype != torch.int16:
        wave = wave.float()
    wave = _c(wave).view(-1)
    if wave.numel() < win:
        return (torch.empty(0, 2, dtype=torch.int64), torch.empty(0, dtype=torch.uint8, device=wave.device),
                torch.empty(0, dtype=torch.float32, device=wave.device))
    loge, partials = L.vad_log_energy(wave, win, shift)
    voiced, buf = L.vad_runs(loge, partials, float(cfg.energy_threshold), float(cfg.energy_mean_scale),
                             int(cfg.frames_context), float(cfg.proportion_threshold))
    host = buf.cpu()
    n = int(host[0])
    return host[1:1 + 2 * n].to(torch.int64).view(n, 2), voiced, loge


def log_mel_spectrogram(wav: torch.Tensor, num_mel_bins: int = 128, padding: int = 0) -> torch.Tensor:
    """wav fp32 [N] at 16 kHz -> fp32 [N // 160, num_mel_bins] (functions.py:159-190)."""
    wav = _c(wav).float().view(-1)
    if padding > 0:
        wav = torch.nn.functional.pad(wav, (0, padding))
    return L.log_mel(wav, slaney_mel_filters(num_mel_bins, wav.device), int(num_mel_bins))


def pcm16_to_float(pcm: torch.Tensor) -> torch.Tensor:
    """int16 PCM on the device -> float32 in [-1, 1) (x / 32768, exact; touchnet/data/datapipe.py:164)."""
    if not pcm.is_cuda or pcm.dtype != torch.int16:
        raise RuntimeError("pcm16_to_float: expects an int16 device tensor")
    return L.pcm16_to_f32(_c(pcm))


def bestrq_tokenize(feat: torch.Tensor, quantizer: torch.Tensor, codebook: torch.Tensor) -> torch.Tensor:
    """BEST-RQ codes (touchnet/tokenizer/tokenizer.py:289-299): feat [T, F], quantizer [F, E], L2-normalised
    codebook [V, E], all fp32 on the device -> int64 [T]."""
    for t in (feat, quantizer, codebook):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise RuntimeError("bestrq_tokenize: expects 2-D fp32 device tensors")
    T, Fdim = feat.shape
    E, V = quantizer.shape[1], codebook.shape[0]
    if quantizer.shape[0] != Fdim or codebook.shape[1] != E:
        raise RuntimeError(f"bestrq_tokenize: shape mismatch feat {tuple(feat.shape)} quantizer {tuple(quantizer.shape)} "
                           f"codebook {tuple(codebook.shape)}")
    if E not in (8, 16, 32):
        raise _C.KernelError(f"bestrq_tokenize: codebook width {E} not in (8, 16, 32)")
    return L.bestrq_tokenize(_c(feat), _c(quantizer), _c(codebook))


SPEED_ZEROS = 32            # zero crossings of the interpolation kernel on each side (at the cutoff's scale)
SPEED_ROLLOFF = 0.95        # pass band as a fraction of the narrower Nyquist band
SPEED_BETA = 14.769656459379492   # Kaiser window: ~ -150 dB side lobes
RESAMPLE_MAX_SPAN = 12288  # samples a workgroup of csrc/resample.hip stages (48 KiB of LDS): ntap + 2 of them for one output
_SPEED_TABLES = {}


def speed_filter_bank(speed: float):
    """(p, q, table [q, ntap] float64) of the polyphase band-limited interpolator for `speed` = p / q:
    h(t) = c sinc(c t) kaiser(t / W), c = rolloff * min(1, 1 / speed), W = zeros / c input samples; row r holds
    h(r / q - (j - ntap / 2 + 1)) for j = 0 .. ntap - 1."""
    import fractions

    import numpy as np
    fr = fractions.Fraction(str(speed)).limit_denominator(1000)
    p_, q_ = fr.numerator, fr.denominator
    c = SPEED_ROLLOFF * min(1.0, q_ / p_)
    W = SPEED_ZEROS / c
    ntap = 2 * int(math.ceil(W))
    j = np.arange(ntap, dtype=np.float64)[None, :] - (ntap // 2 - 1)          # input offset k - i
    t = np.arange(q_, dtype=np.float64)[:, None] / q_ - j                     # (n s - k)
    win = np.where(np.abs(t) < W, np.i0(SPEED_BETA * np.sqrt(np.clip(1.0 - (t / W) ** 2, 0.0, None))) / np.i0(SPEED_BETA), 0.0)
    return p_, q_, c * np.sinc(c * t) * win


def speed_perturb(wave: torch.Tensor, speed: float) -> torch.Tensor:
    """fp32 waveform [N] on the device played `speed` times faster (pitch and tempo), same sample rate:
    floor(N / speed) samples (touchnet/data/functions.py:99-114: sox `speed` + `rate`)."""
    if not wave.is_cuda or wave.dim() != 1:
        raise RuntimeError("speed_perturb: expects a 1-D device waveform")
    if speed == 1.0:
        return wave
    key = (float(speed), wave.device)
    if key not in _SPEED_TABLES:
        p_, q_, tab = speed_filter_bank(speed)
        if tab.shape[1] + 2 > RESAMPLE_MAX_SPAN:
            raise ValueError(f"speed_perturb: speed = {speed} needs {tab.shape[1]} filter taps, more than the "
                             f"{RESAMPLE_MAX_SPAN - 2} tn_resample_sinc stages for one output")
        _SPEED_TABLES[key] = (p_, q_, torch.from_numpy(tab).to(torch.float32).to(wave.device).contiguous())
    p_, q_, tab = _SPEED_TABLES[key]
    n_out = (wave.numel() * q_) // p_
    return L.resample_sinc(_c(wave).float(), tab, p_, q_, max(n_out, 1))


RESAMPLE_WIDTH = 6          # torchaudio's lowpass_filter_width: zero crossings of the sinc on each side
RESAMPLE_ROLLOFF = 0.99     # torchaudio's rolloff: cutoff as a fraction of the narrower Nyquist band
RESAMPLE_MAX_RATIO = 64     # o / n within [1 / 64, 64] ...
RESAMPLE_MAX_TABLE = 2 ** 22   # ... and at most this many table entries (16 MiB of float32)
_RESAMPLE_TABLES = {}


def _resample_geometry(orig: int, new: int):
    """(o, n, base, width, half): the rates in lowest terms, torchaudio's base_freq and padding width, and half the
    number of columns of its kernel that are not zero"""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1:
        raise ValueError(f"resample: sample rates {orig} -> {new} Hz must be positive")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * RESAMPLE_ROLLOFF
    return o, n, base, int(math.ceil(RESAMPLE_WIDTH * o / base)), int(math.floor(RESAMPLE_WIDTH * o / base)) + 1


def sinc_resample_table(orig: int, new: int):
    """(o, n, ntap, table [n, ntap] float64) of `torchaudio.transforms.Resample(orig, new)` at torchaudio's defaults
    (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), o / n = orig / new in lowest terms.  torchaudio's kernel is
        K[j][k] = sinc(t) cos(t pi / 12)^2 base / o,  t = clamp((-j / n + (k - width) / o) base, -6, 6),
        base = 0.99 min(o, n), width = ceil(6 o / base), j < n, k < 2 width + o,
    applied to the waveform padded by (width, width + o) at stride o.  Row r of the table is phase j = r o^-1 mod n of K
    — the phase of every output m with (m o) mod n = r — cut to the ntap = 2 floor(6 o / base) + 2 columns around input
    floor(m o / n) in the layout of tn_resample_sinc; each entry is K's expression evaluated in K's order at its
    (j, k), and the columns left out are exactly 0 once rounded to float32 (|t| clamps to 6 there, where the window is
    cos(pi / 2)^2 ~ 4e-33)."""
    import numpy as np
    o, n, base, width, half = _resample_geometry(orig, new)
    ntap = 2 * half
    r = np.arange(n, dtype=np.int64)
    j = (r * pow(o, -1, n)) % n if n > 1 else r                               # (j o) mod n = r
    k = (width + (j * o) // n - half + 1)[:, None] + np.arange(ntap, dtype=np.int64)[None, :]
    t = (-j.astype(np.float64)[:, None] / n + (k - width).astype(np.float64) / o) * base
    t = np.clip(t, -float(RESAMPLE_WIDTH), float(RESAMPLE_WIDTH))
    w = np.cos(t * math.pi / RESAMPLE_WIDTH / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        tab = np.where(t == 0, 1.0, np.sin(t) / t) * w * (base / o)
    tab[(k < 0) | (k >= 2 * width + o)] = 0.0                                 # (outside K: the padding's zeros)
    return o, n, ntap, tab


def resample(wave: torch.Tensor, orig: int, new: int) -> torch.Tensor:
    """1-D fp32 or int16 PCM waveform [N] on the device at `orig` Hz -> fp32 [ceil(N new / orig)] at `new` Hz
    (touchnet/data/functions.py:83-96: torchaudio.transforms.Resample(orig, new); int16 is read as v / 32768)."""
    o, n, _, _, half = _resample_geometry(orig, new)
    if o == n:
        return wave
    if o > RESAMPLE_MAX_RATIO * n or n > RESAMPLE_MAX_RATIO * o or n * 2 * half > RESAMPLE_MAX_TABLE:
        raise ValueError(f"resample: {orig} -> {new} Hz needs a ratio within [1/{RESAMPLE_MAX_RATIO}, "
                         f"{RESAMPLE_MAX_RATIO}] and a filter table of at most {RESAMPLE_MAX_TABLE} entries "
                         f"(this one: {n} phases x {2 * half} taps)")
    if not wave.is_cuda or wave.dim() != 1 or wave.numel() == 0 or wave.dtype not in (torch.float32, torch.int16):
        raise RuntimeError("resample: expects a non-empty 1-D fp32 or int16 device waveform")
    key = (o, n, wave.device)
    if key not in _RESAMPLE_TABLES:
        _RESAMPLE_TABLES[key] = torch.from_numpy(sinc_resample_table(o, n)[3]).to(torch.float32).to(wave.device).contiguous()
    n_out = -((-wave.numel() * n) // o)
    return L.resample_sinc(_c(wave), _RESAMPLE_TABLES[key], o, n, n_out)


def feat_augment(feat: torch.Tensor, t_masks=(), f_masks=(), subs=(), out_rows: Optional[int] = None) -> torch.Tensor:
    """fp32 [T, F] -> fp32 [out_rows, F]: zero stripes (spec_aug), row substitutions from earlier rows (spec_sub) and the
    tail trim (spec_trim) of touchnet/data/functions.py:193-255 in one pass; the draws come from the caller."""
    if not feat.is_cuda or feat.dim() != 2:
        raise RuntimeError("feat_augment: expects a 2-D device tensor")
    T = feat.shape[0]
    return L.feat_augment(_c(feat).float(), list(t_masks), list(f_masks), list(subs), T if out_rows is None else int(out_rows))


def audiofeat_stack(feat: torch.Tensor, stack: int, stride: int, normalize: bool = True) -> torch.Tensor:
    """feat fp32 [T, F] -> fp32 [ceil(T/stride), F*stack] (functions.py:258-286)."""
    return L.audiofeat_stack(_c(feat).float(), int(stack), int(stride), bool(normalize))


# ------------------------------------------------------------------------------------ KV-cache decoding (generation.py)
def attn_decode(q, k_new, v_new, k_cache, v_cache, cache_len, scale: Optional[float] = None):
    """Attention of ONE new token per row over a KV cache (the per-token attention of HF generate() with use_cache):
    q [B, Nh, D], k_new / v_new [B, Nkv, D] (q and k rotated), caches bf16 [B, S_max, Nkv, D], cache_len int32 [B].
    k_new / v_new are stored at slot cache_len[b]; returns o [B, Nh, D].  cache_len is advanced by `greedy_step`."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    return L.attn_decode_(q, k_new, v_new, k_cache, v_cache, cache_len, float(scale))


def greedy_step(logits, hist, hist_len, cache_len, finished, n_unfinished, penalty: float = 1.0, ngram: int = 0,
                eos: int = -1, pad: int = 0) -> None:
    """Repetition penalty + no-repeat-n-gram ban + argmax of HF generate() on logits [B, V], appended to the device
    history `hist` [B, S_hist] (int32); advances hist_len / cache_len, marks rows that emitted `eos` finished."""
    L.greedy_step_(logits, hist, hist_len, cache_len, finished, n_unfinished, float(penalty), int(ngram), int(eos), int(pad))


def sample_step(logits, hist, hist_len, cache_len, finished, n_unfinished, penalty: float = 1.0, do_sample: bool = True,
                temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, eos=(), pad: int = 0,
                row_key=None, uniforms=None, n_kept=None) -> None:
    """Repetition penalty, temperature, top-k, top-p and a seeded draw of HF generate() on logits [B, V] (argmax when
    `do_sample` is False), appended to the device history `hist` [B, S_hist] (int32); advances hist_len / cache_len, marks
    rows that emitted one of the `eos` ids (at most 8) finished.  The draw of row b depends only on (seed, row_key[b],
    hist_len[b]); `uniforms` fp32 [B] fixes it instead."""
    eos = [int(e) for e in ([eos] if isinstance(eos, int) else eos)]
    L.sample_step_(logits, hist, hist_len, cache_len, finished, n_unfinished, row_key, uniforms, n_kept, float(penalty),
                   bool(do_sample), float(temperature), int(top_k), float(top_p), int(seed), eos, int(pad))


def kimi_text_step(logits, hist, hist_len, cache_len, finished, n_unfinished, prompt_len, embed, x_next,
                   penalty: float = 1.1, window: int = 16, temperature: float = 0.0, top_k: int = 5, seed: int = 0,
                   eos: int = -1, blank: int = 0, audio_token: Optional[int] = None, row_key=None, uniforms=None) -> None:
    """One text-stream step of Kimi-Audio's `_generate_loop` on logits [B, V]: repetition penalty over the last `window`
    generated ids (only once more than `window` were generated, rounded in the logits' dtype), argmax — or, with
    temperature > 1e-6, a draw among the `top_k` largest — appended to the device history; a finished row emits `blank`;
    rows that emitted `eos` are marked finished.  x_next bf16 [B, H] receives embed[token] + embed[audio_token], the next
    step's input (`audio_token` defaults to `blank`: the audio stream of a text-only generation)."""
    L.kimi_text_step_(logits, hist, hist_len, cache_len, finished, n_unfinished, prompt_len, embed, x_next, row_key,
                      uniforms, float(penalty), int(window), float(temperature), int(top_k), int(seed), int(eos), int(blank),
                      int(blank if audio_token is None else audio_token))


# ------------------------------------------------------------------------------------ beam search (generation.py)
def attn_decode_beam(q, k_new, v_new, k_cache, v_cache, cache_len, src, scale: Optional[float] = None):
    """`attn_decode` for R = B * K beam rows whose caches are shared through an ancestry table: key / value s of row r is
    read at cache[src[r, s], s] (src int32 [R, S_max]) for s < cache_len[r]; k_new / v_new are stored at
    cache[r, cache_len[r]].  Nothing is copied when beams are reordered; `beam_step` maintains the table."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    return L.attn_decode_beam_(q, k_new, v_new, k_cache, v_cache, cache_len, src, float(scale))


EARLY_STOPPING_CODE = {False: 0, True: 1, "never": 2}


def constrain_logits_(logits, hist, hist_len, plan, prompt_len=None, num_beams: int = 1, edits=None) -> None:
    """`sequence_bias` (hotword boosts, forbidden sequences at -inf) and `min_new_tokens` of HF generate() on logits
    [R_in, V], matched against the device history `hist` [R, S_hist] / `hist_len` [R] (tn_logits_constrain).  `plan`: a
    `generation.ConstraintPlan` (its table tensors, `min_new`, `vocab`); `prompt_len` int32 [R] is needed when
    plan.min_new > 0.  Without `edits` the logits are edited in place, in their own dtype: logits[t] = T(fp32(logits[t]) +
    total) — for fp32 logits HF's arithmetic, for bf16 logits the sum rounded to bf16 — and only at ids that a matching
    sequence or the eos rule names.  With `edits` = plan.edit_buffers(rows) the logits are left alone and the per-row edit
    list is written for `beam_step(..., edits=edits)`, which adds it to the log-probabilities (`num_beams`: the beam row
    layout, R_in = R / num_beams right after the prefill).  At most 16384 sequences of at most 64 ids each."""
    if logits.shape[1] < plan.vocab:
        raise ValueError(f"constrain_logits_: the plan was checked against a vocabulary of {plan.vocab} ids, the logits have "
                         f"{logits.shape[1]}")
    e_ids, e_val, e_cnt = edits if edits is not None else (None, None, None)
    L.constrain_logits_(logits, hist, hist_len, prompt_len, plan.seq_off, plan.seq_ids, plan.seq_bias, plan.grp_off,
                        plan.grp_tok, plan.grp_eos, e_ids, e_val, e_cnt, int(num_beams), int(plan.min_new))


def token_scores(logits, tok, k: int = 0):
    """How sure was the model of token tok[r] on logits [R, V] (fp32 / bf16)?  -> (logp fp32 [R] = log_softmax(logits)[r,
    tok[r]] — transformers' compute_transition_scores(..., normalize_logits=True) on `output_logits` —, entropy fp32 [R],
    alt_id int32 [R, k], alt_logp fp32 [R, k]: the k <= 8 most likely ids, descending, ties to the lower id, id -1 / -inf
    behind the V-th).  An id outside [0, V) scores NaN; a row with a NaN, a +inf or nothing but -inf gives NaN and ids -1."""
    return L.token_scores(logits, tok.to(torch.int32), int(k))


def token_scores_(logits, hist, hist_len, out, k: int = 0) -> None:
    """`token_scores` behind a step kernel, without a gather: the token is the newest of the device history, hist[r,
    hist_len[r] - 1], and its scores go to column hist_len[r] - 1 of `out`: an object with logp / entropy fp32 [R, S_hist]
    and, for k > 0, alt_id int32 / alt_logp fp32 [R, S_hist, k] (`generation.TokenScores.buffers`).  Hand it the logits as
    lm_head wrote them, not what a logits processor left of them."""
    k = int(k)
    L.token_scores_(logits, hist, hist_len, out.logp, out.entropy, out.alt_id if k else None, out.alt_logp if k else None, k)


def beam_step(logits, state, penalty: float = 1.0, ngram: int = 0, eos=(), n_new: int = 1, length_penalty: float = 1.0,
              early_stopping=False, edits=None) -> None:
    """One step of HF's beam search (`_beam_search` of transformers) on the device: log_softmax, repetition penalty and
    n-gram ban on the log-probabilities, the top continuations of every utterance, running beams, finished set, early-stop
    heuristic, and the reordering of history and ancestry table by parent.  `state`: an object with the tensors of
    `generation.BeamState` (num_beams, hist, hist_len, cache_len, src, run_score, fin_*, gen, unsat, done, n_unfinished,
    out_ids, out_parent).  logits [B, V] on the first step (one live row per utterance), [B * num_beams, V] afterwards.
    `edits`: the (edit_ids, edit_val, edit_cnt) that `constrain_logits_` wrote for these logits rows; the totals are added
    to the log-probabilities before the repetition penalty (HF's processor order)."""
    if early_stopping not in (True, False, "never"):
        raise ValueError(f"early_stopping must be True, False or 'never' (got {early_stopping!r})")
    eos = [int(e) for e in ([eos] if isinstance(eos, int) else eos)]
    s = state
    if edits is None:
        L.beam_step_(logits, s.hist, s.hist_len, s.cache_len, s.src, s.run_score, s.fin_ids, s.fin_len, s.fin_score,
                     s.fin_flag, s.gen, s.unsat, s.done, s.n_unfinished, s.out_ids, s.out_parent, int(s.num_beams),
                     float(penalty), int(ngram), eos, int(n_new), float(length_penalty),
                     EARLY_STOPPING_CODE[early_stopping])
    else:
        L.beam_step_edits_(logits, s.hist, s.hist_len, s.cache_len, s.src, s.run_score, s.fin_ids, s.fin_len, s.fin_score,
                           s.fin_flag, s.gen, s.unsat, s.done, s.n_unfinished, s.out_ids, s.out_parent, *edits,
                           int(s.num_beams), float(penalty), int(ngram), eos, int(n_new), float(length_penalty),
                           EARLY_STOPPING_CODE[early_stopping])


# ------------------------------------------------------------------------------------ Kimi-Audio speech tokenizer (frozen)
@dataclass
class BlockCausalMask:
    """Device-side form of the speech tokenizer's block-causal key mask (`get_block_causal_attention_mask`,
    touchnet/models/kimi_audio/modeling_kimi_audio.py:226-242) for rows that may hold several clips back to back:
    position t of row b belongs to the clip starting at seg_start[b, t] whose valid keys end at key_end[b, t]."""
    seg_start: torch.Tensor   # int32 [B, T]
    key_end: torch.Tensor     # int32 [B, T]
    block: int
    B: int
    T: int


def block_causal_mask(seg_start: torch.Tensor, key_end: torch.Tensor, block: int) -> BlockCausalMask:
    B, T = seg_start.shape
    return BlockCausalMask(_c(seg_start).to(torch.int32), _c(key_end).to(torch.int32), int(block), B, T)


def block_causal_attention(q, k, v, mask: BlockCausalMask, scale: Optional[float] = None):
    """softmax(scale * Q K^T + block-causal key mask) V, forward only (tn_attn_block_causal_fwd): q / k / v bf16
    [B, T, Nh, 64] -> [B, T, Nh, 64].  Query i of a clip starting at s sees the clip's valid keys j with
    (j - s) // block <= (i - s) // block; padded query rows are ordinary rows."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if tuple(q.shape[:2]) != (mask.B, mask.T):
        raise _C.KernelError(f"mask built for {(mask.B, mask.T)}, got q {tuple(q.shape[:2])}")
    return L.attn_block_causal_fwd(q, k, v, mask.seg_start, mask.key_end, mask.block, float(scale))


def vq_nearest(x: torch.Tensor, codebook: torch.Tensor, cnorm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Nearest codebook row of every row of x (`vector_quantize`, modeling_kimi_audio.py:85-98; tn_vq_nearest): x bf16
    [M, d], codebook bf16 [V, d], d % 64 == 0 -> ids int64 [M], the first index on ties.  `cnorm` = fp32 |c|^2 [V]
    (computed here when None; callers with a frozen codebook pass it once computed)."""
    if cnorm is None:
        cnorm = codebook_sqnorm(codebook)
    return L.vq_nearest(x, codebook, cnorm)


def codebook_sqnorm(codebook: torch.Tensor) -> torch.Tensor:
    """fp32 |c|^2 [V] of a codebook: the per-code constant of the nearest-code distance (once per frozen codebook)."""
    return codebook.detach().float().pow(2).sum(1)


# ===================================================================================================== scoring
EDIT_ALIGN_MAX_LEN = 16383                      # tn_edit_align: a cost fits the 16-bit carry column, a length an int32 table


def edit_align_tables(R, H, workspace_bytes: int = 256 << 20):
    """The launches of a batch of pairs with reference lengths R and hypothesis lengths H (int arrays, already within the
    kernel's limits): [(idx, desc)], idx the pairs of the launch, heaviest first by (R + 64) * ceil(max(H, 1) / 64) — the
    forward kernel's steps of one wave —, desc the int32 [len(idx), 6] table {ref_start, R, hyp_start, H, ws_base, ops_base}
    over tokens packed in that order; no launch's workspace exceeds `workspace_bytes`.  ValueError for a single pair above it."""
    import numpy as np
    R, H = np.asarray(R, dtype=np.int64), np.asarray(H, dtype=np.int64)
    words = np.fromiter((L.edit_align_ws_words(int(r), int(h)) for r, h in zip(R, H)), dtype=np.int64, count=R.size)
    cap = int(workspace_bytes) // 4
    if (words > cap).any():
        p = int(np.argmax(words > cap))
        raise ValueError(f"edit_align: workspace_bytes = {int(workspace_bytes)} is below the {int(words[p]) * 4} bytes that pair "
                         f"{p} ({int(R[p])} x {int(H[p])}) needs")
    order = np.argsort(-((R + 64) * np.maximum((H + 63) // 64, 1)), kind="stable")
    starts = lambda a: np.concatenate([[0], np.cumsum(a)[:-1]])
    tables, first = [], 0
    while first < R.size:
        last, used = first, 0
        while last < R.size and used + words[order[last]] <= cap:
            used += words[order[last]]
            last += 1
        idx = order[first:last]
        r, h, w = R[idx], H[idx], words[idx]
        tables.append((idx, np.stack([starts(r), r, starts(h), h, starts(w), starts(r + h)], axis=1).astype(np.int32)))
        first = last
    return tables


def edit_align(refs, hyps, ref_offsets=None, hyp_offsets=None, *, workspace_bytes: int = 256 << 20, device=None):
    """Edit-distance alignment of P (reference, hypothesis) token pairs with the tie rule of the recipe's scorer
    (touchnet/bin/error_rate_zh:44-149: insertion before deletion before the diagonal; tn_edit_align).

    refs / hyps: lists of int sequences, or packed 1-D int tensors with `ref_offsets` / `hyp_offsets` [P + 1].
    -> a list of (C, S, I, D, ops), one per pair in the input order; ops is a numpy uint8 array of the arcs in path order,
    0 = C, 1 = S, 2 = I, 3 = D.  The score the reference prints is -(S + I + D).

    The pairs go to the device heaviest first ((R + 64) * ceil(max(H, 1) / 64): the forward kernel's steps of one wave),
    in as many launches as keep each launch's direction workspace within `workspace_bytes`; the results come back in
    the input order.  ValueError, by name, for an empty reference, a length above 16383 and a single pair whose
    workspace exceeds `workspace_bytes`."""
    import numpy as np

    def packed(seqs, offsets, what):
        if offsets is None:
            lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            flat = [t for s in seqs for t in s]
            tok = np.asarray(flat, dtype=np.int64) if flat else np.zeros(0, dtype=np.int64)
        else:
            tok = (seqs.detach().cpu().numpy() if isinstance(seqs, torch.Tensor) else np.asarray(seqs)).astype(np.int64).ravel()
            off = (offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)).astype(np.int64)
            if off.ndim != 1 or off.size < 1 or off[0] != 0 or off[-1] != tok.size or (np.diff(off) < 0).any():
                raise ValueError(f"edit_align: {what}_offsets must ascend from 0 to the number of {what} tokens")
        if tok.size and (tok.min() < -2 ** 31 or tok.max() >= 2 ** 31):
            raise ValueError(f"edit_align: {what} token ids must fit int32")
        return tok.astype(np.int32), off

    rtok, roff = packed(refs, ref_offsets, "ref")
    htok, hoff = packed(hyps, hyp_offsets, "hyp")
    P = roff.size - 1
    if hoff.size - 1 != P:
        raise ValueError(f"edit_align: {P} references but {hoff.size - 1} hypotheses")
    if P == 0:
        return []
    R, H = np.diff(roff), np.diff(hoff)
    if (R < 1).any():
        raise ValueError(f"edit_align: empty reference (pair {int(np.argmax(R < 1))}); the scorer skips such utterances")
    if (R > EDIT_ALIGN_MAX_LEN).any() or (H > EDIT_ALIGN_MAX_LEN).any():
        p = int(np.argmax((R > EDIT_ALIGN_MAX_LEN) | (H > EDIT_ALIGN_MAX_LEN)))
        raise ValueError(f"edit_align: length over {EDIT_ALIGN_MAX_LEN} (pair {p}: reference {int(R[p])}, hypothesis {int(H[p])})")
    tables = edit_align_tables(R, H, workspace_bytes)    # (refuses before the device is touched)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    pending = []
    for idx, desc in tables:
        ref_l = np.concatenate([rtok[roff[i]:roff[i + 1]] for i in idx])
        hyp_l = np.concatenate([htok[hoff[i]:hoff[i + 1]] for i in idx])
        counts, ops = L.edit_align(torch.from_numpy(ref_l).to(dev), torch.from_numpy(hyp_l).to(dev), torch.from_numpy(desc))
        pending.append((idx, desc, counts, ops))
    out = [None] * P
    for idx, desc, counts, ops in pending:       # the only synchronisation: the results' way back
        counts, ops = counts.cpu().numpy(), ops.cpu().numpy()
        for k, i in enumerate(idx):
            c, s, ins, d, n = (int(v) for v in counts[k])
            stop = int(desc[k, 5]) + int(desc[k, 1]) + int(desc[k, 3])
            out[int(i)] = (c, s, ins, d, ops[stop - n:stop].copy())
    return out
