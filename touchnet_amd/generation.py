"""Greedy decoding with a KV cache on the HIP kernels — what the reference gets from HF `generate()` in
touchnet/models/touch_audio/inference_touch_audio.py:177-192 (use_cache=True, do_sample=False, num_beams=1,
repetition_penalty=1.5, no_repeat_ngram_size=2, max_new_tokens=256, eos / pad).

    prefill   the packed, document-masked forward of the training path under no_grad: ONE packed row, one document per
              prompt (no left padding); only the last slot of every document reaches lm_head (`keep_rows`), and every
              layer hands out its rotated keys and values (`kv_out`), which are scattered into the caches
    step      per layer RMSNorm -> q/k/v projection with RoPE at the per-row position -> tn_attn_decode (appends the new
              key / value and attends over the cache) -> o_proj -> RMSNorm -> SwiGLU MLP; final norm, lm_head on B rows,
              tn_greedy_step (repetition penalty, n-gram ban, argmax, history / length bookkeeping on the device)

There is no host synchronisation inside the loop: the host reads the count of unfinished rows every `check_every` steps.
Device state invariant after every greedy step: cache_len[b] = hist_len[b] - 1 (the newest token is not cached yet; its
position is cache_len[b]).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from . import _C
from . import functional as F


@dataclass
class GenerationConfig:
    """The knobs of the reference's generate() call (top_k / top_p / temperature are inert there: do_sample=False)."""
    max_new_tokens: int = 256
    repetition_penalty: float = 1.5
    no_repeat_ngram_size: int = 2
    eos_token_id: Optional[int] = None       # None: the model config's
    pad_token_id: Optional[int] = None
    bos_token_id: Optional[int] = None
    check_every: int = 16                    # steps between two host reads of the unfinished count


@dataclass
class Prompts:
    """One prompt per utterance: token ids int64 [n_b] and, for TouchAudio, feature rows [n_b, F] (projected and added to
    the token embeddings; zero rows contribute nothing).  Positions are 0 .. n_b - 1."""
    input_ids: List[torch.Tensor]
    input_features: Optional[List[torch.Tensor]] = None

    def __len__(self):
        return len(self.input_ids)


@dataclass
class KVCache:
    """L layers of keys / values [B, S_max, Nkv, D] bf16, S_max = longest prompt + max_new_tokens, and the per-row device
    state of the greedy loop (all int32): cache_len [B], hist [B, S_max] (prompt ids then generated ids), hist_len [B],
    finished [B], n_unfinished [1]."""
    k: List[torch.Tensor]
    v: List[torch.Tensor]
    cache_len: torch.Tensor
    hist: torch.Tensor
    hist_len: torch.Tensor
    finished: torch.Tensor
    n_unfinished: torch.Tensor

    @classmethod
    def allocate(cls, num_layers: int, B: int, S_max: int, Nkv: int, D: int, device, dtype=torch.bfloat16) -> "KVCache":
        z = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=device)
        return cls(k=[torch.empty(B, S_max, Nkv, D, dtype=dtype, device=device) for _ in range(num_layers)],
                   v=[torch.empty(B, S_max, Nkv, D, dtype=dtype, device=device) for _ in range(num_layers)],
                   cache_len=z(B), hist=z(B, S_max), hist_len=z(B), finished=z(B), n_unfinished=z(1))


def _parts(model):
    """-> (PackedCausalLM, projector weight or None) of a TouchAudioForCausalLM or a plain PackedCausalLM."""
    lm = getattr(model, "language_model", None)
    if lm is not None:
        return lm, model.projector.weight
    return model, None


def _special(cfg: GenerationConfig, lm):
    c = lm.config
    eos = cfg.eos_token_id if cfg.eos_token_id is not None else c.eos_token_id
    pad = cfg.pad_token_id if cfg.pad_token_id is not None else c.pad_token_id
    if isinstance(eos, (list, tuple)):
        if len(eos) != 1:
            raise ValueError("generate: one eos id only")
        eos = eos[0]
    if pad is None:
        pad = eos if eos is not None else 0        # (HF: pad defaults to eos)
    return (-1 if eos is None else int(eos)), int(pad)


def _check_model(model, lm):
    p = lm.model.embed_tokens.weight
    if not p.is_cuda:
        raise _C.KernelError("generate: the model must live on the MI355X (device tensors only; there is no CPU path)")
    if p.dtype != torch.bfloat16:
        raise _C.KernelError("generate: bf16 model weights only (the KV cache and tn_attn_decode are bf16)")
    D, Nh, Nkv = lm.config.head_dim, lm.config.num_attention_heads, lm.config.num_key_value_heads
    if D not in (64, 128) or Nh % Nkv or Nh // Nkv > 16:
        raise _C.KernelError(f"generate: head_dim {D} with {Nh}/{Nkv} heads is not a decode geometry "
                             "(D 64 / 128, Nh % Nkv == 0, Nh / Nkv <= 16)")


def _prefill(lm, proj_w, prompts: Prompts, cache: KVCache, device):
    """Packed forward over all prompts (one row, one document each) -> logits [B, V] of every prompt's last position;
    keys / values of every layer scattered into the caches."""
    lens = [int(t.numel()) for t in prompts.input_ids]
    B, T = len(lens), sum(lens)
    Tp = (T + 255) // 256 * 256
    ids = torch.zeros(Tp, dtype=torch.int64)
    pos = torch.zeros(Tp, dtype=torch.int64)
    doc = torch.zeros(Tp, dtype=torch.int32)
    src = []
    o = 0
    for b, t in enumerate(prompts.input_ids):
        n = lens[b]
        ids[o:o + n] = t.reshape(-1).cpu()
        pos[o:o + n] = torch.arange(n)
        doc[o:o + n] = b + 1
        src.append(torch.arange(n) + o)
        o += n
    last = torch.tensor([sum(lens[:b + 1]) - 1 for b in range(B)], dtype=torch.int64)
    S_max = cache.k[0].shape[1]
    dst = torch.cat([torch.arange(n) + b * S_max for b, n in enumerate(lens)])
    ids, pos, doc, last, src, dst = (x.to(device, non_blocking=True) for x in (ids, pos, doc, last, torch.cat(src), dst))
    emb = lm.model.embed_tokens(ids)                                                       # [Tp, H]
    if proj_w is not None and prompts.input_features is not None:
        feats = torch.zeros(Tp, proj_w.shape[1], dtype=proj_w.dtype, device=device)
        o = 0
        for b, f in enumerate(prompts.input_features):
            if f.shape[0] != lens[b]:
                raise ValueError(f"prompt {b}: {f.shape[0]} feature rows for {lens[b]} ids")
            feats[o:o + lens[b]] = f.to(device=device, dtype=proj_w.dtype)
            o += lens[b]
        emb = torch.addmm(emb, feats, proj_w.t())              # embed(ids) + projector(features): TouchAudio's forward
    kv = []
    h = lm.model(inputs_embeds=emb[None], position_ids=pos[None], attention_mask=doc[None], keep_rows=last, kv_out=kv)
    for (k, v), kc, vc in zip(kv, cache.k, cache.v):
        Nkv, D = k.shape[2], k.shape[3]
        kc.view(-1, Nkv, D).index_copy_(0, dst, k[0].index_select(0, src))
        vc.view(-1, Nkv, D).index_copy_(0, dst, v[0].index_select(0, src))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=device)
    cache.hist.view(-1).index_copy_(0, torch.cat([torch.arange(n, device=device) + b * cache.hist.shape[1]
                                                  for b, n in enumerate(lens)]), ids.index_select(0, src).to(torch.int32))
    cache.hist_len.copy_(lens_d)
    cache.cache_len.copy_(lens_d - 1)        # the greedy step counts the prompt's last row (see the module docstring)
    cache.finished.zero_()
    cache.n_unfinished.fill_(B)
    return lm.lm_head(h[0])                                                                # [B, V]


def _decode_layer(layer, delta, residual, cos, sin, kc, vc, cache_len):
    attn = layer.self_attn
    B = delta.shape[0]
    if residual is None:
        residual = delta
        x = layer.input_layernorm(delta)
    else:
        x, residual = layer.input_layernorm(delta, residual)
    q, k, v = F.linear_group(x, [(attn.q_proj.weight, attn.q_proj.bias), (attn.k_proj.weight, attn.k_proj.bias),
                                 (attn.v_proj.weight, attn.v_proj.bias)], rope=(cos, sin, attn.head_dim, (0, 1)))
    D = attn.head_dim
    o = F.attn_decode(q.view(B, attn.num_heads, D), k.view(B, attn.num_kv_heads, D), v.view(B, attn.num_kv_heads, D),
                      kc, vc, cache_len, attn.scaling)
    a = F.linear_group(o.view(B, attn.num_heads * D), [(attn.o_proj.weight, None)])[0]
    x, residual = layer.post_attention_layernorm(a, residual)
    return layer.mlp(x), residual


def decode_logits(lm, cache: KVCache) -> torch.Tensor:
    """One decode step of every row: the newest token of the history at position cache_len -> logits [B, V]
    (its key / value are appended to the caches; cache_len itself is advanced by the greedy step)."""
    tok = cache.hist.gather(1, (cache.hist_len.to(torch.int64) - 1)[:, None])[:, 0]
    x = lm.model.embed_tokens(tok.to(torch.int64))                                          # [B, H]
    cos, sin = lm.model.rotary_emb(cache.cache_len.to(torch.int64), x.dtype)
    delta, residual = x, None
    for layer, kc, vc in zip(lm.model.layers, cache.k, cache.v):
        delta, residual = _decode_layer(layer, delta, residual, cos, sin, kc, vc, cache.cache_len)
    h, _ = lm.model.norm(delta, residual)
    return lm.lm_head(h)


@torch.no_grad()
def generate(model, prompts: Prompts, cfg: Optional[GenerationConfig] = None, return_cache: bool = False):
    """Greedy generation for a batch of prompts -> int64 [B, N] generated ids (the prompt excluded), `pad` after a row's
    `eos` — the tensor HF generate() returns behind the prompt columns.  `model`: TouchAudioForCausalLM or
    PackedCausalLM, bf16, on the device."""
    cfg = cfg or GenerationConfig()
    lm, proj_w = _parts(model)
    _check_model(model, lm)
    if len(prompts) == 0:
        raise ValueError("generate: no prompts")
    if any(int(t.numel()) == 0 for t in prompts.input_ids):
        raise ValueError("generate: empty prompt")
    device = lm.model.embed_tokens.weight.device
    eos, pad = _special(cfg, lm)
    c = lm.config
    B = len(prompts)
    lens = [int(t.numel()) for t in prompts.input_ids]
    n_new = int(cfg.max_new_tokens)
    if n_new <= 0:
        return torch.empty(B, 0, dtype=torch.int64, device=device)
    S_max = max(lens) + n_new
    cache = KVCache.allocate(len(lm.model.layers), B, S_max, c.num_key_value_heads, c.head_dim, device)
    penalty, ngram = float(cfg.repetition_penalty), int(cfg.no_repeat_ngram_size)
    logits = _prefill(lm, proj_w, prompts, cache, device)
    F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, penalty, ngram,
                  eos, pad)
    steps = 1
    while steps < n_new:
        if steps % max(1, int(cfg.check_every)) == 0 and int(cache.n_unfinished.item()) == 0:
            break
        logits = decode_logits(lm, cache)
        F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, penalty,
                      ngram, eos, pad)
        steps += 1
    idx = torch.tensor(lens, dtype=torch.int64, device=device)[:, None] + torch.arange(steps, device=device)[None]
    out = cache.hist.gather(1, idx).to(torch.int64)
    # HF stops at the first step after which every row is finished: drop the all-pad columns the check interval added
    if eos >= 0:
        is_eos = (out == eos)
        first = torch.where(is_eos.any(1), is_eos.to(torch.int8).argmax(1), torch.full_like(out[:, 0], steps - 1))
        out = out[:, :int(first.max()) + 1]
    return (out, cache) if return_cache else out


def trim_at_eos(ids: torch.Tensor, eos: int) -> List[List[int]]:
    """[B, N] generated ids -> per row the ids in front of the first eos (the eos and the padding behind it dropped)."""
    rows = []
    for r in ids.tolist():
        rows.append(r[:r.index(eos)] if eos in r else r)
    return rows
