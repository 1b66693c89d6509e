"""Kimi-Audio's speech tokenizer on the MI355X kernels: GLM-4-voice's `WhisperVQEncoder`
(touchnet/models/kimi_audio/modeling_kimi_audio.py:140-319, configuration_kimi_audio.py:9-43), frozen, forward only.

  stem      CausalConv1d(mel -> d, k 3) + GELU, CausalConv1d(d -> d, k 3, stride 2) + GELU (:101-137, left pad 2), then the
            LEARNED position table embed_positions[:T]
  layers    `quantize_position` pre-LN Whisper encoder layers (the Qwen2-Audio tower's EncoderLayer) whose self-attention
            takes the block-causal key mask of :226-242: allowed(i, j) = m[j] and j // block <= i // block,
            m = attention_mask[:, ::2] (tn_attn_block_causal_fwd)
  pooling   after layer `pooling_position` (= the last): right zero-pad to a multiple of the kernel, avg / max pool
  quantise  ids = argmin_c |c|^2 - 2 x . c over codebook.weight (:85-98; tn_vq_nearest).  embed_positions2 is added only
            after the ids are taken (:317): it does not affect them, and the ids are all the model reads (:957-963).

A k = 3 conv with left pad 2 equals the symmetric pad-1 conv of the input shifted right by one zero frame (output t reads
frames t s - 2 .. t s either way), so the stem runs on the hand-written conv1d_k3 GEMM path of the Qwen2-Audio tower.

Trimming (exact): the stem is causal, the attention block-causal, everything else per frame; pooled token k reads frames
p k .. p k + p - 1, which see frames of blocks <= (p k + p - 1) // block only.  A clip whose first K tokens are read needs
its first min(T, block * ceil(p K / block)) frames; `forward(.., clip_tokens=[K per clip])` runs the layers on exactly
those, packed clip after clip into one row (the kernel's per-position clip start / key end; `packed_layout`), and
returns 0 for the ids past K.  Without `clip_tokens` every clip runs all T frames (the reference's schedule).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as TF

from ..backend import ops
from ..qwen2_audio.modeling_qwen2_audio import AudioEncoderConfig, EncoderAttention, EncoderLayer


@dataclass
class WhisperVQConfig:
    """configuration_kimi_audio.py:9-43 (WhisperVQConfig's own defaults) over transformers' WhisperConfig defaults for the
    encoder keys; keys this path does not use are ignored."""
    num_mel_bins: int = 80
    d_model: int = 384
    encoder_attention_heads: int = 6
    encoder_ffn_dim: int = 1536
    max_source_positions: int = 1500
    activation_function: str = "gelu"
    init_std: float = 0.02
    pooling_kernel_size: Optional[int] = 4
    pooling_type: str = "avg"
    pooling_position: Optional[int] = 16
    quantize_vocab_size: Optional[int] = 16384
    quantize_position: int = 16
    quantize_ema_decay: Optional[float] = 0.99
    quantize_encoder_only: bool = True
    quantize_causal_block_size: Optional[int] = 200
    encoder_causal_convolution: bool = True

    @classmethod
    def from_dict(cls, d: Optional[dict]) -> "WhisperVQConfig":
        names = {f.name for f in fields(cls)}
        cfg = cls(**{k: v for k, v in (d or {}).items() if k in names})
        cfg.validate()
        return cfg

    def validate(self):
        """What the reference asserts (:164, :171, :187, :197-200, :274) or cannot run, refused up front."""
        bad = []
        if not self.encoder_causal_convolution:
            bad.append("encoder_causal_convolution must be true (:163-164)")
        if not self.quantize_encoder_only:
            bad.append("quantize_encoder_only must be true (:170-171)")
        if self.quantize_causal_block_size is None:
            bad.append("quantize_causal_block_size must be set (:274-276)")
        elif int(self.quantize_causal_block_size) < 1:
            bad.append("quantize_causal_block_size must be >= 1")
        if self.quantize_vocab_size is None:
            bad.append("quantize_vocab_size must be set (:197)")
        if self.pooling_kernel_size is None:
            bad.append("pooling_kernel_size must be set (:187)")
        if self.pooling_type not in ("avg", "max"):
            bad.append(f"pooling_type {self.pooling_type!r}: avg or max (:188-193)")
        if self.pooling_position != self.quantize_position:
            bad.append("pooling_position must equal quantize_position: the reference builds its mask at the unpooled "
                       "length, so layers after the pooling cannot run there")
        if self.activation_function != "gelu":
            bad.append(f"activation_function {self.activation_function!r}: the encoder layers run exact-erf GELU")
        if self.d_model % self.encoder_attention_heads or self.d_model // self.encoder_attention_heads != 64:
            bad.append("head_dim d_model / encoder_attention_heads must be 64 (tn_attn_block_causal_fwd)")
        if bad:
            raise ValueError("speech_tokenizer_config: " + "; ".join(bad))

    def encoder_dims(self) -> AudioEncoderConfig:
        return AudioEncoderConfig(num_mel_bins=self.num_mel_bins, d_model=self.d_model, encoder_layers=self.quantize_position,
                                  encoder_attention_heads=self.encoder_attention_heads, encoder_ffn_dim=self.encoder_ffn_dim,
                                  max_source_positions=self.max_source_positions, init_std=self.init_std)


def needed_frames(tokens: int, T: int, block: int, pool: int) -> int:
    """Post-conv frames a clip needs so that its first `tokens` pooled ids are exact (module docstring)."""
    if tokens <= 0:
        return 0
    return min(T, block * -(-pool * tokens // block))


class BlockCausalAttention(EncoderAttention):
    """EncoderAttention (same parameters) with the tokenizer's block-causal key mask (functional.BlockCausalMask)."""

    def attend(self, q, k, v, mask):
        return ops().block_causal_attention(q, k, v, mask, self.head_dim ** -0.5)


class WhisperVQEncoder(nn.Module):
    """Parameter and buffer names of the reference's module, so `speech_tokenizer.*` of a Kimi-Audio checkpoint loads
    with strict=True.  Always frozen."""

    def __init__(self, cfg: WhisperVQConfig):
        super().__init__()
        self.config = cfg
        d, V = cfg.d_model, cfg.quantize_vocab_size
        enc = cfg.encoder_dims()
        self.conv1 = nn.Conv1d(cfg.num_mel_bins, d, kernel_size=3)
        self.conv2 = nn.Conv1d(d, d, kernel_size=3, stride=2)
        self.embed_positions = nn.Embedding(cfg.max_source_positions, d)
        self.layers = nn.ModuleList([EncoderLayer(enc) for _ in range(cfg.quantize_position)])
        for layer in self.layers:
            old = layer.self_attn
            layer.self_attn = BlockCausalAttention(d, cfg.encoder_attention_heads)
            layer.self_attn.load_state_dict(old.state_dict())
        self.codebook = nn.Embedding(V, d)
        self.embed_positions2 = nn.Embedding(math.ceil(cfg.max_source_positions / cfg.pooling_kernel_size), d)
        if cfg.quantize_ema_decay is not None:                                  # (:210-213; unused at inference)
            self.register_buffer("ema_count", torch.ones(V, dtype=torch.float))
            self.register_buffer("ema_weight", torch.zeros(V, d, dtype=torch.float))
        self.requires_grad_(False)
        self._cnorm = None
        self._apply(lambda t: t)                                                 # (parameters in bf16 from the start)

    def reset_parameters(self):
        """The reference's post-init relations: embed_positions2 starts as embed_positions[:n] (:207-208), ema_weight as
        the codebook (:213)."""
        with torch.no_grad():
            n = self.embed_positions2.weight.shape[0]
            self.embed_positions2.weight.copy_(self.embed_positions.weight[:n])
            if hasattr(self, "ema_weight"):
                self.ema_weight.copy_(self.codebook.weight.float())
        self._cnorm = None

    def _apply(self, fn, recurse=True):
        """The kernels take bf16 weights and the tokenizer is frozen, so its parameters are bf16 wherever the model is
        placed: after `.to()`, `.float()`, `to_empty()` and the like they are rounded here, once per placement (a
        data-parallel engine leaves frozen parameters in the dtype the model held, utils/zero_dp.py).  The EMA buffers
        keep the placement's dtype; nothing reads them."""
        super()._apply(fn, recurse)
        for prm in self.parameters():
            if prm.is_floating_point() and prm.dtype != torch.bfloat16:
                prm.data = prm.data.to(torch.bfloat16)
        self._cnorm = None
        return self

    def _check_weights(self):
        if self.conv1.weight.dtype != torch.bfloat16 or self.codebook.weight.dtype != torch.bfloat16:
            raise ValueError("WhisperVQEncoder runs from bf16 weights (set at placement, `_apply`); got "
                             f"{self.conv1.weight.dtype} / {self.codebook.weight.dtype}")

    def _codebook_norms(self):
        w = self.codebook.weight
        key = (w.data_ptr(), w._version)
        if self._cnorm is None or self._cnorm[0] != key:
            self._cnorm = (key, ops().codebook_sqnorm(w))
        return self._cnorm[1]

    def stem(self, input_features, frames: Optional[int] = None):
        """mel [n, bins, Tm] -> [n, T, d] (T = `frames` or Tm / 2) after the causal conv stem and the position table."""
        n, _, Tm = input_features.shape
        T = Tm // 2 if frames is None else frames
        x = input_features[:, :, :2 * T].to(torch.bfloat16).transpose(1, 2)       # [n, 2T, bins]
        x = TF.pad(x, (0, 0, 1, 0))                                               # causal: one zero frame in front
        h, _ = ops().conv1d_k3(x, self.conv1.weight, self.conv1.bias, 1, need_dx=False)
        h = TF.pad(ops().gelu(h[:, :2 * T]), (0, 0, 1, 0))
        h, _ = ops().conv1d_k3(h, self.conv2.weight, self.conv2.bias, 2, need_dx=False)
        h = ops().gelu(h[:, :T])
        return h + self.embed_positions.weight[:T][None].to(h.dtype)

    def _layers(self, h, mask):
        delta, residual = None, h
        for layer in self.layers:
            delta, residual = layer(delta, residual, mask)
        return residual + delta

    @staticmethod
    def key_lengths(attention_mask, n, Tm, device):
        """valid post-conv frames per clip: m = attention_mask[:, ::2] (:273), a prefix of the clip -> int32 [n]"""
        if attention_mask is None:
            return torch.full((n,), (Tm + 1) // 2, dtype=torch.int32, device=device)
        return attention_mask[:, ::2].to(device).sum(-1).to(torch.int32)

    @torch.no_grad()
    def hidden_states(self, input_features, attention_mask=None):
        """The reference's schedule up to the pooling: every clip on all T = Tm / 2 frames -> [n, T, d] bf16."""
        self._check_weights()
        n, _, Tm = input_features.shape
        if Tm % 2:
            raise ValueError("WhisperVQEncoder: an even number of mel frames (the reference's seq_length = Tm // 2, :271)")
        h = self.stem(input_features)
        T = h.shape[1]
        kl = self.key_lengths(attention_mask, n, Tm, h.device)
        mask = ops().block_causal_mask(torch.zeros(n, T, dtype=torch.int32, device=h.device),
                                       kl[:, None].expand(n, T).contiguous(), self.config.quantize_causal_block_size)
        return self._layers(h, mask)

    def _pool(self, h):
        """[rows, p, d] -> [rows, d]: the reference's AvgPool1d / MaxPool1d over one window"""
        if self.config.pooling_type == "avg":
            return h.float().mean(1).to(h.dtype)
        return h.amax(1)

    @torch.no_grad()
    def pooled(self, input_features, attention_mask=None, clip_tokens: Optional[List[int]] = None):
        """The states the quantiser sees -> (x bf16 [rows, d], slots): without `clip_tokens` every id of every clip
        (rows = n * S in order, slots None); with them the first clip_tokens[i] ids of clip i, slots int64 [rows] = their
        flat index into [n, S]."""
        self._check_weights()
        cfg = self.config
        p, block = cfg.pooling_kernel_size, cfg.quantize_causal_block_size
        n, _, Tm = input_features.shape
        if Tm % 2:
            raise ValueError("WhisperVQEncoder: an even number of mel frames (the reference's seq_length = Tm // 2, :271)")
        T = Tm // 2
        S = -(-T // p)
        if clip_tokens is None:
            h = self.hidden_states(input_features, attention_mask)                 # [n, T, d]
            if T % p:
                h = TF.pad(h, (0, 0, 0, p - T % p))                                # (:305-307: zeros behind the clip)
            return self._pool(h.reshape(n * S, p, -1)), None
        if len(clip_tokens) != n:
            raise ValueError(f"clip_tokens: {len(clip_tokens)} counts for {n} clips")
        lay = packed_layout(clip_tokens, T, block, p)
        dev = input_features.device
        if lay.rows == 0:
            return input_features.new_empty(0, cfg.d_model, dtype=torch.bfloat16), torch.zeros(0, dtype=torch.int64, device=dev)
        host = torch.tensor(lay.src + lay.clip + lay.start + lay.cap + lay.taps + lay.slots, dtype=torch.int64)
        buf = host.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else host.to(dev)
        R, nt = lay.rows, len(lay.slots)
        src_d, clip_d, start_d, cap_d = (buf[i * R:(i + 1) * R] for i in range(4))
        taps_d, slots_d = buf[4 * R:4 * R + p * nt], buf[4 * R + p * nt:]
        h = self.stem(input_features, lay.frames)                                   # [n, Tk, d]
        d = h.shape[-1]
        hp = h.reshape(n * lay.frames, d).index_select(0, src_d)[None]               # [1, R, d]
        kl = self.key_lengths(attention_mask, n, Tm, dev).to(torch.int64)
        key_end = torch.minimum(start_d + kl.index_select(0, clip_d), cap_d)
        mask = ops().block_causal_mask(start_d.to(torch.int32)[None], key_end.to(torch.int32)[None], block)
        hp = TF.pad(self._layers(hp, mask)[0], (0, 0, 0, 1))                        # [R + 1, d]: row R is the zero pad
        return self._pool(hp.index_select(0, taps_d).view(nt, p, d)), slots_d

    @torch.no_grad()
    def forward(self, input_features, attention_mask=None, clip_tokens: Optional[List[int]] = None):
        """mel [n, bins, Tm] (+ attention_mask [n, Tm], 1 on the first L frames of a clip; None = all valid) -> ids int64
        [n, ceil(Tm / 2 / p)].  `clip_tokens` (host ints, one per clip): only those first ids are needed; the layers then
        run on the frames they depend on and the ids past them are 0.  No host synchronisation either way."""
        n, _, Tm = input_features.shape
        S = -(-(Tm // 2) // self.config.pooling_kernel_size)
        x, slots = self.pooled(input_features, attention_mask, clip_tokens)
        got = ops().vq_nearest(x, self.codebook.weight, self._codebook_norms()) if x.shape[0] else x.new_empty(0, dtype=torch.int64)
        if slots is None:
            return got.view(n, S)
        ids = torch.zeros(n * S, dtype=torch.int64, device=input_features.device)
        return ids.index_copy_(0, slots, got).view(n, S)


@dataclass
class PackedLayout:
    """Host-side layout of the trimmed schedule's packed row (`packed_layout`)."""
    frames: int          # post-conv frames the stem computes per clip (the largest need)
    rows: int            # rows of the packed row
    src: List[int]       # per row: source row in the stem's [n * frames] output
    clip: List[int]      # per row: clip index
    start: List[int]     # per row: first row of its clip
    cap: List[int]       # per row: end of its clip's kept frames (no key at or past it)
    taps: List[int]      # p per read id: packed rows pooled into it; `rows` = the zero row behind the packed row
    slots: List[int]     # per read id: flat index into [n, S]


def packed_layout(clip_tokens: List[int], T: int, block: int, pool: int, align: int = 64) -> PackedLayout:
    """Clip c keeps needed_frames(K_c) frames; each clip starts at a multiple of `align` (the attention's key tile), so a
    clip's keys are grouped into tiles exactly as in its own padded row.  The rows between a clip's kept frames and the
    next start repeat its last kept frame: they are queries only (`cap` keeps them out of every key range) and are never
    pooled.  A pooling window reaching past the clip's T frames reads the zero row, the reference's right zero-padding
    (:305-307)."""
    S = -(-T // pool)
    K = [min(max(int(k), 0), S) for k in clip_tokens]
    need = [needed_frames(k, T, block, pool) for k in K]
    Tk = max(need, default=0)
    src, clip, start, cap, taps, slots = [], [], [], [], [], []
    off = 0
    for c, (k, f) in enumerate(zip(K, need)):
        if f == 0:
            continue
        span = -(-f // align) * align
        src += [c * Tk + min(t, f - 1) for t in range(span)]
        clip += [c] * span
        start += [off] * span
        cap += [off + f] * span
        taps += [off + t if t < f else -1 for t in range(pool * k)]
        slots += range(c * S, c * S + k)
        off += span
    taps = [t if t >= 0 else off for t in taps]
    return PackedLayout(Tk, off, src, clip, start, cap, taps, slots)
