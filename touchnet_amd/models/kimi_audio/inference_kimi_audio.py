"""ASR transcription with a Kimi-Audio checkpoint — touchnet/models/kimi_audio/inference_kimi_audio.py:92-145 and
MoonshotKimiaForCausalLM.generate / _generate_loop (modeling_kimi_audio.py:1084-1214) on the HIP path.

Per utterance, as the reference builds it:
  features  128-bin log-mel of the waveform zero-padded / truncated to 30 s, on the device (Qwen2-Audio's frontend); valid
            frames L; `attention_mask[:, ::2][:, ::4].sum()` = ceil(L / 8) audio tokens
  prompts   two aligned id streams from the S2T templates: the text stream carries the instruction, the audio stream
            blanks in its place; both carry ceil(L / 8) blanks for <|AUDIO|> (between the media markers in the audio stream)
  input     embed(audio ids), the positions between the markers replaced by `prepare_audio_input_embs` (speech encoder,
            VQ adaptor, embeddings of the speech tokenizer's ids — the tokenizer runs trimmed to the ids that are read),
            plus embed(text ids)
  prefill   the packed, document-masked forward: one row, one document per utterance, no padding; `keep_rows` = every
            prompt's last row, `kv_out` into the KV cache (generation._prefill)
  step      generation.decode_logits on the row tn_kimi_text_step wrote (embed[text token] + embed[blank]), then
            tn_kimi_text_step: windowed repetition penalty, argmax or top-k draw, history, finished rows, next input row

generate() never asks `_generate_loop` for audio output, so every audio-stream token is the blank and `mimo_output`'s
logits are computed only to be dropped: the six mimo layers and the second 168 448-way head are not run here.  The
reference left-pads a batch with the pad id and hands the decoder no attention mask, so its pads are attended; here no
padding enters a prompt (results are the reference's at batch size 1 or with prompts of one length).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from ... import functional as F
from ... import generation as G
from ...generation import KimiGenerationConfig, KVCache, Prompts
from ..qwen2_audio.inference_qwen2_audio import features  # noqa: F401  (128-bin device log-mel, valid frames per clip)
from .processing_kimi_audio import AUDIO_TEMPLATE_S2T, BLANK, DEFAULT_INSTRUCT, TEXT_TEMPLATE_S2T, WHISPER_FRAMES


@dataclass
class KimiPrompts:
    """One prompt per utterance as two aligned id streams (int64 [n_b] each), and — for a model with the audio-input side —
    the clips' log-mel [B, n_mels, frames] with the valid frames of each clip (one media-marker pair per utterance)."""
    text_ids: List[torch.Tensor]
    audio_ids: List[torch.Tensor]
    whisper_input_features: Optional[torch.Tensor] = None
    valid_frames: Optional[List[int]] = None

    def __len__(self):
        return len(self.text_ids)


def audio_token_count(valid_frames: int) -> int:
    """`attention_mask[:, ::2][:, ::4].sum()` of the reference's script (:100) for a clip with that many valid frames."""
    return -(-int(valid_frames) // 8)


def _ids(tokenizer, text: str) -> List[int]:
    enc = tokenizer(text, add_special_tokens=False)
    ids = enc["input_ids"] if isinstance(enc, dict) else enc.input_ids
    return [int(i) for i in ids]


def build_prompts(tokenizer, instruct: str, num_audio_tokens: Sequence[int]) -> KimiPrompts:
    """The reference's two prompt streams (:102-120) for utterances with those audio-token counts, without its left
    padding."""
    n_task = len(_ids(tokenizer, instruct))
    text, audio = [], []
    for n in num_audio_tokens:
        tp = TEXT_TEMPLATE_S2T.replace("<|INSTRUCT|>", instruct).replace("<|AUDIO|>", BLANK * int(n))
        ap = AUDIO_TEMPLATE_S2T.replace("<|INSTRUCT|>", BLANK * n_task).replace("<|AUDIO|>", BLANK * int(n))
        t, a = _ids(tokenizer, tp), _ids(tokenizer, ap)
        if len(t) != len(a):
            raise ValueError(f"text / audio prompt streams differ in length: {len(t)} vs {len(a)}")
        text.append(torch.tensor(t, dtype=torch.int64))
        audio.append(torch.tensor(a, dtype=torch.int64))
    return KimiPrompts(text_ids=text, audio_ids=audio)


class _Stack:
    """KimiDecoderModel as generation._prefill / decode_logits drive a decoder: the text stream's hidden states only."""

    def __init__(self, model):
        self._model = model
        self.embed_tokens, self.layers, self.norm, self.rotary_emb = (model.embed_tokens, model.layers, model.norm,
                                                                      model.rotary_emb)

    def __call__(self, **kw):
        return self._model(**kw)[0]


class _TextDecoder:
    def __init__(self, model):
        self.config, self.lm_head, self.model = model.config, model.lm_head, _Stack(model.model)


def kimi_embedder(model, prompts: KimiPrompts):
    """The prefill's embedding builder: generation._prefill packs the TEXT stream (it is the history the step kernel
    extends); this adds the packed audio stream's embeddings with the speech positions filled in."""
    cfg = model.config
    audio = torch.cat([a.reshape(-1) for a in prompts.audio_ids])
    mel, valid = prompts.whisper_input_features, prompts.valid_frames
    if mel is not None:
        if model.speech_encoder is None or model.speech_tokenizer is None:
            raise ValueError("whisper_input_features need a model with the speech encoder and the speech tokenizer "
                             "(use_whisper_feature and speech_tokenizer_config)")
        if valid is None or len(valid) != len(prompts) or mel.shape[0] != len(prompts):
            raise ValueError("whisper_input_features: one clip and one valid-frame count per utterance")
        clip_tokens = [audio_token_count(L) for L in valid]
        for b, a in enumerate(prompts.audio_ids):
            a = a.reshape(-1)
            nb, ne = (a == cfg.kimia_media_begin).nonzero().reshape(-1), (a == cfg.kimia_media_end).nonzero().reshape(-1)
            if nb.numel() != 1 or ne.numel() != 1 or int(ne) - int(nb) - 1 != clip_tokens[b]:
                raise ValueError(f"utterance {b}: the audio stream needs one media marker pair around {clip_tokens[b]} "
                                 "positions")

    def embed(text_ids, lens, Tp):
        device = text_ids.device
        emb = model.model.embed_tokens
        a = torch.zeros(Tp, dtype=torch.int64)
        a[:audio.numel()] = audio
        a = a.to(device, non_blocking=True)
        x = emb(a)
        if mel is not None:
            feats = mel.to(device)
            frames = feats.shape[-1]
            mask = (torch.arange(frames)[None] < torch.tensor(list(valid))[:, None]).to(torch.int32).to(device)
            sp_ids = model.speech_tokenizer(feats, mask, clip_tokens=clip_tokens)
            x = model.prepare_audio_input_embs(a[None], x[None], feats, sp_ids)[0]
        return x + emb(text_ids)
    return embed


@torch.no_grad()
def generate_kimi(model, prompts: KimiPrompts, cfg: Optional[KimiGenerationConfig] = None,
                  row_keys: Optional[torch.Tensor] = None, return_raw: bool = False, return_scores: bool = False):
    """MoonshotKimiaForCausalLM.generate() for a batch of prompts -> per utterance the text ids it returns: what the row
    emitted before its `<|im_kimia_text_eos|>`, blanks and ids >= kimia_token_offset dropped.  `model`:
    KimiAudioPackedForCausalLM, bf16, on the device.  `row_keys` int64 [B] (default arange(B)) key the draws of a sampled
    run with cfg.seed and the step.  `return_raw`: also the raw tokens int64 [B, steps] of every step (eos and blanks
    included) and the KV cache.  `return_scores`, cfg.output_scores or cfg.top_alternatives > 0: a generation.TokenScores
    over the raw tokens [B, steps] (one tn_token_scores launch per step on lm_head's logits) comes back as the last
    element; its confidence covers a row's tokens up to and including its eos."""
    cfg = cfg or KimiGenerationConfig()
    cfg.check()
    scored = bool(return_scores) or cfg.wants_scores
    n_alt = int(cfg.top_alternatives)
    lm = _TextDecoder(model)
    G._check_model(model, lm)
    B = len(prompts)
    if B == 0:
        raise ValueError("generate_kimi: no prompts")
    lens = [int(t.numel()) for t in prompts.text_ids]
    if any(n == 0 for n in lens) or lens != [int(a.numel()) for a in prompts.audio_ids]:
        raise ValueError("generate_kimi: every prompt needs two non-empty id streams of one length")
    c = model.config
    w = lm.model.embed_tokens.weight.detach()
    device = w.device
    blank, eos = int(cfg.kimia_text_blank), int(cfg.kimia_text_eos)
    if not 0 <= blank < c.vocab_size:
        raise ValueError(f"generate_kimi: kimia_text_blank {blank} is outside the vocabulary ({c.vocab_size})")
    n_new = cfg.new_tokens(max(lens))
    if n_new <= 0 and scored:
        raise ValueError("generate_kimi: no room for a new token: nothing to score")
    if n_new <= 0:
        return ([[] for _ in range(B)], torch.empty(B, 0, dtype=torch.int64, device=device), None) if return_raw \
            else [[] for _ in range(B)]
    if row_keys is None:
        row_keys = torch.arange(B, dtype=torch.int64, device=device)
    row_keys = row_keys.to(device=device, dtype=torch.int64).contiguous()
    if tuple(row_keys.shape) != (B,):
        raise ValueError(f"generate_kimi: row_keys must have shape [{B}]")
    chunk = max(1, int(cfg.cache_chunk))
    cache = KVCache.allocate(len(lm.model.layers), B, max(lens) + min(n_new, chunk), c.num_key_value_heads, c.head_dim,
                             device)
    S_full = max(lens) + n_new
    prompt_len = torch.tensor(lens, dtype=torch.int32, device=device)
    x_next = torch.empty(B, c.hidden_size, dtype=torch.bfloat16, device=device)
    scores = G.TokenScores.buffers(B, cache.capacity, n_alt, device) if scored else None

    def step(logits):
        F.kimi_text_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished,
                         prompt_len, w, x_next, cfg.text_repetition_penalty, cfg.text_repetition_window_size,
                         cfg.text_temperature, cfg.text_top_k, cfg.seed, eos, blank, blank, row_key=row_keys)
        if scored:                                 # the token the step kernel has just appended, in its history column
            F.token_scores_(logits, cache.hist, cache.hist_len, scores, n_alt)

    step(G._prefill(lm, None, Prompts(input_ids=list(prompts.text_ids)), cache, device, kimi_embedder(model, prompts)))
    steps = 1
    while steps < n_new:
        if steps % max(1, int(cfg.check_every)) == 0 and int(cache.n_unfinished.item()) == 0:
            break
        if max(lens) + steps >= cache.capacity:
            cache.grow(min(S_full, 2 * cache.capacity))
            if scored:
                scores.grow(cache.capacity)
        step(G.decode_logits(lm, cache, inputs_embeds=x_next))
        steps += 1
    idx = prompt_len.to(torch.int64)[:, None] + torch.arange(steps, device=device)[None]
    raw = cache.hist.gather(1, idx).to(torch.int64)
    off = int(c.kimia_token_offset)
    out = [[t for t in row if t != blank and t != eos and t < off] for row in raw.tolist()]
    if scored:
        result = scores.columns(idx).close(G._generated_lengths(raw, [eos]))
        return (out, raw, cache, result) if return_raw else (out, result)
    return (out, raw, cache) if return_raw else out


def transcribe(model, wavs: Sequence[torch.Tensor], tokenizer, instruct: str = DEFAULT_INSTRUCT,
               cfg: Optional[KimiGenerationConfig] = None, row_keys: Optional[torch.Tensor] = None, details: bool = False):
    """Transcripts of a batch of utterances (int16 PCM or float waveforms, 16 kHz) -> (the text ids generate() returns,
    their text: `tokenizer.detokenize(ids)` as in the reference's script, `decode` where a tokenizer has no such method).
    `details`: a third element, per utterance the extra record keys that cfg.output_scores / top_alternatives ask for
    (generation.score_fields): the per-token lists cover the tokens that are text — what `ids` holds —, the confidence
    every raw token up to and including the eos."""
    device = model.model.embed_tokens.weight.device
    mel, valid = features(wavs, device)
    if mel.shape[-1] != WHISPER_FRAMES:
        raise ValueError(f"features: {mel.shape[-1]} frames, expected {WHISPER_FRAMES}")
    prompts = build_prompts(tokenizer, instruct, [audio_token_count(L) for L in valid])
    prompts.whisper_input_features, prompts.valid_frames = mel, list(valid)
    to_text = getattr(tokenizer, "detokenize", None) or tokenizer.decode
    cfg = cfg or KimiGenerationConfig()
    if not cfg.wants_scores:
        ids = generate_kimi(model, prompts, cfg, row_keys=row_keys)
        texts = [to_text(r) for r in ids]
        return (ids, texts, [{} for _ in ids]) if details else (ids, texts)
    ids, raw, _, scores = generate_kimi(model, prompts, cfg, row_keys=row_keys, return_raw=True)
    blank, eos, off = int(cfg.kimia_text_blank), int(cfg.kimia_text_eos), int(model.config.kimia_token_offset)
    n_tok = G._generated_lengths(raw, [eos]).tolist()
    extras = [G.score_fields(scores, b, keep=[c for c, t in enumerate(row[:n_tok[b]]) if t != blank and t != eos and t < off])
              for b, row in enumerate(raw.tolist())]
    texts = [to_text(r) for r in ids]
    return (ids, texts, extras) if details else (ids, texts)
