"""ASR transcription with a Qwen2-Audio checkpoint — the decode half of touchnet/models/qwen2_audio/inference_qwen2_audio.py
on the HIP path (touchnet_amd.generation), with the decoding knobs of the checkpoint's generation_config.json
(`GenerationConfig.from_hf`).

Per utterance, as the reference builds it (:94-120):
  features  128-bin log-mel of the waveform zero-padded / truncated to 30 s (WhisperFeatureExtractor(padding="max_length",
            truncation=True)), computed on the device; valid frames L = the extractor's attention_mask sum
  prompt    TEMPLATE_S2T with the instruction, <|AUDIO|> expanded to ((L - 1) // 2 + 1 - 2) // 2 + 1 tokens, tokenised
            without padding
  prefill   audio_tower.forward_valid over the batch's clips -> multi_modal_projector -> index_copy into the AUDIO positions
            of the packed prompt row (one document per utterance), then the decoder with keep_rows / kv_out
The reference left-pads the batch with pad = <|endoftext|>: here no padding enters a prompt.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from ...generation import GenerationConfig, Prompts, eos_ids, generate, record_fields
from ..backend import ops
from .processing_qwen2_audio import DEFAULT_INSTRUCT, HOP, TEMPLATE_S2T, WHISPER_FRAMES, audio_token_count

N_MELS = 128
SAMPLES = WHISPER_FRAMES * HOP                     # 30 s at 16 kHz


def valid_frames(num_samples: int) -> int:
    """The attention_mask sum of WhisperFeatureExtractor(padding="max_length", truncation=True) for a clip of that many
    samples: its sample mask taken every 160th sample, over the clip truncated to 30 s."""
    return -(-min(int(num_samples), SAMPLES) // HOP)


def features(wavs: Sequence[torch.Tensor], device) -> Tuple[torch.Tensor, List[int]]:
    """Waveforms (int16 PCM or float in [-1, 1), 16 kHz) -> log-mel fp32 [n, 128, 3000] on the device and the valid frames
    of each clip."""
    out, valid = [], []
    for w in wavs:
        w = w.reshape(-1)[:SAMPLES].to(device)
        w = ops().pcm16_to_float(w) if w.dtype == torch.int16 else w.float()
        valid.append(valid_frames(w.numel()))
        out.append(ops().log_mel_spectrogram(w, N_MELS, padding=SAMPLES - w.numel())[:WHISPER_FRAMES].t())
    return torch.stack(out), valid


def prompt_ids(tokenizer, n_audio: int, instruct: str = DEFAULT_INSTRUCT) -> List[int]:
    """The reference's prompt (:111-120): the S2T template, <|AUDIO|> expanded n_audio times, no padding."""
    text = TEMPLATE_S2T.replace("<|INSTRUCT|>", instruct)
    text = text.replace("<|AUDIO|>", "<|AUDIO|>" * int(n_audio), 1)
    ids = tokenizer(text, padding=False)["input_ids"]
    if ids and isinstance(ids[0], (list, tuple)):
        ids = ids[0]
    return [int(i) for i in ids]


def build_prompts(tokenizer, valid: Sequence[int], instruct: str = DEFAULT_INSTRUCT) -> Prompts:
    return Prompts(input_ids=[torch.tensor(prompt_ids(tokenizer, audio_token_count(L), instruct), dtype=torch.int64)
                              for L in valid])


def audio_embedder(model, mel: torch.Tensor, valid: Sequence[int], prompts: Prompts):
    """The prefill's embedding builder: embed(ids) with the tower's rows written at the AUDIO positions of the packed row —
    the training forward's code path (forward_valid, projector, index_copy)."""
    audio_id = int(model.config.audio_token_index)
    out_len = [audio_token_count(L) for L in valid]
    pos, o = [], 0
    for b, t in enumerate(prompts.input_ids):
        t = t.reshape(-1)
        p = (t == audio_id).nonzero().reshape(-1)
        if p.numel() != out_len[b]:
            raise ValueError(f"utterance {b}: {p.numel()} AUDIO tokens in the prompt for {out_len[b]} audio frames")
        pos.append(p + o)
        o += t.numel()
    lm = model.language_model

    def embed(ids, lens, Tp):
        device = ids.device
        positions = torch.cat(pos).to(device, non_blocking=True)
        lengths = torch.tensor(out_len, dtype=torch.int64).to(device, non_blocking=True)
        emb = lm.model.embed_tokens(ids)
        feats = model.multi_modal_projector(model.audio_tower.forward_valid(mel.to(device), lengths, positions.numel()))
        return emb.index_copy(0, positions, feats.to(emb.dtype))

    # the same builder for other documents over the same clips, each clip `repeat` times in a row (generation.
    # score_continuations: prompt + hypothesis, one document per returned hypothesis)
    embed.for_documents = lambda documents, repeat=1: audio_embedder(
        model, mel.repeat_interleave(repeat, 0), [L for L in valid for _ in range(repeat)], documents)
    return embed


def transcribe(model, wavs: Sequence[torch.Tensor], tokenizer, instruct: str = DEFAULT_INSTRUCT,
               cfg: Optional[GenerationConfig] = None, row_keys: Optional[torch.Tensor] = None, details: bool = False):
    """Transcripts of a batch of utterances -> (per utterance the generated ids cut at the first eos, their text decoded
    with skip_special_tokens=True).  `row_keys` int64 [B] key the draws when sampling (default: the batch index).
    `details`: a third element, per utterance the extra record keys that cfg.output_scores / top_alternatives / nbest ask
    for (generation.record_fields; every "nbest" entry with its "predict")."""
    cfg = cfg or GenerationConfig.from_hf({})
    device = model.language_model.model.embed_tokens.weight.device
    mel, valid = features(wavs, device)
    prompts = build_prompts(tokenizer, valid, instruct)
    out = generate(model, prompts, cfg, row_keys=row_keys, embed=audio_embedder(model, mel, valid, prompts))
    ids, extras = record_fields(out, cfg, eos_ids(cfg, model.language_model))
    decode = lambda r: tokenizer.decode(r, skip_special_tokens=True, clean_up_tokenization_spaces=False)
    texts = [decode(r) for r in ids]
    if not details:
        return ids, texts
    for extra in extras:
        if "nbest" in extra:
            extra["nbest"] = [{"predict_ids": h["predict_ids"], "predict": decode(h["predict_ids"]),
                               **{k: v for k, v in h.items() if k != "predict_ids"}} for h in extra["nbest"]]
    return ids, texts, extras
