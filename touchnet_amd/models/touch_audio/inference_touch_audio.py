"""ASR transcription with a LlamaForASR (TouchAudioForCausalLM) checkpoint — the decode half of
touchnet/models/touch_audio/inference_touch_audio.py on the HIP path (touchnet_amd.generation).

Prompt of one utterance (`feature_extraction`, :51-100 there): its n stacked feature rows plus one zero row; ids
pad x n followed by bos; positions 0 .. n; embedding = embed(ids) + projector(features).  The reference left-pads the
batch to a rectangle; here every prompt is its own document of one packed row, so no padding enters the computation.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from ...generation import GenerationConfig, Prompts, generate, record_fields


def build_prompts(feats: List[torch.Tensor], pad_token_id: int, bos_token_id: int) -> Prompts:
    """[n_i, F] stacked features per utterance -> Prompts (ids pad x n_i + bos, features + one zero row)."""
    ids, fs = [], []
    for f in feats:
        n = int(f.shape[0])
        fs.append(torch.cat([f, f.new_zeros(1, f.shape[1])], dim=0))
        ids.append(torch.tensor([pad_token_id] * n + [bos_token_id], dtype=torch.int64))
    return Prompts(input_ids=ids, input_features=fs)


def prompt_positions(prompts: Prompts) -> List[torch.Tensor]:
    """Positions of every prompt: 0 .. len - 1 (restarting per utterance, as in the reference's unpadded rows)."""
    return [torch.arange(int(t.numel()), dtype=torch.int64) for t in prompts.input_ids]


def _special_ids(model, cfg: GenerationConfig):
    tc = model.config.text_config
    pad = cfg.pad_token_id if cfg.pad_token_id is not None else (
        model.config.pad_token_id if model.config.pad_token_id is not None else tc.pad_token_id)
    bos = cfg.bos_token_id if cfg.bos_token_id is not None else tc.bos_token_id
    eos = cfg.eos_token_id if cfg.eos_token_id is not None else tc.eos_token_id
    if isinstance(eos, (list, tuple)):
        eos = eos[0]
    if pad is None or bos is None or eos is None:
        raise ValueError("transcribe: pad / bos / eos token ids are needed (GenerationConfig or the model config)")
    return int(pad), int(bos), int(eos)


def transcribe(model, feats: List[torch.Tensor], cfg: Optional[GenerationConfig] = None, details: bool = False):
    """Greedy (or, with cfg.num_beams > 1, beam-search) transcripts of a batch of utterances -> per utterance the
    generated ids (the prompt excluded), cut in front of the first eos.  `details`: (those ids, per utterance the extra
    record keys that cfg.output_scores / top_alternatives / nbest ask for — generation.record_fields)."""
    cfg = cfg or GenerationConfig()
    pad, bos, eos = _special_ids(model, cfg)
    gcfg = GenerationConfig(max_new_tokens=cfg.max_new_tokens, repetition_penalty=cfg.repetition_penalty,
                            no_repeat_ngram_size=cfg.no_repeat_ngram_size, eos_token_id=eos, pad_token_id=pad,
                            bos_token_id=bos, check_every=cfg.check_every, num_beams=cfg.num_beams,
                            length_penalty=cfg.length_penalty, early_stopping=cfg.early_stopping,
                            sequence_bias=cfg.sequence_bias, min_new_tokens=cfg.min_new_tokens,
                            output_scores=cfg.output_scores, top_alternatives=cfg.top_alternatives, nbest=cfg.nbest)
    out = generate(model, build_prompts(feats, pad, bos), gcfg)
    ids, extras = record_fields(out, gcfg, [eos])
    return (ids, extras) if details else ids
