"""ASR decoding of a data list with a Qwen2-Audio checkpoint on one MI355X — the command of
touchnet/models/qwen2_audio/inference_qwen2_audio.py (same inputs, same output lines), decoded by touchnet_amd.generation
with the knobs of the checkpoint's generation_config.json.

    python -m touchnet_amd.bin.infer_qwen2_audio --model_path CKPT_DIR --instruct "Generate the transcription:"
        --data_list data.list --output_dir OUT [--batch_size 12] [--max_length 70000] [--max_new_tokens N] [--seed S]
        [--shard_index i --num_shards n]

CKPT_DIR is an HF checkpoint directory: config.json, generation_config.json, *.safetensors and the tokenizer files
(loaded locally with AutoTokenizer).  Parameter names: Qwen2AudioForConditionalGeneration's of transformers 4.51
(`audio_tower.*`, `multi_modal_projector.*`, `language_model.model.*`, `language_model.lm_head.*`) or of transformers 5
(`model.audio_tower.*`, `model.multi_modal_projector.*`, `model.language_model.*`, `lm_head.*`).
`data.list`: one JSON object per line with at least "wav" (16-bit PCM; a rate
other than 16 kHz is resampled on the device, infer_asr.read_wav).  As in the reference, a batch whose longest
prompt exceeds --max_length is skipped; the budget is max_length minus the longest prompt unless the generation config
sets max_new_tokens.  Output: OUT/part_{i+1}_of_{n}, one JSON line per utterance, {"label": the input line, "predict":
text}.  The draws of an utterance are keyed by its line number in the data list, so it decodes the same whatever its
batch or shard.
Hotwords and forbidden words: `--hotwords FILE` (one phrase per line, tokenised with the checkpoint's tokenizer without
special tokens; every token along a phrase gets `--hotword_bias`, default 2.0 — a starting point that nobody has tuned —
once the tokens before it were emitted), `--forbid_words FILE` (phrases whose token sequence can never be completed) and
`--min_new_tokens N` (no eos before N tokens); see generation.hotword_bias and DESIGN 9.6.  They merge with the `sequence_bias` of
generation_config.json: the file's entries first, then the hotwords, then the forbidden phrases.
Confidences and N-best lists: `--output_scores` adds "confidence", "token_logprobs" and "token_entropy" to every record
(one entry per generated token up to and including the eos), `--top_alternatives K` adds "alternatives" ([[id, logp], ...]
per token), `--nbest N` (beam search with at least N beams) adds "nbest", the N best finished hypotheses with their ids;
see DESIGN 9.7.  Without these flags the output file is what it was.
Long recordings: `--long_form` cuts a recording longer than `--max_segment_s` (30: what the feature extractor keeps) into
segments with an energy VAD on the device (`--vad_*`, untuned defaults; infer_asr's docstring and DESIGN 9.9), decodes
them pooled and writes the "predict" of their concatenation plus "segments".  Segment i of line n draws with the key
n + (i + 1) 2^40 and a sampled run decodes one segment per call, so it does not depend on --batch_size.  Other records
are what they were.
"""
from __future__ import annotations

import argparse
import glob
import json
import os

import torch

from touchnet_amd.bin.infer_asr import read_wav
from touchnet_amd.generation import (GenerationConfig, add_constraint_arguments, add_longform_arguments,
                                     add_score_arguments, constraints_from_args)
from touchnet_amd.longform import longform_from_args, qwen2_audio_decoder, transcribe_long
from touchnet_amd.models.qwen2_audio import Qwen2AudioConfig, Qwen2AudioPackedForConditionalGeneration
from touchnet_amd.models.qwen2_audio.inference_qwen2_audio import build_prompts, transcribe, valid_frames
from touchnet_amd.models.qwen2_audio.processing_qwen2_audio import DEFAULT_INSTRUCT

# transformers 5 names -> the 4.51 names the packed model keeps
_RENAMES = (("model.audio_tower.", "audio_tower."), ("model.multi_modal_projector.", "multi_modal_projector."),
            ("model.language_model.", "language_model.model."), ("lm_head.", "language_model.lm_head."))


def hf_names(sd: dict) -> dict:
    out = {}
    for k, v in sd.items():
        for old, new in _RENAMES:
            if k.startswith(old):
                k = new + k[len(old):]
                break
        out[k] = v
    return out


def load_model(model_path: str, device) -> Qwen2AudioPackedForConditionalGeneration:
    from safetensors.torch import load_file
    with open(os.path.join(model_path, "config.json")) as f:
        d = json.load(f)
    cfg = Qwen2AudioConfig.from_dict(d)
    for k in ("pad_token_id", "bos_token_id", "eos_token_id"):      # (top-level ids of an HF config reach the decoder)
        if getattr(cfg.text_config, k) is None and d.get(k) is not None:
            setattr(cfg.text_config, k, d[k])
    model = Qwen2AudioPackedForConditionalGeneration(cfg)
    files = sorted(glob.glob(os.path.join(model_path, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no *.safetensors in {model_path}")
    sd = {}
    for f in files:
        sd.update(load_file(f))
    missing, unexpected = model.load_state_dict(hf_names(sd), strict=False)
    tied = cfg.text_config.tie_word_embeddings
    missing = [k for k in missing if not (k == "language_model.lm_head.weight" and tied)]
    if missing or unexpected:
        raise RuntimeError(f"checkpoint does not match Qwen2-Audio: missing {missing}, unexpected {unexpected}")
    if tied:
        model.language_model.tie_weights()
    return model.to(device).to(torch.bfloat16).eval()


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--instruct", default=DEFAULT_INSTRUCT)
    ap.add_argument("--data_list", required=True)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--max_length", type=int, default=70000)
    ap.add_argument("--max_new_tokens", type=int, default=None, help="overrides the budget (default: HF's rule)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num_beams", type=int, default=None, help="overrides the checkpoint's generation config")
    ap.add_argument("--length_penalty", type=float, default=None)
    ap.add_argument("--early_stopping", default=None, choices=["true", "false", "never"])
    ap.add_argument("--shard_index", type=int, default=0)
    ap.add_argument("--num_shards", type=int, default=1)
    add_constraint_arguments(ap)
    add_score_arguments(ap)
    add_longform_arguments(ap)
    return ap


def generation_config(args, tokenizer=None) -> GenerationConfig:
    over = dict(max_length=args.max_length, seed=args.seed)
    if args.output_scores or args.top_alternatives or args.nbest != 1:
        over.update(output_scores=args.output_scores, top_alternatives=args.top_alternatives, nbest=args.nbest)
    if args.num_beams is not None:
        over["num_beams"] = args.num_beams
    if args.length_penalty is not None:
        over["length_penalty"] = args.length_penalty
    if args.early_stopping is not None:
        over["early_stopping"] = {"true": True, "false": False}.get(args.early_stopping, "never")
    gen_file = os.path.join(args.model_path, "generation_config.json")
    cfg = GenerationConfig.from_hf(gen_file if os.path.exists(gen_file) else {}, **over)
    if args.max_new_tokens is not None:
        cfg.max_new_tokens = args.max_new_tokens
    cfg.sequence_bias = constraints_from_args(args, tokenizer, cfg.sequence_bias)
    if args.min_new_tokens is not None:
        cfg.min_new_tokens = args.min_new_tokens
    return cfg


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("infer_qwen2_audio needs the MI355X (there is no CPU path)")
    from transformers import AutoTokenizer
    device = torch.device("cuda", torch.cuda.current_device())
    model = load_model(args.model_path, device)
    tokenizer = AutoTokenizer.from_pretrained(args.model_path)
    cfg = generation_config(args, tokenizer)
    long_cfg = longform_from_args(args)
    to_text = lambda r: tokenizer.decode(r, skip_special_tokens=True, clean_up_tokenization_spaces=False)
    with open(args.data_list) as f:
        items = [(n, json.loads(line)) for n, line in enumerate(f) if line.strip()]
    items = items[args.shard_index::args.num_shards]
    os.makedirs(args.output_dir, exist_ok=True)
    out_path = os.path.join(args.output_dir, f"part_{args.shard_index + 1}_of_{args.num_shards}")
    with open(out_path, "w") as writer:
        for i in range(0, len(items), args.batch_size):
            batch = items[i:i + args.batch_size]
            wavs = [read_wav(it["wav"]) for _, it in batch]
            longest = max(len(p) for p in build_prompts(tokenizer, [valid_frames(w.numel()) for w in wavs],
                                                        args.instruct).input_ids)
            if longest > args.max_length:
                print(f"longest prompt {longest} > max_length {args.max_length}, skip")
                continue
            keys = torch.tensor([n for n, _ in batch], dtype=torch.int64)
            if long_cfg is not None:
                done = transcribe_long(qwen2_audio_decoder(model, tokenizer, args.instruct, cfg), wavs, 16000, long_cfg,
                                       args.batch_size, row_keys=keys.tolist(), to_text=to_text, nbest=cfg.nbest,
                                       output_scores=cfg.wants_scores, sampled=cfg.do_sample, device=device)
                texts, extras = [d["predict"] for d in done], [d["extra"] for d in done]
            else:
                _, texts, extras = transcribe(model, wavs, tokenizer, args.instruct, cfg, row_keys=keys, details=True)
            for (_, it), text, extra in zip(batch, texts, extras):
                writer.write(json.dumps({"label": json.dumps(it, ensure_ascii=False), "predict": text, **extra},
                                        ensure_ascii=False) + "\n")
    return out_path


if __name__ == "__main__":
    main()
