"""ASR decoding of a data list with a Kimi-Audio checkpoint on one MI355X — the command of
touchnet/models/kimi_audio/inference_kimi_audio.py (same inputs, same output lines), decoded by
touchnet_amd.models.kimi_audio.inference_kimi_audio.generate_kimi with the defaults of the reference's generate().

    python -m touchnet_amd.bin.infer_kimi_audio --model_path CKPT_DIR --instruct "Generate the transcription:"
        --data_list data.list --output_dir OUT [--batch_size 12] [--max_new_tokens 2048] [--text_temperature 0.0]
        [--text_top_k 5] [--text_repetition_penalty 1.1] [--text_repetition_window_size 16] [--seed S]
        [--shard_index i --num_shards n]

CKPT_DIR is an HF checkpoint directory: config.json (the keys of Kimi-Audio-7B.json, with `speech_encoder_config` and
`speech_tokenizer_config`), *.safetensors under MoonshotKimiaForCausalLM's parameter names (`model.*`, `lm_head.*`,
`mimo_output.*`, `speech_encoder.*`, `speech_tokenizer.*`) and the tokenizer files (loaded locally with AutoTokenizer,
trust_remote_code as in the reference).  `data.list`: one JSON object per line with at least "wav" (16-bit PCM; a rate
other than 16 kHz is resampled on the device, infer_asr.read_wav).
Output: OUT/part_{i+1}_of_{n}, one JSON line per utterance, {"label": the input line, "predict": text}.  The draws of a
sampled run are keyed by the utterance's line number in the data list, so it decodes the same whatever its batch or shard.
Long recordings: `--long_form` cuts a recording longer than `--max_segment_s` (30: what the feature extractor keeps) into
segments with an energy VAD on the device (`--vad_*`, untuned defaults; infer_asr's docstring and DESIGN 9.9), decodes
them pooled and writes the "predict" of their concatenation plus "segments".  Segment i of line n draws with the key
n + (i + 1) 2^40, and a sampled run (--text_temperature above 1e-6) decodes one segment per call.  Other records, and
every record without the flag, are what they were.
"""
from __future__ import annotations

import argparse
import glob
import json
import os

import torch

from touchnet_amd.bin.infer_asr import read_wav
from touchnet_amd.generation import KimiGenerationConfig, add_longform_arguments, add_score_arguments
from touchnet_amd.longform import kimi_audio_decoder, longform_from_args, transcribe_long
from touchnet_amd.models.kimi_audio import KimiAudioConfig, KimiAudioPackedForCausalLM
from touchnet_amd.models.kimi_audio.inference_kimi_audio import transcribe
from touchnet_amd.models.kimi_audio.processing_kimi_audio import BLANK, DEFAULT_INSTRUCT, EOS


def load_model(model_path: str, device) -> KimiAudioPackedForCausalLM:
    from safetensors.torch import load_file
    with open(os.path.join(model_path, "config.json")) as f:
        cfg = KimiAudioConfig.from_dict(json.load(f))
    model = KimiAudioPackedForCausalLM(cfg)
    files = sorted(glob.glob(os.path.join(model_path, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no *.safetensors in {model_path}")
    sd = {}
    for f in files:
        sd.update(load_file(f))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if missing or unexpected:
        raise RuntimeError(f"checkpoint does not match Kimi-Audio: missing {missing}, unexpected {unexpected}")
    return model.to(device).to(torch.bfloat16).eval()


def special_id(tokenizer, token: str, default: int) -> int:
    """The id the tokenizer gives a special token of the prompt format; the id KimiASampler hard-codes where it has none."""
    to_id = getattr(tokenizer, "convert_tokens_to_ids", None)
    i = to_id(token) if to_id is not None else None
    return int(default) if i is None or i == getattr(tokenizer, "unk_token_id", None) else int(i)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--instruct", default=DEFAULT_INSTRUCT)
    ap.add_argument("--data_list", required=True)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--max_new_tokens", type=int, default=2048, help="-1: 7500 minus the longest prompt")
    ap.add_argument("--text_temperature", type=float, default=0.0)
    ap.add_argument("--text_top_k", type=int, default=5)
    ap.add_argument("--text_repetition_penalty", type=float, default=1.1)
    ap.add_argument("--text_repetition_window_size", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--shard_index", type=int, default=0)
    ap.add_argument("--num_shards", type=int, default=1)
    add_score_arguments(ap, nbest=False)
    add_longform_arguments(ap)
    return ap


def generation_config(args) -> KimiGenerationConfig:
    return KimiGenerationConfig(text_temperature=args.text_temperature, text_top_k=args.text_top_k,
                                text_repetition_penalty=args.text_repetition_penalty,
                                text_repetition_window_size=args.text_repetition_window_size,
                                max_new_tokens=args.max_new_tokens, seed=args.seed, output_scores=args.output_scores,
                                top_alternatives=args.top_alternatives)


def main(argv=None):
    args = build_parser().parse_args(argv)
    cfg = generation_config(args)
    long_cfg = longform_from_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("infer_kimi_audio needs the MI355X (there is no CPU path)")
    from transformers import AutoTokenizer
    device = torch.device("cuda", torch.cuda.current_device())
    model = load_model(args.model_path, device)
    tokenizer = AutoTokenizer.from_pretrained(args.model_path, trust_remote_code=True)
    cfg.kimia_text_blank = special_id(tokenizer, BLANK, cfg.kimia_text_blank)
    cfg.kimia_text_eos = special_id(tokenizer, EOS, cfg.kimia_text_eos)
    with open(args.data_list) as f:
        items = [(n, json.loads(line)) for n, line in enumerate(f) if line.strip()]
    items = items[args.shard_index::args.num_shards]
    os.makedirs(args.output_dir, exist_ok=True)
    out_path = os.path.join(args.output_dir, f"part_{args.shard_index + 1}_of_{args.num_shards}")
    with open(out_path, "w") as writer:
        for i in range(0, len(items), args.batch_size):
            batch = items[i:i + args.batch_size]
            wavs = [read_wav(it["wav"]) for _, it in batch]
            keys = torch.tensor([n for n, _ in batch], dtype=torch.int64)
            if long_cfg is not None:
                to_text = getattr(tokenizer, "detokenize", None) or tokenizer.decode
                done = transcribe_long(kimi_audio_decoder(model, tokenizer, args.instruct, cfg), wavs, 16000, long_cfg,
                                       args.batch_size, row_keys=keys.tolist(), to_text=to_text,
                                       output_scores=cfg.wants_scores, sampled=cfg.text_temperature > 1e-6, device=device)
                texts, extras = [d["predict"] for d in done], [d["extra"] for d in done]
            else:
                _, texts, extras = transcribe(model, wavs, tokenizer, args.instruct, cfg, row_keys=keys, details=True)
            for (_, it), text, extra in zip(batch, texts, extras):
                writer.write(json.dumps({"label": json.dumps(it, ensure_ascii=False), "predict": text, **extra},
                                        ensure_ascii=False) + "\n")
    return out_path


if __name__ == "__main__":
    main()
