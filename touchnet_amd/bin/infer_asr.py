"""Greedy ASR decoding of a data list with a LlamaForASR (TouchAudioForCausalLM) checkpoint on one MI355X — the command of
touchnet/models/touch_audio/inference_touch_audio.py (same inputs, same output lines), decoded by touchnet_amd.generation.

    python -m touchnet_amd.bin.infer_asr --model_path CKPT_DIR --data_list data.list --output_dir OUT [--batch_size 12]
        [--shard_index i --num_shards n]

CKPT_DIR holds HF-format `*.safetensors` (the parameter names of TouchAudioForCausalLM are Hugging Face's) and a model
config (`config.json` in the directory, else `../../model_config.json` as the reference reads it); the data config comes
from `--data_config` or `CKPT_DIR/../../data_config.json` (fbank, 80 bins, stacking to the projector width when absent;
`audio_feat_type` fbank, mfcc or log_mel_spectrogram as the reference's command takes them).
`data.list`: one JSON object per line with at least "key" and "wav" (16-bit PCM wav of any sample rate; other rates
than the data config's `audio_resample_rate`, 16 kHz by default, are resampled on the device, see read_wav).  Output:
OUT/part_{i+1}_of_{n}, one JSON line per utterance: {"label": the input line, "predict_ids": [...], "predict": text} —
"predict" only when CKPT_DIR has a tokenizer.  One GPU per process; `--shard_index / --num_shards` split the list
without collectives.
Hotwords and forbidden words: `--hotwords FILE` (one phrase per line, tokenised with the checkpoint's tokenizer without
special tokens; every token along a phrase gets `--hotword_bias`, default 2.0 — a starting point that nobody has tuned —
once the tokens before it were emitted), `--forbid_words FILE` (phrases whose token sequence can never be completed) and
`--min_new_tokens N` (no eos before N tokens); see generation.hotword_bias and DESIGN 9.6.  A phrase file needs the
tokenizer: without one in CKPT_DIR the command refuses.
Confidences and N-best lists: `--output_scores` adds "confidence", "token_logprobs" and "token_entropy" to every record
(one entry per generated token up to and including the eos), `--top_alternatives K` adds "alternatives" ([[id, logp], ...]
per token), `--nbest N` (with --num_beams >= N) adds "nbest", the N best finished hypotheses; see DESIGN 9.7.  Without
these flags the output file is what it was.
Long recordings: `--long_form` cuts a recording longer than `--max_segment_s` (30) into segments with an energy VAD on the
device (`--vad_*`: Kaldi's compute-vad-energy defaults and common segmenting values, which nobody has tuned for this use),
decodes the segments of a batch pooled, and writes "predict_ids" / "predict" of their concatenation plus "segments"
(start, end in seconds and each segment's own fields); see longform.transcribe_long and DESIGN 9.9.  Records of shorter
recordings, and every record without the flag, are what they were.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import types
import wave

import numpy as np
import torch

from touchnet_amd.data import functions as stages
from touchnet_amd.generation import (GenerationConfig, add_constraint_arguments, add_longform_arguments,
                                     add_score_arguments, constraints_from_args)
from touchnet_amd.longform import longform_from_args, touch_audio_decoder, transcribe_long
from touchnet_amd.models.backend import ops
from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
from touchnet_amd.models.touch_audio.inference_touch_audio import transcribe

_DATA_DEFAULTS = dict(audio_feat_type="fbank", audiofeat_num_mel_bins=80, audiofeat_dither=0.0, audiofeat_frame_length=25,
                      audiofeat_frame_shift=10, audiofeat_n_fft=400, audiofeat_hop_length=160, audiofeat_padding=0,
                      audiofeat_stack_length=None, audiofeat_stride_length=None, audiofeat_normalize=True,
                      audio_resample_rate=16000, audiofeat_num_ceps=40, audiofeat_low_freq=20.0, audiofeat_high_freq=0.0)


def _first(*paths):
    for p in paths:
        if p and os.path.exists(p):
            return p
    return None


def load_model(model_path: str, device) -> TouchAudioForCausalLM:
    from safetensors.torch import load_file
    cfg_path = _first(os.path.join(model_path, "config.json"), os.path.join(model_path, "..", "..", "model_config.json"))
    if cfg_path is None:
        raise FileNotFoundError(f"no config.json / ../../model_config.json beside {model_path}")
    with open(cfg_path) as f:
        d = json.load(f)
    cfg = TouchAudioConfig.from_dict(d)
    for k in ("pad_token_id", "bos_token_id", "eos_token_id"):      # (top-level ids of an HF config reach the decoder)
        if getattr(cfg.text_config, k) is None and d.get(k) is not None:
            setattr(cfg.text_config, k, d[k])
    model = TouchAudioForCausalLM(cfg)
    sd = {}
    files = sorted(glob.glob(os.path.join(model_path, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no *.safetensors in {model_path}")
    for f in files:
        sd.update(load_file(f))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not (k == "language_model.lm_head.weight" and cfg.text_config.tie_word_embeddings)]
    if missing or unexpected:
        raise RuntimeError(f"checkpoint does not match TouchAudioForCausalLM: missing {missing}, unexpected {unexpected}")
    model.language_model.tie_weights()
    return model.to(device).to(torch.bfloat16).eval()


def data_config(args, model) -> types.SimpleNamespace:
    d = dict(_DATA_DEFAULTS)
    p = _first(args.data_config, os.path.join(args.model_path, "..", "..", "data_config.json"))
    if p is not None:
        with open(p) as f:
            d.update(json.load(f))
    if d["audiofeat_stack_length"] is None:
        d["audiofeat_stack_length"] = max(1, model.config.input_size // int(d["audiofeat_num_mel_bins"]))
    if d["audiofeat_stride_length"] is None:
        d["audiofeat_stride_length"] = d["audiofeat_stack_length"]
    return types.SimpleNamespace(**d)


def read_wav(path: str, target_rate: int = 16000) -> torch.Tensor:
    """16-bit PCM wav (first channel) -> the waveform [1, N] at `target_rate` Hz (the data config's `audio_resample_rate`;
    16 kHz in every recipe): the int16 samples themselves, on the host, for a file at that rate; a file of any other rate
    is resampled on the device (functional.resample: torchaudio's windowed-sinc formula) and comes back as fp32
    [1, ceil(N target_rate / rate)] there.  The reference's scripts resample with `ffmpeg -ar 16000`, a different
    algorithm: the same band-limited signal, not the same samples, and no parity with it is claimed."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError(f"{path}: 16-bit PCM only")
        ch, rate = w.getnchannels(), w.getframerate()
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).reshape(-1, ch)[:, 0].copy()
    pcm = torch.from_numpy(pcm)
    if rate != target_rate:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{path}: {rate} Hz is resampled on the MI355X (there is no CPU path)")
        return ops().resample(pcm.to(torch.device("cuda", torch.cuda.current_device())), rate, int(target_rate))[None]
    return pcm[None]


def features(wavs, dcfg) -> list:
    """The device frontend stages of the data config: fbank / MFCC / log-mel, then stacking.  The waveforms are at the
    data config's `audio_resample_rate` (read_wav) and the samples say so."""
    if dcfg.audio_feat_type == "fbank":
        feat_stage = stages.audio_compute_fbank
    elif dcfg.audio_feat_type == "mfcc":
        feat_stage = stages.audio_compute_mfcc
    elif dcfg.audio_feat_type == "log_mel_spectrogram":
        feat_stage = stages.audio_compute_log_mel_spectrogram
    else:
        raise ValueError(f"unsupported audio_feat_type {dcfg.audio_feat_type!r}")
    rate = int(getattr(dcfg, "audio_resample_rate", 16000))
    samples = [{"sample_rate": rate, "waveform": w} for w in wavs]
    return [s["audiofeat"] for s in stages.audiofeat_stack(feat_stage(iter(samples), dcfg), dcfg)]


def record_line(item, ids, extra: dict, tokenizer=None) -> str:
    """One output line: {"label", "predict_ids"[, "predict"]} and the extra keys of generation.record_fields behind them
    (every "nbest" entry gains its "predict" too).  No extra keys: the line this command has always written."""
    text = lambda row: tokenizer.decode(row, skip_special_tokens=True, clean_up_tokenization_spaces=False)
    rec = {"label": json.dumps(item, ensure_ascii=False), "predict_ids": ids}
    if tokenizer is not None:
        rec["predict"] = text(ids)
    for key, value in extra.items():
        if key == "nbest" and tokenizer is not None:
            value = [{"predict_ids": h["predict_ids"], "predict": text(h["predict_ids"]),
                      **{k: v for k, v in h.items() if k != "predict_ids"}} for h in value]
        rec[key] = value
    return json.dumps(rec, ensure_ascii=False) + "\n"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--data_list", required=True)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--data_config", default=None)
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--max_new_tokens", type=int, default=256)
    ap.add_argument("--repetition_penalty", type=float, default=1.5)
    ap.add_argument("--no_repeat_ngram_size", type=int, default=2)
    ap.add_argument("--num_beams", type=int, default=1, help="> 1: beam search")
    ap.add_argument("--length_penalty", type=float, default=1.0)
    ap.add_argument("--early_stopping", default="false", choices=["true", "false", "never"])
    ap.add_argument("--shard_index", type=int, default=0)
    ap.add_argument("--num_shards", type=int, default=1)
    add_constraint_arguments(ap)
    add_score_arguments(ap)
    add_longform_arguments(ap)
    return ap


def generation_config(args, tokenizer=None) -> GenerationConfig:
    cfg = GenerationConfig(max_new_tokens=args.max_new_tokens, repetition_penalty=args.repetition_penalty,
                           no_repeat_ngram_size=args.no_repeat_ngram_size, num_beams=args.num_beams,
                           length_penalty=args.length_penalty,
                           early_stopping={"true": True, "false": False}.get(args.early_stopping, "never"),
                           sequence_bias=constraints_from_args(args, tokenizer), min_new_tokens=args.min_new_tokens or 0,
                           output_scores=args.output_scores, top_alternatives=args.top_alternatives, nbest=args.nbest)
    cfg.check_beams()
    return cfg


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("infer_asr needs the MI355X (there is no CPU path)")
    device = torch.device("cuda", torch.cuda.current_device())
    model = load_model(args.model_path, device)
    dcfg = data_config(args, model)
    tokenizer = None
    if _first(os.path.join(args.model_path, "tokenizer.json"), os.path.join(args.model_path, "tokenizer_config.json")):
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(args.model_path)
    with open(args.data_list) as f:
        items = [json.loads(line) for line in f if line.strip()]
    items = items[args.shard_index::args.num_shards]
    cfg = generation_config(args, tokenizer)
    long_cfg = longform_from_args(args)
    rate = int(dcfg.audio_resample_rate)
    text = None if tokenizer is None else (
        lambda row: tokenizer.decode(row, skip_special_tokens=True, clean_up_tokenization_spaces=False))
    os.makedirs(args.output_dir, exist_ok=True)
    out_path = os.path.join(args.output_dir, f"part_{args.shard_index + 1}_of_{args.num_shards}")
    with open(out_path, "w") as writer:
        for i in range(0, len(items), args.batch_size):
            batch = items[i:i + args.batch_size]
            wavs = [read_wav(it["wav"], rate) for it in batch]
            if long_cfg is not None:
                done = transcribe_long(touch_audio_decoder(model, cfg, lambda ws: features(ws, dcfg)), wavs, rate, long_cfg,
                                       args.batch_size, to_text=text, nbest=cfg.nbest, output_scores=cfg.wants_scores,
                                       device=device)
                ids, extras = [d["predict_ids"] for d in done], [d["extra"] for d in done]
            else:
                ids, extras = transcribe(model, features(wavs, dcfg), cfg, details=True)
            for it, row, extra in zip(batch, ids, extras):
                writer.write(record_line(it, row, extra, tokenizer))
    return out_path


if __name__ == "__main__":
    main()
