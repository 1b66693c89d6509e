"""Transcribing recordings longer than one utterance: energy VAD on the device (functional.vad_energy, csrc/vad.hip), a
segment planner on the host, and a driver that decodes the segments through a model's existing `transcribe`.

The reference's inference scripts cut every waveform at 30 s (touchnet/models/qwen2_audio/inference_qwen2_audio.py:101,
touchnet/models/kimi_audio/processing_kimi_audio.py:73) and its LlamaForASR command feeds a recording of any length to a
model trained on utterances; this goes beyond them.  What it does not do: no model-based VAD, no timestamp tokens, no
overlap-and-stitch of text across cut points, no streaming.

Frames are the VAD's (VadConfig.frame_length / frame_shift); segment [start, end) in frames is the samples
[start * shift, (end - 1) * shift + win).  Everything but `vad_energy` is host code.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import functional as F
from .functional import VadConfig

SEGMENT_KEY_STRIDE = 1 << 40             # segment i of the recording with row key k draws with k + (i + 1) * this


@dataclass
class LongFormConfig:
    """How a long recording becomes segments (plan_segments applies the rules in this order).  The VAD values are Kaldi's
    program defaults and the four here are common starting points: nobody has tuned any of them for this use."""
    max_segment_s: float = 30.0          # no segment is longer; recordings up to this length are not segmented at all
    min_silence_ms: float = 300.0        # shorter gaps between voiced runs are closed
    min_speech_ms: float = 100.0         # shorter runs are dropped
    pad_ms: float = 100.0                # every run grows by this on both sides
    vad: VadConfig = field(default_factory=VadConfig)

    def __post_init__(self):
        if not (math.isfinite(self.max_segment_s) and self.max_segment_s * 1000.0 >= self.vad.frame_length):
            raise ValueError(f"max_segment_s = {self.max_segment_s} must be finite and at least one VAD frame "
                             f"({self.vad.frame_length} ms)")
        for name in ("min_silence_ms", "min_speech_ms", "pad_ms"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"{name} = {v} must be finite and >= 0")

    def frames(self) -> Tuple[int, int, int, int]:
        """(min_silence, min_speech, pad, max_segment) in VAD frames.  max_segment is the largest n whose samples,
        (n - 1) frame_shift + frame_length ms, fit in max_segment_s."""
        shift = float(self.vad.frame_shift)
        n = lambda ms: int(round(ms / shift))
        most = int(math.floor((self.max_segment_s * 1000.0 - self.vad.frame_length) / shift + 1e-9)) + 1
        return n(self.min_silence_ms), n(self.min_speech_ms), n(self.pad_ms), max(most, 1)


def _lowest(loge, lo: int, hi: int) -> int:
    """the frame of lowest loge in [lo, hi), the lowest index on a tie"""
    best = lo
    for t in range(lo + 1, hi):
        if loge[t] < loge[best]:
            best = t
    return best


def plan_segments(runs, T: int, loge, cfg: LongFormConfig) -> List[Tuple[int, int]]:
    """The voiced runs of a recording of T frames ([(start, end)], ordered, disjoint, end exclusive) -> its segments, by
    these rules in this order:
      1. gaps shorter than min_silence are closed;
      2. runs shorter than min_speech are dropped;
      3. every run is padded by pad on both sides, clamped to [0, T); runs that now touch are merged;
      4. a run longer than max_segment is cut in front of the frame of lowest loge in [start + max / 2, start + max) (the
         lowest index on a tie), and the remainder again;
      5. consecutive runs are merged greedily, left to right, while end_j - start_i <= max_segment: the silence between
         them stays inside the segment, so timestamps stay linear.
    `loge` (indexable by frame, or a function that returns such a thing) is only looked at by rule 4: it may be None when
    no run is that long, and a function is called only then — the driver copies it to the host only when it is needed."""
    min_sil, min_speech, pad, most = cfg.frames()
    runs = [(int(s), int(e)) for s, e in (runs.tolist() if hasattr(runs, "tolist") else runs)]
    T = int(T)
    closed: List[List[int]] = []
    for s, e in runs:
        if not 0 <= s < e <= T or (closed and s < closed[-1][1]):
            raise ValueError(f"plan_segments: run ({s}, {e}) is not an ordered, disjoint interval inside [0, {T})")
        if closed and s - closed[-1][1] < min_sil:
            closed[-1][1] = e
        else:
            closed.append([s, e])
    padded: List[List[int]] = []
    for s, e in closed:
        if e - s < min_speech:
            continue
        s, e = max(0, s - pad), min(T, e + pad)
        if padded and s <= padded[-1][1]:
            padded[-1][1] = max(padded[-1][1], e)
        else:
            padded.append([s, e])
    cut: List[Tuple[int, int]] = []
    for s, e in padded:
        while e - s > most:
            if callable(loge):
                loge = loge()
            if loge is None:
                raise ValueError(f"plan_segments: a run of {e - s} frames exceeds max_segment = {most} frames and needs "
                                 "loge to be cut")
            c = _lowest(loge, s + most // 2, s + most)
            c = max(c, s + 1)
            cut.append((s, c))
            s = c
        cut.append((s, e))
    out: List[Tuple[int, int]] = []
    for s, e in cut:
        if out and e - out[-1][0] <= most:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
    return out


def segment_samples(segments: Sequence[Tuple[int, int]], win: int, shift: int) -> List[Tuple[int, int]]:
    """segments in frames -> [first sample, sample behind the last) of each"""
    return [(s * shift, (e - 1) * shift + win) for s, e in segments]


def segment_recording(wave: torch.Tensor, sample_rate: int, cfg: LongFormConfig, device=None) -> List[Tuple[int, int]]:
    """VAD and plan of one recording ([N] or [1, N], int16 PCM or fp32, anywhere) -> its segments as sample ranges.  The
    log-energies come to the host only when a run has to be cut."""
    win, shift = F.vad_geometry(sample_rate, cfg.vad)
    if device is None:
        device = wave.device if wave.is_cuda else torch.device("cuda", torch.cuda.current_device())
    runs, voiced, loge = F.vad_energy(wave.to(device), sample_rate, cfg.vad)
    return segment_samples(plan_segments(runs, voiced.numel(), lambda: loge.cpu().numpy(), cfg), win, shift)


def needs_segments(wave: torch.Tensor, sample_rate: int, cfg: LongFormConfig) -> bool:
    return wave.numel() > cfg.max_segment_s * sample_rate


def pool_order(lengths: Sequence[int]) -> List[int]:
    """the order in which the pooled segments are decoded: heaviest (longest) first, ties in pool order"""
    return sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))


def segment_key(key: int, index: int) -> int:
    """the row key of segment `index` of the recording with row key `key`: the draws of a sampled run do not depend on how
    the segments are batched"""
    return int(key) + (int(index) + 1) * SEGMENT_KEY_STRIDE


def check_nbest(nbest: int) -> None:
    if int(nbest) > 1:
        raise ValueError(f"long-form transcription: nbest = {nbest} with a recording that is cut into segments is not "
                         "supported (hypotheses do not combine across segments); use nbest = 1 or recordings within "
                         "max_segment_s")


DecodeFn = Callable[[List[torch.Tensor], torch.Tensor], tuple]


def transcribe_long(decode: DecodeFn, wavs: Sequence[torch.Tensor], sample_rate: int, cfg: LongFormConfig,
                    batch_size: int, row_keys: Optional[Sequence[int]] = None, to_text: Optional[Callable] = None,
                    nbest: int = 1, output_scores: bool = False, sampled: bool = False, device=None) -> List[dict]:
    """Transcripts of a batch of recordings of any length.  `decode(wavs, keys) -> (ids, texts or None, extras)` is a
    model's `transcribe` with details (touch_audio_decoder, qwen2_audio_decoder, kimi_audio_decoder); `keys` int64 [n]
    key the draws of a sampled run.

    A recording longer than cfg.max_segment_s is segmented (segment_recording); a shorter one is one segment: the whole
    waveform, untouched, under its own key.  All segments are pooled, decoded `batch_size` at a time heaviest first
    (pool_order) and scattered back.  `sampled` (the decoder draws: do_sample, or Kimi's text_temperature above 1e-6):
    every segment is decoded in a call of its own, whatever `batch_size` says.  The keys make the random numbers of a
    segment independent of the batching, but the decoders' logits are not: an utterance's forward differs in the last
    bf16 bits with its place in a packed batch, which is enough to move a draw across a boundary.  One
    segment per call is the only batching under which a sampled transcript does not depend on `batch_size`; greedy and
    beam search, where such a difference all but never changes a token, keep the batches.  Per recording a dict:
      predict_ids  the segments' ids in time order (each already cut in front of its eos)
      predict      the decode of that concatenation (`to_text`; None without it) — for an unsegmented recording, what
                   `decode` returned
      extra        unsegmented: the extra record keys `decode` returned.  Segmented: "confidence" with output_scores (exp
                   of the mean log-probability over the listed tokens of all segments) and "segments": [{"start", "end"
                   (seconds), "predict_ids", "predict", ...that segment's extra keys}]
      segments     None for an unsegmented recording, else the sample ranges
    No voiced frame: no segment, an empty transcript."""
    B = len(wavs)
    keys = list(range(B)) if row_keys is None else [int(k) for k in row_keys]
    if len(keys) != B:
        raise ValueError(f"transcribe_long: {len(keys)} row keys for {B} recordings")
    if int(batch_size) < 1:
        raise ValueError(f"transcribe_long: batch_size = {batch_size} must be >= 1")
    cut = [needs_segments(w, sample_rate, cfg) for w in wavs]
    if any(cut):
        check_nbest(nbest)
    spans = [segment_recording(w, sample_rate, cfg, device) if c else None for w, c in zip(wavs, cut)]
    pool = []                                        # (recording, segment index or None, waveform, key)
    for r, (w, sp) in enumerate(zip(wavs, spans)):
        if sp is None:
            pool.append((r, None, w, keys[r]))
        else:
            flat = w.reshape(1, -1)
            pool.extend((r, i, flat[:, a:b], segment_key(keys[r], i)) for i, (a, b) in enumerate(sp))
    order = pool_order([p[2].numel() for p in pool])
    done = [None] * len(pool)
    per_call = 1 if sampled else int(batch_size)
    for o in range(0, len(order), per_call):
        chunk = order[o:o + per_call]
        ids, texts, extras = decode([pool[i][2] for i in chunk], torch.tensor([pool[i][3] for i in chunk], dtype=torch.int64))
        for n, i in enumerate(chunk):
            done[i] = (ids[n], None if texts is None else texts[n], extras[n])
    text = lambda ids, given=None: given if given is not None else (to_text(ids) if to_text is not None else None)
    results = [None] * B
    per_rec = [[] for _ in range(B)]
    for p, d in zip(pool, done):
        per_rec[p[0]].append((p[1], d))
    for r in range(B):
        if spans[r] is None:
            ids, given, extra = per_rec[r][0][1]
            results[r] = dict(predict_ids=ids, predict=text(ids, given), extra=extra, segments=None)
            continue
        segs, all_ids, logps = [], [], []
        for (i, (ids, given, extra)), (a, b) in zip(sorted(per_rec[r], key=lambda t: t[0]), spans[r]):
            entry = {"start": a / sample_rate, "end": b / sample_rate, "predict_ids": ids}
            t = text(ids, given)
            if t is not None:
                entry["predict"] = t
            entry.update(extra)
            segs.append(entry)
            all_ids.extend(ids)
            logps.extend(v for v in extra.get("token_logprobs", ()) if v is not None)
        extra = {}
        if output_scores:
            extra["confidence"] = math.exp(sum(logps) / len(logps)) if logps else None
        extra["segments"] = segs
        results[r] = dict(predict_ids=all_ids, predict=(to_text(all_ids) if to_text is not None else None), extra=extra,
                          segments=list(spans[r]))
    return results


# ------------------------------------------------------------------------------------------- the three models' decoders
def touch_audio_decoder(model, gen_cfg, features: Callable) -> DecodeFn:
    """LlamaForASR: `features(wavs)` are the data config's frontend stages (bin.infer_asr.features); no draws, no keys"""
    from .models.touch_audio.inference_touch_audio import transcribe

    def decode(wavs, keys):
        ids, extras = transcribe(model, features(wavs), gen_cfg, details=True)
        return ids, None, extras
    return decode


def qwen2_audio_decoder(model, tokenizer, instruct, gen_cfg) -> DecodeFn:
    from .models.qwen2_audio.inference_qwen2_audio import transcribe
    return lambda wavs, keys: transcribe(model, wavs, tokenizer, instruct, gen_cfg, row_keys=keys, details=True)


def kimi_audio_decoder(model, tokenizer, instruct, gen_cfg) -> DecodeFn:
    from .models.kimi_audio.inference_kimi_audio import transcribe
    return lambda wavs, keys: transcribe(model, wavs, tokenizer, instruct, gen_cfg, row_keys=keys, details=True)


def longform_from_args(args) -> Optional[LongFormConfig]:
    """The flags of generation.add_longform_arguments -> a LongFormConfig, or None without --long_form"""
    if not getattr(args, "long_form", False):
        return None
    return LongFormConfig(max_segment_s=args.max_segment_s, min_silence_ms=args.vad_min_silence_ms,
                          min_speech_ms=args.vad_min_speech_ms, pad_ms=args.vad_pad_ms,
                          vad=VadConfig(energy_threshold=args.vad_energy_threshold,
                                        energy_mean_scale=args.vad_energy_mean_scale,
                                        frames_context=args.vad_frames_context,
                                        proportion_threshold=args.vad_proportion_threshold))
