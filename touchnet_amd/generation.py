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

Sampling (do_sample, several eos ids: what a Qwen2-Audio checkpoint's generation_config.json asks for,
`GenerationConfig.from_hf`) runs the same loop with tn_sample_step in place of tn_greedy_step.  The caches start at
`longest prompt + min(new tokens, cache_chunk)` rows and double when the host's step counter reaches their capacity (the
host knows the step count: no sync), so a max_length of 70 000 does not allocate 70 000 rows per layer up front.

`sequence_bias` (hotword boosts; -inf forbids a sequence) and `min_new_tokens` — transformers' SequenceBiasLogitsProcessor
and MinNewTokensLengthLogitsProcessor — are matched against the device history by tn_logits_constrain, one launch right before
the step kernel and only when the config carries them (`ConstraintPlan`, built once per call).  Greedy and sampling: the logits
are edited in place, logit[t] = T(fp32(logit[t]) + total) in the logits' own dtype (bf16 logits: the sum is rounded to bf16;
fp32: HF's arithmetic), before penalty, n-gram ban and the warpers: HF's order.  Beam search: the kernel emits the edits and
tn_beam_step_edits adds them to the log-probabilities, after log_softmax and before the penalty.  At most MAX_BIAS_SEQS
sequences of at most MAX_BIAS_LEN ids.

Confidences and N-best lists (`output_scores`, `top_alternatives`, `nbest`; all off by default, and then nothing of this
runs).  Greedy, sampling and Kimi-Audio: one tn_token_scores launch per step behind the step kernel, in history mode, on the
logits as lm_head wrote them (a `sequence_bias` plan edits a copy then): log-probability and entropy of the appended token and
the k most likely ids, written to that token's history column of a `TokenScores` workspace that grows with the cache.  Beam
search keeps sums, not per-token terms: `BeamState.nbest` reads the finished set, and the per-token scores of the returned
hypotheses come from ONE teacher-forced packed forward behind the search, `score_continuations`, which is also the rescoring
entry point.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, fields
from typing import Callable, List, Optional, Sequence, Union

import torch

from . import _C
from . import functional as F


# generation_config.json keys this path does not implement, with the value that leaves them inert (HF's defaults)
_UNSUPPORTED = {"num_beam_groups": 1, "penalty_alpha": None, "typical_p": 1.0, "min_p": None,
                "epsilon_cutoff": 0.0, "eta_cutoff": 0.0, "top_h": None, "bad_words_ids": None, "force_words_ids": None,
                "constraints": None, "min_length": 0, "suppress_tokens": None, "begin_suppress_tokens": None,
                "forced_bos_token_id": None, "forced_eos_token_id": None, "encoder_repetition_penalty": 1.0,
                "encoder_no_repeat_ngram_size": 0, "exponential_decay_length_penalty": None, "guidance_scale": None,
                "watermarking_config": None, "renormalize_logits": False, "num_return_sequences": 1, "assistant_model": None,
                "prompt_lookup_num_tokens": None, "max_time": None, "stop_strings": None, "dola_layers": None,
                "diversity_penalty": 0.0}


MAX_BEAMS, MAX_BEAM_EOS = 8, 3             # tn_beam_step's limits
MAX_BIAS_SEQS, MAX_BIAS_LEN = 16384, 64    # tn_logits_constrain's limits: biased sequences, ids per sequence

# what replaces the two refused keys that forbid tokens (NoBadWordsLogitsProcessor is a SequenceBiasLogitsProcessor at -inf)
_FORBID_HINT = {k: "; forbid token sequences with sequence_bias instead: [[ids], -inf] per sequence, which is what "
                   "NoBadWordsLogitsProcessor reduces to" for k in ("bad_words_ids", "suppress_tokens")}
# N-best lists are a knob of this decoder, not the HF key (which also multiplies sampled rows)
_FORBID_HINT["num_return_sequences"] = ("; for the N best hypotheses of a beam search set this decoder's own knob instead: "
                                        "nbest = N with num_beams >= N (GenerationConfig(nbest=N) or from_hf(..., nbest=N))")
MAX_ALTERNATIVES = 8                       # tn_token_scores' limit: runner-up tokens per position


def normalize_sequence_bias(value) -> Optional[dict]:
    """`sequence_bias` as a dict {tuple(ids): float}, from that dict or from HF's list form [[ids], bias].  Duplicates
    resolve as a Python dict resolves them: the later value wins and the first position is kept.  Refused: an empty
    sequence, ids that are no non-negative integers, more than MAX_BIAS_SEQS sequences or MAX_BIAS_LEN ids in one, and
    biases of +inf or NaN (-inf forbids the sequence)."""
    if value is None or (isinstance(value, (list, tuple, dict)) and len(value) == 0):
        return None
    if isinstance(value, dict):
        pairs = list(value.items())
    elif isinstance(value, (list, tuple)):
        if any(not isinstance(e, (list, tuple)) or len(e) != 2 for e in value):
            raise ValueError("generation config: sequence_bias must be a dict {tuple(ids): bias} or a list of [[ids], bias]")
        pairs = [(e[0], e[1]) for e in value]
    else:
        raise ValueError("generation config: sequence_bias must be a dict {tuple(ids): bias} or a list of [[ids], bias]")
    out = {}
    for ids, bias in pairs:
        if isinstance(ids, (int, str)) or not hasattr(ids, "__len__"):
            raise ValueError(f"generation config: sequence_bias key {ids!r} must be a sequence of token ids")
        if len(ids) == 0:
            raise ValueError("generation config: sequence_bias holds an empty sequence")
        if len(ids) > MAX_BIAS_LEN:
            raise ValueError(f"generation config: a biased sequence of {len(ids)} ids exceeds {MAX_BIAS_LEN}")
        if any(isinstance(t, bool) or not isinstance(t, int) or t < 0 for t in ids):
            raise ValueError(f"generation config: sequence_bias ids must be non-negative integers (got {list(ids)!r})")
        if isinstance(bias, bool) or not isinstance(bias, (int, float)):
            raise ValueError(f"generation config: sequence_bias value {bias!r} must be a number")
        b = float(bias)
        if b != b or b == float("inf"):
            raise ValueError(f"generation config: sequence_bias value {b} must be finite or -inf")
        out[tuple(int(t) for t in ids)] = b
    if len(out) > MAX_BIAS_SEQS:
        raise ValueError(f"generation config: {len(out)} biased sequences exceed {MAX_BIAS_SEQS}")
    return out


def hotword_bias(phrases_ids, bias: float = 2.0) -> dict:
    """A `sequence_bias` dict that boosts every token along every phrase (shallow-fusion style): every prefix of every
    phrase (each a list of token ids) is a biased sequence with `bias`, so the first token is boosted always, the second
    once the first was emitted, and so on.  Prefixes that different phrases share appear once.  There is no back-off: a
    phrase abandoned halfway keeps the boost its emitted tokens already received.  `bias` 2.0 is a starting point that
    nobody has tuned."""
    out = {}
    for ids in phrases_ids:
        ids = tuple(int(t) for t in ids)
        for n in range(1, len(ids) + 1):
            out.setdefault(ids[:n], float(bias))
    return normalize_sequence_bias(out) or {}


def constraint_tables(sequence_bias: Optional[dict], min_new_tokens: int, eos: Sequence[int], vocab: int) -> Optional[dict]:
    """The host side of tn_logits_constrain's table, as Python lists (None: nothing to do).  Sequences are grouped by their
    last id, the groups in ascending order of that id; within a group the length-1 sequence first, then the longer ones in
    dict order — HF's order of summation (SequenceBiasLogitsProcessor adds the length-1 biases first).  With
    min_new_tokens > 0 every eos id is a group of its own (possibly empty), marked in grp_eos."""
    seqs = normalize_sequence_bias(sequence_bias) or {}
    m = int(min_new_tokens or 0)
    if m < 0:
        raise ValueError(f"generation config: min_new_tokens = {min_new_tokens} must be >= 0")
    for ids in seqs:
        if any(t >= vocab for t in ids):
            raise ValueError(f"generation config: sequence_bias id in {list(ids)} is outside the vocabulary [0, {vocab})")
    groups = {}
    for ids, b in seqs.items():
        groups.setdefault(ids[-1], []).append((ids, b))
    hold = sorted({int(e) for e in eos if 0 <= int(e) < vocab}) if m > 0 else []
    for e in hold:
        groups.setdefault(e, [])
    if not groups:
        return None
    t = dict(seq_off=[0], seq_ids=[], seq_bias=[], grp_off=[0], grp_tok=[], grp_eos=[], min_new=m if hold else 0,
             vocab=int(vocab))
    for tok in sorted(groups):
        members = sorted(groups[tok], key=lambda sb: len(sb[0]) != 1)           # (stable: dict order otherwise)
        for ids, b in members:
            t["seq_ids"].extend(ids)
            t["seq_off"].append(len(t["seq_ids"]))
            t["seq_bias"].append(b)
        t["grp_off"].append(len(t["seq_bias"]))
        t["grp_tok"].append(tok)
        t["grp_eos"].append(int(tok in hold))
    return t


@dataclass
class ConstraintPlan:
    """tn_logits_constrain's table on the device (see `constraint_tables`), built once per generate() call."""
    seq_off: torch.Tensor
    seq_ids: torch.Tensor
    seq_bias: torch.Tensor
    grp_off: torch.Tensor
    grp_tok: torch.Tensor
    grp_eos: torch.Tensor
    min_new: int
    vocab: int

    @classmethod
    def build(cls, sequence_bias, min_new_tokens, eos, vocab, device) -> Optional["ConstraintPlan"]:
        t = constraint_tables(sequence_bias, min_new_tokens, eos, vocab)
        if t is None:
            return None
        parts = [t["seq_off"], t["seq_ids"] or [0], t["grp_off"], t["grp_tok"], t["grp_eos"]]
        ints = torch.tensor([x for p in parts for x in p], dtype=torch.int32).to(device)        # one upload
        cuts, o = [], 0
        for p in parts:
            cuts.append(ints[o:o + len(p)])
            o += len(p)
        bias = torch.tensor(t["seq_bias"] or [0.0], dtype=torch.float32).to(device)[:len(t["seq_bias"])]
        return cls(seq_off=cuts[0], seq_ids=cuts[1][:len(t["seq_ids"])], seq_bias=bias,
                   grp_off=cuts[2], grp_tok=cuts[3], grp_eos=cuts[4], min_new=t["min_new"], vocab=t["vocab"])

    def edit_buffers(self, rows: int):
        """(edit_ids int32, edit_val fp32 [rows, n_grp], edit_cnt int32 [rows]): the workspace of the emit mode."""
        n, dev = self.grp_tok.shape[0], self.grp_tok.device
        return (torch.empty(rows, n, dtype=torch.int32, device=dev), torch.empty(rows, n, dtype=torch.float32, device=dev),
                torch.empty(rows, dtype=torch.int32, device=dev))


def _check_alternatives(what: str, k) -> None:
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= MAX_ALTERNATIVES:
        raise ValueError(f"{what}: top_alternatives = {k!r} must be an integer in [0, {MAX_ALTERNATIVES}]")


@dataclass
class GenerationConfig:
    """The knobs of the reference's generate() call (top_k / top_p / temperature are inert there: do_sample=False).
    `from_hf` reads a checkpoint's generation_config.json instead."""
    max_new_tokens: Optional[int] = 256      # None: max_length - the longest prompt (HF's rule)
    repetition_penalty: float = 1.5
    no_repeat_ngram_size: int = 2
    eos_token_id: Optional[Union[int, List[int]]] = None       # None: the model config's; a list: any of them finishes
    pad_token_id: Optional[int] = None
    bos_token_id: Optional[int] = None
    check_every: int = 16                    # steps between two host reads of the unfinished count
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 50                          # 0: off (inert unless do_sample)
    top_p: float = 1.0                       # 1: off (inert unless do_sample)
    seed: int = 0                            # Philox key of the draws (with the row key and the step)
    max_length: Optional[int] = None         # prompt + new tokens, used when max_new_tokens is None
    cache_chunk: int = 1024                  # new-token rows of the first KV-cache allocation (it doubles on demand)
    num_beams: int = 1                       # > 1: beam search (tn_beam_step), without do_sample
    length_penalty: float = 1.0              # finished hypotheses score sum(log p) / length ** length_penalty
    early_stopping: Union[bool, str] = False  # True, False or "never" (HF's three heuristics)
    sequence_bias: Optional[dict] = None     # {tuple(ids): bias}: hotword boosts; -inf forbids a sequence (`hotword_bias`)
    min_new_tokens: int = 0                  # every eos id is held at -inf until this many tokens were generated
    output_scores: bool = False              # per-token log-probability and entropy of the raw lm_head logits (`TokenScores`)
    top_alternatives: int = 0                # 0 .. 8 most likely tokens per position with their log-probabilities (implies output_scores)
    nbest: int = 1                           # beam search: the first `nbest` finished hypotheses (1 .. num_beams) — not HF's
                                             # num_return_sequences key, which from_hf goes on refusing

    def __post_init__(self):
        self.check_scores()

    def check_scores(self) -> None:
        """What the three score knobs accept."""
        _check_alternatives("generation config", self.top_alternatives)
        n = self.nbest
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"generation config: nbest = {n!r} must be an integer >= 1")
        if n > 1 and int(self.num_beams) <= 1:
            raise ValueError(f"generation config: nbest = {n} needs beam search (num_beams > 1): greedy search and sampling "
                             "follow one hypothesis")
        if n > int(self.num_beams):
            raise ValueError(f"generation config: nbest = {n} exceeds num_beams = {self.num_beams} (the finished set holds "
                             "num_beams hypotheses)")

    @property
    def wants_scores(self) -> bool:
        return bool(self.output_scores) or int(self.top_alternatives) > 0

    @classmethod
    def from_hf(cls, path_or_dict, **overrides) -> "GenerationConfig":
        """A generation_config.json (its path, its directory or its parsed dict) resolved as HF generate() resolves it:
        HF's defaults for absent keys, the sampling warpers inert without do_sample, a file `max_new_tokens` taking
        precedence over `max_length`.  Keys this path does not implement raise instead of being ignored.  `overrides`
        (field names of this class) win over the file, except that the file's max_new_tokens still beats max_length."""
        if isinstance(path_or_dict, dict):
            d = dict(path_or_dict)
        else:
            p = str(path_or_dict)
            if os.path.isdir(p):
                p = os.path.join(p, "generation_config.json")
            with open(p) as f:
                d = json.load(f)
        known = {f.name for f in fields(cls)}
        bad = [k for k in overrides if k not in known]
        if bad:
            raise TypeError(f"GenerationConfig.from_hf: unknown overrides {bad}")
        for k, inert in _UNSUPPORTED.items():
            v = overrides.get(k, d.get(k, inert))
            if v not in (inert, None, [], {}):
                raise ValueError(f"generation config: {k} = {v!r} is not supported by this decoder "
                                 f"(greedy, sampled or beam search, one sequence per prompt){_FORBID_HINT.get(k, '')}")
        num = lambda k, default: overrides[k] if k in overrides else d.get(k, default)
        cfg = cls(max_new_tokens=d.get("max_new_tokens"), repetition_penalty=float(num("repetition_penalty", 1.0)),
                  no_repeat_ngram_size=int(num("no_repeat_ngram_size", 0)), eos_token_id=num("eos_token_id", None),
                  pad_token_id=num("pad_token_id", None), bos_token_id=num("bos_token_id", None),
                  do_sample=bool(num("do_sample", False)), temperature=float(num("temperature", 1.0)),
                  top_k=int(num("top_k", 50) or 0), top_p=float(num("top_p", 1.0)), seed=int(num("seed", 0)),
                  max_length=int(num("max_length", 20)), check_every=int(num("check_every", 16)),
                  cache_chunk=int(num("cache_chunk", 1024)), num_beams=int(num("num_beams", 1) or 1),
                  length_penalty=float(num("length_penalty", 1.0)), early_stopping=num("early_stopping", False),
                  sequence_bias=normalize_sequence_bias(num("sequence_bias", None)),
                  min_new_tokens=int(num("min_new_tokens", 0) or 0),
                  # this decoder's own knobs: overrides only (the file's `output_scores` means HF's processed scores)
                  output_scores=bool(overrides.get("output_scores", False)),
                  top_alternatives=overrides.get("top_alternatives", 0), nbest=overrides.get("nbest", 1))
        if cfg.min_new_tokens < 0:
            raise ValueError(f"generation config: min_new_tokens = {cfg.min_new_tokens} must be >= 0")
        if cfg.max_new_tokens is None and "max_new_tokens" in overrides:
            cfg.max_new_tokens = overrides["max_new_tokens"]
        if cfg.do_sample:
            if not cfg.temperature > 0.0:
                raise ValueError(f"generation config: temperature {cfg.temperature} must be > 0 when sampling")
            if not 0.0 < cfg.top_p <= 1.0:
                raise ValueError(f"generation config: top_p {cfg.top_p} must be in (0, 1]")
            if cfg.top_k < 0:
                raise ValueError(f"generation config: top_k {cfg.top_k} must be >= 0")
        else:
            cfg.temperature, cfg.top_k, cfg.top_p = 1.0, 0, 1.0        # the warpers are inert without do_sample
        cfg.check_beams()
        return cfg

    def check_beams(self, eos: Optional[Sequence[int]] = None) -> None:
        """What beam search accepts (tn_beam_step's limits); `eos`: the resolved eos ids (default: this config's)."""
        if self.early_stopping not in (True, False, "never"):
            raise ValueError(f"generation config: early_stopping = {self.early_stopping!r} must be True, False or 'never'")
        if self.num_beams < 1:
            raise ValueError(f"generation config: num_beams = {self.num_beams} must be >= 1")
        if self.num_beams == 1:
            return
        if self.do_sample:
            raise ValueError(f"generation config: num_beams = {self.num_beams} with do_sample is not supported by this "
                             "decoder (beam search is deterministic here; beam sampling is not implemented)")
        if self.num_beams > MAX_BEAMS:
            raise ValueError(f"generation config: num_beams = {self.num_beams} exceeds {MAX_BEAMS}")
        if eos is None:
            e = self.eos_token_id
            eos = [] if e is None else (list(e) if isinstance(e, (list, tuple)) else [e])
        if len(eos) > MAX_BEAM_EOS:
            raise ValueError(f"generation config: beam search takes at most {MAX_BEAM_EOS} eos ids (got {len(eos)})")

    def new_tokens(self, longest_prompt: int) -> int:
        """The token budget of a batch: max_new_tokens, else max_length minus the longest prompt (HF's rule)."""
        if self.max_new_tokens is not None:
            return int(self.max_new_tokens)
        if self.max_length is None:
            raise ValueError("GenerationConfig: neither max_new_tokens nor max_length is set")
        return int(self.max_length) - int(longest_prompt)


KIMI_MAX_WINDOW, KIMI_MAX_TOP_K = 64, 64     # tn_kimi_text_step's limits


@dataclass
class KimiGenerationConfig:
    """The arguments of MoonshotKimiaForCausalLM.generate() (touchnet/models/kimi_audio/modeling_kimi_audio.py:1084-1101)
    with its defaults, and the ids KimiASampler hard-codes.  The text stream is all that generate() returns: it never asks
    `_generate_loop` for audio output, so the audio-stream token of every step is the blank.  The four audio_* knobs and
    kimia_text_audiodelaytokens are therefore accepted and ignored here (models/kimi_audio/inference_kimi_audio.py)."""
    text_temperature: float = 0.0            # <= 1e-6: argmax
    text_top_k: int = 5                      # candidates of a draw (inert at temperature <= 1e-6)
    text_repetition_penalty: float = 1.1     # > 1: on, over the last `window` generated tokens once more than that exist
    text_repetition_window_size: int = 16
    audio_temperature: float = 0.8           # ignored (see above)
    audio_top_k: int = 10                    # ignored
    audio_repetition_penalty: float = 1.0    # ignored
    audio_repetition_window_size: int = 64   # ignored
    kimia_text_audiodelaytokens: int = 6     # ignored
    max_new_tokens: int = 2048               # the inference script's value; -1: 7500 - the longest prompt (generate()'s rule)
    kimia_text_blank: int = 151666           # <|im_kimia_text_blank|>
    kimia_text_eos: int = 151667             # <|im_kimia_text_eos|>
    cache_chunk: int = 1024                  # new-token rows of the first KV-cache allocation (it doubles on demand)
    check_every: int = 16                    # steps between two host reads of the unfinished count
    seed: int = 0                            # Philox key of the draws (with the row key and the step)
    output_scores: bool = False              # per-token log-probability and entropy of the raw lm_head logits (`TokenScores`)
    top_alternatives: int = 0                # 0 .. 8 most likely tokens per position (implies output_scores)

    def __post_init__(self):
        self.check()

    @property
    def wants_scores(self) -> bool:
        return bool(self.output_scores) or int(self.top_alternatives) > 0

    def check(self) -> None:
        """Refuses what tn_kimi_text_step refuses."""
        _check_alternatives("Kimi generation config", self.top_alternatives)
        if not self.text_repetition_penalty > 0.0:
            raise ValueError(f"Kimi generation config: text_repetition_penalty {self.text_repetition_penalty} must be > 0")
        if not 1 <= int(self.text_repetition_window_size) <= KIMI_MAX_WINDOW:
            raise ValueError(f"Kimi generation config: text_repetition_window_size {self.text_repetition_window_size} "
                             f"must be in [1, {KIMI_MAX_WINDOW}]")
        if not 0 <= int(self.text_top_k) <= KIMI_MAX_TOP_K:
            raise ValueError(f"Kimi generation config: text_top_k {self.text_top_k} must be in [0, {KIMI_MAX_TOP_K}]")
        if self.text_temperature > 1e-6 and int(self.text_top_k) == 0:
            raise ValueError("Kimi generation config: text_temperature > 1e-6 with text_top_k = 0 (a draw over the whole "
                             "vocabulary) is not supported by this decoder")
        if not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError("Kimi generation config: seed must fit in 64 unsigned bits")
        if int(self.max_new_tokens) < -1:
            raise ValueError(f"Kimi generation config: max_new_tokens {self.max_new_tokens} must be >= -1")

    def new_tokens(self, longest_prompt: int) -> int:
        n = int(self.max_new_tokens)
        return 7500 - int(longest_prompt) if n == -1 else n


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

    @property
    def capacity(self) -> int:
        return self.hist.shape[1]

    def grow(self, S_new: int) -> None:
        """Reallocate caches and history with S_new >= S_max rows and copy the old contents (lengths are unchanged)."""
        S = self.capacity
        if S_new <= S:
            return
        def bigger(t):
            n = t.new_empty(t.shape[0], S_new, *t.shape[2:]) if t.dim() > 2 else t.new_zeros(t.shape[0], S_new)
            n[:, :S].copy_(t)
            return n
        self.k = [bigger(t) for t in self.k]
        self.v = [bigger(t) for t in self.v]
        self.hist = bigger(self.hist)


@dataclass
class TokenScores:
    """How sure the model was of every generated token, from the logits as lm_head wrote them (transformers'
    `output_logits`; no hotword edit, penalty or temperature): logp fp32 [B, N] = log_softmax(logits)[token] — equal to
    compute_transition_scores(sequences, out.logits, normalize_logits=True) —, entropy fp32 [B, N] of the step's
    distribution, alt_id int32 / alt_logp fp32 [B, N, k]: the k most likely tokens of the step, best first (ties to the
    lower id).  confidence fp32 [B] = exp(mean logp) over a row's tokens up to and including its first eos (all of them
    when it never finished).  Columns behind a row's end read 0 (ids: -1).  The same class is the in-loop workspace
    (`buffers`): one column per HISTORY slot, prompt included, written by tn_token_scores in history mode."""
    logp: torch.Tensor
    entropy: torch.Tensor
    alt_id: Optional[torch.Tensor] = None
    alt_logp: Optional[torch.Tensor] = None
    confidence: Optional[torch.Tensor] = None

    @classmethod
    def buffers(cls, rows: int, S: int, k: int, device) -> "TokenScores":
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=device)
        return cls(logp=f(rows, S), entropy=f(rows, S), alt_logp=f(rows, S, k),
                   alt_id=torch.full((rows, S, k), -1, dtype=torch.int32, device=device))

    @property
    def k(self) -> int:
        return 0 if self.alt_id is None else int(self.alt_id.shape[-1])

    def grow(self, S_new: int) -> None:
        """More history columns, as KVCache.grow (contents kept)."""
        S = self.logp.shape[1]
        if S_new <= S:
            return
        new = TokenScores.buffers(self.logp.shape[0], S_new, self.k, self.logp.device)
        for name in ("logp", "entropy", "alt_id", "alt_logp"):
            getattr(new, name)[:, :S].copy_(getattr(self, name))
            setattr(self, name, getattr(new, name))

    def columns(self, idx: torch.Tensor) -> "TokenScores":
        """The history columns idx int64 [B, N] of the workspace, as a result of N columns."""
        i3 = idx[:, :, None].expand(-1, -1, self.k)
        return TokenScores(logp=self.logp.gather(1, idx), entropy=self.entropy.gather(1, idx),
                           alt_id=self.alt_id.gather(1, i3), alt_logp=self.alt_logp.gather(1, i3))

    def close(self, n_tokens: torch.Tensor) -> "TokenScores":
        """Blank the columns behind every row's n_tokens [B] tokens (the kernel scored padding there) and set `confidence`."""
        N = self.logp.shape[1]
        n = n_tokens.to(device=self.logp.device, dtype=torch.int64).clamp(max=N)
        live = torch.arange(N, device=n.device)[None] < n[:, None]
        self.logp = torch.where(live, self.logp, torch.zeros_like(self.logp))
        self.entropy = torch.where(live, self.entropy, torch.zeros_like(self.entropy))
        self.alt_id = torch.where(live[:, :, None], self.alt_id, torch.full_like(self.alt_id, -1))
        self.alt_logp = torch.where(live[:, :, None], self.alt_logp, torch.zeros_like(self.alt_logp))
        self.confidence = torch.exp(self.logp.sum(1) / n.clamp(min=1).to(torch.float32))
        return self


def _generated_lengths(ids: torch.Tensor, eos: Sequence[int]) -> torch.Tensor:
    """[B, N] generated ids -> int64 [B]: the tokens up to and including a row's first eos, N when it has none."""
    N = ids.shape[1]
    if not len(eos) or N == 0:
        return torch.full((ids.shape[0],), N, dtype=torch.int64, device=ids.device)
    is_eos = torch.isin(ids, torch.tensor(list(eos), dtype=ids.dtype, device=ids.device))
    return torch.where(is_eos.any(1), is_eos.to(torch.int8).argmax(1) + 1, torch.full_like(ids[:, 0], N))


@dataclass
class BeamState:
    """Beam search over R = B * K rows (utterance b owns rows b K .. b K + K - 1).  k / v [R, S_max, Nkv, D] per layer: a
    key / value stays in the row that wrote it, and src int32 [R, S_max] names, per row and position, the row to read
    (tn_attn_decode_beam).  hist / hist_len / cache_len as in KVCache, per row.  run_score fp32 [R]: the running beams'
    sums of log-probabilities.  The finished set, K slots per utterance, best first: fin_ids int32 [R, S_max] (the whole
    sequence, prompt included), fin_len, fin_flag int32 [R], fin_score fp32 [R] (-1e9 = empty).  Per utterance (int32 [B]):
    gen (tokens generated), unsat (HF's early-stop heuristic still unsatisfied), done; n_unfinished int32 [1].  out_ids /
    out_parent int32 [R]: the last step's ids and parent rows."""
    num_beams: int
    k: List[torch.Tensor]
    v: List[torch.Tensor]
    cache_len: torch.Tensor
    hist: torch.Tensor
    hist_len: torch.Tensor
    src: torch.Tensor
    run_score: torch.Tensor
    fin_ids: torch.Tensor
    fin_len: torch.Tensor
    fin_score: torch.Tensor
    fin_flag: torch.Tensor
    gen: torch.Tensor
    unsat: torch.Tensor
    done: torch.Tensor
    n_unfinished: torch.Tensor
    out_ids: torch.Tensor
    out_parent: torch.Tensor

    @classmethod
    def allocate(cls, num_layers: int, B: int, K: int, S_max: int, Nkv: int, D: int, device,
                 dtype=torch.bfloat16) -> "BeamState":
        R = B * K
        z = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=device)
        first = torch.arange(R, dtype=torch.int32, device=device) // K * K          # the row the prompt is stored in
        return cls(num_beams=K, k=[torch.empty(R, S_max, Nkv, D, dtype=dtype, device=device) for _ in range(num_layers)],
                   v=[torch.empty(R, S_max, Nkv, D, dtype=dtype, device=device) for _ in range(num_layers)],
                   cache_len=z(R), hist=z(R, S_max), hist_len=z(R), src=first[:, None].repeat(1, S_max),
                   run_score=torch.zeros(R, dtype=torch.float32, device=device), fin_ids=z(R, S_max), fin_len=z(R),
                   fin_score=torch.full((R,), -1.0e9, dtype=torch.float32, device=device), fin_flag=z(R), gen=z(B),
                   unsat=torch.ones(B, dtype=torch.int32, device=device), done=z(B),
                   n_unfinished=torch.full((1,), B, dtype=torch.int32, device=device), out_ids=z(R), out_parent=z(R))

    @property
    def finished(self) -> torch.Tensor:
        return self.done

    @property
    def capacity(self) -> int:
        return self.hist.shape[1]

    def grow(self, S_new: int) -> None:
        """Reallocate caches, history, finished ids and table with S_new >= S_max columns, keeping their contents."""
        S = self.capacity
        if S_new <= S:
            return
        def bigger(t):
            n = t.new_empty(t.shape[0], S_new, *t.shape[2:]) if t.dim() > 2 else t.new_zeros(t.shape[0], S_new)
            n[:, :S].copy_(t)
            return n
        self.k = [bigger(t) for t in self.k]
        self.v = [bigger(t) for t in self.v]
        self.hist, self.fin_ids, self.src = bigger(self.hist), bigger(self.fin_ids), bigger(self.src)

    def best(self, prompt_lens: Sequence[int], pad: int):
        """-> (ids int64 [B, N] of every utterance's best finished hypothesis behind its prompt, `pad` after its end;
        scores fp32 [B])."""
        K = self.num_beams
        lens = torch.tensor(list(prompt_lens), dtype=torch.int64, device=self.hist.device)
        n = self.fin_len[::K].to(torch.int64) - lens
        N = max(int(n.max()), 0)
        idx = lens[:, None] + torch.arange(N, device=lens.device)[None]
        ids = self.fin_ids[::K].gather(1, idx.clamp(max=self.capacity - 1)).to(torch.int64)
        ids = torch.where(torch.arange(N, device=lens.device)[None] < n[:, None], ids, torch.full_like(ids, pad))
        return ids, self.fin_score[::K].clone()

    def nbest(self, prompt_lens: Sequence[int], pad: int, n: int):
        """-> (ids int64 [B, n, N]: every utterance's first `n` finished hypotheses behind its prompt, best first, `pad`
        after their ends; scores fp32 [B, n]; count int64 [B]).  The finished set is kept best first and its empty slots
        (fin_score <= -1e9) come last, so these are slots 0 .. n - 1.  An utterance that finished fewer than n hypotheses
        says so in `count`; its remaining entries are all `pad` with score -inf.  (transformers' num_return_sequences fills
        such entries with whatever rows its scorer has left; here they are marked.)"""
        K = self.num_beams
        if not 1 <= int(n) <= K:
            raise ValueError(f"nbest: n = {n} must be in [1, num_beams = {K}]")
        B = self.fin_len.shape[0] // K
        dev = self.hist.device
        lens = torch.tensor(list(prompt_lens), dtype=torch.int64, device=dev)
        score = self.fin_score.view(B, K)[:, :n]
        have = score > -1.0e9
        m = torch.where(have, self.fin_len.view(B, K)[:, :n].to(torch.int64) - lens[:, None], torch.zeros_like(lens[:, None]))
        N = max(int(m.max()), 0)
        col = torch.arange(N, device=dev)
        idx = (lens[:, None, None] + col[None, None]).clamp(max=self.capacity - 1).expand(B, n, N)
        ids = self.fin_ids.view(B, K, -1)[:, :n].gather(2, idx).to(torch.int64)
        ids = torch.where(col[None, None] < m[:, :, None], ids, torch.full_like(ids, pad))
        return ids, torch.where(have, score, torch.full_like(score, -math.inf)), have.sum(1)


def _parts(model):
    """-> (PackedCausalLM, projector weight or None) of a TouchAudioForCausalLM, a Qwen2-Audio model (its audio rows come
    from an embedding builder) or a plain PackedCausalLM."""
    lm = getattr(model, "language_model", None)
    if lm is not None:
        proj = getattr(model, "projector", None)
        return lm, (proj.weight if proj is not None else None)
    return model, None


def eos_ids(cfg: GenerationConfig, lm) -> List[int]:
    """The eos ids of a generation (the config's, else the model's), as a list (possibly empty)."""
    eos = cfg.eos_token_id if cfg.eos_token_id is not None else lm.config.eos_token_id
    if eos is None:
        return []
    return [int(e) for e in eos] if isinstance(eos, (list, tuple)) else [int(eos)]


def _special(cfg: GenerationConfig, lm):
    eos = eos_ids(cfg, lm)
    pad = cfg.pad_token_id if cfg.pad_token_id is not None else lm.config.pad_token_id
    if pad is None:
        pad = eos[0] if eos else 0                 # (HF: pad defaults to the first eos)
    return eos, int(pad)


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


def _embed_touch_audio(lm, proj_w, prompts: Prompts, ids, lens, Tp, device):
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
    return emb


_MAX_EOS = 8                                 # eos ids tn_sample_step takes


# embedding builder of a prefill: (packed ids [Tp] on the device, prompt lengths, Tp) -> embeddings [Tp, H]
EmbedFn = Callable[[torch.Tensor, List[int], int], torch.Tensor]


def _prefill(lm, proj_w, prompts: Prompts, cache, device, embed: Optional[EmbedFn] = None, row_stride: int = 1):
    """Packed forward over all prompts (one row, one document each) -> logits [B, V] of every prompt's last position;
    keys / values of every layer scattered into the caches.  `embed` builds the packed embeddings for a model of its own
    (Qwen2-Audio: the audio tower's rows at the AUDIO positions); by default embed(ids), plus projector(features) for
    TouchAudio.  Prompt b goes to cache row b * row_stride (beam search: the first row of the utterance's K)."""
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
    dst = torch.cat([torch.arange(n) + b * row_stride * S_max for b, n in enumerate(lens)])
    ids, pos, doc, last, src, dst = (x.to(device, non_blocking=True) for x in (ids, pos, doc, last, torch.cat(src), dst))
    if embed is not None:
        emb = embed(ids, lens, Tp)                                                         # [Tp, H]
    else:
        emb = _embed_touch_audio(lm, proj_w, prompts, ids, lens, Tp, device)
    kv = []
    h = lm.model(inputs_embeds=emb[None], position_ids=pos[None], attention_mask=doc[None], keep_rows=last, kv_out=kv)
    for (k, v), kc, vc in zip(kv, cache.k, cache.v):
        Nkv, D = k.shape[2], k.shape[3]
        kc.view(-1, Nkv, D).index_copy_(0, dst, k[0].index_select(0, src))
        vc.view(-1, Nkv, D).index_copy_(0, dst, v[0].index_select(0, src))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=device)
    cache.hist.view(-1).index_copy_(0, torch.cat([torch.arange(n, device=device) + b * row_stride * cache.hist.shape[1]
                                                  for b, n in enumerate(lens)]), ids.index_select(0, src).to(torch.int32))
    cache.hist_len[::row_stride].copy_(lens_d)
    cache.cache_len[::row_stride].copy_(lens_d - 1)   # the step kernels count the prompt's last row (module docstring)
    cache.finished.zero_()
    cache.n_unfinished.fill_(B)
    return lm.lm_head(h[0])                                                                # [B, V]


def _decode_layer(layer, delta, residual, cos, sin, kc, vc, cache_len, table=None):
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
    if table is None:
        o = F.attn_decode(q.view(B, attn.num_heads, D), k.view(B, attn.num_kv_heads, D), v.view(B, attn.num_kv_heads, D),
                          kc, vc, cache_len, attn.scaling)
    else:
        o = F.attn_decode_beam(q.view(B, attn.num_heads, D), k.view(B, attn.num_kv_heads, D),
                               v.view(B, attn.num_kv_heads, D), kc, vc, cache_len, table, attn.scaling)
    a = F.linear_group(o.view(B, attn.num_heads * D), [(attn.o_proj.weight, None)])[0]
    x, residual = layer.post_attention_layernorm(a, residual)
    return layer.mlp(x), residual


def decode_logits(lm, cache, table: Optional[torch.Tensor] = None,
                  inputs_embeds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decode step of every row: the newest token of the history at position cache_len -> logits [B, V]
    (its key / value are appended to the caches; cache_len itself is advanced by the greedy step).  `table` int32
    [B, S_max]: the rows are beams that read their cached keys / values through it (BeamState.src).  `inputs_embeds`
    [B, H]: the step's input rows where they are not embed(newest token) (Kimi-Audio: the sum of two embeddings, written
    by tn_kimi_text_step); by default they are gathered from the history."""
    if inputs_embeds is None:
        tok = cache.hist.gather(1, (cache.hist_len.to(torch.int64) - 1)[:, None])[:, 0]
        x = lm.model.embed_tokens(tok.to(torch.int64))                                      # [B, H]
    else:
        x = inputs_embeds
    cos, sin = lm.model.rotary_emb(cache.cache_len.to(torch.int64), x.dtype)
    delta, residual = x, None
    for layer, kc, vc in zip(lm.model.layers, cache.k, cache.v):
        delta, residual = _decode_layer(layer, delta, residual, cos, sin, kc, vc, cache.cache_len, table)
    h, _ = lm.model.norm(delta, residual)
    return lm.lm_head(h)


@torch.no_grad()
def generate(model, prompts: Prompts, cfg: Optional[GenerationConfig] = None, return_cache: bool = False,
             row_keys: Optional[torch.Tensor] = None, embed: Optional[EmbedFn] = None, return_scores: bool = False):
    """Greedy, sampled or beam-search generation for a batch of prompts -> int64 [B, N] generated ids (the prompt
    excluded), `pad` after a row's eos — the tensor HF generate() returns behind the prompt columns.  `model`: TouchAudioForCausalLM,
    Qwen2AudioPackedForConditionalGeneration (with its `embed` builder) or PackedCausalLM, bf16, on the device.

    Without do_sample and with at most one eos id every step is tn_greedy_step (repetition penalty, n-gram ban, argmax);
    otherwise tn_sample_step (penalty, temperature, top-k, top-p, draw).  `row_keys` int64 [B] (default arange(B)) key
    the draws with cfg.seed and the step: a row draws the same tokens whatever batch it is decoded in.

    With cfg.num_beams > 1 (and no do_sample): HF's beam search, tn_beam_step per token; the result is every utterance's
    best finished hypothesis, and `return_cache` hands out the BeamState that holds the scores.

    `return_scores`, cfg.output_scores or cfg.top_alternatives > 0: a `TokenScores` of the generated tokens comes back as
    the last element, (ids, scores) or (ids, cache, scores) — one tn_token_scores launch per step on the raw logits (when a
    `sequence_bias` plan edits the logits, it edits a copy).  cfg.nbest > 1 (beam search): (ids [B, nbest, N], scores
    [B, nbest], count [B]) of `BeamState.nbest` in place of ids, the TokenScores then [B * nbest, N] in that order.  With
    no knob set nothing of this runs."""
    cfg = cfg or GenerationConfig()
    cfg.check_scores()
    scored = bool(return_scores) or cfg.wants_scores
    n_alt = int(cfg.top_alternatives)
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
    n_new = cfg.new_tokens(max(lens))
    if n_new <= 0:
        if scored or int(cfg.nbest) > 1:
            raise ValueError("generate: no room for a new token (max_length <= the longest prompt): nothing to score")
        return torch.empty(B, 0, dtype=torch.int64, device=device)
    penalty, ngram = float(cfg.repetition_penalty), int(cfg.no_repeat_ngram_size)
    if int(cfg.num_beams) != 1:
        return _beam_search(model, lm, proj_w, prompts, cfg, eos, pad, lens, n_new, device, embed, return_cache, scored)
    greedy = not cfg.do_sample and len(eos) <= 1
    if not greedy:
        if ngram > 0:
            raise ValueError("generate: no_repeat_ngram_size > 0 is only supported for greedy search with one eos id "
                             f"(do_sample={cfg.do_sample}, eos ids {eos})")
        if len(eos) > _MAX_EOS:
            raise ValueError(f"generate: at most {_MAX_EOS} eos ids (got {len(eos)})")
        if row_keys is None:
            row_keys = torch.arange(B, dtype=torch.int64, device=device)
        row_keys = row_keys.to(device=device, dtype=torch.int64).contiguous()
        if tuple(row_keys.shape) != (B,):
            raise ValueError(f"generate: row_keys must have shape [{B}]")
    chunk = max(1, int(cfg.cache_chunk))
    cache = KVCache.allocate(len(lm.model.layers), B, max(lens) + min(n_new, chunk), c.num_key_value_heads, c.head_dim,
                             device)
    S_full = max(lens) + n_new
    plan = ConstraintPlan.build(cfg.sequence_bias, cfg.min_new_tokens, eos, int(c.vocab_size), device)
    prompt_len = torch.tensor(lens, dtype=torch.int32, device=device) if plan is not None else None
    scores = TokenScores.buffers(B, cache.capacity, n_alt, device) if scored else None

    def step(raw):
        logits = raw
        if plan is not None:                       # HF's order: SequenceBiasLogitsProcessor before the repetition penalty
            if scored:
                logits = raw.clone()               # the scores are those of lm_head's logits, not of the edited ones
            F.constrain_logits_(logits, cache.hist, cache.hist_len, plan, prompt_len)
        if greedy:
            F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, penalty,
                          ngram, eos[0] if eos else -1, pad)
        else:
            F.sample_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, penalty,
                          cfg.do_sample, cfg.temperature, cfg.top_k, cfg.top_p, cfg.seed, eos, pad, row_key=row_keys)
        if scored:                                 # the token the step kernel has just appended, in its history column
            F.token_scores_(raw, cache.hist, cache.hist_len, scores, n_alt)

    step(_prefill(lm, proj_w, prompts, cache, device, embed))
    steps = 1
    while steps < n_new:
        if steps % max(1, int(cfg.check_every)) == 0 and int(cache.n_unfinished.item()) == 0:
            break
        # the next step writes key / value slot lens[b] + steps - 1 and history slot lens[b] + steps
        if max(lens) + steps >= cache.capacity:
            cache.grow(min(S_full, 2 * cache.capacity))
            if scored:
                scores.grow(cache.capacity)
        step(decode_logits(lm, cache))
        steps += 1
    idx = torch.tensor(lens, dtype=torch.int64, device=device)[:, None] + torch.arange(steps, device=device)[None]
    out = cache.hist.gather(1, idx).to(torch.int64)
    # HF stops at the first step after which every row is finished: drop the all-pad columns the check interval added
    if eos:
        is_eos = torch.isin(out, torch.tensor(eos, dtype=torch.int64, device=device))
        first = torch.where(is_eos.any(1), is_eos.to(torch.int8).argmax(1), torch.full_like(out[:, 0], steps - 1))
        out = out[:, :int(first.max()) + 1]
    if scored:
        result = scores.columns(idx[:, :out.shape[1]]).close(_generated_lengths(out, eos))
        return (out, cache, result) if return_cache else (out, result)
    return (out, cache) if return_cache else out


def _beam_search(model, lm, proj_w, prompts: Prompts, cfg: GenerationConfig, eos, pad, lens, n_new, device, embed,
                 return_cache, scored: bool = False):
    """generate() with num_beams > 1: HF's beam search, one tn_beam_step per token.  The prompts are prefilled once, into
    the first row of every utterance; the K beams of an utterance read them, and every later key, through the table."""
    cfg.check_beams(eos)
    K, c = int(cfg.num_beams), lm.config
    chunk = max(1, int(cfg.cache_chunk))
    st = BeamState.allocate(len(lm.model.layers), len(lens), K, max(lens) + min(n_new, chunk), c.num_key_value_heads,
                            c.head_dim, device)
    S_full = max(lens) + n_new
    kw = dict(penalty=float(cfg.repetition_penalty), ngram=int(cfg.no_repeat_ngram_size), eos=eos, n_new=n_new,
              length_penalty=float(cfg.length_penalty), early_stopping=cfg.early_stopping)
    plan = ConstraintPlan.build(cfg.sequence_bias, cfg.min_new_tokens, eos, int(c.vocab_size), device)
    if plan is not None:
        prompt_len = torch.tensor(lens, dtype=torch.int32, device=device).repeat_interleave(K)
        edits = plan.edit_buffers(len(lens) * K)

    def step(logits):
        if plan is None:
            F.beam_step(logits, st, **kw)
        else:                                      # the totals go onto the log-probabilities inside the step
            F.constrain_logits_(logits, st.hist, st.hist_len, plan, prompt_len, num_beams=K, edits=edits)
            F.beam_step(logits, st, edits=edits, **kw)

    step(_prefill(lm, proj_w, prompts, st, device, embed, row_stride=K))                      # one live row per utterance
    steps = 1
    while steps < n_new:
        if steps % max(1, int(cfg.check_every)) == 0 and int(st.n_unfinished.item()) == 0:
            break
        if max(lens) + steps >= st.capacity:
            st.grow(min(S_full, 2 * st.capacity))
        step(decode_logits(lm, st, table=st.src))
        steps += 1
    n_best = int(cfg.nbest)
    if n_best == 1 and not scored:
        out, _ = st.best(lens, pad)
        return (out, st) if return_cache else out
    # N-best lists and per-token scores read the finished set; the scores of every returned hypothesis come from ONE
    # teacher-forced forward behind the search (tn_beam_step keeps sums, not per-token terms)
    ids, hyp_score, count = st.nbest(lens, pad, n_best)
    out = (ids, hyp_score, count) if n_best > 1 else (ids[:, 0],)
    if return_cache:
        out += (st,)
    if scored:
        rows = ids.reshape(len(lens) * n_best, -1)
        n_tok = _generated_lengths(rows, eos)
        n_tok = torch.where((hyp_score.reshape(-1) > -math.inf), n_tok, torch.zeros_like(n_tok))     # (missing hypotheses)
        repeated = Prompts(input_ids=[t for t in prompts.input_ids for _ in range(n_best)],
                           input_features=None if prompts.input_features is None
                           else [f for f in prompts.input_features for _ in range(n_best)])
        conts = [r[:int(n)].cpu() for r, n in zip(rows, n_tok.tolist())]
        if embed is not None:                      # the builder was made for the prompts alone: ask it for the documents'
            rebuild = getattr(embed, "for_documents", None)
            if rebuild is None:
                raise ValueError("generate: per-token scores of a beam search need an `embed` builder that offers "
                                 "for_documents(documents, repeat) (models.qwen2_audio.inference_qwen2_audio.audio_embedder)")
            embed = rebuild(with_continuations(repeated, conts), n_best)
        out += (score_continuations(model, repeated, conts, k=int(cfg.top_alternatives), embed=embed),)
    return out[0] if len(out) == 1 else out


def with_continuations(prompts: Prompts, continuations) -> Prompts:
    """Every prompt with its continuation appended: the documents `score_continuations` packs (feature rows of the
    continuation's slots are zero).  An `embed` builder for those documents is built from this."""
    if len(continuations) != len(prompts):
        raise ValueError(f"score_continuations: {len(continuations)} continuations for {len(prompts)} prompts")
    conts = [torch.as_tensor(c, dtype=torch.int64).reshape(-1).cpu() for c in continuations]
    ids = [torch.cat([p.reshape(-1).cpu().to(torch.int64), c]) for p, c in zip(prompts.input_ids, conts)]
    feats = None
    if prompts.input_features is not None:
        feats = [torch.cat([f, f.new_zeros(c.numel(), f.shape[1])]) for f, c in zip(prompts.input_features, conts)]
    return Prompts(input_ids=ids, input_features=feats)


@torch.no_grad()
def score_continuations(model, prompts: Prompts, continuations, k: int = 0, embed: Optional[EmbedFn] = None,
                        rows_per_chunk: int = 4096) -> TokenScores:
    """Teacher-forced scores of given continuations — the rescoring entry point: `TokenScores` [B, N] (N the longest
    continuation; columns behind a shorter one read 0 / -1) of continuation b (token ids, possibly none) behind prompt b.
    One packed, document-masked forward over prompt + continuation, the prefill's construction with `keep_rows` = the row
    in front of every continuation token; lm_head runs on at most `rows_per_chunk` of those rows at a time and
    tn_token_scores (token mode) scores each chunk, so the [rows, V] logits never exist as a whole.  `confidence` is
    exp(mean logp) over the whole continuation (1 for an empty one).  `model` as for `generate`; `embed`: the embedding
    builder of the documents `with_continuations(prompts, continuations)` (Qwen2-Audio: audio_embedder over them)."""
    _check_alternatives("score_continuations", k)
    if int(rows_per_chunk) < 1:
        raise ValueError(f"score_continuations: rows_per_chunk = {rows_per_chunk} must be >= 1")
    lm, proj_w = _parts(model)
    _check_model(model, lm)
    if len(prompts) == 0:
        raise ValueError("score_continuations: no prompts")
    if any(int(t.numel()) == 0 for t in prompts.input_ids):
        raise ValueError("score_continuations: empty prompt")
    device = lm.model.embed_tokens.weight.device
    docs = with_continuations(prompts, continuations)
    plens = [int(t.numel()) for t in prompts.input_ids]
    lens = [int(t.numel()) for t in docs.input_ids]
    clens = [n - p for n, p in zip(lens, plens)]
    B, T, N = len(lens), sum(lens), max(clens)
    result = TokenScores.buffers(B, N, int(k), device)
    n_rows = sum(clens)
    if n_rows == 0:
        return result.close(torch.tensor(clens))
    Tp = (T + 255) // 256 * 256
    ids = torch.zeros(Tp, dtype=torch.int64)
    pos = torch.zeros(Tp, dtype=torch.int64)
    doc = torch.zeros(Tp, dtype=torch.int32)
    rows, toks, slot = [], [], []
    o = 0
    for b, t in enumerate(docs.input_ids):
        n, p, c = lens[b], plens[b], clens[b]
        ids[o:o + n] = t
        pos[o:o + n] = torch.arange(n)
        doc[o:o + n] = b + 1
        rows.append(torch.arange(c) + (o + p - 1))                # the row in front of continuation token j
        toks.append(t[p:])
        slot.append(torch.arange(c) + b * N)
        o += n
    ids, pos, doc, rows, toks, slot = (x.to(device, non_blocking=True) for x in
                                       (ids, pos, doc, torch.cat(rows), torch.cat(toks).to(torch.int32), torch.cat(slot)))
    if embed is not None:
        emb = embed(ids, lens, Tp)
    else:
        emb = _embed_touch_audio(lm, proj_w, docs, ids, lens, Tp, device)
    h = lm.model(inputs_embeds=emb[None], position_ids=pos[None], attention_mask=doc[None], keep_rows=rows)[0]   # [n_rows, H]
    step = int(rows_per_chunk)
    for a in range(0, n_rows, step):
        logp, ent, alt_id, alt_logp = F.token_scores(lm.lm_head(h[a:a + step]), toks[a:a + step], int(k))
        at = slot[a:a + step]
        result.logp.view(-1).index_copy_(0, at, logp)
        result.entropy.view(-1).index_copy_(0, at, ent)
        result.alt_id.view(B * N, -1).index_copy_(0, at, alt_id)
        result.alt_logp.view(B * N, -1).index_copy_(0, at, alt_logp)
    return result.close(torch.tensor(clens))


def trim_at_eos(ids: torch.Tensor, eos: Union[int, Sequence[int]]) -> List[List[int]]:
    """[B, N] generated ids -> per row the ids in front of the first eos (the eos and the padding behind it dropped);
    `eos` one id or several."""
    stop = {int(eos)} if isinstance(eos, int) else {int(e) for e in eos}
    rows = []
    for r in ids.tolist():
        cut = next((i for i, t in enumerate(r) if t in stop), len(r))
        rows.append(r[:cut])
    return rows


# ------------------------------------------------------------------------------------ command-line side of the scores
def add_score_arguments(ap, nbest: bool = True) -> None:
    """--output_scores / --top_alternatives (and --nbest) of the inference command lines."""
    ap.add_argument("--output_scores", action="store_true",
                    help='records gain "confidence" (exp of the mean token log-probability), "token_logprobs" and '
                         '"token_entropy": one entry per generated token up to and including the eos, from the logits as '
                         "lm_head wrote them (no hotword edit, penalty or temperature)")
    ap.add_argument("--top_alternatives", type=int, default=0, metavar="K",
                    help=f'records gain "alternatives": per token its K <= {MAX_ALTERNATIVES} most likely ids as [id, logp] '
                         "(implies --output_scores)")
    if nbest:
        ap.add_argument("--nbest", type=int, default=1, metavar="N",
                        help='beam search (--num_beams >= N): records gain "nbest", the N best finished hypotheses as '
                             '{"predict_ids", "predict", "score"[, "confidence"]}, rank 1 being the prediction itself; an '
                             "utterance that finished fewer lists fewer")


def add_longform_arguments(ap, switch: bool = True) -> None:
    """--long_form and the knobs of longform.LongFormConfig (longform.longform_from_args reads them back).  The defaults
    are Kaldi's compute-vad-energy defaults and common segmenting values; nobody has tuned them for these decoders."""
    if switch:
        ap.add_argument("--long_form", action="store_true",
                        help="recordings longer than --max_segment_s are cut into segments by an energy VAD on the device "
                             'and decoded segment by segment; their records gain "segments".  Shorter recordings and '
                             "runs without this flag are decoded as before")
    ap.add_argument("--max_segment_s", type=float, default=30.0, help="longest segment, and the length from which a "
                                                                      "recording is segmented at all")
    ap.add_argument("--vad_energy_threshold", type=float, default=5.0)
    ap.add_argument("--vad_energy_mean_scale", type=float, default=0.5)
    ap.add_argument("--vad_frames_context", type=int, default=0)
    ap.add_argument("--vad_proportion_threshold", type=float, default=0.6)
    ap.add_argument("--vad_min_silence_ms", type=float, default=300.0, help="shorter gaps between voiced runs are closed")
    ap.add_argument("--vad_min_speech_ms", type=float, default=100.0, help="shorter voiced runs are dropped")
    ap.add_argument("--vad_pad_ms", type=float, default=100.0, help="every voiced run grows by this on both sides")


def _json_number(x: float):
    return x if math.isfinite(x) else None


def score_fields(scores: TokenScores, row: int, n: Optional[int] = None, keep: Optional[Sequence[int]] = None) -> dict:
    """The record keys of one row of a `TokenScores` (tensors anywhere): "confidence", "token_logprobs", "token_entropy"
    and, with alternatives, "alternatives" ([[id, logp], ...] per token; a logp of -inf reads null).  `n`: the row's tokens
    (default: all columns); `keep`: the columns to list instead (Kimi-Audio: the tokens that are text)."""
    cols = list(range(scores.logp.shape[1] if n is None else int(n))) if keep is None else [int(c) for c in keep]
    lp, ent = scores.logp[row].tolist(), scores.entropy[row].tolist()
    out = {"confidence": _json_number(float(scores.confidence[row])),
           "token_logprobs": [_json_number(lp[c]) for c in cols], "token_entropy": [_json_number(ent[c]) for c in cols]}
    if scores.k:
        ai, al = scores.alt_id[row].tolist(), scores.alt_logp[row].tolist()
        out["alternatives"] = [[[int(i), _json_number(v)] for i, v in zip(ai[c], al[c]) if i >= 0] for c in cols]
    return out


def record_fields(out, cfg: GenerationConfig, eos: Sequence[int]):
    """What generate() returned under `cfg` -> (per utterance the ids in front of the first eos, per utterance the extra
    record keys as a dict: the `score_fields` of the prediction and "nbest", a list of {"predict_ids", "score"[,
    "confidence"]} — the command line adds "predict").  No knob set: empty dicts."""
    n_best, scored = int(cfg.nbest), cfg.wants_scores
    if n_best == 1 and not scored:
        return trim_at_eos(out, eos), [{} for _ in range(out.shape[0])]
    parts = list(out) if isinstance(out, tuple) else [out]
    ts = parts.pop() if scored else None
    if n_best > 1:
        ids3, hyp_score, count = (t.cpu() for t in parts[:3])
    else:
        ids3, hyp_score, count = parts[0].cpu()[:, None], None, None
    B = ids3.shape[0]
    n_tok = _generated_lengths(ids3.reshape(B * n_best, -1), eos).tolist()
    top = trim_at_eos(ids3[:, 0], eos)
    extras = []
    for b in range(B):
        extra = score_fields(ts, b * n_best, n_tok[b * n_best]) if scored else {}
        if n_best > 1:
            hyps = trim_at_eos(ids3[b, :int(count[b])], eos)
            extra["nbest"] = [dict(predict_ids=h, score=float(hyp_score[b, j]),
                                   **({"confidence": _json_number(float(ts.confidence[b * n_best + j]))} if scored else {}))
                              for j, h in enumerate(hyps)]
        extras.append(extra)
    return top, extras


# ------------------------------------------------------------------------------------ command-line side of the constraints
def add_constraint_arguments(ap) -> None:
    """--hotwords / --hotword_bias / --forbid_words / --min_new_tokens of the inference command lines."""
    ap.add_argument("--hotwords", default=None, metavar="FILE",
                    help="one phrase per line, tokenised with the checkpoint's tokenizer (no special tokens); every token "
                         "along a phrase is boosted by --hotword_bias once the tokens before it were emitted")
    ap.add_argument("--hotword_bias", type=float, default=2.0,
                    help="added to the logit (beam search: the log-probability) of a hotword's next token; 2.0 is a "
                         "starting point that nobody has tuned")
    ap.add_argument("--forbid_words", default=None, metavar="FILE",
                    help="one phrase per line; its token sequence can never be completed (sequence_bias at -inf)")
    ap.add_argument("--min_new_tokens", type=int, default=None, help="no eos before this many generated tokens")


def read_phrases(path: str, tokenizer) -> List[List[int]]:
    """The token ids of every non-empty line of `path`, without special tokens.  No tokenizer: refused."""
    if tokenizer is None:
        raise ValueError(f"{path}: phrases are tokenised with the checkpoint's tokenizer, and the checkpoint directory "
                         "holds none (tokenizer.json / tokenizer_config.json)")
    out = []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            text = line.strip()
            if not text:
                continue
            ids = [int(t) for t in tokenizer.encode(text, add_special_tokens=False)]
            if not ids:
                raise ValueError(f"{path}:{n}: {text!r} has no tokens")
            out.append(ids)
    return out


def constraints_from_args(args, tokenizer, sequence_bias: Optional[dict] = None) -> Optional[dict]:
    """`sequence_bias` of a command line: what the generation config carries, then the hotwords (every prefix at
    --hotword_bias), then the forbidden phrases (whole sequences at -inf); a later entry replaces an earlier one."""
    out = dict(normalize_sequence_bias(sequence_bias) or {})
    if args.hotwords:
        out.update(hotword_bias(read_phrases(args.hotwords, tokenizer), args.hotword_bias))
    if args.forbid_words:
        out.update({tuple(ids): float("-inf") for ids in read_phrases(args.forbid_words, tokenizer)})
    return normalize_sequence_bias(out)
