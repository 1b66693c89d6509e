"""The recipe's scoring step (examples/audio/sft/asr/wenetspeech/run.sh stage 4): token and sentence error rates of a set
of hypotheses against their references, with the per-utterance alignments, as touchnet/bin/error_rate_zh prints them, and
the reading of the decoders' `part_* / final.jsonl` files that local/extract_trans_and_pred.py does before it.

The alignment itself — the scorer's dynamic programme with its tie rule, insertion before deletion before the diagonal —
runs on the device (functional.edit_align -> tn_edit_align); everything here is the host's share: reading, tokenizing,
mapping tokens to int32 ids, selecting the utterances and printing.  `evaluate(..., align_fn=...)` takes another aligner
with the same signature (the tests pass a plain-Python one, so the printing can be checked without a GPU).

Text normalisation (touchnet/bin/textnorm_zh.py) is not part of this module."""
from __future__ import annotations

import json
import os
import sys
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

EDIT_LETTERS = "CSID"                        # the arc codes of functional.edit_align: 0 = C, 1 = S, 2 = I, 3 = D
_C, _S, _I, _D = range(4)


@dataclass
class Utterance:
    uid: str
    text: str


def load_utterances(path: str, format: str = "text") -> Dict[str, Utterance]:
    """`uid text...` per line; a line with a uid alone has the empty text; a later line of the same uid replaces an earlier one"""
    if format != "text":
        raise RuntimeError(f"Unsupported text format {format}")
    utts: Dict[str, Utterance] = {}
    with open(path, "r", encoding="utf8") as f:
        for line in f:
            cols = line.strip().split(maxsplit=1)
            if cols:
                utts[cols[0]] = Utterance(cols[0], cols[1] if len(cols) == 2 else "")
    return utts


def tokenize_text(text: str, tokenizer: str) -> List[str]:
    """`whitespace`: the words (WER); `char`: every character once all whitespace is dropped (CER)"""
    if tokenizer == "whitespace":
        return text.split()
    if tokenizer == "char":
        return list("".join(text.split()))
    raise RuntimeError(f"ERROR: Unsupported tokenizer {tokenizer}")


def token_error_rate(c: int, s: int, i: int, d: int) -> float:
    return 100.0 * (s + d + i) / (s + d + c)


@dataclass
class EvaluationResult:
    """the scorer's result record: the field names and their order are its JSON line's"""
    num_ref_utts: int = 0
    num_hyp_utts: int = 0
    num_eval_utts: int = 0                   # in both the references and the hypotheses, reference not empty
    num_hyp_without_ref: int = 0
    C: int = 0
    S: int = 0
    I: int = 0
    D: int = 0
    token_error_rate: float = 0.0
    num_utts_with_error: int = 0
    sentence_error_rate: float = 0.0
    details: List[str] = field(default_factory=list, repr=False, compare=False)   # the per-utterance lines, not in the JSON

    def to_json(self) -> str:
        return json.dumps({k: v for k, v in self.__dict__.items() if k != "details"})

    def to_kaldi(self) -> str:
        return (f"%WER {self.token_error_rate:.2f} [ {self.S + self.D + self.I} / {self.C + self.S + self.D}, {self.I} ins, "
                f"{self.D} del, {self.S} sub ]\n"
                f"%SER {self.sentence_error_rate:.2f} [ {self.num_utts_with_error} / {self.num_eval_utts} ]\n")

    def to_summary(self) -> str:
        rows = [("tokens:", self.C + self.S + self.D), ("edits: ", self.S + self.I + self.D), ("cor:   ", self.C),
                ("sub:   ", self.S), ("ins:   ", self.I), ("del:   ", self.D)]
        return ("==================== Overall Statistics ====================\n"
                f"num_ref_utts: {self.num_ref_utts}\n"
                f"num_hyp_utts: {self.num_hyp_utts}\n"
                f"num_hyp_without_ref: {self.num_hyp_without_ref}\n"
                f"num_eval_utts: {self.num_eval_utts}\n"
                f"sentence_error_rate: {self.sentence_error_rate:.2f}%\n"
                f"token_error_rate: {self.token_error_rate:.2f}%\n"
                "token_stats:\n"
                + "".join(f"  - {name}{value:>7}\n" for name, value in rows)
                + "============================================================\n")

    def write_details(self, stream) -> None:
        """the result file: every utterance's lines, then the summary and the blank line `print` adds after it"""
        for line in self.details:
            stream.write(line + "\n")
        stream.write(self.to_summary() + "\n")


def _display_width(s: str) -> int:
    """terminal columns: two for a CJK unified ideograph of U+4E00 .. U+9FA5, one for anything else"""
    return sum(2 if "\u4e00" <= ch <= "\u9fa5" else 1 for ch in s)


def alignment_lines(ref: Sequence[str], hyp: Sequence[str], ops: Sequence[int]) -> Tuple[str, str, str]:
    """the REF / HYP / EDIT lines of one alignment: `*` for a gap, nothing under a correct token, every column one wider
    than its widest entry"""
    rows = ["  REF  : ", "  HYP  : ", "  EDIT : "]
    r = h = 0
    for code in ops:
        cells = ["*" if code == _I else ref[r], "*" if code == _D else hyp[h], "" if code == _C else EDIT_LETTERS[code]]
        r += code != _I
        h += code != _D
        widths = [_display_width(c) for c in cells]
        for k in range(3):
            rows[k] += cells[k] + " " * (max(widths) + 1 - widths[k])
    assert r == len(ref) and h == len(hyp), "the arcs do not spell the two sequences"
    return rows[0], rows[1], rows[2]


def device_align(refs: List[List[int]], hyps: List[List[int]]):
    """the default aligner: tn_edit_align through functional.edit_align"""
    from .. import functional as F
    return F.edit_align(refs, hyps)


def evaluate(ref_utts: Dict[str, Utterance], hyp_utts: Dict[str, Utterance], tokenizer: str,
             align_fn: Optional[Callable] = None, warn=None) -> EvaluationResult:
    """Score the hypotheses that have a non-empty reference, in sorted uid order.  `align_fn(refs, hyps)` takes two lists
    of int id sequences and returns (C, S, I, D, ops) per pair; the default is the device op.  `warn(message)` is told
    about every hypothesis that is skipped."""
    align_fn = align_fn or device_align
    warn = warn or (lambda message: None)
    res = EvaluationResult(num_ref_utts=len(ref_utts), num_hyp_utts=len(hyp_utts))
    uids = []
    for uid in sorted(hyp_utts):
        if uid not in ref_utts:
            warn(f"Found {uid} without reference, skipping...")
            res.num_hyp_without_ref += 1
        elif not ref_utts[uid].text.strip():
            warn(f"Found {uid} with empty reference, skipping...")
        else:
            uids.append(uid)
    res.num_eval_utts = len(uids)
    if not uids:
        raise ValueError("no hypothesis has a non-empty reference: there is nothing to score")
    ids: Dict[str, int] = {}                                      # the call's own dictionary: equal tokens, equal ids
    to_ids = lambda tokens: [ids.setdefault(t, len(ids)) for t in tokens]
    refs = [tokenize_text(ref_utts[u].text, tokenizer) for u in uids]
    hyps = [tokenize_text(hyp_utts[u].text, tokenizer) for u in uids]
    aligned = align_fn([to_ids(t) for t in refs], [to_ids(t) for t in hyps])
    for uid, ref, hyp, pair in zip(uids, refs, hyps, aligned):
        _count(res, uid, ref, hyp, pair)
    return _close(res)


def _count(res: EvaluationResult, uid: str, ref: Sequence[str], hyp: Sequence[str], pair) -> None:
    """one aligned utterance into the result: its detail lines and its counts"""
    c, s, i, d, ops = pair
    ter = token_error_rate(c, s, i, d)
    res.details.append(f'{{"uid":{uid}, "score":{0.0 - (s + i + d)}, "ter":{ter:.2f}, "cor":{c}, "sub":{s}, "ins":{i}, '
                       f'"del":{d}}}')
    res.details.extend(alignment_lines(ref, hyp, [int(k) for k in ops]))
    res.C, res.S, res.I, res.D = res.C + c, res.S + s, res.I + i, res.D + d
    res.num_utts_with_error += ter > 0


def _close(res: EvaluationResult) -> EvaluationResult:
    res.sentence_error_rate = 100.0 * res.num_utts_with_error / res.num_eval_utts
    res.token_error_rate = token_error_rate(res.C, res.S, res.I, res.D)
    return res


def evaluate_oracle(ref_utts: Dict[str, Utterance], hyp_sets: Sequence[Dict[str, Utterance]], tokenizer: str,
                    align_fn: Optional[Callable] = None) -> EvaluationResult:
    """The oracle error rate of an N-best list: `hyp_sets` holds the hypothesis files in rank order (the scored file
    first); for every utterance that `evaluate` scores for the first set, the hypothesis with the fewest errors (S + I + D)
    among the sets that hold its key — ties to the earlier set, a set without the key is skipped — is the one counted.  All
    (utterance, set) pairs are aligned in ONE `align_fn` call.  The record's utterance counts are the first set's."""
    align_fn = align_fn or device_align
    first = hyp_sets[0]
    res = EvaluationResult(num_ref_utts=len(ref_utts), num_hyp_utts=len(first))
    uids = [u for u in sorted(first) if u in ref_utts and ref_utts[u].text.strip()]
    res.num_hyp_without_ref = sum(u not in ref_utts for u in first)
    res.num_eval_utts = len(uids)
    if not uids:
        raise ValueError("no hypothesis has a non-empty reference: there is nothing to score")
    ids: Dict[str, int] = {}
    to_ids = lambda tokens: [ids.setdefault(t, len(ids)) for t in tokens]
    pairs = [(u, n) for u in uids for n, hs in enumerate(hyp_sets) if u in hs]
    refs = {u: tokenize_text(ref_utts[u].text, tokenizer) for u in uids}
    hyps = [tokenize_text(hyp_sets[n][u].text, tokenizer) for u, n in pairs]
    aligned = align_fn([to_ids(refs[u]) for u, _ in pairs], [to_ids(h) for h in hyps])
    best: Dict[str, int] = {}
    for k, ((u, _), (c, s, i, d, _ops)) in enumerate(zip(pairs, aligned)):
        if u not in best or s + i + d < sum(aligned[best[u]][1:4]):          # (strictly fewer: ties stay with the earlier set)
            best[u] = k
    for u in uids:
        _count(res, u, refs[u], hyps[best[u]], aligned[best[u]])
    return _close(res)


def extract_trans_and_pred(jsonl_path: str, warn=None) -> Tuple[str, str]:
    """One decoder output file (a `part_i_of_n` or their concatenation `final.jsonl`) -> `trans.txt` and `raw_rec.txt` beside
    it, the scorer's two inputs.  A line is {"label": a JSON string holding `key` and `txt`, "predict": text, or a JSON
    object with `transcription`}; the first line of a key wins; a prediction that is empty once its spaces are removed
    leaves no `raw_rec.txt` line; a line that cannot be read is reported to `warn` and skipped.  Records with an "nbest" list
    (the decoders' --nbest) also leave `raw_rec.2.txt` .. `raw_rec.N.txt`, the lower-ranked hypotheses in the same format
    (`nbest_rec_path`), so the text normaliser applies to each file as it is."""
    warn = warn or (lambda message: None)
    out_dir = os.path.dirname(jsonl_path)
    trans_path, rec_path = os.path.join(out_dir, "trans.txt"), os.path.join(out_dir, "raw_rec.txt")
    seen = set()
    ranked = {}                                                   # rank (2 ..) -> the open raw_rec.{rank}.txt
    with open(jsonl_path, "r", encoding="utf-8") as fin, open(trans_path, "w", encoding="utf-8") as ftrans, \
            open(rec_path, "w", encoding="utf-8") as frec:
        for line in fin:
            line = line.strip()
            if not line:
                continue
            try:
                record = json.loads(line)
                label = json.loads(record["label"])
                key, txt, predict = label["key"], label["txt"], record["predict"]
                if isinstance(predict, str):                      # the text itself, or a JSON value written as a string
                    try:
                        predict = json.loads(predict)
                    except ValueError:
                        pass
                text = predict["transcription"] if isinstance(predict, dict) and "transcription" in predict else str(predict)
                if key in seen:
                    continue
                seen.add(key)
                ftrans.write(f"{key} {txt}\n")
                if text.replace(" ", ""):
                    frec.write(f"{key} {text}\n")
                for rank, hyp in enumerate(record.get("nbest") or [], 1):
                    if rank == 1:                                 # rank 1 is the prediction itself: raw_rec.txt
                        continue
                    if rank not in ranked:
                        ranked[rank] = open(nbest_rec_path(jsonl_path, rank), "w", encoding="utf-8")
                    if str(hyp["predict"]).replace(" ", ""):
                        ranked[rank].write(f"{key} {hyp['predict']}\n")
            except Exception as e:                                # noqa: BLE001  (a damaged line costs one utterance, not the run)
                warn(f"skipping a line of {jsonl_path}: {e!r}")
    for f in ranked.values():
        f.close()
    return trans_path, rec_path


def nbest_rec_path(jsonl_path: str, rank: int) -> str:
    """`raw_rec.{rank}.txt` beside a decoder output file: the rank-th hypothesis of every record that carries an "nbest"
    list of at least that length, in raw_rec.txt's format (rank 1 is raw_rec.txt itself)."""
    return os.path.join(os.path.dirname(jsonl_path), f"raw_rec.{int(rank)}.txt")


def main(argv=None) -> int:
    import argparse
    import logging
    ap = argparse.ArgumentParser(description="token / sentence error rate of hypotheses against references, aligned on the device")
    ap.add_argument("--tokenizer", choices=["whitespace", "char"], default="whitespace", help="whitespace for WER, char for CER")
    ap.add_argument("--ref-format", choices=["text"], default="text", help="first column the utterance id, the rest the text")
    ap.add_argument("--hyp-format", choices=["text"], default="text", help="first column the utterance id, the rest the text")
    ap.add_argument("--ref", type=str, help="reference file")
    ap.add_argument("--hyp", type=str, help="hypothesis file")
    ap.add_argument("--jsonl", type=str, nargs="+", metavar="FILE",
                    help="decoder outputs (part_i_of_n / final.jsonl): write trans.txt and raw_rec.txt beside each one; alone, "
                         "nothing is scored (text normalisation comes between the two steps)")
    ap.add_argument("--oracle", type=str, nargs="+", metavar="FILE", default=None,
                    help="further hypothesis files of the same utterances (raw_rec.2.txt ...): after the normal output, the "
                         "error rate of the per-utterance best hypothesis among --hyp and these, ties to the earlier file, "
                         "printed with the prefix `oracle: `")
    ap.add_argument("result_file", type=str, nargs="?")
    args = ap.parse_args(argv)
    logging.basicConfig(stream=sys.stderr, level=logging.INFO, format="[%(levelname)s] %(message)s")
    logging.info(args)
    for path in args.jsonl or []:
        trans, rec = extract_trans_and_pred(path, warn=logging.warning)
        logging.info(f"wrote {trans} and {rec}")
    ref, hyp = args.ref, args.hyp
    if args.jsonl and ref is None and hyp is None and args.result_file is None:
        return 0                                                  # extraction only
    if ref is None or hyp is None or args.result_file is None:
        ap.error("--ref, --hyp and result_file are required (or --jsonl alone, to write trans.txt / raw_rec.txt only)")
    res = evaluate(load_utterances(ref, args.ref_format), load_utterances(hyp, args.hyp_format), args.tokenizer,
                   warn=logging.warning)
    with open(args.result_file, "w+", encoding="utf8") as fo:
        res.write_details(fo)
    print(res.to_json())
    print(res.to_kaldi())
    if args.oracle:
        sets = [load_utterances(hyp, args.hyp_format)] + [load_utterances(p, args.hyp_format) for p in args.oracle]
        best = evaluate_oracle(load_utterances(ref, args.ref_format), sets, args.tokenizer)
        print("oracle: " + best.to_json())
        print("".join(f"oracle: {line}\n" for line in best.to_kaldi().splitlines()))
    return 0
