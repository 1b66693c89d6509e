"""Fixtures of the scoring step, tests/golden/error_rate/, produced by running the REFERENCE's scorer on the CPU:

    ref.txt, hyp.txt             about 150 utterances of Chinese characters and ASCII words; among them a hypothesis with no
                                 reference, a reference whose text is empty, a hypothesis line holding only a uid, and a
                                 duplicated uid in either file
    DETAILS_<tok>.txt            the result file of `touchnet/bin/error_rate_zh --tokenizer <tok>` (whole program, subprocess)
    stdout_<tok>.txt             what it printed, for tok in whitespace, char
    final.jsonl                  a small decoder output; trans.txt / raw_rec.txt: what the recipe's
                                 local/extract_trans_and_pred.py writes from it
    edit_align.npz               about 400 token pairs (alphabets of 2, 3, 5 and 50 symbols, lengths 0-40, half of them noisy
                                 copies; the two witnesses of the tie rule first) with the arcs, counts and score of the
                                 reference's EditDistance / CountEdits, loaded from the file itself

Runs only in the build container (the reference is not on the GPU box, and no test imports this module):
    python tests/golden/make_golden_error_rate.py"""
import importlib.machinery
import importlib.util
import json
import os
import random
import runpy
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
SCORER = f"{REF}/touchnet/bin/error_rate_zh"
EXTRACTOR = f"{REF}/examples/audio/sft/asr/wenetspeech/local/extract_trans_and_pred.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "error_rate")
SEED = 20260
HANZI = "的一是在不了有和人这中大为上个国我以要他时来用们生到作地于出就分对成会可主发年动同工也能下过子说产种面而方后多定行学法所民得经"
WORDS = ["AI", "GPU", "ok", "wifi", "APP", "5G", "hello", "world", "B", "x1"]
CODES = {"C": 0, "S": 1, "I": 2, "D": 3}


def load_scorer():
    """the scorer has no .py suffix: a SourceFileLoader by hand; its __main__ block does not run"""
    loader = importlib.machinery.SourceFileLoader("error_rate_zh_reference", SCORER)
    spec = importlib.util.spec_from_loader(loader.name, loader)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    loader.exec_module(mod)
    return mod


def noisy(rng, seq, alphabet, rate=0.25):
    out = []
    for tok in seq:
        u = rng.random()
        if u < rate / 3:
            continue                                       # deletion
        if u < 2 * rate / 3:
            out.append(rng.choice(alphabet))               # substitution (may draw the same token)
        else:
            out.append(tok)
        if rng.random() < rate / 3:
            out.append(rng.choice(alphabet))               # insertion
    return out


def utterance(rng):
    units = []
    for _ in range(rng.randint(2, 9)):
        units.append(rng.choice(WORDS) if rng.random() < 0.25 else "".join(rng.choice(HANZI) for _ in range(rng.randint(1, 4))))
    return units


def make_corpus(rng):
    ref_lines, hyp_lines = [], []
    for n in range(150):
        uid = f"utt_{n:04d}"
        ref = utterance(rng)
        kind = rng.random()
        if kind < 0.25:
            hyp = list(ref)
        elif kind < 0.85:                                   # noise inside the units (characters) and among them (words)
            hyp = ["".join(noisy(rng, u, HANZI, 0.2)) if u not in WORDS else u for u in noisy(rng, ref, WORDS + list(HANZI[:8]), 0.2)]
            hyp = [u for u in hyp if u]
        else:
            hyp = utterance(rng)
        ref_lines.append(f"{uid} {' '.join(ref)}")
        hyp_lines.append(f"{uid} {' '.join(hyp)}".rstrip())
    hyp_lines.insert(17, "extra_hyp_without_ref 没有 参考")
    ref_lines.insert(40, "utt_empty_reference")
    hyp_lines.insert(41, "utt_empty_reference 空 的 参考")
    ref_lines.insert(60, "utt_only_uid_in_hyp 只有 编号 ok")
    hyp_lines.insert(61, "utt_only_uid_in_hyp")
    ref_lines.insert(5, "utt_0100 这 一 行 被 后 面 的 替 换")       # the later line of utt_0100 replaces these two
    hyp_lines.insert(6, "utt_0101 这 一 行 也 被 替 换 GPU")
    ref_lines.append("ref_without_hyp 没有 假设")
    ref_lines.append("")                                     # blank lines are skipped
    hyp_lines.insert(3, "   ")
    return "\n".join(ref_lines) + "\n", "\n".join(hyp_lines) + "\n"


def run_scorer(tokenizer, ref_path, hyp_path):
    with tempfile.TemporaryDirectory() as tmp:
        details = os.path.join(tmp, "DETAILS.txt")
        r = subprocess.run([sys.executable, "-B", SCORER, "--tokenizer", tokenizer, "--ref", ref_path, "--hyp", hyp_path, details],
                           capture_output=True, check=True)
        return open(details, "rb").read(), r.stdout


def make_jsonl(rng):
    lines = []
    for n in range(24):
        key, txt = f"BAC009S{n:04d}", " ".join(utterance(rng))
        label = json.dumps({"key": key, "wav": f"/data/{key}.wav", "txt": txt}, ensure_ascii=False)
        pred = txt if n % 3 else "".join(noisy(rng, txt, HANZI, 0.2))
        if n % 5 == 1:
            predict = json.dumps({"transcription": pred, "lang": "zh"}, ensure_ascii=False)     # a JSON object in a string
        elif n % 5 == 2:
            predict = {"transcription": pred}                                                      # a JSON object
        else:
            predict = pred
        if n == 7:
            predict = "   "                                                                        # empty without spaces
        if n == 9:
            predict = ""
        lines.append(json.dumps({"label": label, "predict_ids": [1, 2, 3], "predict": predict}, ensure_ascii=False))
    lines.insert(10, lines[4].replace("predict_ids", "again"))                                     # the first of a key wins
    lines.insert(12, json.dumps({"label": json.dumps({"key": "BAC009S0003", "txt": "重 复"}, ensure_ascii=False), "predict": "别 的"},
                                ensure_ascii=False))
    lines.insert(15, "")
    lines.insert(16, "{not json")
    lines.insert(18, json.dumps({"label": json.dumps({"key": "no_predict", "txt": "x"})}))
    return "\n".join(lines) + "\n"


def run_extractor(jsonl_text):
    try:
        import tqdm  # noqa: F401
    except ImportError:                                     # the extractor only wraps its loop in tqdm(...)
        stub = types.ModuleType("tqdm")
        stub.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = stub
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "final.jsonl")
        with open(path, "w", encoding="utf-8") as f:
            f.write(jsonl_text)
        argv, sys.argv = sys.argv, [EXTRACTOR, "--jsonl", path]
        try:
            runpy.run_path(EXTRACTOR, run_name="__main__")
        finally:
            sys.argv = argv
        for name in ("trans.txt", "raw_rec.txt"):
            shutil.copyfile(os.path.join(tmp, name), os.path.join(OUT, name))


def make_pairs(rng, scorer):
    pairs = [(list(b"ab"), list(b"ba")), (list(b"aab"), list(b"ab"))]            # D C I; C D C
    for n in range(400):
        alphabet = list(range([2, 3, 5, 50][n % 4]))
        ref = [rng.choice(alphabet) for _ in range(rng.randint(1, 40))]
        hyp = noisy(rng, ref, alphabet, 0.3)[:40] if n % 2 else [rng.choice(alphabet) for _ in range(rng.randint(0, 40))]
        pairs.append((ref, hyp))
    ref_tok, hyp_tok, ops, ref_off, hyp_off, ops_off, counts, score = [], [], [], [0], [0], [0], [], []
    for ref, hyp in pairs:
        path, s = scorer.EditDistance(ref, hyp)
        ops += [CODES[arc.edit_type] for arc in path]
        counts.append(scorer.CountEdits(path))
        score.append(s)
        ref_tok += ref
        hyp_tok += hyp
        ref_off.append(len(ref_tok)); hyp_off.append(len(hyp_tok)); ops_off.append(len(ops))
    np.savez_compressed(os.path.join(OUT, "edit_align.npz"), seed=SEED, ref_tok=np.asarray(ref_tok, np.int32),
                        hyp_tok=np.asarray(hyp_tok, np.int32), ops=np.asarray(ops, np.uint8), ref_off=np.asarray(ref_off, np.int32),
                        hyp_off=np.asarray(hyp_off, np.int32), ops_off=np.asarray(ops_off, np.int32),
                        counts=np.asarray(counts, np.int32), score=np.asarray(score, np.float64))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(SEED)
    ref_text, hyp_text = make_corpus(rng)
    for name, text in (("ref.txt", ref_text), ("hyp.txt", hyp_text)):
        with open(os.path.join(OUT, name), "w", encoding="utf8") as f:
            f.write(text)
    for tok in ("whitespace", "char"):
        details, stdout = run_scorer(tok, os.path.join(OUT, "ref.txt"), os.path.join(OUT, "hyp.txt"))
        open(os.path.join(OUT, f"DETAILS_{tok}.txt"), "wb").write(details)
        open(os.path.join(OUT, f"stdout_{tok}.txt"), "wb").write(stdout)
    jsonl = make_jsonl(rng)
    with open(os.path.join(OUT, "final.jsonl"), "w", encoding="utf-8") as f:
        f.write(jsonl)
    run_extractor(jsonl)
    make_pairs(rng, load_scorer())
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"wrote {sorted(os.listdir(OUT))}: {total} bytes")


if __name__ == "__main__":
    main()
