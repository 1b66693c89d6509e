"""The scoring step, the parts that need no GPU:
  - the plain-Python restatement of the scorer's tie rule (tests/edit_align_reference.py) against the arcs, counts and
    score that the reference's own EditDistance gave (tests/golden/error_rate/edit_align.npz, made by
    tests/golden/make_golden_error_rate.py);
  - metrics.error_rate.evaluate with that restatement as the aligner against the reference program's result file and
    stdout, byte for byte, for both tokenizers; the --jsonl extractor against the reference extractor's two files;
  - the refusals, by name, of functional.edit_align, and of the C entry point, which checks the whole descriptor table on
    the host and returns -22 before it uploads or launches anything;
  - the op's registration, prototype, header line and fake kernel."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

import edit_align_reference as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "error_rate")


@pytest.fixture(scope="module")
def pairs(golden):
    g = golden(os.path.join("error_rate", "edit_align.npz"))
    cut = lambda a, off, p: a[off[p]:off[p + 1]].tolist()
    n = g["counts"].shape[0]
    return [dict(ref=cut(g["ref_tok"], g["ref_off"], p), hyp=cut(g["hyp_tok"], g["hyp_off"], p),
                 ops=cut(g["ops"], g["ops_off"], p), counts=tuple(g["counts"][p].tolist()), score=float(g["score"][p]))
            for p in range(n)]


def _gold(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------ the restatement
def test_fixture_holds_what_its_maker_says(pairs):
    assert len(pairs) == 402
    assert all(1 <= len(p["ref"]) <= 40 and 0 <= len(p["hyp"]) <= 40 for p in pairs)
    assert any(len(p["hyp"]) == 0 for p in pairs) and any(len(p["ref"]) == 1 for p in pairs)
    assert {max(p["ref"]) < 2 for p in pairs[2:]} == {True, False}
    total = sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD))
    assert total < 300 * 1024, total


def test_restatement_equals_the_reference_on_every_fixture_pair(pairs):
    for n, p in enumerate(pairs):
        ops, counts, score = R.align(p["ref"], p["hyp"])
        assert ops == p["ops"], n
        assert counts == p["counts"] and score == p["score"] and repr(score) == repr(p["score"]), n


def test_the_two_witnesses_of_the_tie_rule(pairs):
    """a diagonal-first rule reaches the same cost with `S S` and `C C D`"""
    assert (bytes(pairs[0]["ref"]), bytes(pairs[0]["hyp"])) == (b"ab", b"ba") and R.letters(pairs[0]["ops"]) == "DCI"
    assert (bytes(pairs[1]["ref"]), bytes(pairs[1]["hyp"])) == (b"aab", b"ab") and R.letters(pairs[1]["ops"]) == "CDC"
    assert R.letters(R.align("ab", "ba")[0]) == "DCI" and R.align("ab", "ba")[1] == (1, 0, 1, 1)
    assert R.letters(R.align("aab", "ab")[0]) == "CDC"
    assert R.letters(R.align("abc", "")[0]) == "DDD" and R.align("abc", "")[2] == -3.0
    assert repr(R.align("abc", "abc")[2]) == "0.0"


# ------------------------------------------------------------------------------------------------------ the scorer
@pytest.mark.parametrize("tokenizer", ["whitespace", "char"])
def test_evaluate_reproduces_the_reference_program_byte_for_byte(tokenizer, tmp_path):
    from touchnet_amd.metrics import error_rate as E
    ref = E.load_utterances(os.path.join(GOLD, "ref.txt"))
    hyp = E.load_utterances(os.path.join(GOLD, "hyp.txt"))
    warnings = []
    res = E.evaluate(ref, hyp, tokenizer, align_fn=R.align_fn, warn=warnings.append)
    out = tmp_path / "DETAILS.txt"
    with open(out, "w+", encoding="utf8") as f:
        res.write_details(f)
    assert out.read_bytes() == _gold(f"DETAILS_{tokenizer}.txt")
    assert (res.to_json() + "\n" + res.to_kaldi() + "\n").encode("utf8") == _gold(f"stdout_{tokenizer}.txt")
    assert res.num_hyp_without_ref == 1 and res.num_eval_utts == 151 and res.num_ref_utts == res.num_hyp_utts == 153
    assert sorted(w.split()[1] for w in warnings) == ["extra_hyp_without_ref", "utt_empty_reference"]
    assert list(vars(res))[:11] == ["num_ref_utts", "num_hyp_utts", "num_eval_utts", "num_hyp_without_ref", "C", "S", "I", "D",
                                    "token_error_rate", "num_utts_with_error", "sentence_error_rate"]


def test_loading_and_tokenizing():
    from touchnet_amd.metrics import error_rate as E
    ref = E.load_utterances(os.path.join(GOLD, "ref.txt"))
    hyp = E.load_utterances(os.path.join(GOLD, "hyp.txt"))
    assert ref["utt_empty_reference"].text == "" and hyp["utt_only_uid_in_hyp"].text == ""
    assert not ref["utt_0100"].text.startswith("这 一 行") and not hyp["utt_0101"].text.startswith("这 一 行")   # the later line
    assert "ref_without_hyp" in ref and "ref_without_hyp" not in hyp
    assert E.tokenize_text(" 你好 GPU  ok ", "whitespace") == ["你好", "GPU", "ok"]
    assert E.tokenize_text(" 你好 GPU\tok ", "char") == list("你好GPUok")
    with pytest.raises(RuntimeError, match="tokenizer"):
        E.tokenize_text("a", "bpe")
    with pytest.raises(RuntimeError, match="format"):
        E.load_utterances(os.path.join(GOLD, "ref.txt"), "trn")
    assert E.alignment_lines(["中", "ab"], ["中", "c", "d"], [0, 1, 2]) == ("  REF  : 中 ab * ", "  HYP  : 中 c  d ",
                                                                          "  EDIT :    S  I ")


def test_command_line_writes_the_reference_files(tmp_path, capsys):
    """the whole command line with the aligner swapped for the restatement: result file and stdout of the reference"""
    from touchnet_amd.metrics import error_rate as E
    out = tmp_path / "DETAILS.txt"
    real, E.device_align = E.device_align, R.align_fn
    try:
        rc = E.main(["--tokenizer", "char", "--ref", os.path.join(GOLD, "ref.txt"), "--hyp", os.path.join(GOLD, "hyp.txt"),
                     str(out)])
    finally:
        E.device_align = real
    assert rc == 0 and out.read_bytes() == _gold("DETAILS_char.txt")
    assert capsys.readouterr().out.encode("utf8") == _gold("stdout_char.txt")


def test_jsonl_extractor_reproduces_the_reference_files(tmp_path):
    from touchnet_amd.metrics import error_rate as E
    shutil.copyfile(os.path.join(GOLD, "final.jsonl"), tmp_path / "final.jsonl")
    warnings = []
    trans, rec = E.extract_trans_and_pred(str(tmp_path / "final.jsonl"), warn=warnings.append)
    assert (trans, rec) == (str(tmp_path / "trans.txt"), str(tmp_path / "raw_rec.txt"))
    assert open(trans, "rb").read() == _gold("trans.txt") and open(rec, "rb").read() == _gold("raw_rec.txt")
    assert len(warnings) == 2                                             # the damaged line and the one without `predict`
    assert E.main(["--jsonl", str(tmp_path / "final.jsonl")]) == 0       # extraction alone: nothing to score, no device
    assert open(trans, "rb").read() == _gold("trans.txt")


# ------------------------------------------------------------------------------------------------------ refusals
def test_functional_layer_refuses_by_name():
    import touchnet_amd.functional as F
    with pytest.raises(ValueError, match="empty reference"):
        F.edit_align([[1, 2], []], [[1], [2]])
    with pytest.raises(ValueError, match="length over 16383"):
        F.edit_align([[1] * 16384], [[1]])
    with pytest.raises(ValueError, match="length over 16383"):
        F.edit_align([[1]], [[1] * 16384])
    with pytest.raises(ValueError, match="workspace_bytes"):
        F.edit_align([[1] * 100], [[1] * 100], workspace_bytes=7 * 128 * 4 - 1)      # ceil(100 / 16) * 128 words
    with pytest.raises(ValueError, match="hypotheses"):
        F.edit_align([[1]], [[1], [2]])
    assert F.edit_align([], []) == []


def test_workspace_words_are_the_headers_layout():
    from touchnet_amd import _C
    lib = _C.lib()
    for r, h in [(1, 0), (1, 1), (16, 64), (17, 65), (200, 129), (2048, 2048), (2049, 1), (16383, 16383)]:
        want = -(-r // 16) * (-(-h // 64) * 64) + (r if r > 2048 else 0)
        assert lib.tn_edit_align_ws_words(r, h) == want, (r, h)
    for r, h in [(0, 5), (16384, 5), (5, -1), (5, 16384)]:
        assert lib.tn_edit_align_ws_words(r, h) == -1, (r, h)


def test_entry_point_refuses_every_rule_on_the_host():
    """tn_edit_align reads the table on the host and returns -22 before the upload and before any launch: one altered field
    of an otherwise valid table per case, with device addresses that are null or never dereferenced"""
    from touchnet_amd import _C
    lib = _C.lib()
    raw = (C.c_char * 4096)()
    p = (C.addressof(raw) + 255) // 256 * 256
    words = lib.tn_edit_align_ws_words
    # pair 0: ref [0, 20) x hyp [0, 70); pair 1: ref [20, 50) x hyp [70, 70) (empty); pair 2: ref [50, 60) x hyp [70, 100)
    w0, w1, w2 = words(20, 70), words(30, 0), words(10, 30)
    assert (w0, w1, w2) == (2 * 128, 0, 64)
    valid = [[0, 20, 0, 70, 0, 0], [20, 30, 70, 0, w0, 90], [50, 10, 70, 30, w0 + w1, 120]]
    ok = dict(n_ref=60, n_hyp=100, ws_words=w0 + w1 + w2, n_ops=160, P=3, ref=p, hyp=p, desc_dev=p, ws=p, ops=p, counts=p)

    def call(table=valid, **kw):
        a = dict(ok, **kw)
        host = (C.c_int * (6 * len(table)))(*[v for row in table for v in row]) if table is not None else None
        return lib.tn_edit_align(a["ref"], a["n_ref"], a["hyp"], a["n_hyp"], host, a["desc_dev"], a["P"], a["ws"], a["ws_words"],
                                 a["ops"], a["n_ops"], a["counts"], None)

    def altered(pair, column, value):
        table = [list(row) for row in valid]
        table[pair][column] = value
        return table

    REF0, RLEN, HYP0, HLEN, WS, OPS = range(6)
    cases = dict(
        empty_reference=altered(1, RLEN, 0), negative_reference=altered(1, RLEN, -3), reference_16384=altered(0, RLEN, 16384),
        hypothesis_16384=altered(0, HLEN, 16384), negative_hypothesis=altered(2, HLEN, -1),
        ref_start_negative=altered(0, REF0, -1), ref_past_the_array=altered(2, REF0, 51), ref_longer_than_the_array=altered(2, RLEN, 11),
        hyp_start_negative=altered(0, HYP0, -1), hyp_past_the_array=altered(2, HYP0, 71), hyp_longer_than_the_array=altered(0, HLEN, 101),
        ws_negative=altered(0, WS, -1), ws_overlaps_the_pair_before=altered(2, WS, w0 - 1), ws_descends=altered(1, WS, 0),
        ws_past_the_end=altered(2, WS, w0 + 1), ws_too_small_for_more_rows=altered(2, RLEN, 17),
        ops_negative=altered(0, OPS, -1), ops_overlap=altered(1, OPS, 89), ops_overlap_out_of_order=altered(2, OPS, 100),
        ops_past_the_end=altered(2, OPS, 121))
    for what, table in cases.items():
        assert call(table) == -22, what
    for what, kw in dict(ws_words_short=dict(ws_words=w0 + w1 + w2 - 1), n_ops_short=dict(n_ops=159), n_ref_short=dict(n_ref=59),
                         n_hyp_short=dict(n_hyp=99), negative_pairs=dict(P=-1), null_ref=dict(ref=None), null_hyp=dict(hyp=None),
                         null_device_table=dict(desc_dev=None), null_ws=dict(ws=None), null_ops=dict(ops=None),
                         null_counts=dict(counts=None), negative_ws_words=dict(ws_words=-1)).items():
        assert call(**kw) == -22, what
    assert call(None) == -22                                               # no host table
    # (ws_too_small_for_more_rows: 17 rows need two words per column where the table leaves one, and the reference array
    #  could hold them: n_ref is raised so that only the workspace rule can refuse)
    assert call(altered(2, RLEN, 17), n_ref=67, n_ops=167) == -22
    assert call(P=0) == 0 and call(None, P=0, ref=None, hyp=None, ws=None, ops=None, counts=None, desc_dev=None) == 0


# ------------------------------------------------------------------------------------------------------ the op
def test_op_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import touchnet_amd.library as L
    from touchnet_amd import _C
    assert "edit_align" in L.OPS and "tn_edit_align" in _C.PROTOTYPES and "tn_edit_align_ws_words" in _C.PROTOTYPES
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "touchnet_amd.h")).read()
    assert "int tn_edit_align(" in text and "touchnet/bin/error_rate_zh:44-149,192-205" in text
    assert torch._C._dispatch_has_kernel_for_dispatch_key("mi355_touch::edit_align", "Meta")
    with FakeTensorMode():
        for n_ref, n_hyp, P in ((60, 100, 3), (1, 0, 1), (5, 5, 0)):
            ref = torch.empty(n_ref, dtype=torch.int32, device="cuda")
            hyp = torch.empty(n_hyp, dtype=torch.int32, device="cuda")
            counts, ops = torch.ops.mi355_touch.edit_align(ref, hyp, torch.empty(P, 6, dtype=torch.int32))
            assert tuple(counts.shape) == (P, 5) and counts.dtype == torch.int32 and counts.device.type == "cuda"
            assert tuple(ops.shape) == (n_ref + n_hyp,) and ops.dtype == torch.uint8 and ops.device.type == "cuda"


def test_backend_exposes_the_aligner():
    from touchnet_amd.models.backend import ops
    assert callable(getattr(ops(), "edit_align"))
