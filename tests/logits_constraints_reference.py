"""A plain torch / Python restatement of transformers' SequenceBiasLogitsProcessor and MinNewTokensLengthLogitsProcessor
(generation/logits_process.py) on the history layout of touchnet_amd.generation (hist rows with the prompt included) — the
oracle of tn_logits_constrain and tn_beam_step_edits.  test_logits_constraints_cpu.py pins it against transformers.  Tests
only: the product does not import it.

For a history row of n ids: a length-1 sequence (t) always contributes its bias to t; a sequence of length L > 1 contributes
to its last id iff L <= n (HF ignores a sequence longer than the context, although only L - 1 ids are compared) and the
row's last L - 1 ids equal its first L - 1 ids.  The total of an id is an fp32 sum in HF's order: the length-1 bias first,
then the matching longer sequences in dict order.  min_new_tokens = m: while n - prompt_len < m every eos id is -inf."""
import contextlib
import math

import torch


def bias_row(hist, sequence_bias, V):
    """fp32 [V]: the bias SequenceBiasLogitsProcessor adds to the scores of a row whose context is `hist` (a list)."""
    n = len(hist)
    bias = torch.zeros(V, dtype=torch.float32)
    for ids, b in sequence_bias.items():
        if len(ids) == 1:
            bias[ids[0]] = b                                    # (HF: zeros += length_1_bias)
    for ids, b in sequence_bias.items():
        L = len(ids)
        if L == 1 or L > n:
            continue
        if list(hist[n - (L - 1):]) == list(ids[:-1]):
            bias[ids[-1]] += torch.tensor(b, dtype=torch.float32)
    return bias


def targets(hist, prompt_len, sequence_bias, min_new, eos, V):
    """{id: fp32 total} of the ids the kernel writes for this row: ids with a matching sequence, and the eos ids while
    fewer than min_new ids were generated (their total is -inf)."""
    n = len(hist)
    out = {}
    bias = bias_row(hist, sequence_bias or {}, V)
    for ids in (sequence_bias or {}):
        L = len(ids)
        if L == 1 or (L <= n and list(hist[n - (L - 1):]) == list(ids[:-1])):
            out[ids[-1]] = float(bias[ids[-1]])
    if min_new > 0 and n - prompt_len < min_new:
        for e in eos:
            out[int(e)] = -math.inf
    return out


def constrain(scores, hists, prompt_lens, sequence_bias=None, min_new=0, eos=()):
    """scores [R, V] fp32 or bf16 -> the processed scores: T(fp32(scores) + bias), then -inf on the eos ids of rows that
    generated fewer than min_new ids.  For fp32 this is HF's arithmetic (scores + bias)."""
    R, V = scores.shape
    out = scores.clone()
    for r in range(R):
        if sequence_bias:
            out[r] = (scores[r].float() + bias_row(hists[r], sequence_bias, V)).to(scores.dtype)
        if min_new > 0 and len(hists[r]) - prompt_lens[r] < min_new:
            out[r, torch.tensor(list(eos), dtype=torch.int64)] = -math.inf
    return out


def processed_log_probs(row, hist, prompt_len, sequence_bias, min_new, eos, penalty, ngram, dtype):
    """HF's order for beam search: log_softmax, then the processors ON the log-probabilities — sequence bias, repetition
    penalty, n-gram ban, min_new_tokens."""
    V = row.shape[-1]
    lp = torch.log_softmax(row.to(dtype), -1)
    if sequence_bias:
        lp = lp + bias_row(hist, sequence_bias, V).to(dtype)
    if penalty != 1.0 and hist:
        idx = torch.tensor(sorted(set(hist)), dtype=torch.int64)
        x = lp[idx]
        lp[idx] = torch.where(x < 0, x * penalty, x / penalty)
    L = len(hist)
    if ngram > 0 and L + 1 >= ngram:
        pre = hist[L - (ngram - 1):]
        for i in range(L - ngram + 1):
            if hist[i:i + ngram - 1] == pre:
                lp[hist[i + ngram - 1]] = -math.inf
    if min_new > 0 and L - prompt_len < min_new:
        for e in eos:
            lp[int(e)] = -math.inf
    return lp


@contextlib.contextmanager
def composed(bsr, logits, K_in, prompt_lens, sequence_bias, min_new, eos):
    """Within the block, beam_search_reference.beam_step(st, logits, ...) evaluates its candidates with the constraints:
    the module's `processed_log_probs` is replaced by the composed one above.  The row that module hands over is a view of
    `logits` (contiguous, [B * K_in, V]); its offset names the utterance and so the prompt length."""
    assert logits.is_contiguous()
    V = logits.shape[1]
    plain = bsr.processed_log_probs

    def with_constraints(row, hist, penalty, ngram, dtype):
        assert row.data_ptr() >= logits.data_ptr() and row.numel() == V
        row_in = (row.data_ptr() - logits.data_ptr()) // (V * logits.element_size())
        return processed_log_probs(row, hist, prompt_lens[row_in // K_in], sequence_bias, min_new, eos, penalty, ngram, dtype)

    bsr.processed_log_probs = with_constraints
    try:
        yield
    finally:
        bsr.processed_log_probs = plain


def beam_step(bsr, st, logits, K, prompt_lens, sequence_bias=None, min_new=0, **kw):
    """beam_search_reference.beam_step with sequence_bias / min_new_tokens; returns its decision margin."""
    B = st["hist"].shape[0] // K
    with composed(bsr, logits, logits.shape[0] // B, prompt_lens, sequence_bias, min_new, list(kw.get("eos", ()))):
        return bsr.beam_step(st, logits, K, **kw)
