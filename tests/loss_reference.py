"""Plain float64 restatements of the loss path — the cross-entropy kernels (csrc/cross_entropy.hip) and the chunked
lm_head + cross-entropy (functional._FusedLinearCE) — and the error budgets their GPU tests hold them to.  No GPU, no
HIP: torch on the CPU only.  `Ref`, `rnd`, `ulp`, `budget` and `check` are those of tests/row_kernel_reference.py:

    budget = roundings x half an ulp of T  +  FP32_REL x scale  +  flip  +  TINY

`scale` is the sum of the absolute values of the terms of a result, `flip` an absolute allowance for roundings of
INPUTS of the restated step that the kernel path applies and the restatement does not (named at each use).
tests/test_loss_reference_cpu.py holds both restatements to torch.autograd in float64 and to oracle.loss, shows that a
bf16-storage / fp32-arithmetic emulation of the fused path passes `check`, and that planted errors fail it.

ce_rows          what the kernels compute from logits ALREADY in their dtype T (fp32 or bf16), widened exactly
ce_stats         the four statistics of ce_reduce_kernel from per-row nll / hit
fused_linear_ce  loss, statistics, d(hidden), d(weight) from hidden and weight, on UNROUNDED logits h W^T
"""
import math

import torch

from row_kernel_reference import F64, FP32_REL, Ref, _flush, _ref, budget, check, d, rnd, ulp  # noqa: F401

VEC = {torch.float32: 4, torch.bfloat16: 8}          # elements of a 16-byte load
BLOCK = 256                                          # threads of a row block
BF16_REL = 2.0 ** -9                                 # half an ulp of bf16, relative (at most)


def sum_exp_rel(V, dtype):
    """Relative error of the kernel's sum-exp that follows from its summation tree: a thread adds ceil(V / (256 N)) N
    terms one after the other (each addition and each rescale rounds once: 2^-24), the merges over 64 lanes and 4 waves
    add 6 + 3 levels, logf one more.  Relative on s = absolute on ln s."""
    N = VEC[dtype]
    return (math.ceil(V / (BLOCK * N)) * N + 10) * 2.0 ** -24


def _softmax_parts(x):
    """row max, sum-exp about it, log-sum-exp and probabilities of float64 logits; -inf entries have probability 0"""
    m = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(dim=1, keepdim=True)
    lse = m + torch.log(s)
    return m[:, 0], s[:, 0], lse[:, 0], e / s


def ce_stats(nll, hit, labels, sentence_lens, num_sentence, ignore_index=-100, nll_budget=None):
    """{per_sample, per_token, accuracy, n_valid} of per-row nll / hit, with the reference's rule per_token = 0 if
    sum(nll) <= 1e-6 or nothing is labelled.  `nll_budget`: what each row's nll may already be off by (it is summed
    into the flips); None = the nll are the kernel's exact inputs.  Scales: the sums of |terms|."""
    nll, hit, sl = d(nll), d(hit), d(sentence_lens)
    valid = (labels.detach().cpu() != ignore_index)
    v = valid.to(F64)
    ns = float(num_sentence)
    nb = torch.zeros_like(nll) if nll_budget is None else nll_budget
    cnt = v.sum()
    tot = (nll * v).sum()
    one = lambda t: t.reshape(1)
    per_sample = _ref(one((nll * v / sl).sum() / ns), one((nll.abs() * v / sl).sum() / abs(ns)),
                      flip=one((nb * v / sl).sum() / abs(ns)))
    if float(tot) > 1e-6 and float(cnt) > 0:
        per_token = _ref(one(tot / cnt), one((nll.abs() * v).sum() / cnt), flip=one((nb * v).sum() / cnt))
    else:
        per_token = _ref(torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64))
    acc = (hit * v).sum() / cnt if float(cnt) > 0 else torch.zeros((), dtype=F64)
    return dict(per_sample=per_sample, per_token=per_token, accuracy=_ref(one(acc), one(acc)),
                n_valid=_ref(one(cnt), torch.zeros(1, dtype=F64)))


def ce_rows(logits, labels, sentence_lens, num_sentence, g=1.0, ignore_index=-100, lse=None):
    """logits [n, V] in the kernel's dtype.  -> dict of Refs: lse, nll (0 on ignored rows), hit (argmax == label, first
    index on ties; exact), per_sample / per_token / accuracy / n_valid, and
    dlogits = (p - onehot) g / (sentence_len num_sentence), zero on ignored rows.
    `lse`: the fp32 statistic the backward kernel reads (as rmsnorm_bwd takes rstd); None = the float64 one.

    lse, nll   scale |max| + |ln s| + |x_label|;  flip: sum_exp_rel (the summation tree of the sum-exp, absolute on ln s)
    dlogits    scale c (p (1 + |x| + |lse|) + onehot): the fp32 argument x log2 e - lse log2 e of exp2f carries |x| + |lse|;
               flush: exp2f may hand back 0 for a probability below the smallest normal"""
    dtype = logits.dtype
    x = d(logits)
    n, V = x.shape
    lab = labels.detach().cpu().to(torch.int64)
    valid = lab != ignore_index
    v = valid.to(F64)
    safe = torch.where(valid, lab, torch.zeros_like(lab)).clamp(0, V - 1)
    m, s, l64, p = _softmax_parts(x)
    xl = torch.where(valid, x.gather(1, safe[:, None])[:, 0], torch.zeros_like(m))     # (an ignored row is never read)
    sc = (m.abs() + torch.log(s).abs() + xl.abs()) * v
    tree = torch.full_like(sc, sum_exp_rel(V, dtype)) * v
    lse_ref = _ref(l64 * v, sc, flip=tree)
    nll_ref = _ref((l64 - xl) * v, sc, flip=tree)
    amax = x.argmax(dim=1)                                  # torch: the first index among equal values
    hit = ((amax == lab) & valid).to(F64)
    out = dict(lse=lse_ref, nll=nll_ref, hit=_ref(hit, torch.zeros_like(hit)))
    out.update(ce_stats(nll_ref.value, hit, lab, sentence_lens, num_sentence, ignore_index,
                        nll_budget=budget(nll_ref, torch.float32)))
    # backward
    lb = l64 if lse is None else d(lse)
    pb = torch.exp(x - lb[:, None])
    onehot = torch.zeros_like(x).scatter_(1, safe[:, None], 1.0)
    c = (float(g) / (d(sentence_lens) * float(num_sentence)) * v)[:, None]
    fin = torch.isfinite(x)
    arg = torch.where(fin, x.abs(), torch.zeros_like(x)) + lb.abs()[:, None]
    out["dlogits"] = _ref((pb - onehot) * c, c.abs() * (pb * (1 + arg) + onehot), flush=c.abs() * _flush(pb))
    return out


def fused_linear_ce(hidden, weight, labels, sentence_lens, num_sentence, g=1.0, ignore_index=-100):
    """The fused lm_head + cross-entropy on UNROUNDED logits x = h W^T (float64).  -> dict of Refs: nll, per_sample
    (the loss), per_token, accuracy, n_valid, dhidden, dweight — the gradients of g x loss.

    The budget carries the roundings _FusedLinearCE documents, and no others:
      * the logits are stored in bf16: every x, and with it the row's log-sum-exp, is off by at most half a bf16 ulp at
        the row's largest |logit| (`hx`); nll = lse - x_label by 2 hx;
      * dlogits are stored in bf16 (2^-9 relative) and the upstream gradient is cast to bf16 in backward (2^-9);
      * fp32 arithmetic: FP32_REL of the uncancelled terms, as everywhere.
    Per dlogit  dabs = p c 2 hx + |d| (2^-8 + FP32_REL);  d(hidden) may move by dabs @ |W| + FP32_REL (|d| @ |W|),
    d(weight) by dabs^T @ |h| + FP32_REL (|d|^T @ |h|); both are stored in bf16 and multiplied by g in bf16 (check them
    with roundings = 2).
      * d(weight) is summed over all chunks in fp32 and rounded once: the chunking does not enter the budget.
      * accuracy: the argmax of the bf16 logits may be any index whose logit is within 2 hx of the row's largest; a row
        where that changes `hit` moves the accuracy by 1 / n_valid."""
    h, w = d(hidden), d(weight)
    n = h.shape[0]
    lab = labels.detach().cpu().to(torch.int64)
    valid = lab != ignore_index
    v = valid.to(F64)
    V = w.shape[0]
    safe = torch.where(valid, lab, torch.zeros_like(lab)).clamp(0, V - 1)
    x = h @ w.t()
    m, s, lse, p = _softmax_parts(x)
    hx = 0.5 * ulp(x.abs().max(dim=1).values, torch.bfloat16)
    xl = x.gather(1, safe[:, None])[:, 0]
    sc = (m.abs() + torch.log(s).abs() + xl.abs()) * v
    nll_ref = _ref((lse - xl) * v, sc, flip=(2 * hx + sum_exp_rel(V, torch.bfloat16)) * v)
    amax = x.argmax(dim=1)
    hit = ((amax == lab) & valid).to(F64)
    top = x.max(dim=1).values
    near = x >= (top - 2 * hx)[:, None]                     # what the argmax of the rounded logits may be
    lab_near = near.gather(1, safe[:, None])[:, 0]
    unsure = valid & lab_near & (near.sum(dim=1) > 1)       # the label is among several candidates
    out = dict(nll=nll_ref)
    out.update(ce_stats(nll_ref.value, hit, lab, sentence_lens, num_sentence, ignore_index,
                        nll_budget=budget(nll_ref, torch.float32)))
    cnt = float(v.sum())
    acc = out["accuracy"]
    out["accuracy"] = Ref(acc.value, acc.scale, acc.flip + (float(unsure.sum()) / cnt if cnt else 0.0), acc.flush)
    # gradients
    onehot = torch.zeros_like(x).scatter_(1, safe[:, None], 1.0)
    c = (float(g) / (d(sentence_lens) * float(num_sentence)) * v)[:, None]
    dl = (p - onehot) * c
    dabs = p * c.abs() * 2 * hx[:, None] + dl.abs() * (2 * BF16_REL + FP32_REL)
    out["dhidden"] = _ref(dl @ w, dl.abs() @ w.abs(), flip=dabs @ w.abs())
    out["dweight"] = _ref(dl.t() @ h, dl.abs().t() @ h.abs(), flip=dabs.t() @ h.abs())
    return out


# ------------------------------------------------------------------------------------------------------ inputs
def fused_inputs(n, H, V, n_ignored, row0_labelled, seed=0):
    """bf16 hidden [n, H] and weight [V, H] with logits of standard deviation 2.4 (max |x| about 12: larger logits make
    the half ulp of their bf16 storage swallow the signal), labels with exactly `n_ignored` rows ignored (row 0 as asked,
    a label in the first and in the last column, the last row labelled), sentence_lens 1 .. 9."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(n, H, generator=gen).to(torch.bfloat16)
    w = (torch.randn(V, H, generator=gen) * (2.4 / math.sqrt(H))).to(torch.bfloat16)
    lab = torch.randint(0, V, (n,), generator=gen)
    lab[1], lab[2] = 0, V - 1
    perm = torch.randperm(n - 4, generator=gen) + 3         # rows 0 .. 2 are placed by hand, the last row is labelled
    lab[perm[:n_ignored - (0 if row0_labelled else 1)]] = -100
    if not row0_labelled:
        lab[0] = -100
    assert int((lab == -100).sum()) == n_ignored
    sl = torch.randint(1, 10, (n,), generator=gen)
    return h, w, lab, sl
