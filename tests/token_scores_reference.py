"""Plain float64 restatement of tn_token_scores (csrc/token_scores.hip) and the error budget the GPU test holds the kernel
to.  No GPU, no HIP: torch on the CPU only.

What is computed, per row of the kernel's own logits (bf16 / fp32 widened to float64, so the inputs are exact):
  lse      = log sum_v exp(l_v)                 (log_softmax's normaliser)
  logp(t)  = l_t - lse                          NaN for t outside [0, V)
  entropy  = lse - sum_v p_v l_v                a -inf logit contributes 0
  top-k    the ids of the k largest logits, descending, ties to the LOWER id; id -1 / logp -inf behind the V-th
A row with a NaN or +inf, or with nothing but -inf, is `sick`: every float is NaN, every id -1.

The budget.  The kernel evaluates, in fp32 with u = 2^-24 per operation,
  m = max l    d_v = l_v - m    e_v = expf(d_v)    s = sum e_v    w = sum e_v d_v    logp = d_t - logf(s)    H = logf(s) - w / s
(m cancels in H).  Thread t of 1024 owns the chunks t, t + 1024, ... of N consecutive ids (N = 4 fp32 / 8 bf16), so a
partial sum has at most n = ceil(ceil(V / N) / 1024) N terms, and DEPTH = 6 (xor tree of a wave) + 15 (the 16 wave partials
in order) more additions follow: a sum of same-signed terms (e_v > 0, e_v d_v <= 0) is off by at most (n + DEPTH) u
relatively.  With p_v the true probabilities, A = sum_v p_v |d_v| and A2 = sum_v p_v d_v^2, to first order in u:
  d_v     one rounding, u |d_v|; through exp a relative u |d_v| on e_v: u A relative on s, u A2 on w / s
  e_v     expf: C_EXP u relative (1 ulp = 2 u: the device library's documented bound)
  s       rel(s) = (C_EXP + n + DEPTH) u + u A
  log s   err(log s) = rel(s) + C_LOG u |log s|                                     (logf: 1 ulp)
  logp    err = u |d_t| + err(log s) + u |logp|                                     (d_t's rounding, the final subtraction)
  w / s   every term e_v d_v carries e_v's, d_v's and the product's rounding (the fma spares the last; it is kept):
          err(w / s) = ((C_EXP + 2 + n + DEPTH) A + A2) u + A rel(s) + C_DIV u A    (the sum, s below it, the division)
  H       err = err(log s) + err(w / s) + u |H|                                     (the final subtraction)
  FLUSH   = V 2^-126: an e_v below the normal range may be flushed (s >= 1, so this is absolute and relative at once)
The second-order terms are covered by evaluating every (k u) as k u / (1 - k u).  There is no free multiplier.

`budget_ok` is the condition that keeps the budget from hiding a wrong token or a dropped tail: on the test inputs
(|l| <= 32) it must stay under 1e-4 for logp and under 1e-3 for entropy — the GPU test asserts it for every row it
compares.  (A wrong token moves logp by the gap between two logits, a dropped chunk moves lse by its share of s.)"""
import math

import torch

U32 = 2.0 ** -24
C_EXP, C_LOG, C_DIV = 2.0, 2.0, 2.0
THREADS, DEPTH = 1024, 6 + 15
LOGP_CEILING, ENTROPY_CEILING = 1e-4, 1e-3
MAX_ALT, MAX_VOCAB = 8, 262144
F64 = torch.float64


def chunk(dtype) -> int:
    return 8 if dtype == torch.bfloat16 else 4


def serial_terms(V: int, dtype) -> int:
    """the longest per-thread partial sum of the kernel"""
    N = chunk(dtype)
    chunks = -(-V // N)
    return -(-chunks // THREADS) * N


def _g(k: float) -> float:
    """k roundings: k u / (1 - k u)"""
    return k * U32 / (1.0 - k * U32)


def sick(row: torch.Tensor) -> bool:
    r = row.to(F64)
    return bool(torch.isnan(r).any() or (r == math.inf).any() or (r == -math.inf).all())


def topk(row: torch.Tensor, k: int):
    """ids of the k largest, descending, ties to the lower id; -1 behind the V-th"""
    r = row.to(F64)
    # a stable descending sort keeps equal values in ascending id order
    ids = torch.sort(r, descending=True, stable=True).indices.tolist()[:k]
    return ids + [-1] * (k - len(ids))


def row_scores(row: torch.Tensor, tok: int, k: int = 0):
    """-> dict(logp, entropy, alt_id [k], alt_logp [k], budget_logp, budget_entropy, budget_alt [k]) of one row"""
    V = row.numel()
    nan = float("nan")
    if sick(row):
        return dict(logp=nan, entropy=nan, alt_id=[-1] * k, alt_logp=[nan] * k, budget_logp=0.0, budget_entropy=0.0,
                    budget_alt=[0.0] * k)
    r = row.to(F64)
    m = r.max()
    d = r - m
    live = d > -math.inf
    e = torch.where(live, torch.exp(d), torch.zeros_like(d))
    s = e.sum()
    p = e / s
    dd = torch.where(live, d, torch.zeros_like(d))
    log_s = float(torch.log(s))
    A = float((p * dd.abs()).sum())
    A2 = float((p * dd * dd).sum())
    H = log_s + A                                   # lse - sum p l = log s - sum p d = log s + sum p |d|
    n = serial_terms(V, row.dtype)
    flush = V * 2.0 ** -126
    rel_s = _g(C_EXP + n + DEPTH) + U32 * A + flush
    err_log_s = rel_s + C_LOG * U32 * abs(log_s)

    def logp_of(t):
        if t < 0 or t >= V:
            return nan, 0.0
        dt = float(d[t])
        if dt == -math.inf:
            return -math.inf, 0.0
        lp = dt - log_s
        return lp, U32 * abs(dt) + err_log_s + U32 * abs(lp)

    err_ws = _g(C_EXP + 2 + n + DEPTH) * A + U32 * A2 + A * rel_s + C_DIV * U32 * A
    lp, b_lp = logp_of(int(tok))
    ids = topk(row, k)
    alts = [logp_of(i) if i >= 0 else (-math.inf, 0.0) for i in ids]
    return dict(logp=lp, entropy=H, alt_id=ids, alt_logp=[a[0] for a in alts], budget_logp=b_lp,
                budget_entropy=err_log_s + err_ws + U32 * abs(H), budget_alt=[a[1] for a in alts])


def scores(logits: torch.Tensor, tok, k: int = 0):
    """row_scores of every row of logits [R, V], stacked: float64 / int64 tensors"""
    rows = [row_scores(logits[r], int(tok[r]), k) for r in range(logits.shape[0])]
    f = lambda key: torch.tensor([x[key] for x in rows], dtype=F64).reshape(len(rows), *([k] if "alt" in key else []))
    out = {key: f(key) for key in ("logp", "entropy", "alt_logp", "budget_logp", "budget_entropy", "budget_alt")}
    out["alt_id"] = torch.tensor([x["alt_id"] for x in rows], dtype=torch.int64).reshape(len(rows), k)
    return out


def budget_ok(ref) -> bool:
    """the ceilings of the module docstring (valid for |l| <= 32)"""
    return bool(ref["budget_logp"].max() < LOGP_CEILING and ref["budget_entropy"].max() < ENTROPY_CEILING
                and (ref["budget_alt"].numel() == 0 or ref["budget_alt"].max() < LOGP_CEILING))


def close(got: torch.Tensor, want: torch.Tensor, budget: torch.Tensor):
    """-> (ok, worst fraction of the budget): NaN where NaN, the same infinities, |got - want| <= budget elsewhere"""
    got, want, budget = got.detach().cpu().to(F64), want.to(F64), budget.to(F64)
    if got.shape != want.shape:
        return False, math.inf
    special = torch.isnan(want) | torch.isinf(want)
    same = (torch.isnan(got) == torch.isnan(want)).all() and bool((got[torch.isinf(want)] == want[torch.isinf(want)]).all())
    same = bool(same) and not bool(torch.isinf(got[~special]).any())
    err = (got - want).abs()[~special]
    b = budget[~special]
    if err.numel() == 0:
        return same, 0.0
    frac = float((err / b.clamp_min(1e-300)).max())
    return same and bool((err <= b).all()), frac


def fp32_partial_sum_evaluation(row: torch.Tensor, tok: int):
    """The kernel's arithmetic restated in fp32 on the CPU with its partition (1024 strided chunk owners, a xor tree of 64,
    16 partials in order): what the budget must cover.  -> (logp, entropy) as Python floats"""
    N = chunk(row.dtype)
    l = row.to(torch.float32)
    V = l.numel()
    m = l.max()
    d = l - m
    e = torch.exp(d)
    pad = -(-V // (N * THREADS)) * N * THREADS - V
    def tree(x):
        x = torch.cat([x, torch.zeros(pad, dtype=torch.float32)]).view(-1, THREADS, N)      # [round, thread, element]
        acc = torch.zeros(THREADS, dtype=torch.float32)
        for rnd in range(x.shape[0]):
            for j in range(N):
                acc = acc + x[rnd, :, j]
        w = acc.view(16, 64)
        off = 32
        while off:
            w = w + w[:, torch.arange(64) ^ off]
            off >>= 1
        tot = torch.zeros((), dtype=torch.float32)
        for i in range(16):
            tot = tot + w[i, 0]
        return tot
    s = tree(e)
    w = tree(torch.where(d > -math.inf, e * d, torch.zeros_like(d)))
    log_s = torch.log(s)
    return float(d[tok] - log_s), float(log_s - w / s)


# ------------------------------------------------------------------------------------------------ the inputs of the tests
def make_rows(kind: str, R: int, V: int, dtype, seed: int = 0) -> torch.Tensor:
    """[R, V] logits with |l| <= 32 (or -inf), exactly representable in `dtype`"""
    g = torch.Generator().manual_seed(seed * 7919 + V * 31 + R)
    if kind == "random":
        x = (torch.randn(R, V, generator=g) * 4.0).clamp(-32, 32)
    elif kind == "equal":
        x = torch.full((R, V), 1.5)
    elif kind == "dominant":
        x = (torch.randn(R, V, generator=g)).clamp(-8, 8) - 20.0
        x[torch.arange(R), torch.randint(0, V, (R,), generator=g)] = 30.0
    elif kind == "ties":
        # few distinct bf16 values, so the k-th place falls inside a run of duplicates
        x = torch.randint(0, 4, (R, V), generator=g).float() * 0.5 + 3.0
    elif kind == "neg_inf":
        x = (torch.randn(R, V, generator=g) * 4.0).clamp(-32, 32)
        x[torch.rand(R, V, generator=g) < 0.4] = -math.inf
        x[:, V // 2] = 1.0                                        # (never a row of nothing but -inf)
    else:
        raise ValueError(kind)
    return x.to(dtype)
