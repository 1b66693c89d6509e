"""A plain torch / Python restatement of one step of transformers' vectorised `_beam_search` (generation/utils.py:
_get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic), on
the state layout of touchnet_amd.generation.BeamState — the oracle of tn_beam_step.  test_beam_search_cpu.py pins it
against `model.generate(num_beams=K, ...)`.  Tests only: the product does not import it.

Per utterance, not per batch: an utterance that is done is left untouched (HF keeps stepping it until the whole batch stops,
with every candidate masked out of its finished set, so its result cannot change)."""
import math

import torch

EMPTY = -1.0e9


def new_state(prompts, K, S, float_dtype=torch.float64):
    """State right after a prefill: prompt b in row b K; one live row per utterance."""
    B, R = len(prompts), len(prompts) * K
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    st = dict(hist=i32(R, S), hist_len=i32(R), cache_len=i32(R), src=(torch.arange(R, dtype=torch.int32) // K * K)[:, None]
              .repeat(1, S), run_score=torch.zeros(R, dtype=float_dtype), fin_ids=i32(R, S), fin_len=i32(R),
              fin_score=torch.full((R,), EMPTY, dtype=float_dtype), fin_flag=i32(R), gen=i32(B),
              unsat=torch.ones(B, dtype=torch.int32), done=i32(B), n_unfinished=torch.tensor([B], dtype=torch.int32),
              out_ids=i32(R), out_parent=i32(R))
    for b, p in enumerate(prompts):
        st["hist"][b * K, :len(p)] = torch.as_tensor(p, dtype=torch.int32)
        st["hist_len"][b * K] = len(p)
        st["cache_len"][b * K] = len(p) - 1
    return st


def processed_log_probs(row, hist, penalty, ngram, dtype):
    """HF's order for beam search: log_softmax first, then the processors ON the log-probabilities."""
    lp = torch.log_softmax(row.to(dtype), -1)
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
    return lp


def _gaps(values, structural=()):
    """Smallest difference between neighbours of a descending list.  Ignored: pairs of equal infinities, and the pairs
    whose first index is in `structural` — two candidates of ONE row with the SAME logit and the same processing, whose
    scores are equal by construction in any arithmetic; the index rule orders them, here and in the kernel alike."""
    g = math.inf
    for n, (a, b) in enumerate(zip(values, values[1:])):
        if not (math.isinf(a) and math.isinf(b)) and n not in structural:
            g = min(g, abs(a - b))
    return g


def beam_step(st, logits, K, penalty=1.0, ngram=0, eos=(), n_new=1, length_penalty=1.0, early_stopping=False,
              dtype=torch.float64):
    """Advance `st` in place by one step; logits [B * K_in, V].  Returns the smallest margin of any decision taken (the
    order of the kept candidates, the cut behind them, the order of the finished set, the heuristic's comparison);
    see `_gaps` for the one kind of equality that is not a decision of the arithmetic."""
    R, S = st["hist"].shape
    B = R // K
    K_in, V = logits.shape[0] // B, logits.shape[1]
    assert K_in in (1, K)
    eos = list(eos)
    keep = max(2, 1 + len(eos)) * K
    margin = math.inf
    for b in range(B):
        if int(st["done"][b]):
            continue
        r0 = b * K
        L, cl = int(st["hist_len"][r0]), int(st["cache_len"][r0])
        assert 1 <= L < S
        acc = []
        for k in range(K_in):
            h = st["hist"][r0 + k, :L].tolist()
            lp = processed_log_probs(logits[b * K_in + k], h, penalty, ngram, dtype)
            acc.append(lp.to(torch.float64) + float(st["run_score"][r0 + k]))
        flat = torch.cat(acc)
        order = torch.sort(flat, descending=True, stable=True).indices[:keep + 1].tolist()   # ties: the lower flat index
        vals = [float(flat[i]) for i in order]
        same = lambda i, j: (i // V == j // V and vals[order.index(i)] == vals[order.index(j)]
                             and float(logits[b * K_in + i // V, i % V]) == float(logits[b * K_in + j // V, j % V]))
        tied = {n for n in range(len(order) - 1) if same(order[n], order[n + 1])}
        margin = min(margin, _gaps(vals, tied))
        cand = [(vals[n], order[n] // V, order[n] % V) for n in range(keep)]
        g1 = int(st["gen"][b]) + 1
        hit = [g1 >= n_new or c[2] in eos for c in cand]
        # running beams: topk of acc - 1e9 * hit
        sel = [n for n in range(keep) if not hit[n]][:K]
        sel += [n for n in range(keep) if hit[n]][:K - len(sel)]
        # finished set: the held slots, then the hits among the first K candidates; stable top K
        div = float(g1) ** length_penalty
        merged = [(float(st["fin_score"][r0 + h]), ("held", h)) for h in range(K)]
        merged += [(cand[n][0] / div, ("new", n)) for n in range(K) if hit[n]]
        merged.sort(key=lambda t: -t[0])                                                     # (stable)
        real = [m for m in merged if m[0] > EMPTY / 2]
        margin = min(margin, _gaps([m[0] for m in real],
                                   {i for i in range(len(real) - 1) if real[i][1][0] == real[i + 1][1][0] == "new"
                                    and real[i + 1][1][1] == real[i][1][1] + 1 and real[i][1][1] in tied}))
        merged = merged[:K]
        old = {k: st[k][r0:r0 + K].clone() for k in ("hist", "src", "fin_ids", "fin_len", "fin_flag")}
        for j, (score, (kind, n)) in enumerate(merged):
            r = r0 + j
            st["fin_score"][r] = score
            if kind == "held":
                st["fin_ids"][r] = old["fin_ids"][n]
                st["fin_len"][r] = old["fin_len"][n]
                st["fin_flag"][r] = old["fin_flag"][n]
            else:
                st["fin_ids"][r, :L] = old["hist"][cand[n][1], :L]
                st["fin_ids"][r, L] = cand[n][2]
                st["fin_len"][r] = L + 1
                st["fin_flag"][r] = 1
        for j, n in enumerate(sel):
            r = r0 + j
            v, parent, tok = cand[n]
            st["run_score"][r] = v + (EMPTY if hit[n] else 0.0)
            st["out_ids"][r] = tok
            st["out_parent"][r] = r0 + parent
            st["hist"][r, :L] = old["hist"][parent, :L]
            st["hist"][r, L] = tok
            st["src"][r, :cl] = old["src"][parent, :cl]
            st["src"][r, cl] = r0 + parent
            st["hist_len"][r] = L + 1
            st["cache_len"][r] = cl + 1
        Lh = n_new if (early_stopping == "never" and length_penalty > 0.0) else g1
        best = float(st["run_score"][r0]) / (float(Lh) ** length_penalty)
        worst = min(float(st["fin_score"][r0 + j]) for j in range(K))
        full = all(int(st["fin_flag"][r0 + j]) for j in range(K))
        if int(st["unsat"][b]) and worst > EMPTY / 2 and best > EMPTY / 2:
            margin = min(margin, abs(best - worst))
        unsat = bool(int(st["unsat"][b])) and best > worst
        st["gen"][b] = g1
        st["unsat"][b] = int(unsat)
        if (not unsat) or (full and early_stopping is True) or all(hit):
            st["done"][b] = 1
            st["n_unfinished"][0] -= 1
    return margin


def best_hypotheses(st, K, prompt_lens):
    """-> (generated ids of every utterance's best finished hypothesis, its score)."""
    out = []
    for b, P in enumerate(prompt_lens):
        r = b * K
        out.append((st["fin_ids"][r, P:int(st["fin_len"][r])].tolist(), float(st["fin_score"][r])))
    return out
