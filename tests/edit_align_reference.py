"""Plain-Python restatement of the alignment rule of the recipe's scorer (touchnet/bin/error_rate_zh:44-149), in integer
costs, written from the rule: the yardstick for shapes the fixtures under tests/golden/error_rate/ do not hold.

    match 0; substitution, insertion, deletion 1 each
    D[r][0] = r (deletions only), D[0][h] = h (insertions only)
    at (r, h): the INSERTION arc (from (r, h-1)) wins if it costs no more than both others,
               otherwise the DELETION arc (from (r-1, h)) if it costs no more than the diagonal,
               otherwise the DIAGONAL (from (r-1, h-1): C on equal tokens, S otherwise)
    the backtrace starts at (R, H)

(The scorer keeps scores = -cost and updates a cell's backpointer in the order diagonal, deletion, insertion, each with
`>=`: the last update that holds is the one that stays, hence the order above.)"""
C, S, I, D = 0, 1, 2, 3
LETTERS = "CSID"


def align(ref, hyp):
    """-> (ops, (c, s, i, d), score): ops the arc codes in path order, score = -(s + i + d) as the scorer's float"""
    R, H = len(ref), len(hyp)
    assert R > 0, "the scorer asserts a non-empty reference"
    prev = list(range(H + 1))
    back = [None] * (R + 1)                      # back[r][h]: the arc code into (r, h), for r, h >= 1
    for r in range(1, R + 1):
        cur = [r] + [0] * H
        arcs = bytearray(H + 1)
        token = ref[r - 1]
        for h in range(1, H + 1):
            ne = 0 if token == hyp[h - 1] else 1
            dia, dele, ins = prev[h - 1] + ne, prev[h] + 1, cur[h - 1] + 1
            if ins <= dele and ins <= dia:
                cur[h], arcs[h] = ins, I
            elif dele <= dia:
                cur[h], arcs[h] = dele, D
            else:
                cur[h], arcs[h] = dia, ne
        back[r] = arcs
        prev = cur
    ops, r, h = [], R, H
    while r > 0 or h > 0:
        code = I if r == 0 else D if h == 0 else back[r][h]
        ops.append(code)
        r -= code != I
        h -= code != D
    ops.reverse()
    n = [ops.count(k) for k in (C, S, I, D)]
    assert n[S] + n[I] + n[D] == prev[H]
    return ops, tuple(n), 0.0 - prev[H]


def align_fn(refs, hyps):
    """the `align_fn` of touchnet_amd.metrics.error_rate.evaluate: [(c, s, i, d, ops)] for lists of id sequences"""
    out = []
    for ref, hyp in zip(refs, hyps):
        ops, (c, s, i, d), _ = align(list(ref), list(hyp))
        out.append((c, s, i, d, ops))
    return out


def letters(ops):
    return "".join(LETTERS[k] for k in ops)
