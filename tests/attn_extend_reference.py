"""Float64 restatement of tn_attn_extend (csrc/attn_extend.hip), its error budget, and the inputs the GPU tests share.

Rule: new row i of sequence r (position P + i, P = prefix_len[r]) attends to cache[kv_row[r], 0 .. P) and to the new rows
j <= i of its own sequence.  Only those positions are gathered (`inputs` puts NaN at every cache position no sequence may
read); a sequence with P outside [0, S_max] or kv_row outside [0, B) is NaN.

Budget: half a bf16 ulp plus the block-causal slack of inference_attention_reference.block_causal, which is CALLED, not
copied: the gathered keys of a sequence are one clip of P + n frames with block = 1 (key j allowed iff j <= i), the queries
of the P cached positions are zero rows that are thrown away.  That function's structure is this kernel's: MFMA logits
(D ULP32 terms), one product with scale * log2(e), P through bf16 with the row sum taken from the unrounded P, one rescale
per 64-key stage, 1 / l and one product at the end.  Its n is the keys the row sees (P + i + 1) and its nt = the 64-key
tiles between the first and last allowed key = (P + i) // 64 + 1, the row's stage count: stages start at key 0 of the
virtual stream, as the kernel's do.  A row of a tile passes through the later stages of the tile's longer rows as well;
there all its scores are masked, alpha = 2^0 = 1 and every p = 0 exactly: no further rounding.  No term is added."""
import math

import torch

import inference_attention_reference as IR
from attention_reference import BF, F64, Ref

# (prefix_len, n_r, kv_row): every prefix in {0, 1, 63, 64, 65, 130} and every n_r in {1, 15, 16, 17, 65} in ONE ragged
# call; cache row 2 is shared by three sequences and row 3 by two, with different prefixes; one sequence has no rows
SEQS = ((0, 1, 0), (1, 15, 1), (63, 16, 2), (64, 17, 2), (65, 65, 2), (130, 1, 3), (1, 17, 3), (65, 0, 1), (130, 65, 4),
        (64, 1, 5), (0, 16, 6))
B, S_MAX = 7, 136


def extend(q, k_new, v_new, k_cache, v_cache, seq_start, prefix_len, scale, kv_row=None):       # -> Ref of o [T, Nh, D]
    T, Nh, D = q.shape
    nB, S, Nkv = k_cache.shape[:3]
    val = torch.full((T, Nh, D), math.nan, dtype=F64)
    slack = torch.zeros(T, Nh, D, dtype=F64)
    for r, P in enumerate(int(p) for p in prefix_len):
        a, e = int(seq_start[r]), int(seq_start[r + 1])
        row = r if kv_row is None else int(kv_row[r])
        if e == a or not 0 <= P <= S or not 0 <= row < nB:
            continue
        wide = lambda c, n: torch.cat([c[row, :P], n[a:e]]).repeat_interleave(Nh // Nkv, dim=1)[None]       # [1, P + n, Nh, D]
        qq = torch.cat([torch.zeros(P, Nh, D, dtype=BF), q[a:e]])[None]
        Tt = P + e - a
        ref = IR.block_causal(qq, wide(k_cache, k_new), wide(v_cache, v_new), torch.zeros(1, Tt, dtype=torch.int32),
                              torch.full((1, Tt), Tt, dtype=torch.int32), 1, scale)
        val[a:e], slack[a:e] = ref.value[0, P:], ref.slack[0, P:]
    return Ref(val, slack)


def inputs(D, Nh, Nkv, kind, seed, seqs=SEQS, nB=B, S=S_MAX):
    """-> (q, k_new, v_new, k_cache, v_cache, seq_start, prefix_len, kv_row, scale); "sharp": IR's logits of deviation 16"""
    g = torch.Generator().manual_seed(seed)
    T, scale = sum(n for _, n, _ in seqs), D ** -0.5
    q, kn, vn = (torch.randn(T, h, D, generator=g) for h in (Nh, Nkv, Nkv))
    kc, vc = torch.randn(nB, S, Nkv, D, generator=g), torch.randn(nB, S, Nkv, D, generator=g)
    if kind == "sharp":
        sd = math.sqrt(16.0 / (scale * math.sqrt(D)))
        q, kn, kc = q * sd, kn * sd, kc * sd
    q, kn, vn, kc, vc = (t.to(BF) for t in (q, kn, vn, kc, vc))
    for row in range(nB):
        valid = max([p for p, _, rr in seqs if rr == row and 0 <= p <= S] + [0])
        kc.view(torch.int16)[row, valid:] = IR.NAN_BITS
        vc.view(torch.int16)[row, valid:] = IR.NAN_BITS
    start = torch.tensor([0] + [n for _, n, _ in seqs]).cumsum(0).to(torch.int32)
    i32 = lambda i: torch.tensor([s[i] for s in seqs], dtype=torch.int32)
    return q, kn, vn, kc, vc, start, i32(0), i32(2), scale
