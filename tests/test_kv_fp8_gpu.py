"""The FP8 (e4m3) KV cache: tn_kv_quantize bit for bit against a torch restatement of the format (csrc/kv_fp8.h);
tn_attn_decode_fp8 / tn_attn_decode_beam_fp8 and tn_attn_extend_fp8 against the float64 restatements and budgets the bf16
kernels are held to (inference_attention_reference.decode, attn_extend_reference.extend), applied to the DEQUANTISED
tensors — dequantisation is exact, so no budget term is new; and the generation loop on an FP8 cache, exactly.  Every
cache position a kernel may not read holds scale NaN.

MEASURED on an MI355X, worst error as a multiple of the budget: decode 0.995 (dense and beam, one split) / 0.989 (four
splits), extend 0.788; the quantiser's codes and scales equalled the restatement on the first run (the hardware
conversion needs no integer fix-up).  The file's 32 tests take 4 s."""
import math

import pytest
import torch

import attn_extend_reference as X
import inference_attention_reference as IR

pytestmark = pytest.mark.gpu
DEV, BF, U8, I32 = "cuda", torch.bfloat16, torch.uint8, torch.int32


def quantize(x):
    """the format, restated: bf16 [.., D] -> (codes uint8 [.., D], scales fp32 [..])"""
    xf = x.float()
    amax = xf.abs().amax(-1)
    fin = torch.isfinite(amax)
    m, ex = torch.frexp(torch.where(fin, amax, torch.ones_like(amax)))                 # amax = m 2^ex, m in [0.5, 1)
    e = torch.where(amax == 0, torch.full_like(ex, -100), torch.where(m <= 0.875, ex - 9, ex - 8).clamp(min=-100))
    one = torch.ones_like(amax)
    codes = (xf * torch.ldexp(one, -e)[..., None]).to(torch.float8_e4m3fn).view(U8)
    return (torch.where(fin[..., None], codes, torch.zeros_like(codes)),
            torch.where(fin, torch.ldexp(one, e), torch.full_like(one, math.nan)))


def dequantize(codes, scales):
    import touchnet_amd.functional as F
    return F.kv_dequantize(codes, scales)


def same(a, b):                                   # bit for bit (a NaN scale is one bit pattern)
    return a.shape == b.shape and torch.equal(a.contiguous().view(U8), b.contiguous().view(U8))


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("D", [64, 128])
def test_the_quantiser_is_the_format_bit_for_bit(D):
    import touchnet_amd.functional as F
    g = torch.Generator().manual_seed(D)
    x = torch.randn(37, 3, D, generator=g)
    x[0:4] *= 1e-3
    x[4:8] *= 1e3
    x[8:20] = x[8:20].clamp(-3, 3)
    x[8, :, 0] = 56.0                             # amax = 448 * 2^-3 exactly (m = 1.75)
    x[9, :, 0] = 56.25                            # one bf16 step above it: the next exponent
    x[10, :, 0] = 1.75 * 2.0 ** 20
    x[11, :, 0] = -1.75 * 2.0 ** -20
    x[12, :, :8] = torch.tensor([448.0, 17.0, 19.0, -21.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, -(2.0 ** -10)])   # e = 0
    x[13] = 0.0
    x[14, 0, 5], x[14, 1, 63], x[14, 2, D - 1] = math.nan, math.inf, -math.inf
    x[15] *= 2.0 ** -110                          # below the lowest scale: e = -100
    x[16] *= 2.0 ** -130                          # bf16 subnormals
    x[17] *= 2.0 ** 100
    x = x.to(BF)
    codes, scales = F.kv_quantize(x.to(DEV))
    want_c, want_s = quantize(x)
    assert int(torch.isnan(want_s).sum()) == 3 and float(want_s[13, 0]) == 2.0 ** -100 and float(want_s[12, 0]) == 1.0
    assert want_c[12, 0, :8].tolist() == [126, 88, 90, 128 + 90, 1, 0, 2, 128] and float(want_s[9, 0]) == 2 * float(want_s[8, 0])
    assert same(scales.cpu(), want_s), "scales"
    assert same(codes.cpu(), want_c), f"codes differ at {(codes.cpu() != want_c).nonzero()[:8].tolist()}"
    # the round trip: the dequantised values are a fixed point.  (Codes and scale themselves are not always: an amax in
    # (224, 232] 2^e rounds to 224 2^e = 448 2^(e - 1), which the rule then gives the scale 2^(e - 1) and shifted codes.)
    ok = ~torch.isnan(want_s)
    back = dequantize(want_c[ok], want_s[ok])
    again = F.kv_quantize(back[None].to(DEV))
    again_c, again_s = quantize(back[None])
    assert same(again[0].cpu(), again_c) and same(again[1].cpu(), again_s), "the round trip re-quantises differently"
    assert same(dequantize(again_c, again_s), back[None]) and bool(((again_s[0] == want_s[ok]) | (2 * again_s[0] == want_s[ok])).all())
    one = F.kv_quantize(x[5:6].to(DEV))           # a key's codes do not depend on the batch it is quantised in
    assert same(one[0].cpu(), want_c[5:6]) and same(one[1].cpu(), want_s[5:6])


# ------------------------------------------------------------------------------------------------ decode
def _decode_problem(D, G, S_max, Nkv, beam):
    """rows 0 .. 4: cache_len 0, 63, 64, 65, S_max - 1; rows 5, 6: the refused lengths -1 and S_max; beam: row 7 with an
    out-of-range table entry.  Positions at or past cache_len hold scale NaN; table entries there hold junk."""
    lens = [0, 63, 64, 65, S_max - 1, -1, S_max] + ([40] if beam else [])
    B, Nh = len(lens), G * Nkv
    g = torch.Generator().manual_seed(1000 * D + 10 * G + S_max)
    q, kn, vn = (torch.randn(B, h, D, generator=g).to(BF) for h in (Nh, Nkv, Nkv))
    kc, vc = (torch.randn(B, S_max, Nkv, D, generator=g).to(BF) for _ in range(2))
    kc[:, :, :, 0] *= 8.0                                                                  # keys of uneven scales
    valid = [n if 0 <= n < S_max else 0 for n in lens]
    for b, n in enumerate(valid):
        kc[b, n:], vc[b, n:] = math.nan, math.nan
    src = None
    if beam:
        src = torch.full((B, S_max), 1 << 20, dtype=I32)
        for b, n in enumerate(valid):
            for s in range(n):                                                             # a row that holds position s
                rows = [r for r, m in enumerate(valid) if m > s]
                src[b, s] = rows[int(torch.randint(len(rows), (1,), generator=g))]
        src[7, 17] = B
    return q, kn, vn, quantize(kc), quantize(vc), torch.tensor(lens, dtype=I32), src


@pytest.mark.parametrize("beam", [False, True], ids=["dense", "beam"])
@pytest.mark.parametrize("S_max,Nkv", [(70, 74), (200, 2)], ids=["one_split", "four_splits"])
@pytest.mark.parametrize("G", [1, 4, 7])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_on_an_fp8_cache_meets_the_bf16_budget_on_the_dequantised_cache(D, G, S_max, Nkv, beam):
    import touchnet_amd.functional as F
    q, kn, vn, (kc, ks), (vc, vs), lens, src = _decode_problem(D, G, S_max, Nkv, beam)
    B, scale = q.shape[0], D ** -0.5
    assert IR.num_splits(B, Nkv, S_max) == (1 if S_max == 70 else 4)
    knq, vnq = quantize(kn), quantize(vn)
    ref, _, _ = IR.decode(q, dequantize(*knq), dequantize(*vnq), dequantize(kc, ks), dequantize(vc, vs), lens, scale, src)
    dev = [t.to(DEV) for t in (q, kn, vn, kc, vc, ks, vs, lens)]
    with torch.no_grad():
        o = (F.attn_decode_fp8(*dev, scale) if src is None else F.attn_decode_beam_fp8(*dev, src.to(DEV), scale)).cpu()
    bad = torch.isnan(ref.value)
    assert bad[5:].all() and not bad[:5].any() and torch.equal(torch.isnan(o.float()), bad)
    IR.check(o[:5], IR.Ref(ref.value[:5], ref.slack[:5]), f"fp8 {'beam' if beam else 'dense'} decode D{D} G{G} S{S_max}")
    # the slot holds the quantiser's codes and scale of the new key; no other byte of codes or scales has changed
    for got, (codes, scales), (nc, ns) in ((dev[3:6:2], (kc, ks), knq), (dev[4:7:2], (vc, vs), vnq)):
        codes, scales = codes.clone(), scales.clone()
        for b, n in enumerate(lens.tolist()):
            if 0 <= n < S_max:
                codes[b, n], scales[b, n] = nc[b], ns[b]
        assert same(got[0].cpu(), codes) and same(got[1].cpu(), scales)


# ------------------------------------------------------------------------------------------------ extend
# (prefix_len, n_r, kv_row): every prefix in {0, 1, 63, 64, 65} and n_r in {1, 16, 17, 33}; rows 2 and 3 are read twice
SEQS = ((0, 1, 0), (1, 16, 1), (63, 17, 2), (64, 33, 2), (65, 1, 3), (0, 33, 4), (65, 17, 3), (1, 1, 4))


@pytest.mark.parametrize("Nh,Nkv", [(4, 1), (14, 2)], ids=["HPW1", "HPW2"])
@pytest.mark.parametrize("D", [64, 128])
def test_extend_on_fp8_keys_meets_the_bf16_budget_on_the_dequantised_tensors(D, Nh, Nkv):
    import touchnet_amd.functional as F
    q, kn, vn, kc, vc, start, pre, row, scale = X.inputs(D, Nh, Nkv, "gauss", seed=D + Nh, seqs=SEQS, nB=5, S=70)
    (kn, kns), (vn, vns), (kc, kcs), (vc, vcs) = (quantize(t) for t in (kn, vn, kc, vc))      # NaN past every prefix: scale NaN
    assert bool(torch.isnan(kcs[3, 65:]).all()) and not bool(torch.isnan(kcs[3, :65]).any())
    ref = X.extend(q, dequantize(kn, kns), dequantize(vn, vns), dequantize(kc, kcs), dequantize(vc, vcs), start, pre, scale, row)
    with torch.no_grad():
        o = F.attn_extend_fp8(*(t.to(DEV) for t in (q, kn, vn, kns, vns, kc, vc, kcs, vcs)), start, pre, scale, row)
    IR.check(o.cpu(), ref, f"fp8 attn_extend D{D} {Nh}x{Nkv}")


# ------------------------------------------------------------------------------------------------ end to end
def _model():
    from test_generation_gpu import _tiny_touch_audio
    return _tiny_touch_audio("llama", seed=21)[0].to(DEV).to(BF).eval()


def test_generation_on_a_growing_fp8_cache_returns_the_tokens_of_a_preallocated_one():
    from touchnet_amd import generation as G
    m = _model()
    g = torch.Generator().manual_seed(5)
    prompts = G.Prompts([torch.randint(4, 500, (n,), generator=g) for n in (33, 70)])
    run = lambda chunk: G.generate(m, prompts, G.GenerationConfig(max_new_tokens=40, eos_token_id=-1, cache_chunk=chunk,
                                                                  kv_cache_dtype="fp8_e4m3"), return_cache=True)
    (a, ca), (b, cb) = run(8), run(1024)
    assert ca.kv_dtype == "fp8_e4m3" and ca.k[0].dtype == U8 and a.shape[1] == 40          # 70 + 8 rows had to grow
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        G.generate(m, prompts, G.GenerationConfig(max_new_tokens=2, kv_cache_dtype="fp8_e4m3"),
                   past=G.generate(m, prompts, G.GenerationConfig(max_new_tokens=2), return_cache=True)[1])


def test_extend_in_two_chunks_leaves_the_codes_and_scales_of_one(monkeypatch):
    """every linear layer on the small-M kernel, whose rows do not depend on the row count (40, 15 and 25 rows here)"""
    import touchnet_amd.functional as F
    from touchnet_amd import generation as G
    monkeypatch.setattr(F, "DECODE_GEMM", "own")
    m = _model()
    c = m.language_model.config
    g = torch.Generator().manual_seed(6)
    ids = [torch.randint(4, 500, (n,), generator=g) for n in (19, 8, 13)]
    cut = (7, 3, 5)
    new = lambda: G.KVCache.allocate(c.num_hidden_layers, 3, 24, c.num_key_value_heads, c.head_dim, DEV, kv_dtype="fp8_e4m3")
    one, two = new(), new()
    for cache in (one, two):
        for t in cache.k_scale + cache.v_scale:
            t.fill_(math.nan)
    G.extend(m, one, range(3), ids, prefix_len=(0, 0, 0))
    G.extend(m, two, range(3), [t[:n] for t, n in zip(ids, cut)], prefix_len=(0, 0, 0))
    G.extend(m, two, range(3), [t[n:] for t, n in zip(ids, cut)], prefix_len=cut)
    assert torch.equal(one.cache_len, two.cache_len) and one.cache_len.tolist() == [18, 7, 12]
    for a, b in zip(one.k + one.v + one.k_scale + one.v_scale, two.k + two.v + two.k_scale + two.v_scale):
        for r, t in enumerate(ids):
            assert same(a[r, :t.numel()], b[r, :t.numel()]) and not bool(torch.isnan(a[r, :t.numel()].float()).any())
