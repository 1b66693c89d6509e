"""MXFP4 weight-only decode linears: tn_weight_quantize_mxfp4 against a float64 restatement of the format, the MXFP4 arms of
the small-M and mid-M weight-streaming kernels against float64 on the table-decoded weights, their epilogues against the
row kernels, and the decoders after generation.quantize_decoder_weights(model, "mxfp4")."""
import copy
import ctypes as C

import pytest
import torch

from test_gemm_smallm_fp8_gpu import _tiny

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7B7B          # bit pattern the output buffers hold wherever nothing may be written
E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)
KERNELS = ["smallm", "midm"]


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _values(w):
    """float64 [N, K] of an Mxfp4Weight: a table decode of the nibbles (low first) times 2^(b - 127) per block of 32"""
    c = w.codes.cpu().long()
    nib = torch.stack([c & 15, c >> 4], -1).flatten(1)
    return E2M1[nib] * (2.0 ** (w.scales.cpu().double() - 127)).repeat_interleave(32, 1)


def _pitched(t, pad, fill):
    buf = torch.full((t.shape[0] + 3, t.shape[1] + pad), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf[:t.shape[0], :t.shape[1]]


def _exact(kern, M, K, Ns):
    """x in {-1, 0, 1}, codes uniform over all 16 (both zeros), scale bytes 125 + (n + 3 j) % 5, integer biases on segments 0
    and 2: every term is a multiple of 2^-3 with |term| <= 24, so any fp32 order is exact and the result is
    bf16(float64 reference) bit for bit.  Operands are pitched views in NaN (x) / 0xFF (codes, scales), outputs pitched
    views in a sentinel, compared as whole buffers."""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(1000 * M + K)
    x = _pitched(torch.randint(-1, 2, (M, K), generator=g).to(DEV, torch.bfloat16), 8, float("nan"))
    layers = []
    for i, N in enumerate(Ns):
        codes = torch.randint(0, 256, (N, K // 2), generator=g).to(DEV, torch.uint8)
        scales = (125 + (torch.arange(N)[:, None] + 3 * torch.arange(K // 32)[None]) % 5).to(DEV, torch.uint8)
        bias = torch.randint(-8, 9, (N,), generator=g).to(DEV, torch.bfloat16) if i != 1 else None
        layers.append((F.Mxfp4Weight(_pitched(codes, 16, 0xFF), _pitched(scales, 4, 0xFF)), bias))
    bufs = [torch.full((M + 2, N + 8), SENTINEL, dtype=torch.int16, device=DEV) for N in Ns]
    getattr(F, f"linear_{kern}_mxfp4")(x, layers, outs=[b.view(torch.bfloat16)[:M, :N] for b, N in zip(bufs, Ns)])
    for (w, b), buf, N in zip(layers, bufs, Ns):
        ref = x.cpu().double() @ _values(w).t() + (b.cpu().double() if b is not None else 0)
        want = torch.full_like(buf, SENTINEL)
        want[:M, :N] = ref.to(torch.bfloat16).view(torch.int16).to(DEV)
        assert torch.equal(buf, want), (kern, M, K, N, int((buf != want).sum()))


@pytest.mark.parametrize("Ns", [[16], [48], [256, 64, 64]])
@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 37, 128])
def test_smallm_exact_products_and_nothing_else_is_written(M, K, Ns):
    _exact("smallm", M, K, Ns)


@pytest.mark.parametrize("Ns", [[16], [256, 64, 64]])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [49, 129, 256])
def test_midm_exact_products_and_nothing_else_is_written(M, K, Ns):
    _exact("midm", M, K, Ns)


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("kern,N", [("smallm", 16400), ("smallm", 32784), ("midm", 32784)])
def test_exact_products_in_groups_of_two_and_four_strips(kern, N, M):
    """The widths at which a small-M workgroup owns two strips (1025 strips: an odd count) and four (2049: a tail group of
    one), the FP8 arm's thresholds, and at which a mid-M wave owns two (2049 strips)."""
    _exact(kern, M, 128, [N])


@pytest.mark.parametrize("K", [384, 1152])
@pytest.mark.parametrize("kern", KERNELS)
def test_real_products_within_the_bf16_kernels_budget(kern, K):
    """|y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k| on the dequantised weights: one bf16 rounding + fp32 accumulation in
    any order, no term for the format (measured worst / bound on both kernels: 0.894 at K = 384, 0.783 at K = 1152)."""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(K)
    x, w, b = _randn(g, 37, K), F.quantize_weight_mxfp4(_randn(g, 48, K)), _randn(g, 48)
    y = getattr(F, f"linear_{kern}_mxfp4")(x, [(w, b)])[0].cpu().double()
    xd, wd = x.cpu().double(), _values(w)
    ref = xd @ wd.t() + b.cpu().double()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (xd.abs() @ wd.abs().t())
    ratio = float(((y - ref).abs() / bound).max())
    print(f"{kern} K = {K}: worst |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("K", [32, 160, 1152])
def test_quantiser_equals_a_plain_restatement(K):
    """Per block of 32: e the smallest integer >= -100 with amax <= 6 2^e, scale byte e + 127, code = the nearest e2m1
    magnitude of |w| 2^-e, ties to the even code, under the input's sign bit.  Planted blocks: ties (2.5, 5, 0.25, 0.75, 1.25
    beside an amax of 6), amax exactly 6 2^-3, amax just above 6, an all-zero block, a row below the lowest scale, negative
    values that round to zero, two blocks of one row with different scales.  A NaN and a 2^120 are refused by name."""
    from touchnet_amd import _C, functional as F
    w = torch.randn(12, K, generator=torch.Generator().manual_seed(K))
    w[0, :32] = 0
    w[0, :6] = torch.tensor([6.0, 2.5, 5.0, 0.25, 0.75, 1.25])
    w[1, :32] *= 0.01
    w[1, 0] = 0.75
    w[2, 0] = 6.03125
    w[3, :32] = 0
    w[4] *= 2.0 ** -120
    w[5, :32] = 0
    w[5, :3] = torch.tensor([6.0, -0.1, -0.25])
    if K >= 64:
        w[6, :64] *= 0.01
        w[6, 0], w[6, 32] = 6.0, 0.75
    w = w.to(torch.bfloat16)
    q = F.quantize_weight_mxfp4(w.to(DEV))
    blocks = w.double().view(12, K // 32, 32)
    es = torch.arange(-100, 130, dtype=torch.float64)
    e = es[(blocks.abs().amax(-1)[..., None] <= 6 * 2.0 ** es).int().argmax(-1)]
    assert e[:6, 0].tolist() == [0, -3, 1, -100, -100, 0] and (K < 64 or e[6, :2].tolist() == [0, -3])
    dist = ((blocks.abs() * 2.0 ** -e[..., None])[..., None] - E2M1[:8]).abs() + 1e-9 * (torch.arange(8) % 2)
    code = (dist.argmin(-1) + 8 * torch.signbit(blocks)).view(12, K // 2, 2)
    assert code[0, :3].flatten().tolist() == [7, 4, 6, 0, 2, 2] and code[5, :2].flatten().tolist()[:3] == [7, 8, 8]
    assert torch.equal(q.scales.cpu().double(), e + 127)
    assert torch.equal(q.codes.cpu().long(), code[..., 0] | code[..., 1] << 4)
    assert q.shape == (12, K) and torch.equal(F.dequantize_weight_mxfp4(q).cpu().double(), _values(q))
    for bad in (float("nan"), 2.0 ** 120):
        w[7, K - 1] = bad
        with pytest.raises(_C.KernelError, match="quantize_weight_mxfp4.*(NaN|2\\^120)"):
            F.quantize_weight_mxfp4(w.to(DEV))


def _rope_case(g, M, D, nq, nkv, K=384):
    from touchnet_amd import functional as F
    layers = [(F.quantize_weight_mxfp4(_randn(g, n * D, K)), _randn(g, n * D)) for n in (nq, nkv, nkv)]
    pos = ((torch.arange(M) * 37 + 5) % 101)[None].to(DEV)                  # positions that differ per row
    cos, sin = F.rope_tables(pos, F.rope_inv_freq(D, 10000.0, device=DEV), torch.bfloat16)
    return _randn(g, M, K), layers, (cos, sin, D, (0, 1))


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("D,nq,nkv", [(64, 4, 1), (128, 2, 1)])
@pytest.mark.parametrize("kern", KERNELS)
def test_epilogues_are_the_row_kernels_on_the_plain_mxfp4_products(kern, D, nq, nkv, M):
    from touchnet_amd import functional as F
    linear, swiglu = getattr(F, f"linear_{kern}_mxfp4"), getattr(F, f"swiglu_{kern}_mxfp4")
    g = torch.Generator().manual_seed(D + M)
    x, layers, rope = _rope_case(g, M, D, nq, nkv)
    q, k, v = linear(x, layers)
    qr, kr = F.apply_rope(q.view(1, M, nq, D), k.view(1, M, nkv, D), rope[0], rope[1])
    got = linear(x, layers, rope=rope)
    assert torch.equal(got[0], qr.view(M, -1)) and torch.equal(got[1], kr.view(M, -1)) and torch.equal(got[2], v)
    assert not torch.equal(got[0], q)
    wg, wu = (F.quantize_weight_mxfp4(_randn(g, D + 16, 384) * s) for s in (0.1, 0.3))
    gate, up = linear(x, [(wg, None), (wu, None)])
    assert torch.equal(swiglu(x, wg, wu), F.swiglu(gate, up))


@pytest.mark.parametrize("kern", KERNELS)
def test_a_row_does_not_depend_on_its_batch(kern):
    from touchnet_amd import functional as F
    linear = getattr(F, f"linear_{kern}_mxfp4")
    g = torch.Generator().manual_seed(4)
    x, layers, rope = _rope_case(g, 37, 64, 4, 1, K=1152)
    x128 = torch.cat([x, _randn(g, 91, 1152)])
    pos = torch.cat([(torch.arange(37) * 37 + 5) % 101, torch.arange(91)])[None].to(DEV)
    big = (*F.rope_tables(pos, F.rope_inv_freq(64, 10000.0, device=DEV), torch.bfloat16), 64, (0, 1))
    y37, y128 = linear(x, layers, rope=rope), linear(x128, layers, rope=big)
    for i in (0, 16, 36):
        one = linear(x[i:i + 1], layers, rope=(rope[0][i:i + 1], rope[1][i:i + 1], 64, (0, 1)))
        for a, b, c in zip(one, y37, y128):
            assert torch.equal(a[0], b[i]) and torch.equal(a[0], c[i]), i


@pytest.mark.parametrize("case", ["K=192", "N=24", "M=129", "M=257", "codes int8", "scales fp32", "scales [N, K/32+1]",
                                  "misaligned codes"])
def test_refusals_by_name_and_by_code_before_any_launch(case):
    """`functional` raises by name; the C entries return -22 and leave the output alone (they take no dtypes or shapes of
    tensors: those cases are functional's alone).  M = 129 is the small-M arm's refusal, M = 257 both arms'."""
    from touchnet_amd import _C, functional as F
    M, K, N = {"K=192": (16, 192, 16), "N=24": (16, 128, 24), "M=129": (129, 128, 16), "M=257": (257, 128, 16)}.get(case, (16, 128, 16))
    x = torch.ones(M, K, dtype=torch.bfloat16, device=DEV)
    codes = torch.zeros(N * K // 2 + 16, dtype=torch.int8 if case == "codes int8" else torch.uint8, device=DEV)
    codes = codes[1:N * K // 2 + 1].view(N, K // 2) if case == "misaligned codes" else codes[:N * K // 2].view(N, K // 2)
    scales = torch.full((N, K // 32 + (case == "scales [N, K/32+1]")), 127, device=DEV,
                        dtype=torch.float32 if case == "scales fp32" else torch.uint8)
    w = F.Mxfp4Weight(codes, scales)
    arms = ["smallm"] if case == "M=129" else KERNELS
    for kern in arms:
        with pytest.raises(_C.KernelError, match=f"linear_{kern}_mxfp4"):
            getattr(F, f"linear_{kern}_mxfp4")(x, [(w, None)])
        with pytest.raises(_C.KernelError, match=f"swiglu_{kern}_mxfp4"):
            getattr(F, f"swiglu_{kern}_mxfp4")(x, w, w)
    if "scales" not in case and case != "codes int8":
        y = torch.full((M, N), SENTINEL, dtype=torch.int16, device=DEV)
        one = lambda t, v: (t * 1)(v)
        for kern in arms:
            rc = getattr(_C.lib(), f"tn_gemm_{kern}_mxfp4")(
                x.data_ptr(), K, M, K, 1, one(C.c_void_p, codes.data_ptr()), one(C.c_longlong, K // 2),
                one(C.c_void_p, scales.data_ptr()), one(C.c_longlong, K // 32), None, one(C.c_void_p, y.data_ptr()),
                one(C.c_longlong, N), one(C.c_int, N), None, None, 0, 0, None)
            rc2 = getattr(_C.lib(), f"tn_gemm_{kern}_swiglu_mxfp4")(
                x.data_ptr(), codes.data_ptr(), codes.data_ptr(), scales.data_ptr(), scales.data_ptr(), y.data_ptr(), M, N, K,
                K, K // 2, K // 32, N, None)
            assert rc == -22 and rc2 == -22, (kern, rc, rc2)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all())


@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_quantised_decoders_agree_with_bf16_on_the_dequantised_weights(kind):
    """8 greedy steps, both arms from the same cache state at every step and on IDENTICAL weight values (the bf16 arm is a
    copy of the model holding the dequantised weights): logits within the project's cached-vs-recomputed bound — a
    summation-order bound, not a quantisation bound —, the same argmax wherever the bf16 arm's top-2 margin is clear.  Then
    transcribe with MXFP4 weights and an FP8 cache together."""
    from touchnet_amd import _C, functional as F, generation as G
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts, transcribe
    model, feats = _tiny(kind, seed=12)
    ref = copy.deepcopy(model)
    assert G.quantize_decoder_weights(model, "mxfp4") > 0 and G.quantize_decoder_weights(model, "mxfp4") == 0
    swapped = {n: m for n, m in model.named_modules() if isinstance(m, G.Mxfp4Linear)}
    assert len(swapped) == 2 * 7 + 1 and model.language_model.model.embed_tokens.weight.dtype == torch.bfloat16
    for name, m in swapped.items():
        ref.get_submodule(name).weight = torch.nn.Parameter(F.dequantize_weight_mxfp4(m.weight))     # (unties lm_head)
    (lm, _), (lm_ref, proj_w) = G._parts(model), G._parts(ref)
    c = lm.config
    with torch.no_grad():
        cache = G.KVCache.allocate(len(lm.model.layers), 5, 57 + 16, c.num_key_value_heads, c.head_dim, DEV)
        logits = G._prefill(lm_ref, proj_w, build_prompts(feats, 1, 2), cache, DEV)
        for step in range(8):
            F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, 1.0, 0, -1, 1)
            mx = G.decode_logits(lm, cache).float()
            logits = G.decode_logits(lm_ref, cache)               # (written last: the caches follow the bf16 arm)
            bf = logits.float()
            diff = float((mx - bf).abs().max())
            print(f"{kind} step {step}: max|mxfp4 - bf16| = {diff:.4g}, max|bf16| = {float(bf.abs().max()):.4g}")
            assert diff <= 3e-2 * float(bf.abs().max())
            top2 = bf.topk(2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > 2 * diff
            assert torch.equal(mx.argmax(1)[clear], bf.argmax(1)[clear])
        with pytest.raises(_C.KernelError, match="autograd"), torch.enable_grad():
            G.decode_logits(lm, cache)
    ids = transcribe(ref, feats, G.GenerationConfig(max_new_tokens=8, weight_dtype="mxfp4", kv_cache_dtype="fp8_e4m3"))
    assert isinstance(ref.language_model.lm_head, G.Mxfp4Linear) and len(ids) == 5 and all(len(i) <= 8 for i in ids)
