"""FP8 (e4m3) weight-only decode linears: tn_weight_quantize_fp8 against a torch restatement of the format, the FP8 variant
of the small-M kernel (tn_gemm_smallm_fp8, tn_gemm_smallm_swiglu_fp8) against float64 on the dequantised weights, its
epilogues against the row kernels, and the decoders after generation.quantize_decoder_weights."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7B7B          # bit pattern the output buffers hold wherever nothing may be written
SMALL_CODES = torch.tensor(list(range(0x00, 0x51)) + list(range(0x80, 0xD1)), dtype=torch.uint8)    # finite, |value| <= 8


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _values(w):
    """float64 [N, K] of an Fp8Weight, by torch's own e4m3 decoding"""
    return w.codes.cpu().view(torch.float8_e4m3fn).double() * w.scale.cpu().double()[:, None]


def _pitched(t, pad, fill):
    buf = torch.full((t.shape[0] + 3, t.shape[1] + pad), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf[:t.shape[0], :t.shape[1]]


@pytest.mark.parametrize("Ns", [[16], [48], [256, 64, 64]])
@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 37, 128])
def test_exact_products_and_nothing_else_is_written(M, K, Ns):
    """x in {-1, 0, 1}, codes uniform over the finite codes with |value| <= 8 (both zeros and every subnormal), scales
    2^(n % 5 - 2), integer biases on segments 0 and 2: every partial sum is a multiple of 2^-9 below 2^14, so any order
    is exact and the result is bf16(float64(x . code scale) + bias) bit for bit.  Operands are pitched views in NaN (x) /
    the NaN code (codes), outputs pitched views in a sentinel."""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(1000 * M + K)
    x = _pitched(torch.randint(-1, 2, (M, K), generator=g).to(DEV, torch.bfloat16), 8, float("nan"))
    layers = []
    for i, N in enumerate(Ns):
        codes = SMALL_CODES[torch.randint(0, len(SMALL_CODES), (N, K), generator=g)].to(DEV)
        scale = (2.0 ** (torch.arange(N) % 5 - 2)).to(DEV, torch.float32)
        bias = torch.randint(-8, 9, (N,), generator=g).to(DEV, torch.bfloat16) if i != 1 else None
        layers.append((F.Fp8Weight(_pitched(codes, 16, 0x7F), scale), bias))
    bufs = [torch.full((M + 2, N + 8), SENTINEL, dtype=torch.int16, device=DEV) for N in Ns]
    F.linear_smallm_fp8(x, layers, outs=[b.view(torch.bfloat16)[:M, :N] for b, N in zip(bufs, Ns)])
    for (w, b), buf, N in zip(layers, bufs, Ns):
        ref = x.cpu().double() @ _values(w).t() + (b.cpu().double() if b is not None else 0)
        want = torch.full_like(buf, SENTINEL)
        want[:M, :N] = ref.to(torch.bfloat16).view(torch.int16).to(DEV)
        assert torch.equal(buf, want), (M, K, N, int((buf != want).sum()))


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("N", [16400, 32784])
def test_exact_products_in_groups_of_two_and_four_strips(N, M):
    """The widths at which a workgroup owns two strips (1025 strips: an odd count) and four (2049: a tail group of one)."""
    test_exact_products_and_nothing_else_is_written(M, 128, [N])


@pytest.mark.parametrize("K", [384, 1152])
def test_real_products_within_the_bf16_kernels_budget(K):
    """|y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k| on the dequantised weights: one bf16 rounding + fp32 accumulation in
    any order, no term for the format (measured worst / bound: 0.93 at K = 384, 0.74 at K = 1152)."""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(K)
    x, w, b = _randn(g, 37, K), F.quantize_weight_fp8(_randn(g, 48, K)), _randn(g, 48)
    y = F.linear_smallm_fp8(x, [(w, b)])[0].cpu().double()
    xd, wd = x.cpu().double(), _values(w)
    ref = xd @ wd.t() + b.cpu().double()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (xd.abs() @ wd.abs().t())
    ratio = float(((y - ref).abs() / bound).max())
    print(f"K = {K}: worst |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("K", [8, 136, 1152])
def test_quantiser_equals_a_plain_restatement(K):
    """scale = 2^e, e the smallest integer >= -100 with amax <= 448 2^e; codes = (w 2^-e).to(float8_e4m3fn).  Planted rows:
    ties (17 and 19 beside amax 448: halfway between codes), amax exactly 448 2^-3, amax just above 448, an all-zero
    row, a row below the lowest scale.  A NaN row is refused by name."""
    from touchnet_amd import _C, functional as F
    w = torch.randn(12, K, generator=torch.Generator().manual_seed(K)).to(torch.bfloat16)
    w[0, :3] = torch.tensor([448.0, 17.0, 19.0]).to(torch.bfloat16)
    w[1] *= 0.1
    w[1, 0] = 56.0
    w[2, 0] = 450.0
    w[3] = 0
    w[4] *= 2.0 ** -120
    q = F.quantize_weight_fp8(w.to(DEV))
    es = torch.arange(-100, 40, dtype=torch.float64)
    e = es[(w.double().abs().amax(1)[:, None] <= 448 * 2.0 ** es[None]).int().argmax(1)]
    assert e[:5].tolist() == [0, -3, 1, -100, -100]
    codes = (w.double() * 2.0 ** -e[:, None]).float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q.scale.cpu(), (2.0 ** e).float()) and torch.equal(q.codes.cpu(), codes)
    assert torch.equal(F.dequantize_weight_fp8(q).cpu().double(), _values(q))
    w[5, K - 1] = float("nan")
    with pytest.raises(_C.KernelError, match="quantize_weight_fp8.*NaN"):
        F.quantize_weight_fp8(w.to(DEV))


def _rope_case(g, M, D, nq, nkv, K=384):
    from touchnet_amd import functional as F
    layers = [(F.quantize_weight_fp8(_randn(g, n * D, K)), _randn(g, n * D)) for n in (nq, nkv, nkv)]
    pos = ((torch.arange(M) * 37 + 5) % 101)[None].to(DEV)                  # positions that differ per row
    cos, sin = F.rope_tables(pos, F.rope_inv_freq(D, 10000.0, device=DEV), torch.bfloat16)
    return _randn(g, M, K), layers, (cos, sin, D, (0, 1))


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("D,nq,nkv", [(64, 4, 1), (128, 2, 1)])
def test_epilogues_are_the_row_kernels_on_the_plain_fp8_products(D, nq, nkv, M):
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(D + M)
    x, layers, rope = _rope_case(g, M, D, nq, nkv)
    q, k, v = F.linear_smallm_fp8(x, layers)
    qr, kr = F.apply_rope(q.view(1, M, nq, D), k.view(1, M, nkv, D), rope[0], rope[1])
    got = F.linear_smallm_fp8(x, layers, rope=rope)
    assert torch.equal(got[0], qr.view(M, -1)) and torch.equal(got[1], kr.view(M, -1)) and torch.equal(got[2], v)
    assert not torch.equal(got[0], q)
    wg, wu = (F.quantize_weight_fp8(_randn(g, D + 16, 384) * s) for s in (0.1, 0.3))       # (row scales that differ)
    gate, up = F.linear_smallm_fp8(x, [(wg, None), (wu, None)])
    assert torch.equal(F.swiglu_smallm_fp8(x, wg, wu), F.swiglu(gate, up))


def test_a_row_does_not_depend_on_its_batch():
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(4)
    x, layers, rope = _rope_case(g, 37, 64, 4, 1, K=1152)
    x128 = torch.cat([x, _randn(g, 91, 1152)])
    pos = torch.cat([(torch.arange(37) * 37 + 5) % 101, torch.arange(91)])[None].to(DEV)
    big = (*F.rope_tables(pos, F.rope_inv_freq(64, 10000.0, device=DEV), torch.bfloat16), 64, (0, 1))
    y37, y128 = F.linear_smallm_fp8(x, layers, rope=rope), F.linear_smallm_fp8(x128, layers, rope=big)
    for i in (0, 16, 36):
        one = F.linear_smallm_fp8(x[i:i + 1], layers, rope=(rope[0][i:i + 1], rope[1][i:i + 1], 64, (0, 1)))
        for a, b, c in zip(one, y37, y128):
            assert torch.equal(a[0], b[i]) and torch.equal(a[0], c[i]), i


@pytest.mark.parametrize("case", ["K=192", "N=24", "M=129", "codes int8", "scale fp64", "scale [N+1]", "misaligned codes"])
def test_refusals_by_name_and_by_code_before_any_launch(case):
    """`functional` raises by name; the C entries return -22 and leave the output alone (they take no dtypes or shapes of
    tensors: those cases are functional's alone)."""
    from touchnet_amd import _C, functional as F
    M, K, N = {"K=192": (16, 192, 16), "N=24": (16, 128, 24), "M=129": (129, 128, 16)}.get(case, (16, 128, 16))
    x = torch.ones(M, K, dtype=torch.bfloat16, device=DEV)
    codes = torch.zeros(N * K + 16, dtype=torch.int8 if case == "codes int8" else torch.uint8, device=DEV)
    codes = codes[1:N * K + 1].view(N, K) if case == "misaligned codes" else codes[:N * K].view(N, K)
    scale = torch.ones(N + (case == "scale [N+1]"), dtype=torch.float64 if case == "scale fp64" else torch.float32, device=DEV)
    w = F.Fp8Weight(codes, scale)
    with pytest.raises(_C.KernelError, match="linear_smallm_fp8"):
        F.linear_smallm_fp8(x, [(w, None)])
    with pytest.raises(_C.KernelError, match="swiglu_smallm_fp8"):
        F.swiglu_smallm_fp8(x, w, w)
    if "scale" not in case and case != "codes int8":
        y = torch.full((M, N), SENTINEL, dtype=torch.int16, device=DEV)
        one = lambda t, v: (t * 1)(v)
        rc = _C.lib().tn_gemm_smallm_fp8(x.data_ptr(), K, M, K, 1, one(C.c_void_p, codes.data_ptr()), one(C.c_longlong, K),
                                         one(C.c_void_p, scale.data_ptr()), None, one(C.c_void_p, y.data_ptr()),
                                         one(C.c_longlong, N), one(C.c_int, N), None, None, 0, 0, None)
        rc2 = _C.lib().tn_gemm_smallm_swiglu_fp8(x.data_ptr(), codes.data_ptr(), codes.data_ptr(), scale.data_ptr(),
                                                 scale.data_ptr(), y.data_ptr(), M, N, K, K, K, N, None)
        torch.cuda.synchronize()
        assert rc == -22 and rc2 == -22 and bool((y == SENTINEL).all())


def _tiny(kind, seed):
    from touchnet_amd.models.llama import DecoderConfig
    from touchnet_amd.models.touch_audio import TouchAudioConfig, TouchAudioForCausalLM
    text = dict(model_type="llama", hidden_size=256, intermediate_size=512, num_attention_heads=8, num_key_value_heads=2,
                head_dim=64, vocab_size=512, rope_theta=500000.0, tie_word_embeddings=True, rms_norm_eps=1e-5)
    if kind == "qwen2":
        text = dict(model_type="qwen2", hidden_size=512, intermediate_size=768, num_attention_heads=4, num_key_value_heads=1,
                    head_dim=128, vocab_size=640, rope_theta=1000000.0, tie_word_embeddings=False, rms_norm_eps=1e-6)
    text.update(num_hidden_layers=2, initializer_range=0.08, pad_token_id=1, bos_token_id=2, eos_token_id=3)
    torch.manual_seed(seed)
    m = TouchAudioForCausalLM(TouchAudioConfig(text_config=DecoderConfig.from_dict(text), input_size=80, pad_token_id=1))
    m.post_init()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_(0, 0.1)
    g = torch.Generator().manual_seed(5)
    return m.to(DEV).to(torch.bfloat16), [torch.randn(n, 80, generator=g) for n in (23, 1, 57, 8, 40)]


@pytest.mark.parametrize("kind", ["llama", "qwen2"])
def test_quantised_decoders_agree_with_bf16_on_the_dequantised_weights(kind):
    """8 greedy steps, both arms from the same cache state at every step and on IDENTICAL weight values (the bf16 arm is a
    copy of the model holding the dequantised weights): logits within the project's cached-vs-recomputed bound — a
    summation-order bound, not a quantisation bound —, the same argmax wherever the bf16 arm's top-2 margin is clear.  Then
    transcribe with FP8 weights and an FP8 cache together."""
    from touchnet_amd import _C, functional as F, generation as G
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts, transcribe
    model, feats = _tiny(kind, seed=12)
    ref = copy.deepcopy(model)
    assert G.quantize_decoder_weights(model) > 0 and G.quantize_decoder_weights(model) == 0
    swapped = {n: m for n, m in model.named_modules() if isinstance(m, G.Fp8Linear)}
    assert len(swapped) == 2 * 7 + 1 and model.language_model.model.embed_tokens.weight.dtype == torch.bfloat16
    for name, m in swapped.items():
        ref.get_submodule(name).weight = torch.nn.Parameter(F.dequantize_weight_fp8(m.weight))     # (unties lm_head)
    (lm, _), (lm_ref, proj_w) = G._parts(model), G._parts(ref)
    c = lm.config
    with torch.no_grad():
        cache = G.KVCache.allocate(len(lm.model.layers), 5, 57 + 16, c.num_key_value_heads, c.head_dim, DEV)
        logits = G._prefill(lm_ref, proj_w, build_prompts(feats, 1, 2), cache, DEV)
        for step in range(8):
            F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, 1.0, 0, -1, 1)
            fp8 = G.decode_logits(lm, cache).float()
            logits = G.decode_logits(lm_ref, cache)               # (written last: the caches follow the bf16 arm)
            bf = logits.float()
            diff = float((fp8 - bf).abs().max())
            print(f"{kind} step {step}: max|fp8 - bf16| = {diff:.4g}, max|bf16| = {float(bf.abs().max()):.4g}")
            assert diff <= 3e-2 * float(bf.abs().max())
            top2 = bf.topk(2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > 2 * diff
            assert torch.equal(fp8.argmax(1)[clear], bf.argmax(1)[clear])
        with pytest.raises(_C.KernelError, match="autograd"), torch.enable_grad():
            G.decode_logits(lm, cache)
    ids = transcribe(ref, feats, G.GenerationConfig(max_new_tokens=8, weight_dtype="fp8_e4m3", kv_cache_dtype="fp8_e4m3"))
    assert isinstance(ref.language_model.lm_head, G.Fp8Linear) and len(ids) == 5 and all(len(i) <= 8 for i in ids)
