"""The small-M weight-streaming GEMM of the decode step (csrc/gemm_smallm.hip: tn_gemm_smallm, tn_gemm_smallm_swiglu) against
float64, its epilogues against the row kernels they stand in for, and the decoders with it switched on and off."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7B7B          # bit pattern the output buffers hold wherever nothing may be written


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(DEV, torch.bfloat16)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV, torch.bfloat16)


def _pitched(t, rows_behind=0):
    """t as a view with a row pitch above its width inside a NaN-filled buffer (`rows_behind` NaN rows follow it)"""
    buf = torch.full((t.shape[0] + rows_behind, t.shape[1] + 8), float("nan"), dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf[:t.shape[0], :t.shape[1]]


@pytest.mark.parametrize("Ns", [[16], [48], [256, 64, 64]])
@pytest.mark.parametrize("K", [64, 320, 1088])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 37, 128])
def test_integer_products_are_exact_and_nothing_else_is_written(M, K, Ns):
    """|x| <= 1, |w| <= 255: every partial sum is an integer below 2^24, so any summation order is exact and the result is
    bf16(float64 product + bias) bit for bit.  Operands are pitched views in NaN, outputs pitched views in a sentinel."""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(1000 * M + K)
    x = _pitched(_ints(g, -1, 1, M, K), rows_behind=3)
    layers = [(_pitched(_ints(g, -255, 255, N, K)), _ints(g, -8, 8, N) if i != 1 else None) for i, N in enumerate(Ns)]
    bufs = [torch.full((M + 2, N + 8), SENTINEL, dtype=torch.int16, device=DEV) for N in Ns]
    F.linear_smallm(x, layers, outs=[b.view(torch.bfloat16)[:M, :N] for b, N in zip(bufs, Ns)])
    for (w, b), buf, N in zip(layers, bufs, Ns):
        ref = x.double() @ w.double().t() + (b.double() if b is not None else 0)
        want = torch.full_like(buf, SENTINEL)
        want[:M, :N] = ref.to(torch.bfloat16).view(torch.int16)
        assert torch.equal(buf, want), (M, K, N, int((buf != want).sum()))


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("N", [16400, 32784])
def test_integer_products_are_exact_in_groups_of_two_and_four_strips(N, M):
    """The widths at which a workgroup owns two strips (1025 strips: an odd count) and four (2049: a tail group of one) — the
    variants that serve the 7B MLPs and lm_head — on the first test's data and rule."""
    test_integer_products_are_exact_and_nothing_else_is_written(M, 64, [N])


@pytest.mark.parametrize("K", [320, 1088])
def test_real_products_within_one_rounding_of_float64(K):
    """|y - ref| <= 2^-8 |ref| + K 2^-24 sum_k |x_k w_k|: one bf16 rounding + fp32 accumulation in any order"""
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(K)
    x, w, b = _randn(g, 37, K), _randn(g, 48, K), _randn(g, 48)
    y = F.linear_smallm(x, [(w, b)])[0].double()
    ref = x.double() @ w.double().t() + b.double()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t())
    ratio = float(((y - ref).abs() / bound).max())
    print(f"K = {K}: worst |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def _rope_case(g, M, D, nq, nkv, K=320):
    from touchnet_amd import functional as F
    x = _randn(g, M, K)
    layers = [(_randn(g, n * D, K), _randn(g, n * D)) for n in (nq, nkv, nkv)]
    pos = ((torch.arange(M) * 37 + 5) % 101)[None].to(DEV)                  # positions that differ per row
    cos, sin = F.rope_tables(pos, F.rope_inv_freq(D, 10000.0, device=DEV), torch.bfloat16)
    return x, layers, (cos, sin, D, (0, 1))


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("D,nq,nkv", [(64, 4, 1), (128, 2, 1)])
def test_rope_epilogue_is_apply_rope_of_the_plain_product(D, nq, nkv, M):
    from touchnet_amd import functional as F
    x, layers, rope = _rope_case(torch.Generator().manual_seed(D + M), M, D, nq, nkv)
    q, k, v = F.linear_smallm(x, layers)
    qr, kr = F.apply_rope(q.view(1, M, nq, D), k.view(1, M, nkv, D), rope[0], rope[1])
    got = F.linear_smallm(x, layers, rope=rope)
    assert torch.equal(got[0], qr.view(M, -1)) and torch.equal(got[1], kr.view(M, -1)) and torch.equal(got[2], v)
    assert not torch.equal(got[0], q)


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("I", [16, 80])
def test_swiglu_epilogue_is_swiglu_of_the_plain_products(I, M):
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(I + M)
    x, wg, wu = _randn(g, M, 320), _randn(g, I, 320) * 0.1, _randn(g, I, 320) * 0.1
    gate, up = F.linear_smallm(x, [(wg, None), (wu, None)])
    assert torch.equal(F.swiglu_smallm(x, wg, wu), F.swiglu(gate, up))


def test_a_row_does_not_depend_on_its_batch():
    from touchnet_amd import functional as F
    g = torch.Generator().manual_seed(4)
    x, layers, rope = _rope_case(g, 37, 64, 4, 1, K=1088)
    x128 = torch.cat([x, _randn(g, 91, 1088)])
    pos = torch.cat([(torch.arange(37) * 37 + 5) % 101, torch.arange(91)])[None].to(DEV)
    big = (*F.rope_tables(pos, F.rope_inv_freq(64, 10000.0, device=DEV), torch.bfloat16), 64, (0, 1))
    y37, y128 = F.linear_smallm(x, layers, rope=rope), F.linear_smallm(x128, layers, rope=big)
    for i in (0, 16, 36):
        one = F.linear_smallm(x[i:i + 1], layers, rope=(rope[0][i:i + 1], rope[1][i:i + 1], 64, (0, 1)))
        for a, b, c in zip(one, y37, y128):
            assert torch.equal(a[0], b[i]) and torch.equal(a[0], c[i]), i


@pytest.mark.parametrize("case", ["M=0", "M=129", "K=96", "N=24", "fp32", "misaligned"])
def test_refusals_by_name_and_by_code_before_any_launch(case):
    """`functional` raises by name; the C entry returns -22 and leaves the output alone (it takes no dtype: the fp32 case is
    functional's alone)."""
    from touchnet_amd import _C, functional as F
    M, K, N = {"M=0": (0, 64, 16), "M=129": (129, 64, 16), "K=96": (16, 96, 16), "N=24": (16, 64, 24)}.get(case, (16, 64, 16))
    x = torch.ones(M * K + 8, dtype=torch.float32 if case == "fp32" else torch.bfloat16, device=DEV)
    x = x[1:M * K + 1].view(M, K) if case == "misaligned" else x[:M * K].view(M, K)
    w = torch.ones(N, K, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_C.KernelError, match="linear_smallm"):
        F.linear_smallm(x, [(w, None)])
    with pytest.raises(_C.KernelError, match="swiglu_smallm"):
        F.swiglu_smallm(x, w, w)
    if case != "fp32":
        y = torch.full((max(M, 1), N), SENTINEL, dtype=torch.int16, device=DEV)
        one = lambda t, v: (t * 1)(v)
        rc = _C.lib().tn_gemm_smallm(x.data_ptr(), K, M, K, 1, one(C.c_void_p, w.data_ptr()), one(C.c_longlong, K), None,
                                     one(C.c_void_p, y.data_ptr()), one(C.c_longlong, N), one(C.c_int, N), None, None, 0, 0, None)
        rc2 = _C.lib().tn_gemm_smallm_swiglu(x.data_ptr(), w.data_ptr(), w.data_ptr(), y.data_ptr(), M, N, K, K, K, N, None)
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
def test_decoders_agree_between_the_two_switch_positions(kind, monkeypatch):
    """8 greedy steps, both arms from the same cache state at every step: logits within the project's cached-vs-recomputed
    bound, the same argmax wherever the library arm's top-2 margin is clear; then beam search (15 rows) id for id."""
    from touchnet_amd import functional as F, generation as G
    from touchnet_amd.models.touch_audio.inference_touch_audio import build_prompts, transcribe
    model, feats = _tiny(kind, seed=12)          # (seed 11 ends one llama beam on a near-tie between two tokens)
    lm, proj_w = G._parts(model)
    c = lm.config
    prompts = build_prompts(feats, 1, 2)
    with torch.no_grad():
        cache = G.KVCache.allocate(len(lm.model.layers), 5, 57 + 16, c.num_key_value_heads, c.head_dim, DEV)
        logits = G._prefill(lm, proj_w, prompts, cache, DEV)
        ran_own = False
        for step in range(8):
            F.greedy_step(logits, cache.hist, cache.hist_len, cache.cache_len, cache.finished, cache.n_unfinished, 1.0, 0, -1, 1)
            monkeypatch.setattr(F, "DECODE_GEMM", "own")
            own = G.decode_logits(lm, cache).float()
            monkeypatch.setattr(F, "DECODE_GEMM", "lib")
            logits = G.decode_logits(lm, cache)                   # (written last: the caches follow the library arm)
            lib = logits.float()
            diff = float((own - lib).abs().max())
            print(f"{kind} step {step}: max|own - lib| = {diff:.4g}, max|lib| = {float(lib.abs().max()):.4g}")
            assert diff <= 3e-2 * float(lib.abs().max())
            top2 = lib.topk(2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > 2 * diff
            assert torch.equal(own.argmax(1)[clear], lib.argmax(1)[clear])
            ran_own = ran_own or diff > 0
        assert ran_own                    # (two arms of equal bits at every step would both be the library)
    ids = {}
    for arm in ("own", "lib"):
        monkeypatch.setattr(F, "DECODE_GEMM", arm)
        ids[arm] = transcribe(model, feats, G.GenerationConfig(num_beams=3, max_new_tokens=8))
    assert ids["own"] == ids["lib"]
