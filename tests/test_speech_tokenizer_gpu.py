"""Kimi-Audio's speech tokenizer on the MI355X: tn_attn_block_causal_fwd against an fp32 restatement of the reference's
additive mask (modeling_kimi_audio.py:226-242), tn_vq_nearest against an fp64 argmin, the module against the
reference-run fixture (tests/golden/speech_tokenizer.npz, make_golden_speech_tokenizer.py), trimmed against full length
at whisper-large-v3 width, and the Kimi-Audio model computing its own ids."""
import ast
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speech_tokenizer.npz")


def _ref_mask(lengths, T, block):
    """the reference's get_block_causal_attention_mask (:226-242) as a boolean [n, T, T] (True = allowed)"""
    i = torch.arange(T, device=DEV)
    causal = i[None, :] <= i[:, None]
    same = (i[None, :] // block) == (i[:, None] // block)
    m = i[None, :] < torch.as_tensor(lengths, device=DEV)[:, None]            # [n, T] valid keys
    return (causal | same)[None] & m[:, None, :]


def _ref_attention(q, k, v, allowed, scale):
    """fp32 softmax with the reference's additive finfo.min mask"""
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s + (~allowed)[:, None].float() * torch.finfo(torch.float32).min
    return (torch.softmax(s, -1) @ vf).transpose(1, 2)


@pytest.mark.parametrize("block", [200, 64, 100, 1, 1500, 4096])
def test_block_causal_attention_matches_the_reference_mask(block):
    import touchnet_amd.functional as F
    lengths = [1, 63, 64, 199, 200, 201, 777, 1500]
    n, T, Nh, D = len(lengths), 1500, 20, 64
    g = torch.Generator(device=DEV).manual_seed(block)
    q, k, v = (torch.randn(n, T, Nh, D, device=DEV, generator=g).bfloat16() for _ in range(3))
    kl = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    mask = F.block_causal_mask(torch.zeros(n, T, dtype=torch.int32, device=DEV), kl[:, None].expand(n, T), block)
    out = F.block_causal_attention(q, k, v, mask)
    again = F.block_causal_attention(q, k, v, mask)
    ref = _ref_attention(q, k, v, _ref_mask(lengths, T, block), D ** -0.5)
    err = (out.float() - ref).abs()
    assert bool((err <= 2e-2 + 2e-2 * ref.abs()).all()), float(err.max())            # padded query rows included
    assert torch.equal(out, again)


def test_block_causal_attention_packed_clips():
    """Clips back to back in one row (the trimmed schedule): each clip exactly as in its own row."""
    import touchnet_amd.functional as F
    Nh, D, block = 4, 64, 50
    clips = [(150, 150), (100, 37), (200, 1), (50, 50)]                           # (frames, valid keys)
    R = sum(f for f, _ in clips)
    g = torch.Generator(device=DEV).manual_seed(3)
    q, k, v = (torch.randn(1, R, Nh, D, device=DEV, generator=g).bfloat16() for _ in range(3))
    start, end, off = [], [], 0
    for f, L in clips:
        start += [off] * f
        end += [off + L] * f
        off += f
    mask = F.block_causal_mask(torch.tensor([start], dtype=torch.int32, device=DEV),
                               torch.tensor([end], dtype=torch.int32, device=DEV), block)
    out = F.block_causal_attention(q, k, v, mask)
    off = 0
    for f, L in clips:
        sl = slice(off, off + f)
        ref = _ref_attention(q[:, sl], k[:, sl], v[:, sl], _ref_mask([L], f, block), D ** -0.5)
        err = (out[:, sl].float() - ref).abs()
        assert bool((err <= 2e-2 + 2e-2 * ref.abs()).all()), (f, L, float(err.max()))
        off += f


def _check_vq(x, cb, ids):
    """ids against an fp64 argmin over the same bf16 operands: equal, or within the fp32 dot-product error bound"""
    xd, cd = x.double(), cb.double()
    dist = (cd * cd).sum(1)[None] - 2 * xd @ cd.t()
    best = dist.argmin(1)
    bad = ids != best
    if bad.any():
        r = bad.nonzero()[:, 0]
        gap = dist[r, ids[r]] - dist[r, best[r]]
        bound = 4 * x.shape[1] * 2.0 ** -24 * ((xd[r].abs() @ cd.abs().t()).max(1).values + (cd * cd).sum(1).max())
        assert bool((gap <= bound).all()), (int(bad.sum()), float((gap / bound).max()))
        assert int(bad.sum()) <= max(1, x.shape[0] // 1000), int(bad.sum())


@pytest.mark.parametrize("M,V,d", [(1, 16384, 1280), (375, 16384, 1280), (59 * 375, 16384, 1280), (114, 64, 128)])
def test_vq_nearest_against_fp64_argmin(M, V, d):
    import touchnet_amd.functional as F
    g = torch.Generator(device=DEV).manual_seed(M)
    cb = torch.randn(V, d, device=DEV, generator=g).bfloat16()
    x = (cb[torch.randint(0, V, (M,), device=DEV, generator=g)].float()
         + 0.7 * torch.randn(M, d, device=DEV, generator=g)).bfloat16()
    cn = F.codebook_sqnorm(cb)                                                          # (once per frozen codebook)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ids = F.vq_nearest(x, cb, cn)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < max(M * V, 4 << 20)               # no fp32 [M, V] buffer
    assert ids.dtype == torch.int64 and ids.shape == (M,)
    _check_vq(x, cb, ids)
    assert torch.equal(ids, F.vq_nearest(x, cb, cn))
    if M > 1:                                                                            # a row's id ignores its neighbours
        assert torch.equal(ids[M // 2:M // 2 + 1], F.vq_nearest(x[M // 2:M // 2 + 1], cb, cn))


def test_vq_nearest_ties_go_to_the_lowest_index():
    import touchnet_amd.functional as F
    g = torch.Generator(device=DEV).manual_seed(5)
    V, d = 4096, 256
    cb = torch.randn(V, d, device=DEV, generator=g).bfloat16()
    src = torch.randint(0, V, (300,), device=DEV, generator=g)
    dup = torch.randint(0, V, (300,), device=DEV, generator=g)
    cb[dup] = cb[src]                                                   # duplicated rows, in both orders
    x = cb[src].clone()
    ids = F.vq_nearest(x, cb)
    same = (cb[None, :, :] == x[:, None, :]).all(-1)                   # every exact copy of a row's own code
    first = torch.where(same, torch.arange(V, device=DEV)[None], V).min(1).values
    assert torch.equal(ids, first)


def _fixture_model():
    from touchnet_amd.models.kimi_audio.speech_tokenizer import WhisperVQConfig, WhisperVQEncoder
    g = np.load(GOLD)
    m = WhisperVQEncoder(WhisperVQConfig.from_dict(ast.literal_eval(str(g["config_json"]))))
    sd = {k[len("param/"):]: torch.from_numpy(g[k].copy()).view(torch.bfloat16) for k in g.files if k.startswith("param/")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and sorted(missing) == ["ema_count", "ema_weight"], (missing, unexpected)
    return m.to(DEV), g


def _flip_bound(x_a, x_b, cb, i_a, i_b):
    """Rows whose ids differ between two pooled states x_a / x_b of the same tokens: an id can flip only where the
    distance gap between the two choices, at x_a, is within what the state difference can move it, 2 |x_b - x_a| |c - c'|
    (dist_c(x) = |c|^2 - 2 x.c), plus the fp32 dot-product error of the quantiser.  -> (gap, bound) per differing row."""
    xa, xb, cd = x_a.double(), x_b.double(), cb.double()
    r = (i_a != i_b).nonzero()[:, 0]
    ca, cb_ = cd[i_a[r]], cd[i_b[r]]
    gap = ((cb_ * cb_).sum(1) - 2 * (xa[r] * cb_).sum(1)) - ((ca * ca).sum(1) - 2 * (xa[r] * ca).sum(1))
    dx = (xb[r] - xa[r]).norm(dim=1)
    kernel = 4 * cd.shape[1] * 2.0 ** -24 * (xa[r].abs().max(1).values * cd.abs().max() * cd.shape[1] + (cd * cd).sum(1).max())
    return gap.abs(), 2 * dx * (cb_ - ca).norm(dim=1) + 2 * kernel


def _trimmed_against_full(m, feats, mask, K):
    """The trimmed schedule against the full one on the needed ids: the pooled states agree to the bf16 noise of the layers
    (a window that read a wrong frame would be off by the states' own scale), and every id that differs is one the
    measured state difference can flip (_flip_bound).  -> (differing ids, needed ids)"""
    n, S = feats.shape[0], -(-(feats.shape[2] // 2) // m.config.pooling_kernel_size)
    x_f, _ = m.pooled(feats, mask)
    x_t, slots = m.pooled(feats, mask, clip_tokens=K)
    full, trimmed = m(feats, mask).view(-1), m(feats, mask, clip_tokens=K).view(-1)
    assert torch.equal(full, m(feats, mask).view(-1)) and torch.equal(trimmed, m(feats, mask, clip_tokens=K).view(-1))
    need = torch.zeros(n * S, dtype=torch.bool, device=DEV)
    need[slots] = True
    assert bool((trimmed[~need] == 0).all()) and int(need.sum()) == sum(K)
    err = float((x_t.float() - x_f[slots].float()).abs().max()) / float(x_f.abs().max())
    assert err < 2e-2, err
    gap, bound = _flip_bound(x_f[slots], x_t, m.codebook.weight, full[slots], trimmed[slots])
    assert bool((gap <= bound).all()), (gap.tolist(), bound.tolist())
    return int((full[slots] != trimmed[slots]).sum()), int(need.sum()), err


def test_tokenizer_matches_the_reference_run_fixture():
    m, g = _fixture_model()
    feats = torch.from_numpy(g["features"]).to(DEV)
    mask = torch.from_numpy(g["mask"]).to(DEV)
    hid = m.hidden_states(feats, mask).float().cpu()
    ref = torch.from_numpy(g["hidden"].copy()).view(torch.bfloat16).float()
    err = float((hid - ref).abs().max()) / float(ref.abs().max())
    assert err < 2e-2, err
    ids = m(feats, mask).cpu()
    # an id is "clear" when its stored margin (reference, fp64) exceeds what the measured difference between this
    # pipeline's pooled state and the reference's can move a distance gap (+ the stored states' bf16 rounding)
    n, T, d = ref.shape
    p = m.config.pooling_kernel_size
    pool = lambda h: torch.nn.functional.pad(h, (0, 0, 0, (-T) % p)).reshape(n, -1, p, d).double().mean(2)
    x_ours, x_ref = pool(hid), pool(ref)
    dx = (x_ours - x_ref).norm(dim=-1) + 2.0 ** -8 * x_ref.norm(dim=-1)
    cb = m.codebook.weight.double().cpu()
    best = torch.from_numpy(g["ids"])
    reach = (cb[best] [..., None, :] - cb).norm(dim=-1).amax(-1)                  # farthest code from the chosen one
    margin = torch.from_numpy(g["margin"]).double()
    clear = margin > 2 * dx * reach
    print(f"fixture: {int(clear.sum())} of {clear.numel()} ids clear of the measured noise; hidden err {err:.2e}")
    assert float(clear.double().mean()) > 0.75, float(clear.double().mean())
    assert torch.equal(ids[clear], best[clear]), (ids != best) & clear
    # the trimmed schedule on the ids each clip's valid length asks for; T = 150 is not a multiple of p = 4, so a clip that
    # needs all 38 ids pools two zero frames — also with that clip last in the packed row, in front of nothing
    K = [-(-int(L) // 8) for L in g["mask"].sum(1)]
    for order in ([0, 1, 2], [2, 1, 0]):
        diff, total, xerr = _trimmed_against_full(m, feats[order], mask[order], [K[i] for i in order])
        print(f"fixture trimmed vs full, clips {order}: {diff} of {total} ids differ, pooled states {xerr:.2e}")


def test_trimmed_pools_zero_frames_past_a_clip_like_the_reference():
    """T % p != 0 and every clip asks for all S ids (full-length clips, the last one last in the packed row): the last id
    of each clip averages its last T % p frames with p - T % p zero frames, as the reference's right padding does."""
    m, g = _fixture_model()
    feats = torch.from_numpy(g["features"]).to(DEV)
    mask = torch.ones(3, 300, dtype=torch.int32, device=DEV)
    diff, total, xerr = _trimmed_against_full(m, feats, mask, [38, 38, 38])
    assert total == 114


def test_full_width_trimmed_equals_full_length():
    """whisper-large-v3 widths, 16 layers, V 16384, random bf16 weights; clips from 0.1 s to 30 s.  Exact in arithmetic
    (test_trimming_drops_no_frame_a_needed_token_depends_on); in bits the GEMMs of the two schedules may take other
    accumulation orders (their row counts pick the kernel), so ids are held to the measured noise (_flip_bound)."""
    from touchnet_amd.models.kimi_audio.speech_tokenizer import WhisperVQConfig, WhisperVQEncoder
    torch.manual_seed(0)
    m = WhisperVQEncoder(WhisperVQConfig.from_dict({"num_mel_bins": 128, "d_model": 1280, "encoder_attention_heads": 20,
                                                    "encoder_ffn_dim": 5120}))
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn_like(p) * (0.02 if "bias" in n else 1.0 / p.shape[-1] ** 0.5)
                    + (1.0 if "layer_norm.weight" in n else 0.0))
    m = m.to(DEV)
    L = [10, 170, 400, 799, 1601, 2400, 3000]                         # valid mel frames (0.1 s .. 30 s)
    feats = torch.randn(len(L), 128, 3000, device=DEV)
    mask = (torch.arange(3000, device=DEV)[None] < torch.tensor(L, device=DEV)[:, None]).to(torch.int32)
    diff, total, xerr = _trimmed_against_full(m, feats, mask, [-(-x // 8) for x in L])
    print(f"full width trimmed vs full: {diff} of {total} needed ids differ, pooled states {xerr:.2e}")


def _tiny_kimi(tokenizer: bool):
    from touchnet_amd.models.kimi_audio import KimiAudioConfig, KimiAudioPackedForCausalLM
    kw = dict(vocab_size=1024, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
              num_key_value_heads=1, head_dim=64, kimia_mimo_layers=1, kimia_mimo_transformer_from_layer_index=0,
              kimia_token_offset=512, kimia_media_begin=5, kimia_media_end=6, use_whisper_feature=True,
              kimia_adaptor_input_dim=512,
              speech_encoder_config=dict(num_mel_bins=16, d_model=128, encoder_layers=1, encoder_attention_heads=2,
                                         encoder_ffn_dim=128, max_source_positions=160))
    if tokenizer:
        kw["speech_tokenizer_config"] = dict(num_mel_bins=16, d_model=128, encoder_attention_heads=2, encoder_ffn_dim=128,
                                             max_source_positions=160, pooling_position=2, quantize_position=2,
                                             quantize_vocab_size=64, quantize_causal_block_size=50)
    torch.manual_seed(0)
    m = KimiAudioPackedForCausalLM(KimiAudioConfig(**kw))
    m.post_init()
    return m.to(DEV).to(torch.bfloat16)


def _tiny_batch(n_audio=(20, 9)):
    T = 128
    a = torch.full((1, T), 7, dtype=torch.int64)
    t = torch.randint(10, 500, (1, T))
    col = 0
    for na in n_audio:
        a[0, col], a[0, col + na + 1] = 5, 6
        col += na + 2 + 10
    labels = torch.randint(10, 500, (1, T))
    labels[0, :60] = -100
    L = [8 * na for na in n_audio]
    mask = (torch.arange(320)[None] < torch.tensor(L)[:, None]).to(torch.int32)
    return {"audio_input_ids": a.to(DEV), "text_input_ids": t.to(DEV), "labels": labels.to(DEV),
            "attention_mask": torch.ones(1, T, dtype=torch.int64, device=DEV),
            "position_ids": torch.arange(T, device=DEV)[None], "sentence_lens": torch.full((1, T), 68, device=DEV),
            "num_sentence": 1, "whisper_input_features": torch.randn(len(n_audio), 16, 320, device=DEV),
            "whisper_attention_mask": mask.to(DEV), "clip_tokens": list(n_audio)}


def test_model_computes_its_own_ids():
    m = _tiny_kimi(True)
    batch = _tiny_batch()
    with torch.no_grad():
        ids = m.speech_tokenizer(batch["whisper_input_features"], batch["whisper_attention_mask"],
                                 clip_tokens=batch["clip_tokens"])
    runs = []
    for given in (None, ids):
        m.zero_grad(set_to_none=True)
        out = m(**batch, speech_tokenizer_ids=given)
        out.loss.backward()
        runs.append((out.loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys() and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    assert not any(k.startswith("speech_tokenizer.") for k in runs[0][1])
    assert all(p.grad is None and not p.requires_grad for p in m.speech_tokenizer.parameters())
    from touchnet_amd.utils.optimizer import FusedAdamW
    opt = FusedAdamW(m.named_parameters())
    assert not any(n.startswith("speech_tokenizer.") for n in opt.names)
    # no host synchronisation in the tokenizer the forward runs (torch raises on a synchronising call in this mode)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.speech_tokenizer(batch["whisper_input_features"], batch["whisper_attention_mask"], clip_tokens=batch["clip_tokens"])
        m.speech_tokenizer(batch["whisper_input_features"], batch["whisper_attention_mask"])
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_model_without_tokenizer_still_needs_ids():
    m = _tiny_kimi(False)
    assert m.speech_tokenizer is None
    with pytest.raises(ValueError, match="speech_tokenizer_ids"):
        m(**_tiny_batch())
