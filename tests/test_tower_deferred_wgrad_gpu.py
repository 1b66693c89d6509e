"""The audio tower with its weight gradients deferred (functional.DeferredWgrad + tn_gemm_bf16_grouped_table) against the
per-layer path: a 3-layer tower at reduced width (d_model 256, ffn 1024, 4 heads), forward and backward.  The hand-written
GEMM is made to take these few-tile products in every arm (`_OWN_MIN_TILES`), so that the arms differ in nothing but how
the weight gradients are launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


# 2 clips x 200 frames = 400 tokens: 7 stages, `split_k` leaves the per-layer products whole; 2 x 600 = 1200 tokens:
# 19 stages, the per-layer path cuts them in two
@pytest.mark.parametrize("frames", [200, 600])
def test_deferred_tower_weight_gradients_equal_the_unsplit_per_layer_path(frames, monkeypatch):
    import touchnet_amd.functional as F
    from touchnet_amd.models.qwen2_audio import AudioEncoderConfig
    from touchnet_amd.models.qwen2_audio.modeling_qwen2_audio import Qwen2AudioEncoder
    monkeypatch.setattr(F, "_OWN_MIN_TILES", 1)
    torch.manual_seed(7)
    cfg = AudioEncoderConfig(num_mel_bins=16, d_model=256, encoder_layers=3, encoder_attention_heads=4, encoder_ffn_dim=1024,
                             max_source_positions=frames)
    tower = Qwen2AudioEncoder(cfg).to(DEV).to(torch.bfloat16)
    clips = 2
    h = (torch.randn(clips, frames, cfg.d_model) * 0.5).to(torch.bfloat16).to(DEV).requires_grad_()
    dout = torch.randn(clips, frames // 2, cfg.d_model).to(DEV)
    mask = F.causal_mask(clips, frames, DEV)
    layers = tower.deferred_wgrad_layers()

    def run(queue=None):
        h.grad = None
        for p in tower.parameters():
            p.grad = None
        loss = (tower.encode(h, mask).float() * dout).sum()
        loss.backward()
        if queue is not None:
            assert len(queue) > 0
            queue.flush()
            assert len(queue) == 0                                   # empty after the flush
        grads = {n: p.grad.clone() for n, p in tower.named_parameters() if p.grad is not None}
        return loss.detach().clone(), h.grad.clone(), grads

    q3 = F.DeferredWgrad(layers, flush_layers=3)
    deferred = run(q3)
    assert q3.flushes == 1
    q3.close()
    q1 = F.DeferredWgrad(layers, flush_layers=1)                     # a flush per layer: the same bits
    per_layer_flush = run(q1)
    assert q1.flushes == 3
    monkeypatch.setattr(F, "DEFERRED_WGRAD", False)                  # the switch: the queue is still registered
    default = run()                                                  # per layer, split-K where `split_k` says so
    assert len(q1) == 0
    # per layer, every weight gradient as the unsplit launch.  (Not through the global flag F.SPLIT_K: at
    # this width it would also change forward and input-gradient products of 1024-deep contractions, which `split_k` cuts
    # in two once `_OWN_MIN_TILES` lets the hand-written kernel take them — the loss would no longer be comparable.)
    split_k = F.split_k
    monkeypatch.setattr(F, "split_k", lambda M, N, K, a_kmaj, b_kmaj: 1 if (a_kmaj and b_kmaj) else split_k(M, N, K, a_kmaj, b_kmaj))
    unsplit = run()
    q1.close()

    names = sorted(deferred[2])
    assert len(names) == 3 * (6 + 5 + 4) + 2, names                  # 6 weights, 5 biases, 2 LayerNorms per layer + the last norm
    for arm, other in (("a flush per layer", per_layer_flush), ("default", default), ("unsplit", unsplit)):
        assert sorted(other[2]) == names, arm
        assert torch.equal(other[0], deferred[0]), (arm, "loss", float(other[0]), float(deferred[0]))
        assert torch.equal(other[1], deferred[1]), (arm, "input gradient")
    for n in names:
        assert torch.equal(deferred[2][n], unsplit[2][n]), n
        assert torch.equal(deferred[2][n], per_layer_flush[2][n]), n
        # against the default (split-K) arm: the bound of the tower fixture test (tests/test_reference_fixtures_gpu.py)
        a, b = deferred[2][n].double(), default[2][n].double()
        err = float((a - b).abs().max()) / float(b.abs().max())
        assert err < 2e-2, (n, err)
