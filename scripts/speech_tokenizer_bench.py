"""Kimi-Audio speech tokenizer (WhisperVQEncoder at Kimi-Audio-7B's widths, random bf16 weights) at the
`kimi_audio_7b_speech` bench workload's clips (bench.py: synthetic.kimi_audio_plan, B = 1 x T = 8192, seed 0):

  tokenizer ms per batch, full length (every clip on 1500 frames) against trimmed (`clip_tokens`)
  tn_vq_nearest us and TFLOP/s against torch.addmm + min on the same operands (clips x 375 rows, V 16384, d 1280)
  tn_attn_block_causal_fwd TFLOP/s on the full-length and the packed trimmed layout (allowed pairs only)

    python scripts/speech_tokenizer_bench.py
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    import touchnet_amd.functional as F
    from touchnet_amd.data import synthetic
    from touchnet_amd.models.kimi_audio.speech_tokenizer import WhisperVQConfig, WhisperVQEncoder, needed_frames, packed_layout
    dev = torch.device("cuda", 0)
    tok = synthetic.kimi_audio_plan(152064, 152064, 16384, 1, 8192, 0, media_markers=(151661, 151663))
    K = [max(int(k), 1) for k in tok["clip_tokens"]]             # bench.py: clip i holds K_i * 1280 samples = 8 K_i frames
    n = len(K)
    torch.manual_seed(0)
    m = WhisperVQEncoder(WhisperVQConfig.from_dict({"num_mel_bins": 128, "d_model": 1280, "encoder_attention_heads": 20,
                                                    "encoder_ffn_dim": 5120}))
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.randn_like(p) * (0.02 if "bias" in name else 1.0 / p.shape[-1] ** 0.5)
                    + (1.0 if "layer_norm.weight" in name else 0.0))
    m = m.to(dev).to(torch.bfloat16)
    feats = torch.randn(n, 128, 3000, device=dev)
    L = torch.tensor([min(8 * k, 3000) for k in K], device=dev)
    mask = (torch.arange(3000, device=dev)[None] < L[:, None]).to(torch.int32)
    full = timed(lambda: m(feats, mask), reps=5)
    trim = timed(lambda: m(feats, mask, clip_tokens=K), reps=5)
    ids_f, ids_t = m(feats, mask), m(feats, mask, clip_tokens=K)
    same = int(sum(int((ids_f[c, :k] != ids_t[c, :k]).sum()) for c, k in enumerate(K)))
    need = [needed_frames(k, 1500, 200, 4) for k in K]
    out = {"clips": n, "tokens": sum(K), "frames_full": 1500 * n, "frames_trimmed": packed_layout(K, 1500, 200, 4).rows,
           "tokenizer_full_ms": round(full, 3), "tokenizer_trimmed_ms": round(trim, 3),
           "speedup": round(full / trim, 3), "trimmed_ids_differing_from_full": same}
    # ---- VQ at the full-length row count
    M, V, d = n * 375, 16384, 1280
    x = torch.randn(M, d, device=dev).bfloat16()
    cb = m.codebook.weight
    cn = F.codebook_sqnorm(cb)
    t_vq = timed(lambda: F.vq_nearest(x, cb, cn))
    xs = (x.float() ** 2).sum(1, keepdim=True).bfloat16()

    def ref():
        return torch.addmm(cn.bfloat16()[None] + xs, x, cb.t(), alpha=-2.0, beta=1.0).min(1)
    t_ref = timed(ref)
    xf, cf = x.float(), cb.float()
    t_ref32 = timed(lambda: torch.addmm(cn[None] + (xf ** 2).sum(1, keepdim=True), xf, cf.t(), alpha=-2.0, beta=1.0).min(1),
                    reps=3)
    fl = 2.0 * M * V * d
    out.update({"vq_rows": M, "vq_us": round(1e3 * t_vq, 1), "vq_tflops": round(fl / t_vq / 1e9, 1),
                "addmm_min_bf16_us": round(1e3 * t_ref, 1), "addmm_min_bf16_tflops": round(fl / t_ref / 1e9, 1),
                "addmm_min_fp32_us": round(1e3 * t_ref32, 1),
                "vq_peak_fraction_of_2500_tflops": round(fl / t_vq / 1e9 / 2500, 3)})
    # ---- attention: full-length layout and the packed trimmed layout, useful FLOPs = 4 D x allowed pairs x heads
    Nh, D, block = 20, 64, 200
    for tag, segs in (("full", [(1500, min(4 * k, 1500)) for k in K]), ("trimmed", [(f, min(4 * k, f)) for k, f in zip(K, need)])):
        R = sum(f for f, _ in segs)
        start, end, pairs, off = [], [], 0, 0
        for f, Lk in segs:
            start += [off] * f
            end += [off + Lk] * f
            for i in range(f):
                pairs += min(Lk, (i // block + 1) * block)
            off += f
        q, k_, v = (torch.randn(1, R, Nh, D, device=dev).bfloat16() for _ in range(3))
        mk = F.block_causal_mask(torch.tensor([start], dtype=torch.int32, device=dev),
                                 torch.tensor([end], dtype=torch.int32, device=dev), block)
        t = timed(lambda: F.block_causal_attention(q, k_, v, mk))
        out[f"attn_{tag}_us"] = round(1e3 * t, 1)
        out[f"attn_{tag}_tflops"] = round(4.0 * D * pairs * Nh / t / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
