"""Writes tests/golden/speech_tokenizer.npz by RUNNING the reference's WhisperVQEncoder
(touchnet/models/kimi_audio/modeling_kimi_audio.py:140-319) at a tiny width on CPU.  Build container only (it needs the
reference checkout and transformers), like make_golden.py:

    python tests/golden/make_golden_speech_tokenizer.py

Under transformers 5.x a WhisperEncoderLayer returns the hidden-state tensor and takes no `layer_head_mask`; each layer is
wrapped to return the old 1-tuple and drop that keyword (its arithmetic is untouched, like adapt_decoder_layers_to_4_51).
The codebook is drawn near the clips' own pooled states so that most ids win by a clear margin."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

CFG = dict(num_mel_bins=16, d_model=128, encoder_attention_heads=2, encoder_ffn_dim=128, max_source_positions=150,
           pooling_kernel_size=4, pooling_type="avg", pooling_position=2, quantize_position=2, quantize_vocab_size=64,
           quantize_causal_block_size=50, quantize_ema_decay=0.99, encoder_layers=2, decoder_layers=1)
TM, LENS = 300, (300, 171, 9)


def bf16(t):
    return t.to(torch.bfloat16).float()


def main():
    _ref_import.install()
    mk = _ref_import.load_kimi_modeling()
    from touchnet.models.kimi_audio.configuration_kimi_audio import WhisperVQConfig
    torch.manual_seed(0)
    cfg = WhisperVQConfig(**CFG)
    cfg._attn_implementation = "eager"
    enc = mk.WhisperVQEncoder(cfg).eval()
    for layer in enc.layers:
        inner = layer.forward

        def forward(h, mask, *a, _inner=inner, layer_head_mask=None, **kw):
            return (_inner(h, mask, *a, **kw),)
        layer.forward = forward
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if name.endswith("bias"):
                p.copy_(bf16(torch.randn_like(p) * 0.02))
            elif "layer_norm" in name:
                p.copy_(bf16(1.0 + torch.randn_like(p) * 0.05))
            else:
                p.copy_(bf16(torch.randn_like(p) * (0.5 if "embed_positions" in name else 1.0) / p.shape[-1] ** 0.5))
    feats = bf16(torch.randn(len(LENS), CFG["num_mel_bins"], TM))
    mask = torch.zeros(len(LENS), TM, dtype=torch.int64)
    for i, L in enumerate(LENS):
        mask[i, :L] = 1
    hid = {}
    h = enc.layers[-1].register_forward_hook(lambda m, i, o: hid.__setitem__("h", o[0].detach().clone()))
    with torch.no_grad():
        enc(feats, mask)                        # first pass: the pooled states the codebook is drawn around
    h.remove()
    pre = hid["h"]                              # [n, 150, d] = the input of the pooling
    p = CFG["pooling_kernel_size"]
    T = pre.shape[1]
    pooled = torch.nn.functional.pad(pre.transpose(1, 2), (0, (-T) % p)).transpose(1, 2)
    pooled = pooled.reshape(len(LENS), -1, p, pre.shape[2]).mean(2).reshape(-1, pre.shape[2])
    g = torch.Generator().manual_seed(1)
    pick = torch.randperm(pooled.shape[0], generator=g)[:CFG["quantize_vocab_size"]]
    with torch.no_grad():
        enc.codebook.weight.copy_(bf16(pooled[pick] + 0.05 * pooled.std() * torch.randn(len(pick), pre.shape[2], generator=g)))
    hid.clear()
    h = enc.layers[-1].register_forward_hook(lambda m, i, o: hid.__setitem__("h", o[0].detach().clone()))
    with torch.no_grad():
        ids = enc(feats, mask)
    h.remove()
    pre = hid["h"]
    pooled = torch.nn.functional.pad(pre.transpose(1, 2), (0, (-T) % p)).transpose(1, 2)
    pooled = pooled.reshape(len(LENS), -1, p, pre.shape[2]).mean(2).reshape(-1, pre.shape[2]).double()
    cb = enc.codebook.weight.double()
    dist = (cb ** 2).sum(1)[None] - 2 * pooled @ cb.t()
    top2 = dist.topk(2, dim=1, largest=False).values
    margin = (top2[:, 1] - top2[:, 0]).float().view(len(LENS), -1)
    sd = enc.state_dict()
    out = {"config_json": np.array(str(CFG)), "features": feats.numpy(), "mask": mask.numpy(),
           "ids": ids.numpy(), "hidden": pre.to(torch.bfloat16).view(torch.int16).numpy(), "margin": margin.numpy(),
           "keys": np.array(sorted(sd))}
    for k, v in sd.items():
        if k.startswith("ema_"):                 # (training state of the reference's EMA codebook: never read here)
            continue
        out["param/" + k] = bf16(v.float()).to(torch.bfloat16).view(torch.int16).numpy()
    path = os.path.join(HERE, "speech_tokenizer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; ids", ids.tolist()[2][:4], "min margin", float(margin.min()))


if __name__ == "__main__":
    main()
