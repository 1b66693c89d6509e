"""tests/golden/kimi_generate.npz: MoonshotKimiaForCausalLM.generate (touchnet/models/kimi_audio/modeling_kimi_audio.py:
1084-1214) RUN from the reference's source — its own KimiASampler.sample_text_logits / sample_audio_logits and its own
_generate_loop — on the CPU in float32, on a tiny model with bf16-representable weights.  Build container only (it imports
the reference through tests/golden/_ref_import.py); the tests read the .npz alone.

    python tests/golden/make_golden_kimi_generate.py

Model: `self.model` is the REAL MoonshotKimiaModel with its DynamicCache pair (the 4.51 -> 5.x keyword drift of the decoder
layers is bridged by _ref_import.adapt_decoder_layers_to_4_51, as for kimi_decoder_dev.npz; no prefix-recomputing adapter
was needed.  One more drift shows with a cache: the reference's `_update_causal_mask` builds the mask one column wider than
the keys, which 4.51's eager attention cut to the keys' length (`attention_mask[:, :, :, :key_states.shape[-2]]`) and 5.x's
does not; the same cut is applied to what `_update_causal_mask` returns — the columns cut lie beyond every key), use_whisper_feature=False, H 128, 3 + 1 layers, 2 / 1 heads (D 64), I 64, V 320, kimia_token_offset 280.
generate() and _generate_loop are called unbound on a stand-in `self` that carries exactly the attributes they read (the
full class would also build the speech encoder and tokenizer, which generate() does not touch without whisper features).
KimiASampler hard-codes the ids of <|im_kimia_text_blank|> / <|im_kimia_text_eos|> (151666 / 151667); a subclass remaps them
into the tiny vocabulary (301 / 307, the stand-in tokenizer's ids of make_golden.py) and records what the loop hands it.
Recorded per step: the text logits, the penalised logits the sampler feeds to log_softmax (their two largest values give
the margin), and — through the loop's own `text_previous_tokens` buffer (the storage behind the `recent_tokens` view it passes) — the raw token of every row.

Cases: batch 1 and batch 2 (equal-length prompts), window 16 and 4, max_new_tokens 40, greedy (generate()'s defaults:
temperature 0, penalty 1.1).  The model seed and the prompts' seeds are searched so that in every batch-2 case one row
reaches eos before the budget and one does not, and so that few steps have a small margin.

Second block: the two prompt id streams the reference's inference script builds (inference_kimi_audio.py:102-120) for the
stand-in tokenizer, for three audio-token counts.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import as R  # noqa: E402

R.install()

V, H, OFFSET, BLANK, EOS = 320, 128, 280, 301, 307
MAX_NEW = 40
KW = dict(vocab_size=V, hidden_size=H, intermediate_size=64, num_hidden_layers=3, num_attention_heads=2,
          num_key_value_heads=1, rms_norm_eps=1e-6, rope_theta=1e6, kimia_mimo_layers=1,
          kimia_mimo_transformer_from_layer_index=1, kimia_token_offset=OFFSET, use_whisper_feature=False, use_cache=True,
          pad_token_id=None, initializer_range=0.1)


def _bits(t):
    return t.detach().to(torch.bfloat16).view(torch.int16).numpy().copy()


def _bf16_round_(m):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())


class KimiTokenizer:
    """make_golden.py::_KimiTokenizer with the call surface of the inference script (`tokenizer(text,
    add_special_tokens=False).input_ids`, `.pad_token_id`)."""
    SPECIAL = {"<|im_kimia_user_msg_start|>": 300, "<|im_kimia_text_blank|>": 301, "<|im_media_begin|>": 302,
               "<|im_media_end|>": 303, "<|im_kimia_speech_ct_id|>": 304, "<|im_msg_end|>": 305,
               "<|im_kimia_assistant_msg_start|>": 306, "<|im_kimia_text_eos|>": 307}
    pad_token_id = 0

    def __call__(self, text, add_special_tokens=False):
        ids, i = [], 0
        while i < len(text):
            for sp, v in self.SPECIAL.items():
                if text.startswith(sp, i):
                    ids.append(v)
                    i += len(sp)
                    break
            else:
                ids.append(10 + ord(text[i]) % 200)
                i += 1
        return types.SimpleNamespace(input_ids=ids)


def successor_head(E, g):
    """A text head that makes the random decoder speak in a recognisable way instead of emitting one token for ever (which
    is what a Gaussian head does, and which would leave the windowed penalty and eos untested): row j is a little noise
    plus E[t] for the token t whose successor j is, so a step whose input carries E[t] scores s1(t) far above the rest —
    clear margins.  The ordinary tokens form short cycles (the walk repeats itself, so the penalty meets its own window);
    every token has a second successor in another cycle at 0.5 of the weight, every sixth at 0.93: there the penalty of
    1.1 hands the lead over (1 / 1.1 < 0.93).  A few tokens lead to eos, a few to ids above the token offset."""
    W = torch.randn(V, H, generator=g) * 0.02
    ordinary = torch.arange(10, OFFSET)[torch.randperm(OFFSET - 10, generator=g)].tolist()
    s1, s2, i = {}, {}, 0
    while i < len(ordinary):
        n = min(int(torch.randint(3, 7, (1,), generator=g)), len(ordinary) - i)
        cyc = ordinary[i:i + n]
        for a, b in zip(cyc, cyc[1:] + cyc[:1]):
            s1[a] = b
        i += n
    for k, t in enumerate(ordinary):
        s2[t] = ordinary[(k + 37) % len(ordinary)]
    for t in ordinary[::23]:
        s1[t] = EOS
    for k, t in enumerate(ordinary[5::31]):
        s1[t] = OFFSET + 1 + k                     # an id the returned text drops ...
        s1[OFFSET + 1 + k] = ordinary[(5 + 31 * k + 1) % len(ordinary)]      # ... which leads back
    for k, t in enumerate(ordinary):
        W[s2[t]] += (0.93 if k % 6 == 0 else 0.5) * E[t]
    for t, j in s1.items():
        W[j] += E[t]
    return W


def build(mk, seed):
    from touchnet.models.kimi_audio.configuration_kimi_audio import KimiAudioConfig
    cfg = KimiAudioConfig(**KW)
    cfg._attn_implementation = "eager"
    cfg.layer_types = ["full_attention"] * (KW["num_hidden_layers"] + KW["kimia_mimo_layers"])
    torch.manual_seed(seed)
    model = mk.MoonshotKimiaModel(cfg).float().eval()
    R.adapt_decoder_layers_to_4_51(list(model.layers) + list(model.mimo_layers))
    build_mask = model._update_causal_mask

    def mask_as_4_51(attention_mask, input_tensor, cache_position, past_key_values, output_attentions=False):
        m = build_mask(attention_mask, input_tensor, cache_position, past_key_values, output_attentions)
        return m if m is None else m[..., :int(cache_position[-1]) + 1]
    model._update_causal_mask = mask_as_4_51
    lm_head = torch.nn.Linear(H, V, bias=False)
    mimo_output = torch.nn.Linear(H, V, bias=False)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(std=0.05, generator=g)
        mimo_output.weight.normal_(std=0.1, generator=g)
        for layer in model.layers:                 # the layers colour the residual stream, the input token still leads it
            layer.self_attn.o_proj.weight.mul_(0.05)
            layer.mlp.down_proj.weight.mul_(0.05)
        lm_head.weight.copy_(successor_head(model.embed_tokens.weight, g))
    for m in (model, lm_head, mimo_output):
        _bf16_round_(m)
    fake = types.SimpleNamespace(model=model, lm_head=lm_head, mimo_output=mimo_output, config=cfg,
                                 use_whisper_feature=False, get_input_embeddings=lambda: model.embed_tokens)
    fake._generate_loop = lambda **kw: mk.MoonshotKimiaForCausalLM._generate_loop(fake, **kw)
    return fake


def run(mk, fake, text_ids, audio_ids, window):
    """-> what generate() returned and what its sampler saw"""
    rec = dict(logits=[], penalised=[], buffer=None)
    base = mk.KimiASampler

    class Recording(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.kimia_text_blank, self.kimia_text_eos = BLANK, EOS

        def sample_text_logits(self, logits, recent_tokens=None):
            rec["logits"].append(logits[:, -1].clone() if logits.dim() == 3 else logits.clone())
            if recent_tokens is not None and rec["buffer"] is None:
                rec["buffer"] = recent_tokens                        # a view of the loop's text_previous_tokens
            inner = torch.log_softmax

            def spy(x, *a, **kw):
                rec["penalised"].append(x.clone())
                return inner(x, *a, **kw)
            torch.log_softmax = spy
            try:
                return super().sample_text_logits(logits, recent_tokens=recent_tokens)
            finally:
                torch.log_softmax = inner
    mk.KimiASampler = Recording
    try:
        wav, text = mk.MoonshotKimiaForCausalLM.generate(fake, text_input_ids=text_ids, audio_input_ids=audio_ids,
                                                        text_repetition_window_size=window, max_new_tokens=MAX_NEW)
    finally:
        mk.KimiASampler = base
    assert all(len(w) == 0 for w in wav)
    steps = len(rec["logits"])
    if rec["buffer"] is None:                                        # every row finished at the first step: not a case
        return None
    view = rec["buffer"]                                             # [B, 1] of the [B, max_new] buffer, same storage
    full = torch.as_strided(view, (view.shape[0], MAX_NEW), (view.stride(0), 1), view.storage_offset())
    raw = full[:, :steps].clone().long()
    pen = torch.stack(rec["penalised"])                              # [steps, B, V]
    top2 = pen.topk(2, dim=-1).values
    return dict(returned=text, raw=raw, logits=torch.stack(rec["logits"]), margin=top2[..., 0] - top2[..., 1], steps=steps)


def prompts(seed, B, n):
    """Two aligned streams of the S2T shape: instruction ids in the text stream, blanks in the audio stream around a
    marker pair; the text stream ends in an ordinary id of the row's own, where the row's walk starts."""
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(10, 210, (B, n), generator=g)
    audio = torch.full((B, n), BLANK)
    audio[:, 4], audio[:, n - 5] = 302, 303
    audio[:, n - 4:n - 1] = torch.tensor([304, 305, 306])
    text[:, 0] = 300
    text[:, 5:n - 1] = BLANK
    return text, audio


SMALL = 0.04       # of the logits' scale: twice the 2 % the device's logits are off on kimi_decoder_dev.npz (the test that
#                    reads this fixture calls a step a near-tie when its margin is under twice the observed difference)


def quality(out):
    """(rows that hit eos, rows that did not, live steps with a margin under SMALL of the logits' scale, live steps at
    which the penalty changed the argmax, mask of the live steps)"""
    raw = out["raw"]
    hit = (raw == EOS).any(1)
    live = torch.ones_like(raw, dtype=torch.bool)
    for b in range(raw.shape[0]):
        e = (raw[b] == EOS).nonzero().reshape(-1)
        if e.numel():
            live[b, int(e[0]) + 1:] = False
    scale = float(out["logits"].abs().max())
    small = (out["margin"].t() < SMALL * scale) & live
    flips = (out["logits"].argmax(-1).t() != raw) & live
    return int(hit.sum()), int((~hit).sum()), int(small.sum()), int(flips.sum()), live


def main():
    mk = R.load_kimi_modeling()
    cases = [("b1_w16", 1, 16), ("b1_w4", 1, 4), ("b2_w16", 2, 16), ("b2_w4", 2, 4)]
    best = None
    for mseed in range(40, 60):
        fake = build(mk, mseed)
        chosen, ok = {}, True
        for name, B, W in cases:
            found = None
            for pseed in range(100, 160):
                t, a = prompts(pseed, B, 24)
                out = run(mk, fake, t, a, W)
                if out is None:
                    continue
                n_hit, n_not, small, flips, live = quality(out)
                rows_ok = (n_hit >= 1 and n_not >= 1) if B == 2 else (n_hit == (1 if W == 4 else 0))
                # at most 2.5 % of the live steps with a small margin, the penalty deciding at least one step, and a
                # finished row that goes on stepping for a while
                if (rows_ok and 40 * small <= int(live.sum()) and (flips >= 1 or W == 4)
                        and int(live.sum()) >= W + 4 + (MAX_NEW if B == 2 else 0)):
                    found = (pseed, out, t, a, live)
                    break
            if found is None:
                print("model seed", mseed, "no prompts for", name)
                ok = False
                break
            chosen[name] = found
        if ok:
            best = (mseed, fake, chosen)
            break
    assert best is not None, "no seed found"
    mseed, fake, chosen = best
    arrs = {f"param/model.{n}": _bits(p) for n, p in fake.model.named_parameters() if "mimo" not in n}
    arrs["param/lm_head.weight"] = _bits(fake.lm_head.weight)
    arrs["config_json"] = np.array(str({k: v for k, v in KW.items() if k not in ("use_whisper_feature", "use_cache",
                                                                                 "pad_token_id", "initializer_range")}))
    arrs["special"] = np.array([BLANK, EOS, OFFSET, MAX_NEW])
    arrs["model_seed"] = np.array(mseed)
    arrs["model_kind"] = np.array("MoonshotKimiaModel with its DynamicCache pair (no prefix-recomputing adapter)")
    arrs["cases"] = np.array([c[0] for c in cases])
    for name, B, W in cases:
        pseed, out, t, a, live = chosen[name]
        arrs[f"{name}/window"] = np.array(W)
        arrs[f"{name}/prompt_seed"] = np.array(pseed)
        arrs[f"{name}/text_ids"], arrs[f"{name}/audio_ids"] = t.numpy(), a.numpy()
        arrs[f"{name}/raw"] = out["raw"].numpy().astype(np.int32)                       # [B, steps]
        arrs[f"{name}/logits"] = out["logits"].numpy().astype(np.float32)               # [steps, B, V]
        arrs[f"{name}/margin"] = out["margin"].numpy().astype(np.float32)               # [steps, B]
        arrs[f"{name}/live"] = live.numpy()                                             # [B, steps]: up to and with eos
        for b, r in enumerate(out["returned"]):
            arrs[f"{name}/returned{b}"] = np.array(r, dtype=np.int32)
        print(name, "quality (eos rows, other rows, small margins, penalty flips)", quality(out)[:4])
        print(name, "prompt seed", pseed, "steps", out["steps"], "eos rows", int((out["raw"] == EOS).any(1).sum()),
              "min live margin", float(out["margin"].t()[live].min()), "returned", [len(r) for r in out["returned"]])
    # the inference script's prompt construction: its own statements (from `text_prompts = []` up to the padding, :102-111)
    # are executed here, with the stand-in tokenizer, on the template constants of processing_kimi_audio.py
    ns = {}
    for line in open(f"{R.REF}/touchnet/models/kimi_audio/processing_kimi_audio.py").read().splitlines():
        if line.startswith("KIMI_TEXT_TEMPLATE_FOR_S2T") or line.startswith("KIMI_AUDIO_TEMPLATE_FOR_S2T"):
            exec(line, ns)
    script = open(f"{R.REF}/touchnet/models/kimi_audio/inference_kimi_audio.py").read().splitlines()
    first = next(i for i, l in enumerate(script) if l.strip() == "text_prompts = []")
    last = next(i for i, l in enumerate(script) if l.strip().startswith("text_prompt_ids = "))
    import textwrap
    block = textwrap.dedent("\n".join(script[first:last]))
    tok, instruct = KimiTokenizer(), "Generate the transcription:"
    counts = [1, 13, 375]
    ns.update(tokenizer=tok, args=types.SimpleNamespace(instruct=instruct), num_audio_tokens_list=counts)
    exec(block, ns)
    for n, tp, ap in zip(counts, ns["text_prompts"], ns["audio_prompts"]):
        arrs[f"prompt/{n}/text"] = np.array(tok(tp, add_special_tokens=False).input_ids, dtype=np.int64)
        arrs[f"prompt/{n}/audio"] = np.array(tok(ap, add_special_tokens=False).input_ids, dtype=np.int64)
    arrs["prompt/counts"], arrs["prompt/instruct"] = np.array(counts), np.array(instruct)
    path = os.path.join(HERE, "kimi_generate.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
