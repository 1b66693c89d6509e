"""tn_sample_step and the sampled mode of tn_kimi_text_step on the MI355X at their edges: the planted rows of
tests/sampling_reference.py, each one launch, compared exactly — token, history, lengths, finished flags, the unfinished
count and n_kept — with no boundary allowance.  test_sampling_reference_cpu.py has shown that every top_p and every
uniform of these cases keeps 5e-5 (Kimi: 1e-3) from the restatement's nearest decision boundary; which branch of the
kernels each case reaches is in its `reach` string and worked out in the case builder's comments.

n_kept equals the restatement's count whenever the threshold lies less than 1023/16 below the maximum; when the k-th
largest value lies farther down, the kernel keeps the whole last level-0 bin ("can be kept but are never drawn"):
restatement's count <= n_kept <= V, and the token is still exact."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_reference as SR  # noqa: E402
from test_kimi_generation_gpu import _assert_same, _run_both  # noqa: E402
from test_kimi_generation_gpu import _state as _kimi_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.bfloat16]


def _names(builder):
    return [(dt, c["name"]) for dt in DTYPES for c in builder(dt)]


def _ids(builder):
    return [f"{'fp32' if dt == torch.float32 else 'bf16'}-{n}" for dt, n in _names(builder)]


def _case(builder, dtype, name):
    return next(c for c in builder(dtype) if c["name"] == name)


@pytest.mark.parametrize("dtype,name", _names(SR.edge_cases), ids=_ids(SR.edge_cases))
def test_sample_step_at_its_edges(dtype, name):
    import touchnet_amd.functional as F
    c = _case(SR.edge_cases, dtype, name)
    B, V = c["logits"].shape
    st = {n: t.clone().to(DEV) for n, t in c["state"].items()}
    if "forbid" in c:
        # the -inf logits as constrain_logits_ writes them
        from touchnet_amd.generation import ConstraintPlan
        logits = c["pre_logits"].to(DEV)
        F.constrain_logits_(logits, st["hist"], st["hl"], ConstraintPlan.build(c["forbid"], 0, [], V, DEV))
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(logits.cpu().view(bits), c["logits"].view(bits))
    else:
        logits = c["logits"].to(DEV)
    kept = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    F.sample_step(logits, st["hist"], st["hl"], st["cl"], st["fin"], st["nu"], c["penalty"], c["do_sample"], c["T"],
                  c["top_k"], c["top_p"], 0, c["eos"], c["pad"],
                  uniforms=torch.tensor(c["uniforms"], dtype=torch.float32, device=DEV), n_kept=kept)
    torch.cuda.synchronize()
    got = {n: t.cpu() for n, t in st.items()}
    kept = kept.cpu().tolist()
    S = c["S_hist"]
    pos = [min(max(int(n), 0), S) for n in c["state"]["hl"].tolist()]
    toks = [int(got["hist"][b, pos[b]]) if pos[b] < S else None for b in range(B)]
    print(f"{name}: tokens {toks} (want {[r['token'] for r in c['rows']]}), n_kept {kept} "
          f"(restatement {[r['n_kept'] for r in c['rows']]}); reaches: {c['reach']}")
    for n in ("hist", "hl", "cl", "fin", "nu"):
        assert torch.equal(got[n], c["want"][n]), (name, n, got[n], c["want"][n])
    for b, r in enumerate(c["rows"]):
        if r.get("exact_count", True):
            assert kept[b] == r["n_kept"], (name, b, kept[b], r["n_kept"])
        else:
            assert r["n_kept"] <= kept[b] <= V, (name, b, kept[b], r["n_kept"])


def test_vocabulary_beyond_the_bitmap_is_refused():
    from touchnet_amd import _C
    import touchnet_amd.functional as F
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    with pytest.raises(_C.KernelError, match="-22"):
        F.sample_step(torch.zeros(1, 262145, device=DEV), i32(1, 8), i32(1), i32(1), i32(1), i32(1), top_k=5)


@pytest.mark.parametrize("dtype,name", _names(SR.kimi_edge_cases), ids=_ids(SR.kimi_edge_cases))
def test_kimi_sampled_mode_at_its_edges(dtype, name):
    c = _case(SR.kimi_edge_cases, dtype, name)
    B, V = c["logits"].shape
    H = 64
    embed = (torch.randn(V, H, generator=torch.Generator().manual_seed(V)) * 0.5).to(torch.bfloat16)
    d, r, toks = _run_both(c["logits"], _kimi_state(c["hists"], c["prompts"]), embed, c["penalty"], c["window"], c["T"],
                           c["top_k"], V - 1, V - 2, uniforms=torch.tensor(c["uniforms"], dtype=torch.float32))
    print(f"{name}: tokens {toks.tolist()}; reaches: {c['reach']}")
    _assert_same(d, r, (name, dtype))
