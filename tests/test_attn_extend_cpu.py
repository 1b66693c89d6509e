"""tn_attn_extend's Python surface without a device: the fake kernel, refusals by name, generate(past=) under beams."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode


def _operands(T=5, Nh=4, Nkv=2, D=64, B=2, S=8, device="cpu"):
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=device)
    return [bf(T, Nh, D), bf(T, Nkv, D), bf(T, Nkv, D), bf(B, S, Nkv, D), bf(B, S, Nkv, D)]


def test_fake_kernel_returns_the_output_shape_and_dtype():
    import touchnet_amd.library  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
        o = torch.ops.mi355_touch.attn_extend(*_operands(device="cuda"), i32(3), i32(2), None, 0.125)
        assert tuple(o.shape) == (5, 4, 64) and o.dtype == torch.bfloat16 and o.device.type == "cuda"


@pytest.mark.parametrize("kw,start,pre,row,needle", [
    ({}, [0, 3, 2, 5], [0, 0, 0], [0, 1, 0], "ascending"),
    ({}, [0, 3, 4], [0, 0], None, "seq_start[-1]"),
    ({}, [0, 1, 2, 5], [0, 0, 0], None, "need kv_row"),
    ({"D": 96}, [0, 5], [0], None, "64 or 128"),
    ({"Nh": 5}, [0, 5], [0], None, "multiple of Nkv"),
    ({"Nh": 34}, [0, 5], [0], None, "exceeds 16"),
])
def test_functional_refuses_by_name(kw, start, pre, row, needle):
    import touchnet_amd.functional as F
    with pytest.raises(ValueError, match=needle.replace("[", r"\[").replace("]", r"\]")):
        F.attn_extend(*_operands(**kw), start, pre, 0.125, row)


def test_generate_refuses_a_past_cache_under_beam_search():
    from touchnet_amd import generation as G
    with pytest.raises(ValueError, match="past= with num_beams = 2"):
        G.generate(None, G.Prompts([torch.tensor([1])]), G.GenerationConfig(num_beams=2), past=object())
