"""The small-M decode GEMM without a device: the ops trace, the integer rule, and the routing predicate's two guards."""
import pytest
import torch


def test_ops_trace_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from touchnet_amd import library as L
    with FakeTensorMode():
        x = torch.empty(12, 320, dtype=torch.bfloat16, device="cuda")
        ws = [torch.empty(n, 320, dtype=torch.bfloat16, device="cuda") for n in (256, 64, 64)]
        cos = torch.empty(12, 32, dtype=torch.bfloat16, device="cuda")
        outs = L.linear_smallm(x, ws, [None, ws[1][:, 0], None], cos, cos, 64, 3)
        act = L.swiglu_smallm(x, ws[1], ws[2])
    for y, n in zip([*outs, act], (256, 64, 64, 64)):
        assert tuple(y.shape) == (12, n) and y.dtype == torch.bfloat16 and y.stride() == (n, 1) and y.device.type == "cuda"


@pytest.mark.parametrize("M,Ns,K,ok", [(0, [16], 64, False), (129, [16], 64, False), (16, [16], 96, False),
                                       (16, [24], 64, False), (16, [16] * 4, 64, False), (1, [16], 64, True),
                                       (128, [256, 64, 64], 1088, True)])
def test_smallm_supported_is_the_integer_rule(M, Ns, K, ok):
    from touchnet_amd import functional as F
    assert F.smallm_supported(M, Ns, K) is ok


def test_decode_own_keeps_training_and_prefill_where_they_are(monkeypatch):
    """with the switch on and operands the kernel takes, autograd or a 129th row still send the product the old way"""
    from touchnet_amd import functional as F
    monkeypatch.setattr(F, "DECODE_GEMM", "own")
    monkeypatch.setattr(F, "_bf16_rows", lambda *ts, **kw: True)        # (no device here: the operand check is not the subject)
    w = torch.empty(64, 128, dtype=torch.bfloat16)
    x, x129 = torch.empty(48, 128, dtype=torch.bfloat16), torch.empty(129, 128, dtype=torch.bfloat16)
    with torch.no_grad():
        assert F._decode_own(x, (w,)) and not F._decode_own(x129, (w,))
    with torch.enable_grad():
        assert not F._decode_own(x, (w,))
    monkeypatch.setattr(F, "DECODE_GEMM", "lib")
    with torch.no_grad():
        assert not F._decode_own(x, (w,))
