"""Which GEMM runs each product of a linear layer, held to a recorded launch trace.

Every case is one forward + backward of a node of the linear layers (`linear_group`, `swiglu_mlp`, `gelu_mlp`,
`fused_linear_cross_entropy`) under one configuration.  A recorder keeps, in order, every call that reaches the loaded
library (entry point, integers, floats and integer arrays by value; pointers as null / non-null, pointer arrays by length)
and every aten matrix product (operand shapes and strides).  tests/golden/linear_launch_trace.json holds what the package
did before the decision got one owner per product kind; the test only ever compares against it.  Gradient sinks, the
deferred queue and the side stream are tests/test_wgrad_routing_gpu.py's subject."""
import ctypes
import json
import os

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_launch_trace.json")

# (tokens, width D, width W).  whole: five 64-deep stages and a token count that is no multiple of 64 — `split_k` leaves every
# product whole; split: the weight gradients (contraction over 1024 tokens, one output tile) are cut; k200: K % 64 != 0 but
# % 8 == 0 (the transposes apply); n100: N % 8 != 0; m100: M % 8 != 0.
SHAPES = {"whole": (264, 256, 512), "split": (1024, 256, 256), "k200": (264, 200, 512), "n100": (264, 256, 100),
          "m100": (100, 256, 512)}
FLAGS = ["ROPE_EPILOGUE", "MLP_EPILOGUE", "GROUPED_WGRAD", "SPLIT_K", "BIAS_IN_WGRAD", "_MLP_FUSED", "GELU_EPILOGUE"]
GROUPS = ["lg", "lg_rope64", "lg_rope128", "lg_rope64_attn", "lg_norm"]
NODES = GROUPS + ["swiglu", "swiglu_norm", "gelu"]
CE = {"own": (601, 256, 24576, 512, 70), "lib": (300, 64, 2056, 128, 40), "one": (96, 64, 1000, 4096, 20)}
_MATMULS = ("aten::mm", "aten::addmm", "aten::addmm_", "aten::bmm", "aten::linear")


def _cases():
    """name -> (settings of touchnet_amd.functional, shape, node, linear_group's keywords)"""
    own1 = {"LINEAR_GEMM": "own", "_OWN_MIN_TILES": 1}
    out = {}

    def add(config, settings, shape, node, **kw):
        T, D, W = SHAPES.get(shape, (0, 0, 0))
        if "rope" in node and (D % 128 or W % 128):
            return                                                  # (outputs 0 and 1 are W and D wide: whole heads only)
        out[f"{config}/{shape}/{node}"] = (settings, shape, node, kw)

    for node in NODES:
        for shape in SHAPES:
            add("own", own1, shape, node)
            add("lib", {"LINEAR_GEMM": "lib"}, shape, node)
        add("own_few_tiles", {"LINEAR_GEMM": "own"}, "whole", node)
        for flag in FLAGS:
            for shape in ("whole", "split"):
                add(f"own_no_{flag}", {**own1, flag: False}, shape, node)
    for node in GROUPS:
        for wgrad in ("tn", "nt", "nt_fused"):
            for dgrad_tn in (True, False):
                add(f"lib_{wgrad}_{int(dgrad_tn)}", {"LINEAR_GEMM": "lib"}, "whole", node, wgrad=wgrad, dgrad_tn=dgrad_tn)
    for shape in CE:
        out[f"own/{shape}/ce"] = ({"LINEAR_GEMM": "own"}, shape, "ce", {})
        out[f"own_no_SPLIT_K/{shape}/ce"] = ({"LINEAR_GEMM": "own", "SPLIT_K": False}, shape, "ce", {})
        out[f"lib/{shape}/ce"] = ({"LINEAR_GEMM": "lib"}, shape, "ce", {})
    return out


CASES = _cases()


class _Library:
    """stands in for the loaded library: every entry point records its call, then makes it"""

    def __init__(self, handle, events):
        self._handle, self._events = handle, events

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        kinds = fn.argtypes or ()

        def call(*args):
            self._events.append(f"{name}({','.join(_arg(a, k) for a, k in zip(args, kinds))})")
            return fn(*args)
        return call


def _arg(a, kind):
    if kind is ctypes.c_void_p:
        return "p" if (a.value if isinstance(a, ctypes.c_void_p) else a) else "0"
    if isinstance(a, ctypes.Array):
        return f"p*{len(a)}" if a._type_ is ctypes.c_void_p else "[" + " ".join(str(int(v)) for v in a) + "]"
    if a is None:
        return "0"
    return repr(float(a)) if kind is ctypes.c_float else str(int(a))


class _Products(TorchDispatchMode):
    """records the library's (hipBLASLt through torch) matrix products"""

    def __init__(self, events):
        super().__init__()
        self._events = events

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func._schema.name in _MATMULS:
            ops = [a for a in list(args) + [kwargs[k] for k in sorted(kwargs)] if isinstance(a, torch.Tensor)]
            self._events.append(f"{func._schema.name}.{func._overloadname}("
                                + ";".join(f"{list(t.shape)}/{list(t.stride())}" for t in ops) + ")")
        return func(*args, **kwargs)


def _r(g, *s, scale=1.0):
    return (torch.randn(s, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _node(F, shape, node, kw):
    """the forward of one node on fixed values: () -> list of outputs"""
    g = torch.Generator().manual_seed(11)
    p = lambda *s, scale: _r(g, *s, scale=scale).requires_grad_()
    if node == "ce":
        n, H, V, chunk, n_ign = CE[shape]
        h, w = p(n, H, scale=1.0), p(V, H, scale=H ** -0.5)
        lab = torch.randint(0, V, (n,), generator=g)
        lab[torch.randperm(n, generator=g)[:n_ign]] = -100
        sl = torch.full((n,), 50, dtype=torch.int64)
        return lambda: [F.fused_linear_cross_entropy(h, w, lab.to(DEV), sl.to(DEV), 4.0, -100, chunk_tokens=chunk,
                                                     compact=False)[0]]
    T, D, W = SHAPES[shape]
    x = p(2, T // 2, D, scale=1.0)                                  # (two rows of T / 2 tokens, as the models' [B, T, H])
    norm_w = p(D, scale=1.0)
    if node.startswith("lg"):
        layers = [(p(n, D, scale=D ** -0.5), p(n, scale=0.1)) for n in (W, D, W)]
    elif node == "gelu":
        layers = [(p(W, D, scale=D ** -0.5), p(W, scale=0.1)), (p(D, W, scale=W ** -0.5), p(D, scale=0.1))]
    else:
        layers = [p(W, D, scale=D ** -0.5), p(W, D, scale=D ** -0.5), p(D, W, scale=W ** -0.5)]
    rope = None
    if "rope" in node:
        hd = 128 if "128" in node else 64
        cos, sin = F.rope_tables(torch.arange(T, device=DEV).view(1, T), F.rope_inv_freq(hd, 10000.0, device=DEV),
                                 torch.bfloat16)
        rope = (cos, sin, hd, (0, 1))

    def fwd():
        xin, src = x, None
        if node.endswith("norm"):
            xin = F.rms_norm(x, norm_w, 1e-5)
            src = F.norm_source(x, norm_w, 1e-5)
        if node.startswith("lg"):
            return F.linear_group(xin, layers, norm_src=src, rope=rope, rope_grad_in_attention=node.endswith("attn"), **kw)
        if node == "gelu":
            return [F.gelu_mlp(xin, *layers[0], *layers[1])]
        return [F.swiglu_mlp(xin, *layers, norm_src=src)]
    return fwd


def trace(name, monkeypatch):
    """the recorded calls of case `name`"""
    import touchnet_amd._C as _C
    import touchnet_amd.functional as F
    settings, shape, node, kw = CASES[name]
    for k, v in settings.items():
        assert hasattr(F, k), k
        monkeypatch.setattr(F, k, v)
    if shape == "split" and settings.get("SPLIT_K", True):
        T, D, W = SHAPES[shape]
        assert F.split_k(W, D, T, True, True) > 1                   # the case is here for the split weight gradient
    fwd = _node(F, shape, node, kw)
    gs = torch.Generator().manual_seed(23)
    events = []
    handle = _C.lib()
    monkeypatch.setattr(_C, "lib", lambda: _Library(handle, events))
    with _Products(events):
        outs = fwd()
        sum((o.float() * _r(gs, *o.shape)).sum() for o in outs).backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return events


@pytest.fixture(scope="module")
def golden_traces():
    with open(GOLDEN) as f:
        data = json.load(f)
    return {name: [data["events"][e] for e in data["traces"][i]] for name, i in data["cases"].items()}


def test_the_recording_holds_every_case(golden_traces):
    assert sorted(golden_traces) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launches_are_the_recorded_ones(name, golden_traces, monkeypatch):
    got, want = trace(name, monkeypatch), golden_traces[name]
    assert any(e.startswith("tn_") for e in got)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: call {i}"
    assert len(got) == len(want), f"{name}: {got[len(want):] or want[len(got):]}"
