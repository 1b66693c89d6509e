"""Where a linear layer's weight gradient goes (functional._route_wgrad): the three autograd nodes of the linear layers,
each run once per route — no owner, a bf16 gradient sink, an fp32 gradient sink, the deferred queue, the side stream.  The
routes differ in where dW = dY^T x is written, never in its bits.

264 tokens: not a multiple of the 64-deep stage, and five stages — `split_k` leaves every product whole; widths 256 / 512;
the hand-written GEMM is made to take these few-tile products (`_OWN_MIN_TILES`)."""
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, D, W = 264, 256, 512
ROUTES = ["none", "sink_bf16", "sink_f32", "queue", "side_stream"]
# products the deferred queue is handed: every layer's — but for the three of the grouped MLP launch, which stay together
QUEUED = {"linear_group": 3, "gelu_mlp": 2, "swiglu_mlp": 0, "swiglu_mlp_single": 3}


def _r(g, *s, scale=1.0):
    return (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).to(DEV)


class _Sink:
    """a data-parallel engine's side of the protocol: views of one flat buffer, NaN until a launch writes them"""

    def __init__(self, ws, dtype):
        self.ws, self.taken, self.finished = list(ws), 0, 0
        self.flat = torch.full((sum(w.numel() for w in ws),), float("nan"), dtype=dtype, device=DEV)

    def view(self, p):
        o = 0
        for w in self.ws:
            if w is p:
                return self.flat[o:o + w.numel()].view(w.shape)
            o += w.numel()
        raise KeyError("not a weight of this sink")

    def owns(self, p):
        return any(p is w for w in self.ws)

    def take(self, p):
        self.taken += 1
        return self.view(p), False

    def done(self, p):
        self.finished += 1


def _node(F, name, x=None):
    """``(x, [(weight, bias), ...], forward)`` of one node on fixed values"""
    g = torch.Generator().manual_seed(11)
    x = (_r(g, T, D) if x is None else x).requires_grad_()
    p = lambda *s, scale: _r(g, *s, scale=scale).requires_grad_()
    if name == "linear_group":
        layers = [(p(n, D, scale=D ** -0.5), p(n, scale=0.1)) for n in (W, D, W)]
        fwd = lambda: F.linear_group(x, layers)
    elif name == "gelu_mlp":
        layers = [(p(W, D, scale=D ** -0.5), p(W, scale=0.1)), (p(D, W, scale=W ** -0.5), p(D, scale=0.1))]
        fwd = lambda: [F.gelu_mlp(x, *layers[0], *layers[1])]
    else:
        layers = [(p(W, D, scale=D ** -0.5), None), (p(W, D, scale=D ** -0.5), None), (p(D, W, scale=W ** -0.5), None)]
        fwd = lambda: [F.swiglu_mlp(x, *(w for w, _ in layers))]
    return x, layers, fwd


def _run(F, name, route, monkeypatch):
    """forward + backward of `name` on `route`: outputs, dx, [dW], [db] — and the checks that the route meant is the one
    that ran"""
    monkeypatch.setattr(F, "_OWN_MIN_TILES", 1)
    monkeypatch.setattr(F, "GROUPED_WGRAD", name != "swiglu_mlp_single")
    sums = []
    column_sum = F.column_sum
    monkeypatch.setattr(F, "column_sum", lambda t: sums.append(1) or column_sum(t))
    x, layers, fwd = _node(F, name)
    ws = [w for w, _ in layers]
    g = torch.Generator().manual_seed(23)
    sink = queue = None
    if route.startswith("sink"):
        sink = _Sink(ws, torch.float32 if route == "sink_f32" else torch.bfloat16)
        for w in ws:
            monkeypatch.setitem(F.GRAD_SINKS, id(w), weakref.ref(sink))
    elif route == "queue":
        queue = F.DeferredWgrad([layers])
    elif route == "side_stream":
        F.enable_wgrad_stream(True)
    try:
        outs = fwd()
        sum((o.float() * _r(g, *o.shape)).sum() for o in outs).backward()
        if queue is not None:
            assert len(queue) == QUEUED[name]                       # the queue received the products ...
            assert all(w.grad is None for w in ws) or not QUEUED[name]    # ... and nothing else formed them
            queue.flush()
            assert len(queue) == 0
        F.sync_wgrad_stream()
        torch.cuda.synchronize()
    finally:
        if route == "side_stream":
            F.enable_wgrad_stream(False)
        if queue is not None:
            queue._items = []
            queue.close()
    assert F.BIAS_IN_WGRAD and not sums                          # every bias gradient rode on a weight-gradient launch
    if sink is not None:
        assert sink.taken == sink.finished == len(ws)
        assert all(w.grad is None for w in ws)                      # autograd saw no gradient for a sunk weight
        dws = [sink.view(w).to(torch.bfloat16) for w in ws]         # (fp32: the one rounding the bf16 launch does itself)
    else:
        dws = [w.grad for w in ws]
    return [o.detach() for o in outs], x.grad, dws, [b.grad if b is not None else None for _, b in layers]


_NO_OWNER = {}


def _no_owner(F, name, monkeypatch):
    if name not in _NO_OWNER:                                       # computed once, shared by the routes, never written
        _NO_OWNER[name] = _run(F, name, "none", monkeypatch)
    return _NO_OWNER[name]


@pytest.mark.parametrize("route", ROUTES[1:])
@pytest.mark.parametrize("name", sorted(QUEUED))
def test_every_route_forms_the_bits_of_the_route_without_an_owner(name, route, monkeypatch):
    import touchnet_amd.functional as F
    ref = _no_owner(F, name, monkeypatch)
    got = _run(F, name, route, monkeypatch)
    assert all(dw is not None and bool(torch.isfinite(dw.float()).all()) for dw in ref[2])
    for what, a, b in zip(("outputs", "dx", "dW", "db"), got, ref):
        a, b = (a, b) if isinstance(a, list) else ([a], [b])
        assert len(a) == len(b), what
        for i, (u, v) in enumerate(zip(a, b)):
            assert (u is None) == (v is None), (what, i)
            assert u is None or (u.dtype == v.dtype and torch.equal(u, v)), (what, i)


def test_a_queue_that_owns_gate_proj_alone_receives_its_product(monkeypatch):
    """`swiglu_mlp` with one product per weight follows the common rule: the queue is asked"""
    import touchnet_amd.functional as F
    ref = _no_owner(F, "swiglu_mlp_single", monkeypatch)
    monkeypatch.setattr(F, "_OWN_MIN_TILES", 1)
    monkeypatch.setattr(F, "GROUPED_WGRAD", False)
    x, layers, fwd = _node(F, "swiglu_mlp_single")
    (wg, _), (wu, _), (wd, _) = layers
    queue = F.DeferredWgrad([[(wg, None)]])
    try:
        y = fwd()[0]
        (y.float() * _r(torch.Generator().manual_seed(23), *y.shape)).sum().backward()
        assert len(queue) == 1 and wg.grad is None and wu.grad is not None and wd.grad is not None
        queue.flush()
    finally:
        queue._items = []
        queue.close()
    for got, want in zip((wg.grad, wu.grad, wd.grad), ref[2]):
        assert torch.equal(got, want)
    assert torch.equal(x.grad, ref[1])


@pytest.mark.parametrize("grouped", [False, True])
def test_an_operand_the_kernel_refuses_gets_the_library_product(grouped, monkeypatch):
    """`swiglu_mlp` on an input that is not 16-byte aligned: the node keeps the hand-written kernel for every product that
    does not read x, and dW_gate = d(gate)^T x, dW_up = d(up)^T x — which do — come from `torch.mm`; held to the fp64
    product of the same operands at the bound of tests/test_gemm_fused_gpu.py (one bf16 rounding of an fp32 sum)."""
    import touchnet_amd.functional as F
    monkeypatch.setattr(F, "_OWN_MIN_TILES", 1)
    monkeypatch.setattr(F, "GROUPED_WGRAD", grouped)
    base = _r(torch.Generator().manual_seed(11), T * D + 8)
    x, layers, fwd = _node(F, "swiglu_mlp_single", x=base[4:4 + T * D].view(T, D).detach())
    assert x.data_ptr() % 16 == 8
    (wg, _), (wu, _), (wd, _) = layers
    y = fwd()[0]
    calls = []
    mm = torch.mm
    monkeypatch.setattr(torch, "mm", lambda a, b: calls.append((a, b, mm(a, b))) or calls[-1][2])
    (y.float() * _r(torch.Generator().manual_seed(23), *y.shape)).sum().backward()
    monkeypatch.setattr(torch, "mm", mm)
    torch.cuda.synchronize()
    assert len(calls) == 2 and all(b.data_ptr() == x.data_ptr() and tuple(a.shape) == (W, T) for a, b, _ in calls)
    assert wd.grad is not None and tuple(wd.grad.shape) == (D, W)
    for w, (a, b, out) in zip((wg, wu), calls):
        assert torch.equal(w.grad, out)                             # this product is the weight's gradient
        ref = a.detach().double() @ b.detach().double()
        err = float((w.grad.double() - ref).abs().max())
        print(f"grouped={grouped} err {err:.3e} bound {float(ref.abs().max()) * 2 ** -7:.3e}")
        assert err <= float(ref.abs().max()) * 2 ** -7, err
    assert not torch.equal(wg.grad, wu.grad)
