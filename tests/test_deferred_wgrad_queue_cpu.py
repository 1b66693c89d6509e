"""Bookkeeping of the deferred-weight-gradient queue (functional.DeferredWgrad) on meta tensors: what it takes, what it
leaves to the per-layer path, the order it flushes in.  No device work: the launch is replaced by a recorder."""
import weakref

import pytest
import torch

import touchnet_amd.functional as F
from touchnet_amd import _C


def _layer(d=64, ffn=128):
    mk = lambda *s: torch.nn.Parameter(torch.empty(*s, dtype=torch.bfloat16, device="meta"))
    return [(mk(d, d), mk(d)), (mk(d, d), None), (mk(ffn, d), mk(ffn))]


def _operands(w, tokens=40):
    return (torch.empty(tokens, w.shape[0], dtype=torch.bfloat16, device="meta"),
            torch.empty(tokens, w.shape[1], dtype=torch.bfloat16, device="meta"))


def _queue(layers, **kw):
    q = F.DeferredWgrad(layers, **kw)
    calls = []

    def launch(pairs, outs=None, accumulate=False, bias_grads=None):
        calls.append((list(pairs), list(outs), accumulate, list(bias_grads)))
        return outs
    q.launch = launch
    return q, calls


def test_queue_flushes_in_queue_order_and_writes_the_gradients():
    layers = [_layer(), _layer()]
    q, calls = _queue(layers)
    pushed = []
    for layer in reversed(layers):                            # the backward meets the last layer first
        for w, b in reversed(layer):
            dy, x = _operands(w)
            assert F._queue_wgrad(w, dy, x, b is not None)
            pushed.append((w, b, dy, x))
    assert len(q) == 6 and not calls
    q.flush()
    assert len(q) == 0 and q.flushes == 1 and len(calls) == 1
    pairs, outs, accumulate, bgs = calls[0]
    assert not accumulate
    assert all(a is dy and c is x for (a, c), (_, _, dy, x) in zip(pairs, pushed))          # queue order
    for (w, b, _, _), o, bg in zip(pushed, outs, bgs):
        assert w.grad is o and tuple(o.shape) == tuple(w.shape) and o.dtype == torch.bfloat16
        assert (bg is None) == (b is None) and (b is None or b.grad is bg)
    q.flush()                                                 # nothing waiting: nothing runs
    assert len(calls) == 1
    # a second backward adds to the gradients that exist
    for w, b, dy, x in pushed[:2]:
        assert F._queue_wgrad(w, dy, x, False)
    q.flush()
    assert calls[1][2] is True and all(o is w.grad for o, (w, _, _, _) in zip(calls[1][1], pushed[:2]))
    q.close()
    assert not any(id(w) in F.WGRAD_QUEUES for layer in layers for w, _ in layer)


def test_a_weight_queued_twice_without_a_flush_is_refused():
    layers = [_layer()]
    q, _ = _queue(layers)
    w, _ = layers[0][0]
    dy, x = _operands(w)
    assert F._queue_wgrad(w, dy, x, True)
    with pytest.raises(_C.KernelError, match="queued twice"):
        F._queue_wgrad(w, dy, x, True)
    q.flush()
    assert F._queue_wgrad(w, dy, x, True)                     # with a flush in between it is taken again
    q.flush()
    q.close()


def test_the_queue_flushes_by_itself_before_it_holds_more_layers_than_its_threshold():
    layers = [_layer() for _ in range(5)]
    q, calls = _queue(layers, flush_layers=2)
    for layer in layers:
        for w, b in layer:
            assert F._queue_wgrad(w, *_operands(w), b is not None)
    assert [len(c[0]) for c in calls] == [6, 6] and len(q) == 3     # layers 0-1, 2-3 ran; layer 4 waits
    q.flush()
    assert [len(c[0]) for c in calls] == [6, 6, 3] and q.flushes == 3
    q.close()


def test_the_queue_is_bypassed_where_something_else_owns_the_product(monkeypatch):
    layers = [_layer()]
    q, calls = _queue(layers)
    (w, b), (w2, _), _ = layers[0]
    dy, x = _operands(w)

    class Sink:
        def owns(self, p):
            return p is w
    sink = Sink()
    monkeypatch.setitem(F.GRAD_SINKS, id(w), weakref.ref(sink))
    assert not F._queue_wgrad(w, dy, x, True) and len(q) == 0            # a data-parallel engine's sink owns the weight
    assert F._queue_wgrad(w2, *_operands(w2), False) and len(q) == 1     # ... and only that one
    q.flush()
    monkeypatch.delitem(F.GRAD_SINKS, id(w))
    monkeypatch.setattr(F, "DEFERRED_WGRAD", False)                      # the switch
    assert not F._queue_wgrad(w, dy, x, True)
    monkeypatch.setattr(F, "DEFERRED_WGRAD", True)
    monkeypatch.setattr(F, "WGRAD_STREAM", object())                     # the side stream keeps the per-layer path
    assert not F._queue_wgrad(w, dy, x, True)
    monkeypatch.setattr(F, "WGRAD_STREAM", None)
    stranger = torch.nn.Parameter(torch.empty(64, 64, dtype=torch.bfloat16, device="meta"))
    assert not F._queue_wgrad(stranger, dy, x, False)                    # a weight no queue owns
    assert not F._queue_wgrad(w2, *_operands(w2), True)                  # a bias gradient for a layer without a bias
    assert not F._queue_wgrad(w, dy[:, :32], x, True)                    # operands that are not the weight's
    assert len(q) == 0 and len(calls) == 1
    q.close()
