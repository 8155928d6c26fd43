"""The weight-gradient side stream's join rule (ops/side_stream.py join_now) as a table, and GradSink.done()
without a fork: it announces the ready parameters in insertion order and touches no stream."""
import pytest
import torch

from pytorch_distributed_nn_amd.ops import side_stream as SS


def _param(*hooks):
    """A parameter with grad-ready hooks; None = a parameter that never had one registered"""
    p = torch.nn.Parameter(torch.zeros(1))
    if hooks != (None,):
        p._pdnn_grad_hooks = list(hooks)
    return p


def _hook(aware):
    def fn(p):
        pass
    if aware:
        fn._pdnn_side_aware = True
    return fn


@pytest.mark.parametrize("name,returned,ready,join", [
    ("no ready parameters", False, lambda: [], False),
    ("all hooks side-aware", False, lambda: [_param(_hook(True)), _param(_hook(True), _hook(True))], False),
    ("one hook not side-aware", False, lambda: [_param(_hook(True)), _param(_hook(True), _hook(False))], True),
    ("a parameter with no hooks", False, lambda: [_param(None), _param()], False),
    ("returned, all hooks side-aware", True, lambda: [_param(_hook(True))], True),
])
def test_join_now(name, returned, ready, join):
    assert SS.join_now(returned, ready()) is join, name


def test_done_without_fork_announces_in_order(monkeypatch):
    announced = []

    def no_stream(*a, **k):
        raise AssertionError("GradSink.done() without a fork touched a stream")
    monkeypatch.setattr(SS, "grad_ready", announced.append)
    monkeypatch.setattr(SS.K, "stream_wait", no_stream)
    monkeypatch.setattr(SS, "join_at_backward_end", no_stream)
    monkeypatch.setattr(torch.cuda, "current_stream", no_stream)
    sink = SS.GradSink()
    ps = [_param(_hook(False)), _param(None), _param(_hook(True))]
    sink.ready += ps                     # off the GPU direct_grad is None: target() / acc() add nothing
    assert sink.target(ps[0]) is None and sink.acc(ps[1], ps[2]) is None and sink.ready == ps
    sink.done()
    assert [id(p) for p in announced] == [id(p) for p in ps]
    assert not sink.forked and not sink.returned and sink.side is None
