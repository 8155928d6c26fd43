"""ops/side_stream.py on the GPU: GradSink's arena targets, and both join paths of one fused ResNet block's backward
(deferred to the end of the backward under the flat arena with side-aware hooks; immediate for returned gradients)."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def test_grad_sink_targets_are_arena_views():
    from pytorch_distributed_nn_amd.ops.side_stream import GradSink
    from pytorch_distributed_nn_amd.optim import flatten_module
    lin = nn.Linear(8, 4).cuda()
    fp = flatten_module(lin)
    lo, hi = fp.grad.data_ptr(), fp.grad.data_ptr() + 4 * fp.grad.numel()

    def in_arena(t, p):
        return t.data_ptr() == p.grad.data_ptr() and t.shape == p.shape and lo <= t.data_ptr() < hi
    sink = GradSink()
    assert in_arena(sink.target(lin.weight), lin.weight) and sink.ready == [lin.weight]
    tw, tb = sink.acc(lin.weight, lin.bias)
    assert in_arena(tw, lin.weight) and in_arena(tb, lin.bias)
    assert [id(p) for p in sink.ready] == [id(lin.weight), id(lin.weight), id(lin.bias)]
    outside = nn.Parameter(torch.zeros(4, device="cuda"))
    outside.grad = torch.zeros(4, device="cuda")
    assert sink.acc(lin.bias, outside) is None and sink.target(outside) is None and len(sink.ready) == 3


def _block(kind):
    from pytorch_distributed_nn_amd.models.resnet import BasicBlock, Bottleneck
    torch.manual_seed(0)
    return Bottleneck(64, 64, 1) if kind == "bottleneck" else BasicBlock(64, 128, 2)


def _backward(blk, side):
    """One forward + backward of the block on a fixed 8 x 16 x 16 input -> all parameter gradients, flat"""
    from pytorch_distributed_nn_amd import tuning
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 16, 16, 64, generator=g).cuda().to(torch.bfloat16).requires_grad_(True)
    old = tuning.set("side_wgrad", side)
    try:
        y = blk.forward_nhwc(x)
        y.backward(torch.randn(y.shape, generator=g).cuda().to(torch.bfloat16))
        torch.cuda.synchronize()
    finally:
        tuning.set("side_wgrad", old)
    return torch.cat([p.grad.float().flatten() for p in blk.parameters()])


@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_deferred_join_covers_every_fork(kind):
    """Flat arena, every grad-ready hook side-aware: the block's weight gradients (one fork per conv) are joined by
    the end-of-backward callback, which then covers every fork issued on the device."""
    from pytorch_distributed_nn_amd.ops.side_stream import fork_counts
    from pytorch_distributed_nn_amd.optim import flatten_module
    from pytorch_distributed_nn_amd.optim.flat import register_grad_ready_hook
    blk = _block(kind).cuda()
    flatten_module(blk)
    seen = []

    def hook(p):
        seen.append(p)
    hook._pdnn_side_aware = True
    for p in blk.parameters():
        register_grad_ready_hook(p, hook)
    dev = next(blk.parameters()).device
    before, _ = fork_counts(dev)
    _backward(blk, 1)
    forks, joined = fork_counts(dev)
    assert forks == joined
    assert forks - before == sum(isinstance(m, nn.Conv2d) for m in blk.modules())
    assert {id(p) for p in seen} == {id(p) for p in blk.parameters()}


@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_immediate_join_matches_serial(kind):
    """No arena: the weight gradients made on the side stream are returned to autograd, so the backward joins before
    it returns them; they equal the one-stream run's within 10x the serial-vs-serial floor (fp32 atomics ordering) +
    1e-3, the rule of test_side_stream_wgrad_matches_serial."""
    blk = _block(kind)
    side, serial, serial2 = (_backward(copy.deepcopy(blk).cuda(), s) for s in (1, 0, 0))
    floor = rel(serial2, serial)
    r = rel(side, serial)
    print(f"{kind}: side vs serial {r:.3e}, serial vs serial {floor:.3e}")
    assert r < 10 * floor + 1e-3, (r, floor)
