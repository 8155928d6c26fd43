"""The torch-op paths of the fused SGD / Adam / AdamW (loose tensors, CPU arena) against ``torch.optim``: bit-equal
without clipping, within the clip test's tolerance with ``set_grad_clip``, and bit-equal across a
``state_dict()`` / ``load_state_dict()`` round trip."""
import copy

import pytest
import torch

SHAPES = [(7, 5), (5,), (3, 4, 2), ()]          # a 0-dim parameter: the gradient scale must not reshape it
STEPS = 5
CONFIGS = {
    "sgd": ("SGD", dict(lr=0.05)),
    "sgd-momentum": ("SGD", dict(lr=0.05, momentum=0.9)),
    "sgd-nesterov-wd": ("SGD", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-2)),
    "sgd-dampening-wd": ("SGD", dict(lr=0.05, momentum=0.9, dampening=0.3, weight_decay=1e-2)),
    "adam": ("Adam", dict(lr=1e-2)),
    "adam-wd": ("Adam", dict(lr=1e-2, weight_decay=1e-2)),
    "adamw-betas": ("AdamW", dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)),
}


def _tensors(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    gs = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(STEPS)]     # ||g|| ~ sqrt(65) ~ 8 >> 1
    return ps, gs


def _ours(name, ps, layout):
    from pytorch_distributed_nn_amd import optim as O
    from pytorch_distributed_nn_amd.optim.flat import FlatParams
    cls, kw = CONFIGS[name]
    mine = [torch.nn.Parameter(p.clone()) for p in ps]
    fp = FlatParams(mine, device="cpu") if layout == "arena" else None
    return mine, fp, getattr(O, cls)(mine, **kw)


def _set_grads(mine, fp, gs):
    for p, g in zip(mine, gs):
        if fp is not None:
            p.grad.copy_(g)
        else:
            p.grad = g.clone()


def _run(name, layout, grad_scale, clip):
    """(ours, torch's) parameters after every step, plus the two gradient norms of every clipped step."""
    cls, kw = CONFIGS[name]
    ps, gs = _tensors()
    mine, fp, opt = _ours(name, ps, layout)
    refs = [torch.nn.Parameter(p.clone()) for p in ps]
    ropt = getattr(torch.optim, cls)(refs, **kw)
    opt.grad_scale = grad_scale
    if clip:
        opt.set_grad_clip(clip)
    out = []
    for step in gs:
        _set_grads(mine, fp, step)
        for q, g in zip(refs, step):
            q.grad = g * grad_scale
        tn = torch.nn.utils.clip_grad_norm_(refs, clip) if clip else None
        ropt.step()
        opt.step()
        assert all(p.shape == torch.Size(s) for p, s in zip(mine, SHAPES))
        out.append(([p.detach().clone() for p in mine], [q.detach().clone() for q in refs],
                    float(opt.grad_norm) if clip else None, None if tn is None else float(tn)))
    return out


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("layout", ["loose", "arena"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_bit_equal_to_torch_optim(name, layout, grad_scale):
    for mine, refs, _, _ in _run(name, layout, grad_scale, None):
        for p, q in zip(mine, refs):
            assert torch.equal(p, q), (p - q).abs().max()


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("layout", ["loose", "arena"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_clipped_matches_torch_clip(name, layout, grad_scale):
    # tolerances of test_grad_clip_cpu.test_fallback_matches_torch_clip
    for mine, refs, norm, tn in _run(name, layout, grad_scale, 1.0):
        assert tn > 2.0                                            # the clip is active
        assert abs(norm - tn) <= 1e-5 * tn
        for p, q in zip(mine, refs):
            assert torch.allclose(p, q, atol=1e-6, rtol=0), (p - q).abs().max()


@pytest.mark.parametrize("name", ["sgd-momentum", "adamw-betas"])
def test_state_dict_round_trip_on_an_arena(name):
    ps, gs = _tensors()
    mine, fp, opt = _ours(name, ps, "arena")
    for step in gs[:-1]:
        _set_grads(mine, fp, step)
        opt.step()
    # a second optimizer on a second arena picks the run up from the state dict
    mine2, fp2, opt2 = _ours(name, [p.detach() for p in mine], "arena")
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))      # as saved and loaded: state_dict() holds references
    for m, f, o in ((mine, fp, opt), (mine2, fp2, opt2)):
        _set_grads(m, f, gs[-1])
        o.step()
    assert torch.equal(fp.data, fp2.data)
    a, b = opt.state_dict(), opt2.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys()
    for k, st in a["state"].items():
        assert st.keys() == b["state"][k].keys()
        for key, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["state"][k][key])), (k, key)
