"""Muon's torch-op path (optim.fused.Muon._step_param, newton_schulz) against the float64 reference muon_ref.py, the
measured constant the GPU test's allowance comes from, the state_dict round trip and the command line."""
import copy

import pytest
import torch

import muon_ref as R
from layerwise_ref import lamb_step_ref

U = 2.0 ** -24
SHAPES = [(72, 40), (40, 72), (33, 50), (64,), (10,)]
KW = dict(lr=0.05, momentum=0.9, weight_decay=0.1, adam_lr=1e-2, adam_weight_decay=0.05)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g) * 0.1) for s in SHAPES]
    return ps, [[torch.randn(*s, generator=g) for s in SHAPES] for _ in range(2)]


def test_newton_schulz_constant_is_the_measured_one():
    worst = max(R.rel_fro(_ns(x0, s), R.ns_ref(x0, s, 5)) for x0, s in R.ns_inputs())
    print(f"fp32 newton_schulz against float64: worst relative Frobenius error {worst:.4g}")
    assert abs(worst - R.NS_MEASURED) <= 0.05 * R.NS_MEASURED and R.NS_ALLOW == 4.0 * R.NS_MEASURED


def _ns(x0, s, steps=5):
    from pytorch_distributed_nn_amd.optim import newton_schulz
    return newton_schulz(x0, torch.tensor(s), steps)


@pytest.mark.parametrize("nesterov", [False, True])
def test_cpu_step_matches_the_reference(nesterov):
    from pytorch_distributed_nn_amd.optim import Muon
    ps, grads = _params()
    opt = Muon(ps, nesterov=nesterov, **KW)
    opt.grad_scale = 0.5
    for step, gl in enumerate(grads):
        before = [p.detach().clone() for p in ps]
        state = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state.get(p, {}).items()} for p in ps]
        for p, g in zip(ps, gl):
            p.grad = g.clone()
        opt.step()
        xs = iter(opt.ortho())
        for p, w0, g, st in zip(ps, before, gl, state):
            if p.ndim != 2:
                want, _, _ = lamb_step_ref([w0], [g], [st], lr=KW["adam_lr"], betas=(0.9, 0.999), eps=1e-8,
                                           weight_decay=KW["adam_weight_decay"], exclude=lambda t: True, gs=0.5,
                                           decay_excluded=True)
                assert torch.allclose(p.detach().double(), want[0], rtol=1e-5, atol=1e-7), (step, p.shape)
                continue
            r = R.muon_step_ref(w0, g, st.get("exp_avg", torch.zeros_like(w0)), KW["lr"], 0.9, nesterov, 5, 0.1, 1e-7,
                                gs=0.5)
            assert ((opt.state[p]["exp_avg"].double() - r["buf"]).abs() <= 4 * U * r["A_buf"]).all()
            x = next(xs)
            assert x.dtype == torch.bfloat16 and x.shape == r["x"].shape
            assert R.rel_fro(x, r["x"]) <= R.NS_ALLOW, (step, p.shape)
            # the weights from the path's own X: only the final fp32 arithmetic
            xw = (x.t() if p.shape[0] > p.shape[1] else x).double()
            want = w0.double() * (1 - KW["lr"] * 0.1) - KW["lr"] * max(1.0, p.shape[0] / p.shape[1]) ** 0.5 * xw
            assert torch.allclose(p.detach().double(), want, rtol=1e-6, atol=1e-7), (step, p.shape)


def test_state_dict_round_trip():
    from pytorch_distributed_nn_amd.optim import Muon
    ps, grads = _params(1)
    qs = copy.deepcopy(ps)
    a, b = Muon(ps, **KW), Muon(qs, **KW)
    for p, g in zip(ps, grads[0]):
        p.grad = g.clone()
    a.step()
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for o, pl in ((a, ps), (b, qs)):
        for p, g in zip(pl, grads[1]):
            p.grad = g.clone()
        o.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, qs))


def test_cli_parses_muon_and_refuses_trust_coef():
    from pytorch_distributed_nn_amd.cli import parse_args
    args = parse_args(["--optimizer", "muon", "--lr", "0.02", "--momentum", "0.95", "--adam-lr", "1e-3"])
    assert args.optimizer == "muon" and args.adam_lr == 1e-3
    with pytest.raises(SystemExit, match="trust-coef"):
        parse_args(["--optimizer", "muon", "--trust-coef", "0.01"])
    with pytest.raises(SystemExit, match="adam-lr"):
        parse_args(["--optimizer", "adamw", "--adam-lr", "1e-3"])
