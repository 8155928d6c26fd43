"""The fp64 reference of the layer-wise optimizers (layerwise_ref.py) anchored to torch.optim and to a hand-computed
case, and the torch-op paths of ``LARS`` / ``LAMB`` (loose tensors, a CPU arena) against that reference; the host-side
table checks and the command line's PS-mode guard.  No GPU."""
import copy
import math

import pytest
import torch

from layerwise_ref import lamb_step_ref, lars_step_ref

SHAPES = [(8, 3, 3, 3), (8,), (10, 100), (10,), (65,), (7, 9)]


def _tensors(seed, dtype=torch.float64, shapes=SHAPES):
    gen = torch.Generator().manual_seed(seed)
    ps = [(torch.randn(*s, generator=gen) * 0.1).to(dtype) for s in shapes]
    gs = [[torch.randn(*s, generator=gen).to(dtype) for s in shapes] for _ in range(3)]
    return ps, gs


# ------------------------------------------------------------------------------------- anchored to torch.optim
@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_ref_with_everything_excluded_is_torch_sgd(nesterov):
    ps, grads = _tensors(0)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-2, nesterov=nesterov)
    tp = [torch.nn.Parameter(p.clone()) for p in ps]
    topt = torch.optim.SGD(tp, **kw)
    state = [{} for _ in ps]
    for g in grads:
        ps, state, info = lars_step_ref(ps, g, state, exclude=lambda p: True, decay_excluded=True, **kw)
        assert info["ratio"] == [1.0] * len(ps)
        for q, gi in zip(tp, g):
            q.grad = gi.clone()
        topt.step()
        for p, q in zip(ps, tp):
            assert (p - q.detach()).abs().max().item() <= 1e-12


def test_lars_ref_dampening_is_torch_sgd():
    ps, grads = _tensors(1)
    kw = dict(lr=0.05, momentum=0.8, dampening=0.3, weight_decay=0.0)
    tp = [torch.nn.Parameter(p.clone()) for p in ps]
    topt = torch.optim.SGD(tp, **kw)
    state = [{} for _ in ps]
    for g in grads:
        ps, state, _ = lars_step_ref(ps, g, state, exclude=lambda p: True, **kw)
        for q, gi in zip(tp, g):
            q.grad = gi.clone()
        topt.step()
        for p, q in zip(ps, tp):
            assert (p - q.detach()).abs().max().item() <= 1e-12


def test_lamb_ref_with_everything_excluded_is_torch_adamw():
    """torch.optim.AdamW shrinks the weight first (w *= 1 - lr wd) and then subtracts lr m^ / (sqrt(v) / sqrt(bc2) +
    eps); the reference subtracts lr (m^ / (sqrt(v / bc2) + eps) + wd w) from the unshrunk weight.  The two agree to
    rounding: eps is added to the bias-corrected root in both.  The OTHER placement (eps added to sqrt(v) before the
    bias correction, the original Adam paper's epsilon-hat form) is a different update; the last assert shows the
    difference is far above the 1e-12 the equality holds to, so the test would tell the two apart."""
    ps, grads = _tensors(2)
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-3, weight_decay=0.1)
    tp = [torch.nn.Parameter(p.clone()) for p in ps]
    topt = torch.optim.AdamW(tp, **kw)
    state = [{} for _ in ps]
    other = 0.0
    for t, g in enumerate(grads, 1):
        before = [p.clone() for p in ps]
        ps, state, info = lamb_step_ref(ps, g, state, exclude=lambda p: True, decay_excluded=True, **kw)
        assert info["ratio"] == [1.0] * len(ps)
        for q, gi in zip(tp, g):
            q.grad = gi.clone()
        topt.step()
        for p, q, w, st in zip(ps, tp, before, state):
            assert (p - q.detach()).abs().max().item() <= 1e-12
            bc1, bc2 = 1 - 0.9 ** t, 1 - 0.99 ** t
            alt = w - 1e-2 * ((st["exp_avg"] / bc1) / ((st["exp_avg_sq"].sqrt() + 1e-3) / math.sqrt(bc2)) + 0.1 * w)
            other = max(other, (alt - p).abs().max().item())
    assert other > 1e-6


# ------------------------------------------------------------------------------------- by hand
def test_ratio_formulas_by_hand():
    w = torch.tensor([[3.0, 0.0], [0.0, 4.0]], dtype=torch.float64)           # |w| = 5
    b = torch.tensor([1.0, 2.0], dtype=torch.float64)
    g = torch.tensor([[0.0, 6.0], [8.0, 0.0]], dtype=torch.float64)           # |g| = 10
    gb = torch.tensor([0.5, -0.5], dtype=torch.float64)
    # LARS, eta 0.1, wd 0.1, eps 0, no momentum, lr 1:  r = 0.1 * 5 / (10 + 0.1 * 5) = 1 / 21
    (w1, b1), _, info = lars_step_ref([w, b], [g, gb], [{}, {}], lr=1.0, momentum=0.0, weight_decay=0.1,
                                      trust_coef=0.1, eps=0.0)
    assert info["ratio"][0] == pytest.approx(1 / 21, rel=1e-15) and info["ratio"][1] == 1.0
    assert info["wnorm"][0] == 5.0 and info["unorm"][0] == 10.0
    assert torch.allclose(w1, w - (g + 0.1 * w) / 21, rtol=0, atol=1e-15)
    assert torch.equal(b1, b - gb)                                         # the bias: ratio 1, no decay
    # the gradient scale enters the norm: gs = 0.5 -> |g'| = 5, r = 0.5 / 5.5
    _, _, info = lars_step_ref([w, b], [g, gb], [{}, {}], lr=1.0, momentum=0.0, weight_decay=0.1, trust_coef=0.1,
                               eps=0.0, gs=0.5)
    assert info["ratio"][0] == pytest.approx(1 / 11, rel=1e-15) and info["unorm"][0] == 5.0
    # clamp: eta 10 -> r = 50 / 10.5 > 1 -> 1
    _, _, info = lars_step_ref([w], [g], [{}], lr=1.0, weight_decay=0.1, trust_coef=10.0, eps=0.0, clamp=True)
    assert info["ratio"] == [1.0]
    # zero gradient, zero weight: 1
    _, _, info = lars_step_ref([w, 0 * w], [0 * g, g], [{}, {}], lr=1.0, weight_decay=0.1)
    assert info["ratio"] == [1.0, 1.0]
    # LAMB, first step, eps 0: m^ = g, v^ = g^2, u = sign(g) + wd w
    g2 = torch.tensor([[1.0, -2.0], [2.0, -4.0]], dtype=torch.float64)
    (w2, b2), st, info = lamb_step_ref([w, b], [g2, gb], [{}, {}], lr=0.1, eps=0.0, weight_decay=0.5)
    u = torch.tensor([[2.5, -1.0], [1.0, 1.0]], dtype=torch.float64)
    assert info["unorm"][0] == pytest.approx(math.sqrt(9.25), rel=1e-14)
    assert info["ratio"][0] == pytest.approx(5 / math.sqrt(9.25), rel=1e-14) and info["ratio"][1] == 1.0
    assert torch.allclose(w2, w - 0.1 * (5 / math.sqrt(9.25)) * u, rtol=0, atol=1e-14)
    assert torch.allclose(b2, b - 0.1 * torch.sign(gb), rtol=0, atol=1e-14)      # the bias: ratio 1, no decay
    assert st[0]["step"] == 1 and torch.allclose(st[0]["exp_avg"], 0.1 * g2, rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------- the torch-op paths
def _bound(p_ref, lr, r, A):
    """|p - p_ref| <= 2^-22 |p_ref| + 1e-4 lr r A: the final rounding with 2x margin, plus the ratio's error and the
    chain's < 16 roundings of 2^-24, each relative to an operand bounded by A, with 2x margin."""
    return 2.0 ** -22 * p_ref.abs() + 1e-4 * lr * r * A


@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("name", ["lars", "lars_nesterov", "lamb"])
def test_cpu_paths_match_the_reference(name, arena):
    from pytorch_distributed_nn_amd.optim import LAMB, LARS
    from pytorch_distributed_nn_amd.optim.flat import FlatParams
    init, grads = _tensors(3, torch.float32)
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    if arena:
        fp = FlatParams(ps, device="cpu")
        assert not fp.data.is_cuda
    if name == "lamb":
        kw = dict(lr=1e-2, weight_decay=0.1)
        opt, ref = LAMB(ps, **kw), lamb_step_ref
    else:
        kw = dict(lr=0.5, momentum=0.9, weight_decay=1e-2, nesterov=name.endswith("nesterov"), trust_coef=0.02)
        opt, ref = LARS(ps, **kw), lars_step_ref
    opt.grad_scale = 0.5
    for g in grads:
        for p, gi in zip(ps, g):
            if p.grad is None:
                p.grad = gi.clone()
            else:
                p.grad.copy_(gi)
        before = [p.detach().clone() for p in ps]
        state = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state.get(p, {}).items()} for p in ps]
        want, _, info = ref(before, g, state, gs=0.5, **kw)
        opt.step()
        r = opt.trust_ratios().double()
        assert [x == 1.0 for x in r.tolist()] == [len(s) <= 1 for s in SHAPES]       # 1-D: excluded
        for i, (p, q) in enumerate(zip(ps, want)):
            assert abs(r[i].item() - info["ratio"][i]) <= 5e-5 * info["ratio"][i]
            assert abs(opt.param_norms()[i].item() - info["wnorm"][i]) <= 1e-5 * info["wnorm"][i]
            assert abs(opt.update_norms()[i].item() - info["unorm"][i]) <= 1e-5 * info["unorm"][i]
            err = (p.detach().double() - q).abs()
            assert (err <= _bound(q, kw["lr"], info["ratio"][i], info["A"][i])).all(), (i, err.max().item())


def test_exclude_none_adapts_everything_and_state_dict_round_trips():
    from pytorch_distributed_nn_amd.optim import LARS
    init, grads = _tensors(4, torch.float32)
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    opt = LARS(ps, lr=0.1, weight_decay=1e-2, exclude=None)
    for p, g in zip(ps, grads[0]):
        p.grad = g.clone()
    opt.step()
    assert (opt.trust_ratios() < 1.0).all()
    sd = copy.deepcopy(opt.state_dict())        # load_state_dict would otherwise share the buffers
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = LARS(qs, lr=0.1, weight_decay=1e-2, exclude=None)
    opt2.load_state_dict(sd)
    for p, q, g in zip(ps, qs, grads[1]):
        p.grad.copy_(g)
        q.grad = g.clone()
    opt.step()
    opt2.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------------- tables, command line
def test_malformed_tables_raise():
    from pytorch_distributed_nn_amd.ops import kernels as K
    C = K.LW_CHUNK
    assert 4096 <= C <= 65536
    ok = K.LwTables([(0, 5, 0.1, True), (64, 2 * C + 5, 0.0, False)], 64 + 2 * C + 5, "cpu")
    assert (ok.nseg, ok.nchunk) == (2, 4) and ok.chunks[-1] == (64 + 2 * C, 1, 5)
    bad = [
        dict(segments=[], extent=10),                                              # no segment
        dict(segments=[(0, 0, 0.0, True)], extent=10),                             # empty segment
        dict(segments=[(0, 8, 0.0, True), (4, 8, 0.0, True)], extent=64),          # overlap
        dict(segments=[(64, 8, 0.0, True), (0, 8, 0.0, True)], extent=128),        # out of order
        dict(segments=[(0, 8, 0.0, True)], extent=7),                              # past the range
        dict(segments=[(-4, 8, 0.0, True)], extent=64),                            # negative offset
        dict(segments=[(0, 8, float("nan"), True)], extent=8),                     # weight decay not a number
        dict(segments=[(0, 8, 0.0, True)], extent=8, chunks=[(0, 0, 9)]),          # chunk leaves its segment
        dict(segments=[(0, 8, 0.0, True)], extent=8, chunks=[(0, 0, 4)]),          # segment not covered
        dict(segments=[(0, 8, 0.0, True)], extent=8, chunks=[(0, 0, 4), (5, 0, 3)]),   # gap
        dict(segments=[(0, 8, 0.0, True)], extent=8, chunks=[(0, 0, 8), (0, 1, 8)]),   # names a missing segment
        dict(segments=[(0, C + 1, 0.0, True)], extent=C + 1, chunks=[(0, 0, C + 1)]),  # chunk over LW_CHUNK
        dict(segments=[(0, 8, 0.0, True), (64, 8, 0.0, True)], extent=72, chunks=[(64, 1, 8), (0, 0, 8)]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            K.LwTables(device="cpu", **kw)


@pytest.mark.parametrize("argv", [["--optimizer", "lars"], ["--optimizer", "lamb"],
                                  ["--optimizer", "lars", "--trust-coef", "0.01"]])
def test_cli_ps_mode_refuses_the_layerwise_optimizers(argv):
    from pytorch_distributed_nn_amd import cli
    args = cli.parse_args(argv)
    with pytest.raises(SystemExit) as e:
        cli.check_mode_flags(args, "ps", 3)
    assert f"--optimizer {argv[1]}" in str(e.value)
    if "--trust-coef" in argv:
        assert "--trust-coef" in str(e.value)
    cli.check_mode_flags(args, "single", 1)                  # ... and only PS mode does
    cli.check_mode_flags(args, "ddp", 2)


def test_cli_trust_coef_needs_lars():
    from pytorch_distributed_nn_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--optimizer", "sgd", "--trust-coef", "0.01"])
    assert "--trust-coef" in str(e.value)
    assert cli.parse_args(["--optimizer", "lars", "--trust-coef", "0.01"]).trust_coef == 0.01
