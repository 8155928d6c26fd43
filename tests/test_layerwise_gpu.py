"""The layer-wise optimizers on the GPU (optim_layerwise.hip): per-segment norms and trust ratios, every element of
the update, the padding between parameters, the unit-ratio / clamp / NaN cases, the guarded entry points, and the
routing through Trainer / GraphedStep / DDP / the command line.  The reference is layerwise_ref.py (fp64, anchored to
torch.optim in test_layerwise_ref_cpu.py), always run from the GPU's own pre-step state so errors do not compound."""
import copy
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from dist_utils import run_world
from layerwise_ref import lamb_step_ref, lars_step_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# relative tolerance of a norm, by test_grad_clip_gpu.py's count: a chunk is LW_CHUNK = 16384 elements on 256 threads,
# so a thread adds 16 float4 sums of squares serially (each a 2-level tree of 4 squares), then the 8-level block tree,
# then the chunk partials in double: < 32 roundings of 2^-24 on a sum of non-negative terms, < 2e-6 on the sum, 1e-6 on
# the root; 1e-5 leaves 10x
NORM_RTOL = 1e-5
# two norms at 1e-5 each, under 1e-6 for the fp32 formula, and a factor of 2
RATIO_RTOL = 5e-5


def _edge_shapes():
    from pytorch_distributed_nn_amd.ops.kernels import LW_CHUNK as C
    assert C % 2 == 0 and C >= 4096
    # numel 1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 2 C + 5, and a conv weight (channels-last in the arena)
    return [(1,), (3,), (2, 2), (63,), (8, 8), (5, 13), (C - 1,), (2, C // 2), (C + 1,), (2 * C + 5,), (8, 3, 3, 3)]


SMALL = [(8, 3, 3, 3), (64,), (10, 1000), (10,), (5, 13)]


def _arena(shapes, seed=0, scale=0.1):
    from pytorch_distributed_nn_amd.optim.flat import FlatParams
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(*s, generator=gen) * scale).cuda()) for s in shapes]
    fp = FlatParams(ps)
    grads = [torch.randn(fp.numel, generator=gen).cuda() for _ in range(3)]
    return fp, ps, grads


def _make(name, ps, **over):
    from pytorch_distributed_nn_amd.optim import LAMB, LARS
    if name == "lamb":
        kw = dict(lr=1e-2, weight_decay=0.1)
        kw.update(over)
        return LAMB(ps, **kw), lamb_step_ref
    kw = dict(lr=0.5, momentum=0.9, weight_decay=1e-2, nesterov=name == "lars_nesterov", trust_coef=0.02)
    kw.update(over)
    return LARS(ps, **kw), lars_step_ref


_REF_KEYS = {"lars": ("lr", "momentum", "dampening", "weight_decay", "nesterov", "trust_coef", "eps", "clamp"),
             "lamb": ("lr", "betas", "eps", "weight_decay", "clamp")}


def _snapshot(fp, opt, gi=0):
    """The GPU's own state in front of a step: per parameter of group gi its arena slices (weights, gradient, state)."""
    group = opt.param_groups[gi]
    s, _ = opt._group_flat(gi, group)[1]
    st = opt.state.get(f"flat{gi}", {})
    items = []
    for p in group["params"]:
        o, n = fp.offsets[p._pdnn_flat_idx], p.numel()
        state = {k: st[k][o - s:o - s + n].clone() for k in ("momentum_buffer", "exp_avg", "exp_avg_sq") if k in st}
        if "step" in st:
            state["step"] = st["step"]
        items.append(dict(o=o, n=n, w=fp.data[o:o + n].clone(), g=fp.grad[o:o + n].clone(), state=state,
                          excluded=opt._excluded(p)))
    return items


def _ref(opt, ref, items, gi=0, gs=1.0):
    group = opt.param_groups[gi]
    kw = {k: group[k] for k in _REF_KEYS["lamb" if ref is lamb_step_ref else "lars"]}
    ws = [it["w"] for it in items]
    ex = {id(w): it["excluded"] for w, it in zip(ws, items)}
    return ref(ws, [it["g"] for it in items], [it["state"] for it in items], exclude=lambda t: ex[id(t)], gs=gs, **kw)


def _check_norms(opt, info, gi=0, skip=()):
    r, wn, un = (v.double().cpu() for v in (opt.trust_ratios(gi), opt.param_norms(gi), opt.update_norms(gi)))
    worst = 0.0
    for i in range(len(info["ratio"])):
        if i in skip:
            continue
        for got, want, tol in ((wn[i].item(), info["wnorm"][i], NORM_RTOL), (un[i].item(), info["unorm"][i], NORM_RTOL),
                               (r[i].item(), info["ratio"][i], RATIO_RTOL)):
            assert math.isfinite(got) and abs(got - want) <= tol * abs(want), (i, got, want, tol)
            worst = max(worst, abs(got - want) / (tol * abs(want)) if want else 0.0)
    print(f"  norms / ratios: worst error {worst:.3f} of the bound over {len(info['ratio'])} segments")
    return r


def _bound(ref, scale, A):
    """2^-22 |ref| + 1e-4 scale A: the final rounding with 2x margin, plus the ratio's error and the chain's < 16
    roundings of 2^-24, each relative to an operand bounded by A, with 2x margin."""
    return 2.0 ** -22 * ref.abs() + 1e-4 * scale * A


def _check_step(fp, opt, items, out, gi=0, skip=(), label=""):
    want, wstate, info = out
    group = opt.param_groups[gi]
    s, _ = opt._group_flat(gi, group)[1]
    st = opt.state[f"flat{gi}"]
    lr = group["lr"]
    for i, it in enumerate(items):
        if i in skip:
            continue
        o, n, r = it["o"], it["n"], info["ratio"][i]
        checks = [("p", fp.data[o:o + n], want[i], _bound(want[i], lr * r, info["A"][i]))]
        if "momentum_buffer" in wstate[i]:
            b = wstate[i]["momentum_buffer"]
            checks.append(("buf", st["momentum_buffer"][o - s:o - s + n], b, _bound(b, r, info["A_buf"][i])))
        if "exp_avg" in wstate[i]:
            checks.append(("m", st["exp_avg"][o - s:o - s + n], wstate[i]["exp_avg"], 2.0 ** -21 * info["A_m"][i]))
            checks.append(("v", st["exp_avg_sq"][o - s:o - s + n], wstate[i]["exp_avg_sq"],
                           2.0 ** -21 * info["A_v"][i]))
        line = []
        for nm, got, ref, bound in checks:
            err = (got.double() - ref).abs()
            rel = (err / bound.clamp_min(1e-300)).max().item()
            line.append(f"{nm} {rel:.3f}")
            assert (err <= bound).all(), (label, i, nm, n, rel)
        print(f"  {label} n={n:6d} r={r:.3e}: worst error / bound  " + "  ".join(line))
    # the bf16 shadow, as test_grad_clip_gpu._check_params checks it
    assert ((fp.shadow.float() - fp.data).norm() / fp.data.norm()).item() < 5e-3


# ------------------------------------------------------------------------------------------- kernels per segment
@pytest.mark.parametrize("name", ["lars", "lars_nesterov", "lamb"])
def test_edge_segments_norms_ratios_and_every_element(name):
    fp, ps, grads = _arena(_edge_shapes())
    opt, ref = _make(name, ps, exclude=None)
    assert opt._group_flat(0, opt.param_groups[0])[0] is fp
    for step, g in enumerate(grads):
        fp.grad.copy_(g)
        items = _snapshot(fp, opt)
        out = _ref(opt, ref, items)
        opt.step()
        print(f"{name} step {step}")
        r = _check_norms(opt, out[2])
        assert (r != 1.0).all()                                   # exclude=None: every segment is adapted
        _check_step(fp, opt, items, out, label=name)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_padding_is_neither_read_nor_written(name):
    fp, ps, grads = _arena(_edge_shapes(), seed=1)
    opt, ref = _make(name, ps, exclude=None)
    fp.grad.copy_(grads[0])
    opt.step()                                                    # creates the state buffers
    pad = torch.ones(fp.numel, dtype=torch.bool, device="cuda")
    for p, o in zip(fp.params, fp.offsets):
        pad[o:o + p.numel()] = False
    assert pad.sum().item() > 100
    st = opt.state["flat0"]
    bufs = [fp.data, fp.shadow] + [v for v in st.values() if torch.is_tensor(v)]
    assert len(bufs) == (3 if name == "lars" else 4)
    fp.grad.copy_(grads[1])
    fp.grad[pad] = float("nan")
    for b in bufs:
        b[pad] = -7.0
    g_before = fp.grad.clone()
    items = _snapshot(fp, opt)
    out = _ref(opt, ref, items)
    opt.step()
    _check_norms(opt, out[2])                                     # finite and correct: no padding in any norm
    _check_step(fp, opt, items, out, label=name)
    for b in bufs:
        assert torch.equal(b[pad], torch.full_like(b[pad], -7.0))  # bit-unchanged
    assert torch.equal(fp.grad.view(torch.int32), g_before.view(torch.int32))


def _unit_case(name, wd):
    shapes = [(5, 13), (7, 9), (65,), (10, 100)]                  # zero gradient | zero weight | excluded | ordinary
    fp, ps, grads = _arena(shapes, seed=2)
    opt, ref = _make(name, ps, weight_decay=wd)
    fp.grad.copy_(grads[0])
    offs = fp.offsets
    fp.grad[offs[0]:offs[0] + 65] = 0.0
    fp.data[offs[1]:offs[1] + 63] = 0.0
    fp.grad[offs[2]:offs[2] + 65] = 0.0
    fp.refresh_shadow()
    before = fp.data.clone()
    items = _snapshot(fp, opt)
    out = _ref(opt, ref, items)
    opt.step()
    return fp, opt, items, out, before


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_unit_ratio_cases(name):
    # LAMB's "other norm" is that of u = m^/(sqrt(v^) + eps) + wd w, which a zero gradient makes zero only without
    # weight decay: its zero-gradient segment is checked at weight_decay 0, the excluded one at 0.1 like LARS's
    fp, opt, items, out, before = _unit_case(name, 0.1 if name == "lars" else 0.0)
    r = opt.trust_ratios().cpu().tolist()
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == 1.0 and r[3] != 1.0, r
    assert out[2]["ratio"][:3] == [1.0, 1.0, 1.0]
    _check_step(fp, opt, items, out, label=name)
    fp, opt, items, out, before = _unit_case(name, 0.1)
    o = fp.offsets[2]
    assert opt.trust_ratios()[2].item() == 1.0
    assert torch.equal(fp.data[o:o + 65], before[o:o + 65])       # excluded, zero gradient, weight decay set: untouched
    assert not torch.equal(fp.data[fp.offsets[3]:], before[fp.offsets[3]:])


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_clamp_caps_the_ratio_at_one(name):
    fp, ps, grads = _arena(SMALL, seed=3, scale=30.0 if name == "lamb" else 0.1)
    over = dict(clamp=True, exclude=None)
    if name == "lars":
        over["trust_coef"] = 50.0
    opt, ref = _make(name, ps, **over)
    fp.grad.copy_(grads[0])
    items = _snapshot(fp, opt)
    opt.param_groups[0]["clamp"] = False
    free = _ref(opt, ref, items)[2]["ratio"]
    opt.param_groups[0]["clamp"] = True
    out = _ref(opt, ref, items)
    assert all(x > 1.0 for x in free), free                       # the unclamped reference ratios all exceed 1
    opt.step()
    assert opt.trust_ratios().cpu().tolist() == [1.0] * len(SMALL)
    _check_step(fp, opt, items, out, label=name)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_one_nan_stays_in_its_segment(name):
    fp, ps, grads = _arena(_edge_shapes(), seed=4)
    opt, ref = _make(name, ps, exclude=None)
    fp.grad.copy_(grads[0])
    bad = 8                                                       # the C + 1 segment: two chunks
    o, n = fp.offsets[bad], fp.params[bad].numel()
    fp.grad[o + n - 1] = float("nan")                             # in its second chunk
    items = _snapshot(fp, opt)
    out = _ref(opt, ref, items)
    opt.step()
    assert math.isnan(opt.trust_ratios()[bad].item())
    assert torch.isnan(fp.data[o:o + n]).all()
    _check_norms(opt, out[2], skip=(bad,))
    others = [it for i, it in enumerate(items) if i != bad]
    assert all(torch.isfinite(fp.data[it["o"]:it["o"] + it["n"]]).all() for it in others)
    fp.data[o:o + n] = 0.0                                        # keep the shadow norm of _check_step finite
    fp.shadow[o:o + n] = 0.0
    _check_step(fp, opt, items, out, skip=(bad,), label=name)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_repeatable_bitwise(name):
    fp, ps, grads = _arena(_edge_shapes(), seed=5)
    opt, _ = _make(name, ps, exclude=None)
    fp.grad.copy_(grads[0])
    opt.step()
    fp.grad.copy_(grads[1])
    st = opt.state["flat0"]
    keep = [fp.data.clone()] + [v.clone() for v in st.values() if torch.is_tensor(v)]
    step0 = st.get("step")
    res = []
    for _ in range(5):
        fp.data.copy_(keep[0])
        for v, k in zip([v for v in st.values() if torch.is_tensor(v)], keep[1:]):
            v.copy_(k)
        if step0 is not None:
            st["step"] = step0
        opt.step()
        res.append([fp.data.clone(), fp.shadow.clone(), opt.trust_ratios().clone()] +
                   [v.clone() for v in st.values() if torch.is_tensor(v)])
    for other in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], other))


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_two_param_groups_on_one_arena(name):
    from pytorch_distributed_nn_amd.optim import LAMB, LARS
    fp, ps, grads = _arena(SMALL, seed=6)
    groups = [{"params": ps[:2], "lr": 0.3 if name == "lars" else 2e-2, "weight_decay": 1e-2},
              {"params": ps[2:], "weight_decay": 0.2}]
    if name == "lars":
        opt, ref = LARS(groups, lr=0.7, momentum=0.9, trust_coef=0.02), lars_step_ref
    else:
        opt, ref = LAMB(groups, lr=1e-2), lamb_step_ref
    assert [opt._group_flat(i, g)[0] for i, g in enumerate(opt.param_groups)] == [fp, fp]
    for g in grads[:2]:
        fp.grad.copy_(g)
        snaps = [_snapshot(fp, opt, gi) for gi in (0, 1)]
        outs = [_ref(opt, ref, snaps[gi], gi) for gi in (0, 1)]
        opt.step()
        for gi in (0, 1):
            _check_norms(opt, outs[gi][2], gi)
            _check_step(fp, opt, snaps[gi], outs[gi], gi, label=f"{name} group {gi}")
    assert len(opt.trust_ratios(0)) == 2 and len(opt.trust_ratios(1)) == 3


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_scale_folding_with_the_fused_clip(name):
    fp, ps, grads = _arena(SMALL, seed=7)
    opt, ref = _make(name, ps)
    opt.grad_scale = 0.5
    opt.grad_scale_dev = torch.tensor([0.25], device="cuda")
    opt.set_grad_clip(1.0)
    for g in grads[:2]:
        fp.grad.copy_(g)
        g_before = fp.grad.clone()
        items = _snapshot(fp, opt)
        opt.step()
        coef = opt._clip_out[1].item()                            # grad_scale_dev * min(1, max_norm / (norm + 1e-6))
        norm = 0.125 * g.double().norm().item()                   # padding included: the clip is the flat kernel's
        assert norm > 1.0 and abs(coef - 0.25 / (norm + 1e-6)) <= 1e-5 * coef
        out = _ref(opt, ref, items, gs=0.5 * coef)                # the gradient as the update sees it
        _check_norms(opt, out[2])
        _check_step(fp, opt, items, out, label=name)
        assert torch.equal(fp.grad, g_before)


def test_guarded_entries_do_not_launch():
    from pytorch_distributed_nn_amd.ops import _backend, kernels as K
    L, st = _backend.lib(), _backend.stream()
    assert L.pdnn_lw_chunk() == K.LW_CHUNK
    n = 10007
    tab = K.LwTables([(0, 4099, 0.1, True), (4160, 5000, 0.0, False)], n, "cuda")
    x, g, m, v = (torch.full((n,), 3.0, device="cuda") for _ in range(4))
    sh = torch.full((n,), 3.0, device="cuda", dtype=torch.bfloat16)
    ws, out = torch.full((2 * tab.nchunk,), 3.0, device="cuda"), torch.full((3 * tab.nseg,), 3.0, device="cuda")
    P = lambda t: t.data_ptr()                                                        # noqa: E731
    sg, ck, ns, nc = P(tab.seg), P(tab.chk), tab.nseg, tab.nchunk

    def norm(p=P(x), gg=P(g), mm=None, vv=None, s=sg, c=ck, a=ns, b=nc, w=P(ws), lamb=0):
        return L.pdnn_lw_norm_partials(p, gg, mm, vv, s, c, a, b, w, lamb, 0.9, 0.999, 0.1, 0.001, 1e-6, 0.1, 0.001, None,
                                       1.0,
                                       None, st)

    def ratio(w=P(ws), s=sg, a=ns, b=nc, o=P(out)):
        return L.pdnn_lw_ratio(w, s, a, b, 0, 1e-3, 1e-8, 0, None, 1.0, o, st)

    def lars(p=P(x), gg=P(g), bb=P(m), s=sg, c=ck, a=ns, b=nc, r=P(out), mom=0.9, shd=P(sh)):
        return L.pdnn_lars_apply(p, gg, bb, shd, s, c, a, b, r, 0.1, mom, 0.0, 0, 0, None, 1.0, None, st)

    def lamb(p=P(x), mm=P(m), vv=P(v), s=sg, c=ck, a=ns, b=nc, r=P(out), shd=P(sh)):
        return L.pdnn_lamb_apply(p, mm, vv, shd, s, c, a, b, r, 0.1, 1e-6, 0.1, 0.001, None, st)

    rcs = [norm(p=None), norm(gg=None), norm(w=None), norm(s=None), norm(c=None), norm(a=0), norm(b=0), norm(a=-1),
           norm(p=P(x) + 4), norm(gg=P(g) + 4), norm(lamb=1), norm(lamb=1, mm=P(m), vv=P(v) + 4),
           ratio(w=None), ratio(s=None), ratio(o=None), ratio(a=0), ratio(b=0),
           lars(p=None), lars(gg=None), lars(bb=None), lars(r=None), lars(s=None), lars(c=None), lars(a=0), lars(b=-3),
           lars(p=P(x) + 4), lars(bb=P(m) + 8), lars(shd=P(sh) + 2),
           lamb(p=None), lamb(mm=None), lamb(vv=None), lamb(r=None), lamb(c=None), lamb(a=0), lamb(b=0),
           lamb(vv=P(v) + 4), lamb(shd=P(sh) + 4)]
    assert all(rc != 0 for rc in rcs), rcs
    with pytest.raises(ValueError):
        K.LwTables([(0, 4099, 0.1, True), (4096, 5000, 0.0, False)], n, "cuda")       # overlapping segments
    with pytest.raises(ValueError):
        K.LwTables([(0, 4099, 0.1, True)], n, "cuda", chunks=[(0, 0, 5000)])          # chunk leaves its segment
    with pytest.raises(ValueError):
        K.lw_norm_partials(x, g, tab, ws[:2 * nc - 1])                                # chunk count past the workspace
    with pytest.raises(ValueError):
        K.lw_norm_partials(x[:n - 1], g, tab, ws)                                     # range shorter than the tables'
    with pytest.raises(ValueError):
        K.lw_ratio(ws, tab, out[:5], False)
    with pytest.raises(ValueError):
        K.lars_apply(x, g, None, sh, tab, out[:ns], 0.1, 0.9, 0.0, False)             # momentum without a buffer
    with pytest.raises(ValueError):
        K.lamb_apply(x, m, v.double(), sh, tab, out[:ns], 0.1, 1e-6, 0.1, 0.001)
    with pytest.raises(ValueError):
        K.lw_norm_partials(x, g, (tab.seg, tab.chk), ws)                              # raw tensors are not tables
    torch.cuda.synchronize()
    for t in (x, g, m, v, ws, out):
        assert torch.equal(t, torch.full_like(t, 3.0))
    assert torch.equal(sh, torch.full_like(sh, 3.0))


# ------------------------------------------------------------------------------------------- routing
def _lenets(n, name):
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.optim import LAMB, LARS, flatten_module
    torch.manual_seed(0)
    m0 = build_model("LeNet", 10)
    ms = [copy.deepcopy(m0).cuda() for _ in range(n)]
    for m in ms:
        flatten_module(m)
    if name == "lars":
        return ms, [LARS(m.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-4, trust_coef=0.05) for m in ms]
    return ms, [LAMB(m.parameters(), lr=2e-3, weight_decay=0.01) for m in ms]


def test_trainer_lars_lowers_the_loss():
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.trainer import Trainer
    (m,), (o,) = _lenets(1, "lars")
    tr = Trainer(m, o, OF.cross_entropy, torch.device("cuda"), log_interval=1, printer=lambda *a: None)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(32, 1, 28, 28, generator=g).cuda(), torch.randint(0, 10, (32,), generator=g).cuda()
    hist = tr.train(iter([(x, y)] * 3), epochs=1, max_steps=3, steps_per_epoch=3)
    assert len(hist) == 3 and hist[-1]["loss"] < hist[0]["loss"], hist
    r = o.trust_ratios().cpu()
    nd = [p.ndim for p in o.param_groups[0]["params"]]
    assert all((x == 1.0) == (d <= 1) for x, d in zip(r.tolist(), nd)), (r, nd)       # biases: excluded by default


_STATE = ("momentum_buffer", "exp_avg", "exp_avg_sq")


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_graphed_step_replays_match_eager(name):
    """Warm-up, capture and three replays: every replay equals an eager step from the same recorded state within
    test_grad_clip_gpu.py's replay-versus-eager bound (two eager copies give the noise floor), and the trust ratios
    in device memory follow the batch."""
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.utils.graphs import GraphedStep
    (me, me2, mg), (oe, oe2, og) = _lenets(3, name)
    gs = GraphedStep(mg, og, loss_fn=OF.cross_entropy, warmup=2)
    g = torch.Generator().manual_seed(2)
    rec = []
    for i in range(5):
        x, y = torch.randn(32, 1, 28, 28, generator=g).cuda(), torch.randint(0, 10, (32,), generator=g).cuda()
        before = mg._pdnn_flat.data.clone()
        st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in og.state.get("flat0", {}).items()}
        gs(x, y)
        torch.cuda.synchronize()
        rec.append((x, y, before, st, mg._pdnn_flat.data.clone(), og.trust_ratios().clone(), gs.replays))
    assert gs.graph is not None and gs.replays == 3
    assert [r[6] for r in rec] == [0, 0, 1, 2, 3]

    def eager_from(m, o, x, y, before, st):
        m._pdnn_flat.data.copy_(before)
        m._pdnn_flat.refresh_shadow()
        o.state["flat0"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
        o.zero_grad()
        OF.cross_entropy(m(x), y).backward()
        o.step()

    ratios = []
    for i, (x, y, before, st, after, rg, _) in enumerate(rec):
        if i < 2:
            continue                                              # the eager warm-up calls
        eager_from(me, oe, x, y, before, st)
        eager_from(me2, oe2, x, y, before, st)
        torch.cuda.synchronize()
        de = (me._pdnn_flat.data - before).norm()
        noise = ((me2._pdnn_flat.data - me._pdnn_flat.data).norm() / de).item()
        err = ((after - me._pdnn_flat.data).norm() / de).item()
        re_ = oe.trust_ratios()
        print(f"{name} step {i}: replay-vs-eager {err:.2e}, eager-vs-eager {noise:.2e}")
        assert err < 3 * noise + 2e-3, (i, err, noise)
        assert torch.allclose(rg, re_, rtol=2e-3, atol=0), (rg, re_)
        ratios.append(rg)
    assert not torch.equal(ratios[0], ratios[1]) and not torch.equal(ratios[1], ratios[2])


def _ddp_job(rank, world):
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim import LARS, flatten_module
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m0 = build_model("LeNet", 10).to(dev)
    ma, mb, md = copy.deepcopy(m0), copy.deepcopy(m0), copy.deepcopy(m0)
    flatten_module(ma)
    flatten_module(mb)
    net = DistributedDataParallel(md, bucket_cap_mb=0.1, first_bucket_cap_mb=0.02)
    assert net._comm and net.nccl and len(net.buckets) >= 2
    opts = [LARS(m.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-4, trust_coef=0.05) for m in (ma, mb, md)]
    net.attach_optimizer(opts[2])
    declined = net.overlap_optimizer(opts[2]) is None
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(32, 1, 28, 28, generator=g).to(dev), torch.randint(0, 10, (32,), generator=g).to(dev)
    before = ma._pdnn_flat.data.clone()
    for m, o in ((ma, opts[0]), (mb, opts[1]), (net, opts[2])):
        o.zero_grad()
        OF.cross_entropy(m(x), y).backward()
        o.step()
    torch.cuda.synchronize()
    moved = (ma._pdnn_flat.data - before).norm().item()
    noise = (mb._pdnn_flat.data - ma._pdnn_flat.data).norm().item()
    err = (net.flat.data - ma._pdnn_flat.data).norm().item()
    return err, noise, moved, declined, opts[2].trust_ratios().cpu().tolist()


def test_ddp_single_rank_rehearsal_steps_like_unwrapped():
    err, noise, moved, declined, ratios = run_world(
        _ddp_job, 1, (), timeout=150, device=None, backend="nccl",
        env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})[0]
    assert moved > 0 and declined
    assert err < 3 * noise + 1e-3 * moved, (err, noise, moved)
    assert all(math.isfinite(r) and r > 0 for r in ratios)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_cli_runs_to_completion(name, tmp_path):
    m = tmp_path / "metrics.jsonl"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytorch_distributed_nn_amd.cli", "--network", "LeNet", "--synthetic",
                        "--optimizer", name, "--max-steps", "5", "--batch-size", "16", "--test-batch-size", "16",
                        "--log-interval", "1", "--metrics", str(m), "--out-dir", str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    recs = [json.loads(ln) for ln in open(m) if ln.strip()]
    assert len(recs) == 5 and all(math.isfinite(x["loss"]) for x in recs), recs
