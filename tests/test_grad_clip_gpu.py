"""Fused global-norm gradient clipping on the GPU: the deterministic norm kernels of optim.hip at their edge
shapes, the optimizers end to end against ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim``, and the routing
through Trainer / GraphedStep / DDP (no torch clip kernels, capturable, global across param groups)."""
import copy
import math

import pytest
import torch

from dist_utils import run_world

pytestmark = pytest.mark.gpu

SHAPES = [(64, 3, 3, 3), (64,), (10, 1000), (10,)]
# 512 blocks x 256 threads x 4 floats + 5: one float4 more than the grid holds, so a second grid-stride sweep
SIZES = [1, 3, 4, 255, 4099, 10007, 512 * 256 * 4 + 5]
# relative tolerance of the norm: at these sizes a thread adds <= ~16 squares serially, then an 8-level block tree,
# then the double finalize: < 32 roundings of 2^-24 on a sum of non-negative terms, < 2e-6 on the sum, 1e-6 on the
# root; 1e-5 leaves 10x
RTOL = 1e-5


def _bufs():
    from pytorch_distributed_nn_amd.ops import kernels as K
    ws = torch.full((K.CLIP_WS,), float("nan"), device="cuda")      # every partial that is read must have been written
    return ws, torch.full((3,), -7.0, device="cuda")


def _coef(norm, max_norm, dev=1.0):
    return dev * min(1.0, max_norm / (norm + 1e-6))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_norm_kernel_edge_shapes(n, off):
    from pytorch_distributed_nn_amd.ops import kernels as K
    g = torch.Generator().manual_seed(n)
    buf = torch.randn(n + 8, generator=g).cuda()
    x = buf[off:off + n]
    assert x.data_ptr() % 16 == 4 * off
    ref = x.double().pow(2).sum().sqrt().item()
    ws, out = _bufs()
    nparts = K.sumsq_partials(x, ws)
    assert nparts == min(max((n // 4 + 1 + 255) // 256, 1), 512)
    res = []
    for max_norm in (0.5 * ref, 2.0 * ref):                        # below and above the norm
        K.clip_coef(ws, nparts, max_norm, out)
        res.append((max_norm, out.cpu().tolist()))
    for max_norm, (norm, coef, bad) in res:
        print(f"n={n} off={off}: norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.2e} coef {coef!r}")
        assert abs(norm - ref) <= RTOL * ref
        assert bad == 0.0
        if max_norm > ref:
            assert coef == 1.0
        else:
            want = _coef(ref, max_norm)
            assert abs(coef - want) <= RTOL * want


def test_norm_kernel_zero_gradient_and_empty():
    from pytorch_distributed_nn_amd.ops import kernels as K
    ws, out = _bufs()
    nparts = K.sumsq_partials(torch.zeros(4099, device="cuda"), ws)
    K.clip_coef(ws, nparts, 1.0, out)
    assert out.cpu().tolist() == [0.0, 1.0, 0.0]
    ws, out = _bufs()
    # n == 0 (torch gives an empty tensor a null address, so through the entry point): one partial of 0
    from pytorch_distributed_nn_amd.ops import _backend
    ones = torch.ones(8, device="cuda")
    assert _backend.lib().pdnn_sumsq_partials(ones.data_ptr(), 0, ws.data_ptr(), 0, _backend.stream()) == 1
    K.clip_coef(ws, 1, 1.0, out)
    assert out.cpu().tolist() == [0.0, 1.0, 0.0]


def test_norm_kernel_repeatable():
    from pytorch_distributed_nn_amd.ops import kernels as K
    x = torch.randn(10007, generator=torch.Generator().manual_seed(1)).cuda()
    outs = []
    for _ in range(5):
        ws, out = _bufs()
        K.clip_coef(ws, K.sumsq_partials(x, ws), 1.0, out)
        outs.append(out.clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])              # bitwise


def test_norm_over_several_ranges_is_global():
    from pytorch_distributed_nn_amd.ops import kernels as K
    x = torch.randn(30000, generator=torch.Generator().manual_seed(2)).cuda()
    ws, out = _bufs()
    n = 0
    for a, b in ((0, 4099), (4099, 4100), (4100, 30000)):
        n += K.sumsq_partials(x[a:b], ws, n)
    K.clip_coef(ws, n, 1.0, out)
    ref = x.double().norm().item()
    assert abs(out[0].item() - ref) <= RTOL * ref


def test_scale_folding_and_sgd_step():
    from pytorch_distributed_nn_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(10007, generator=gen).cuda()
    p = torch.randn(10007, generator=gen).cuda()
    dev = torch.tensor([0.25], device="cuda")
    ref = g.double().norm().item()
    ws, out = _bufs()
    max_norm = 2.0
    K.clip_coef(ws, K.sumsq_partials(g, ws), max_norm, out, gscale=0.5, dev_scale=dev)
    norm, coef, bad = out.cpu().tolist()
    assert abs(norm - 0.125 * ref) <= RTOL * 0.125 * ref and bad == 0.0
    want = _coef(0.125 * ref, max_norm, dev=0.25)
    assert want < 0.25 and abs(coef - want) <= RTOL * want
    # the update kernel multiplies the coefficient by its by-value gscale: a torch step on 0.125 g, clipped by torch
    q = torch.nn.Parameter(p.clone())
    q.grad = 0.125 * g
    torch.nn.utils.clip_grad_norm_([q], max_norm)
    topt = torch.optim.SGD([q], lr=0.1)
    topt.step()
    K.sgd_step(p, g, None, None, 0.1, 0.0, 0.0, 0.0, False, gscale_dev=out[1:2], gscale=0.5)
    assert torch.allclose(p, q.detach(), atol=1e-6, rtol=0)


def test_one_nan_element():
    from pytorch_distributed_nn_amd.ops import kernels as K
    x = torch.randn(10007, generator=torch.Generator().manual_seed(4)).cuda()
    x[5003] = float("nan")
    ws, out = _bufs()
    K.clip_coef(ws, K.sumsq_partials(x, ws), 1.0, out)
    norm, coef, bad = out.cpu().tolist()
    assert bad == 1.0 and math.isnan(norm) and math.isnan(coef)
    x[5003] = float("inf")
    K.clip_coef(ws, K.sumsq_partials(x, ws), 1.0, out)
    norm, coef, bad = out.cpu().tolist()
    assert bad == 1.0 and norm == float("inf") and coef == 0.0


def test_guarded_entries_do_not_launch():
    from pytorch_distributed_nn_amd.ops import _backend, kernels as K
    L = _backend.lib()
    x = torch.randn(10007, device="cuda")
    ws = torch.full((K.CLIP_WS,), 3.0, device="cuda")
    out = torch.full((3,), -7.0, device="cuda")
    st = _backend.stream()
    assert L.pdnn_sumsq_partials(None, 10, ws.data_ptr(), 0, st) < 0             # null gradient
    assert L.pdnn_sumsq_partials(x.data_ptr(), 10, None, 0, st) < 0              # null workspace
    assert L.pdnn_sumsq_partials(x.data_ptr(), -1, ws.data_ptr(), 0, st) < 0     # negative n
    assert L.pdnn_sumsq_partials(x.data_ptr(), 10007, ws.data_ptr(), K.CLIP_WS - 9, st) < 0   # 10 partials, 9 left
    assert L.pdnn_sumsq_partials(x.data_ptr(), 10, ws.data_ptr(), -1, st) < 0
    with pytest.raises(_backend.HipError):
        _backend.call("pdnn_clip_coef", None, 4, 1.0, 1.0, None, out.data_ptr(), st)
    with pytest.raises(_backend.HipError):
        _backend.call("pdnn_clip_coef", ws.data_ptr(), K.CLIP_WS + 1, 1.0, 1.0, None, out.data_ptr(), st)
    with pytest.raises(ValueError):
        K.sumsq_partials(x, ws[:100])                                            # undersized workspace
    with pytest.raises(ValueError):
        K.sumsq_partials(x, ws, K.CLIP_WS - 9)
    with pytest.raises(ValueError):
        K.sumsq_partials(x.double(), ws)
    with pytest.raises(ValueError):
        K.sumsq_partials(x.cpu(), ws)
    with pytest.raises(ValueError):
        K.clip_coef(ws, 4, 1.0, out[:2])
    torch.cuda.synchronize()
    assert torch.equal(ws, torch.full_like(ws, 3.0)) and torch.equal(out, torch.full_like(out, -7.0))


# ------------------------------------------------------------------------------------------- optimizers end to end
def _arena(seed=0):
    from pytorch_distributed_nn_amd.optim.flat import FlatParams
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=gen) * 0.1 for s in SHAPES]
    grads = [torch.randn(*s, generator=gen).cuda() for s in SHAPES]      # norm ~ 109 >> 1
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    fp = FlatParams(ps)
    refs = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    return fp, ps, refs, grads


def _set_grads(ps, refs, grads):
    for p, q, g in zip(ps, refs, grads):
        p.grad.copy_(g)
        q.grad = g.clone()


def _check_params(fp, ps, refs):
    for p, q in zip(ps, refs):
        assert torch.allclose(p.detach(), q.detach(), atol=1e-6, rtol=0), (p - q).abs().max().item()
    assert ((fp.shadow.float() - fp.data).norm() / fp.data.norm()).item() < 5e-3


@pytest.mark.parametrize("opt_name", ["sgd", "adamw"])
def test_optimizers_match_torch_clip(opt_name):
    from pytorch_distributed_nn_amd.optim import SGD, AdamW
    fp, ps, refs, grads = _arena()
    if opt_name == "sgd":
        kw = dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
        opt, ropt = SGD(ps, **kw), torch.optim.SGD(refs, **kw)
    else:
        kw = dict(lr=1e-3, weight_decay=0.1)
        opt, ropt = AdamW(ps, **kw), torch.optim.AdamW(refs, **kw)
    opt.set_grad_clip(1.0)
    assert opt._group_flat(0, opt.param_groups[0])[0] is fp
    for _ in range(3):
        _set_grads(ps, refs, grads)
        g_before = fp.grad.clone()
        tn = torch.nn.utils.clip_grad_norm_(refs, 1.0)
        ropt.step()
        opt.step()
        assert torch.equal(fp.grad, g_before)                    # only read: not torch's in-place clip
        assert abs(opt.grad_norm.item() - tn.item()) <= 1e-5 * tn.item()
        assert opt.grad_nonfinite.item() == 0.0
        _check_params(fp, ps, refs)


def test_two_groups_share_the_global_norm():
    from pytorch_distributed_nn_amd.optim import SGD
    fp, ps, refs, grads = _arena(1)
    mk = lambda t, c: c([{"params": t[:2], "weight_decay": 1e-2}, {"params": t[2:], "weight_decay": 0.0}],  # noqa: E731
                        lr=0.05, momentum=0.9)
    opt, ropt = mk(ps, SGD), mk(refs, torch.optim.SGD)
    opt.set_grad_clip(1.0)
    assert [opt._group_flat(i, g)[0] for i, g in enumerate(opt.param_groups)] == [fp, fp]
    for _ in range(3):
        _set_grads(ps, refs, grads)
        tn = torch.nn.utils.clip_grad_norm_(refs, 1.0)               # over ALL parameters
        ropt.step()
        opt.step()
        assert abs(opt.grad_norm.item() - tn.item()) <= 1e-5 * tn.item()
        _check_params(fp, ps, refs)


def test_clipping_off_is_bit_identical():
    """set_grad_clip(None) after a clipped step: the following steps equal, bit for bit, those of an optimizer that
    never had clipping and starts from the same weights and momentum."""
    from pytorch_distributed_nn_amd.optim import SGD
    fa, pa, _, grads = _arena(2)
    fb, pb, _, _ = _arena(2)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    oa, ob = SGD(pa, **kw), SGD(pb, **kw)
    for p, g in zip(pa + pb, grads + grads):
        p.grad.copy_(g)
    oa.set_grad_clip(1.0)
    oa.step()                                    # clipped
    ob.step()                                    # unclipped: creates ob's momentum buffer
    assert not torch.equal(fa.data, fb.data)
    fb.data.copy_(fa.data)
    fb.shadow.copy_(fa.shadow)
    ob.state["flat0"]["momentum_buffer"].copy_(oa.state["flat0"]["momentum_buffer"])
    oa.set_grad_clip(None)
    for _ in range(2):
        oa.step()
        ob.step()
        assert torch.equal(fa.data, fb.data) and torch.equal(fa.shadow, fb.shadow)
        assert torch.equal(oa.state["flat0"]["momentum_buffer"], ob.state["flat0"]["momentum_buffer"])


# ------------------------------------------------------------------------------------------- routing
def _lenets(n, lr=0.05):
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.optim import SGD, flatten_module
    torch.manual_seed(0)
    m0 = build_model("LeNet", 10)
    ms = [copy.deepcopy(m0).cuda() for _ in range(n)]
    for m in ms:
        flatten_module(m)
    return ms, [SGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4) for m in ms]


def _no_torch_clip(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("torch.nn.utils.clip_grad_norm_ called: the fused optimizer must clip")
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", boom)


def test_trainer_routes_to_fused_clip(monkeypatch):
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.trainer import Trainer
    _no_torch_clip(monkeypatch)
    (m,), (o,) = _lenets(1)
    tr = Trainer(m, o, OF.cross_entropy, torch.device("cuda"), log_interval=1, printer=lambda *a: None, grad_clip=0.5)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(32, 1, 28, 28, generator=g).cuda(), torch.randint(0, 10, (32,), generator=g).cuda()
    hist = tr.train(iter([(x, y)] * 3), epochs=1, max_steps=3, steps_per_epoch=3)
    assert len(hist) == 3 and o._clip == 0.5
    assert all(h["grad_norm"] > 0 and math.isfinite(h["grad_norm"]) for h in hist), hist
    assert hist[-1]["loss"] < hist[0]["loss"]


def _copy_state(dst_m, dst_o, src_m, src_o):
    dst_m._pdnn_flat.data.copy_(src_m._pdnn_flat.data)
    dst_m._pdnn_flat.refresh_shadow()
    dst = dst_o.state.setdefault("flat0", {})
    for k, v in src_o.state.get("flat0", {}).items():
        if torch.is_tensor(v) and k in dst:
            dst[k].copy_(v)
        else:
            dst[k] = v.clone() if torch.is_tensor(v) else v


def test_graphed_step_captures_the_fused_clip(monkeypatch):
    """Warm-up, capture and three replays with grad_clip: every replay equals an eager clipped step from the same
    state within test_graphs_gpu.py's replay-versus-eager bound, and the norm in device memory follows the batch.

    The state in front of every call (weights, momentum) and its result are recorded while the graphed model runs
    on its own; the eager clipped steps from those states (two copies: their disagreement is the noise floor of
    the bound) run afterwards."""
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.utils.graphs import GraphedStep
    _no_torch_clip(monkeypatch)
    (me, me2, mg), (oe, oe2, og) = _lenets(3)
    for o in (oe, oe2):
        o.set_grad_clip(0.5)
    gs = GraphedStep(mg, og, loss_fn=OF.cross_entropy, warmup=2, grad_clip=0.5)
    g = torch.Generator().manual_seed(2)
    rec = []
    for i in range(5):
        x, y = torch.randn(32, 1, 28, 28, generator=g).cuda(), torch.randint(0, 10, (32,), generator=g).cuda()
        before = mg._pdnn_flat.data.clone()
        mom = og.state.get("flat0", {}).get("momentum_buffer")
        mom = None if mom is None else mom.clone()
        gs(x, y)
        torch.cuda.synchronize()
        rec.append((x, y, before, mom, mg._pdnn_flat.data.clone(), og.grad_norm.item(), gs.replays))
    assert gs.graph is not None and gs.replays == 3
    assert [r[6] for r in rec] == [0, 0, 1, 2, 3]

    def eager_from(m, o, x, y, before, mom):
        m._pdnn_flat.data.copy_(before)
        m._pdnn_flat.refresh_shadow()
        o.state.setdefault("flat0", {})["momentum_buffer"] = mom.clone()
        o.zero_grad()
        OF.cross_entropy(m(x), y).backward()
        o.step()

    norms = []
    for i, (x, y, before, mom, after, ng, _) in enumerate(rec):
        if i < 2:
            continue                                              # the eager warm-up calls
        eager_from(me, oe, x, y, before, mom)
        eager_from(me2, oe2, x, y, before, mom)
        torch.cuda.synchronize()
        de = (me._pdnn_flat.data - before).norm()
        noise = ((me2._pdnn_flat.data - me._pdnn_flat.data).norm() / de).item()
        err = ((after - me._pdnn_flat.data).norm() / de).item()
        ne = oe.grad_norm.item()
        print(f"step {i}: replay-vs-eager {err:.2e}, eager-vs-eager {noise:.2e}, norm {ne:.6f} / {ng:.6f}")
        assert err < 3 * noise + 2e-3, (i, err, noise)
        assert ne > 0.5 and abs(ne - ng) <= 2e-3 * ne, (ne, ng)     # the clip is active, the norm this batch's
        norms.append(ng)
    assert len(set(norms)) == 3, norms                            # changes between replays as the gradient does


# ------------------------------------------------------------------------------------------- DDP, one rank on RCCL
def _ddp_job(rank, world):
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim import SGD, flatten_module
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    from pytorch_distributed_nn_amd.trainer import Trainer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m0 = build_model("LeNet", 10).to(dev)
    ma, mb, md = copy.deepcopy(m0), copy.deepcopy(m0), copy.deepcopy(m0)
    flatten_module(ma)
    flatten_module(mb)
    net = DistributedDataParallel(md, bucket_cap_mb=0.1, first_bucket_cap_mb=0.02)
    assert net._comm and net.nccl and len(net.buckets) >= 2
    opts = [SGD(m.parameters(), lr=0.05, momentum=0.9) for m in (ma, mb, md)]
    for o in opts:
        o.set_grad_clip(0.5)
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
    norms = [o.grad_norm.item() for o in opts]
    od = opts[2]
    declined = net.overlap_optimizer(od) is None              # clipping set: the per-bucket update declines
    od.set_grad_clip(None)
    accepted = net.overlap_optimizer(od) is od                # ... and it was the clipping that made it decline
    tr = Trainer(net, od, OF.cross_entropy, dev, printer=lambda *a: None, grad_clip=0.5)
    try:
        tr.step(x, y)
        raised = False
    except ValueError:
        raised = True
    torch.cuda.synchronize()
    return err, noise, moved, norms, declined, accepted, raised


def test_ddp_single_rank_rehearsal_clips_like_unwrapped():
    err, noise, moved, norms, declined, accepted, raised = run_world(
        _ddp_job, 1, (), timeout=150, device=None, backend="nccl",
        env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})[0]
    assert moved > 0 and norms[0] > 0.5
    assert err < 3 * noise + 1e-3 * moved, (err, noise, moved)
    assert abs(norms[2] - norms[0]) <= 3 * abs(norms[1] - norms[0]) + 1e-3 * norms[0], norms
    assert declined and accepted and raised
