"""DDP with the fused GPU ops (direct arena gradient accumulation + grad-ready hooks) in 2 processes that
share the box's GPU over gloo: the all-reduced gradients equal the average of the two ranks' local
gradients computed without DDP.  (The 8-GPU RCCL run is the driver's; this checks the hook/bucket logic
on the real fused backward.)"""
import copy
import os

import pytest
import torch

from dist_utils import kofn_step, run_world

pytestmark = pytest.mark.gpu


def _job(rank, world, arch):
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim.flat import flatten_module
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    torch.manual_seed(0)
    dev = torch.device("cuda")
    if arch == "gpt2_tiny":
        m = build_model("gpt2_tiny").to(dev)
        data = [torch.randint(0, 512, (2, 129), generator=torch.Generator().manual_seed(r)).to(dev) for r in range(world)]
        run = lambda net, d: net(d[:, :-1].contiguous(), d[:, 1:].contiguous())
    else:
        m = build_model("resnet50").to(dev)
        g = [torch.Generator().manual_seed(r) for r in range(world)]
        data = [(torch.randn(4, 3, 64, 64, generator=g[r]).to(dev), torch.randint(0, 1000, (4,), generator=g[r]).to(dev))
                for r in range(world)]
        run = lambda net, d: OF.cross_entropy(net(d[0]), d[1])
    ref = copy.deepcopy(m)
    fref = flatten_module(ref)
    net = DistributedDataParallel(m, bucket_cap_mb=4.0, first_bucket_cap_mb=0.5)
    net.zero_grad()
    run(net, data[rank]).backward()
    torch.cuda.synchronize()
    # reference: local gradients of every rank's batch, averaged, on an un-wrapped copy
    acc = torch.zeros_like(fref.grad)
    for r in range(world):
        fref.zero_grad()
        run(ref, data[r]).backward()
        acc += fref.grad
    acc /= world
    rel = ((net.flat.grad - acc).norm() / acc.norm()).item()
    return rel, len(net.buckets)


@pytest.mark.parametrize("arch", ["gpt2_tiny", "resnet50_small"])
def test_ddp_fused_backward_allreduce(arch):
    res = run_world(_job, 2, (arch,), timeout=600, device=None)
    for rel, nb in res:
        assert nb >= 2
        assert rel < 2e-3, rel


def _rccl_job(rank, world):
    """One rank over RCCL with communication forced on: the same hooks, buckets and RCCL AVG all-reduces
    (on RCCL's stream, overlapped with the fused backward) as the 8-GPU run, on the box's single GPU.
    The reference copy is re-synced to the DDP weights before every step: a random-init ResNet-50 at
    batch 4 is chaotic after a few SGD steps (5e-8 relative weight noise from split-K atomics -> tens of
    percent gradient difference, measured with tools/ddp_diag.py with and without communication)."""
    import torch.distributed as dist
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim import SGD
    from pytorch_distributed_nn_amd.optim.flat import flatten_module
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    torch.manual_seed(0)
    dev = torch.device("cuda")
    m = build_model("resnet50").to(dev)
    # damped residual branches (BN3 gain 0.1, as tests/test_trajectory_gpu.py): at batch 4 a random-init ResNet-50 is
    # chaotic -- the BN statistic bins' fp32 atomic order (~1e-9) can flip a ReLU mask and move the whole gradient by
    # 5e-3 (dev/probes/det_probe.py, det_trace.py: gpurun_out/r6_04-05), which says nothing about DDP
    with torch.no_grad():
        for mod in m.modules():
            if hasattr(mod, "bn3"):
                mod.bn3.weight.fill_(0.1)
    ref = copy.deepcopy(m)
    fref = flatten_module(ref)
    net = DistributedDataParallel(m, bucket_cap_mb=4.0, first_bucket_cap_mb=0.5)
    assert net._comm and net.nccl
    opt = SGD(m.parameters(), lr=0.01, momentum=0.9)
    g = torch.Generator().manual_seed(1)
    rels, moved = [], []
    for _ in range(3):
        fref.data.copy_(net.flat.data)
        fref.refresh_shadow()
        for b_ref, b in zip(ref.buffers(), m.buffers()):
            b_ref.copy_(b)
        x, y = torch.randn(4, 3, 64, 64, generator=g).to(dev), torch.randint(0, 1000, (4,), generator=g).to(dev)
        fref.zero_grad()
        OF.cross_entropy(ref(x), y).backward()
        before = net.flat.data.clone()
        opt.zero_grad()
        OF.cross_entropy(net(x), y).backward()
        opt.step()
        torch.cuda.synchronize()
        rels.append(((net.flat.grad - fref.grad).norm() / fref.grad.norm()).item())
        moved.append(((net.flat.data - before).norm() / before.norm()).item())
    return rels, moved, len(net.step_comm_log), len(net.buckets)


def test_ddp_rccl_single_rank_rehearsal():
    res = run_world(_rccl_job, 1, (), timeout=600, device=None, backend="nccl",
                    env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})
    rels, moved, ncomm, nb = res[0]
    assert ncomm == 3 and nb >= 2
    assert max(rels) < 1e-3, rels           # AVG over one rank passes gradients through (up to atomic-order drift)
    assert min(moved) > 0, moved


def _rccl_split_tied_job(rank, world):
    """One gpt2_tiny step with the tied wte gradient split (dense LM-head part in bucket 0, embedding rows added at
    the end of the backward by the embedding kernel with the position table absent) and one with it unsplit, from the
    same seed and batch, over RCCL at world 1."""
    import torch.distributed as dist
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    dev = torch.device("cuda")
    data = torch.randint(0, 512, (2, 129), generator=torch.Generator().manual_seed(4))
    data[:, 40:70] = 11                                   # repeated token ids: many rows into one wte row
    data[1, :20] = data[0, :20]
    data = data.to(dev)
    out = {}
    for split in (True, False):
        torch.manual_seed(0)
        m = build_model("gpt2_tiny").to(dev)
        net = DistributedDataParallel(m, bucket_cap_mb=0.25, split_tied=split)
        assert net._comm and net.nccl
        net.zero_grad()
        net(data[:, :-1].contiguous(), data[:, 1:].contiguous()).backward()
        torch.cuda.synchronize()
        wte = m.transformer.wte.weight
        out[split] = {"flat": net.flat.grad.clone(), "wte": wte.grad.clone(),
                      "wpe": m.transformer.wpe.weight.grad.clone(), "split": net._tail is not None,
                      "bucket": net._pbucket[id(wte)], "nb": len(net.buckets), "order": list(net.last_launch_order)}
    return out


def test_ddp_rccl_split_tied_embedding_matches_unsplit():
    """The embedding half of the tied wte gradient in its split form on the GPU kernels: flat gradient, wte.grad and
    wpe.grad equal the unsplit path's to 1e-4 relative L2 (the bound for the same gradient accumulated in another
    atomic order, as in test_gpt2_side_stream_weight_gradients), and the wte bucket is launched first."""
    res = run_world(_rccl_split_tied_job, 1, (), timeout=300, device=None, backend="nccl",
                    env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})[0]
    s, u = res[True], res[False]
    assert s["split"] and not u["split"]
    assert s["nb"] >= 2 and s["bucket"] == 0 and s["order"][0] == 0
    for k in ("flat", "wte", "wpe"):
        assert torch.isfinite(s[k]).all() and u[k].norm().item() > 0, k
        rel = ((s[k] - u[k]).norm() / u[k].norm()).item()
        assert rel <= 1e-4, (k, rel)


def _rccl_kofn_job(rank, world):
    """The k-of-n collective control plane on RCCL at world 1 (PDNN_FORCE_PG): store reports, watcher
    thread, host throttle against CUDA events, zero-fill path and the per-bucket count all-reduce."""
    import torch.distributed as dist
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim.flat import flatten_module
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    assert dist.get_backend() == "nccl"
    torch.manual_seed(0)
    dev = torch.device("cuda")
    m = build_model("resnet18", 10).to(dev)
    ref = copy.deepcopy(m)
    fref = flatten_module(ref)
    net = DistributedDataParallel(m, bucket_cap_mb=4.0, first_bucket_cap_mb=0.5, num_aggregate=1)
    x, y = torch.randn(8, 3, 32, 32, device=dev), torch.randint(0, 10, (8,), device=dev)
    out = []
    for _ in range(2):
        fref.data.copy_(net.flat.data)
        fref.refresh_shadow()
        fref.zero_grad()
        OF.cross_entropy(ref(x), y).backward()
        net.zero_grad()
        aborted = kofn_step(net, lambda: OF.cross_entropy(net(x), y))
        torch.cuda.synchronize()
        rel = ((net.flat.grad - fref.grad).norm() / fref.grad.norm()).item()
        out.append((aborted, rel, net.last_counts.cpu().tolist()))
    net.close()
    return out


def test_ddp_rccl_kofn_single_rank():
    res = run_world(_rccl_kofn_job, 1, (), timeout=600, device=None, backend="nccl",
                    env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})[0]
    for aborted, rel, counts in res:
        assert not aborted and rel < 1e-5 and all(c == 1.0 for c in counts), res


def _rccl_overlap_job(rank, world, opt_name):
    """overlap_optimizer: every bucket's update applied on the optimizer stream right after its all-reduce, during
    the backward.  Lockstep against the update after the backward: before each step the overlapped net is re-synced
    to the reference (weights, buffers, optimizer state); the updated weights must agree to the gradients' own
    run-to-run noise (fp32 atomics), and step() after an overlapped backward must not update a second time."""
    import torch.distributed as dist
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim import SGD, AdamW
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    assert dist.get_backend() == "nccl"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m0 = build_model("resnet18", 10).to(dev)
    nets = [DistributedDataParallel(copy.deepcopy(m0), bucket_cap_mb=4.0, first_bucket_cap_mb=0.5) for _ in range(3)]
    mk = (lambda m: SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)) if opt_name == "sgd" else \
        (lambda m: AdamW(m.parameters(), lr=1e-3, weight_decay=0.1))
    opts = [mk(n.module) for n in nets]
    (nr, nt, no), (orf, ot, oo) = nets, opts
    assert no.overlap_optimizer(oo) is oo
    g = torch.Generator().manual_seed(5)
    out = []
    for i in range(4):
        x = torch.randn(16, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (16,), generator=g).to(dev)
        if i >= 1:
            _sync_state(nt, ot, nr, orf)
            _sync_state(no, oo, nr, orf)
        before = nr.flat.data.clone()
        for n, o in ((nr, orf), (nt, ot), (no, oo)) if i >= 1 else ((nr, orf), (no, oo)):
            o.zero_grad()
            OF.cross_entropy(n(x), y).backward()
            o.step()
        torch.cuda.synchronize()
        if i >= 1:
            d_ref = (nr.flat.data - before).norm().item()
            noise = (nt.flat.data - nr.flat.data).norm().item()
            err = (no.flat.data - nr.flat.data).norm().item()
            out.append((err, noise, d_ref))
    return out


@pytest.mark.parametrize("opt_name", ["sgd", "adamw"])
def test_ddp_overlapped_optimizer_matches_step_after_backward(opt_name):
    res = run_world(_rccl_overlap_job, 1, (opt_name,), timeout=150, device=None, backend="nccl",
                    env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})[0]
    for err, noise, moved in res:
        assert moved > 0
        assert err < 3 * noise + 1e-3 * moved, res


def _sync_state(dst_net, dst_opt, src_net, src_opt):
    """dst := src (flat weights + bf16 shadow, BN buffers, momentum)."""
    dst_net.flat.data.copy_(src_net.flat.data)
    dst_net.flat.refresh_shadow()
    for bd, bs in zip(dst_net.module.buffers(), src_net.module.buffers()):
        bd.copy_(bs)
    dst = dst_opt.state.setdefault("flat0", {})
    for k, v in src_opt.state.get("flat0", {}).items():
        if torch.is_tensor(v) and k in dst:
            dst[k].copy_(v)
        else:
            dst[k] = v.clone() if torch.is_tensor(v) else v


def _rccl_graph_job(rank, world):
    """GraphedStep(allow_collectives=True) at world 1 over RCCL: the bucket all-reduces (and the buffer
    broadcast) are captured into the step's hipGraph.  Lockstep check: before every replay two eager DDP
    copies are re-synced to the graphed model; the replay's update must sit within the eager-vs-eager
    (fp32 atomics) floor of one step — a multi-step trajectory comparison of a BN net at batch 16 is chaotic
    even between two eager runs."""
    import torch.distributed as dist
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim import SGD
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    from pytorch_distributed_nn_amd.utils.graphs import GraphedStep
    assert dist.get_backend() == "nccl"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m0 = build_model("resnet18", 10).to(dev)
    nets = [DistributedDataParallel(copy.deepcopy(m0), bucket_cap_mb=4.0, first_bucket_cap_mb=0.5)
            for _ in range(3)]
    opts = [SGD(n.module.parameters(), lr=0.01, momentum=0.9) for n in nets]
    (na, nc, nb), (oa, oc, ob) = nets, opts
    gstep = GraphedStep(nb, ob, loss_fn=OF.cross_entropy, warmup=2, allow_collectives=True)
    g = torch.Generator().manual_seed(3)
    res = []
    for i in range(7):
        x = torch.randn(16, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (16,), generator=g).to(dev)
        if i >= 2:
            _sync_state(na, oa, nb, ob)
            _sync_state(nc, oc, nb, ob)
        before = nb.flat.data.clone()
        losses = []
        for n, o in ((na, oa), (nc, oc)) if i >= 2 else ((na, oa),):
            o.zero_grad()
            loss = OF.cross_entropy(n(x), y)
            loss.backward()
            o.step()
            losses.append(float(loss.detach()))
        lg = float(gstep(x, y))
        torch.cuda.synchronize()
        if i >= 2:
            de = (na.flat.data - before).norm()
            err = ((nb.flat.data - na.flat.data).norm() / de).item()
            noise = ((nc.flat.data - na.flat.data).norm() / de).item()
            res.append((i, err, noise, losses[0], lg))
    return res, gstep.replays


def test_graphed_step_captures_rccl_collectives():
    res, replays = run_world(_rccl_graph_job, 1, (), timeout=150, device=None, backend="nccl",
                             env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})[0]
    assert replays >= 4
    for i, err, noise, le, lg in res:
        assert err < 3 * noise + 2e-3, res
        assert abs(le - lg) < 1e-2 * max(1.0, abs(lg)), res


def _rccl_timing_job(rank, world):
    """comm_timing on RCCL at world 1: every bucket's all-reduce gets a device time (ready -> reduced), the
    exposed tail and the BN-buffer broadcast are measured, for the fp32 and the bf16 wire, and the timed
    collectives still produce the plain gradients."""
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    torch.manual_seed(0)
    dev = torch.device("cuda")
    m = build_model("resnet50").to(dev)
    net = DistributedDataParallel(m, bucket_cap_mb=8.0, first_bucket_cap_mb=1.0)
    x, y = torch.randn(8, 3, 64, 64, device=dev), torch.randint(0, 1000, (8,), device=dev)
    net.zero_grad()
    OF.cross_entropy(net(x), y).backward()
    plain = net.flat.grad.clone()
    out = {}
    for name, dt in (("fp32", None), ("bf16", torch.bfloat16)):
        net.set_comm_dtype(dt)
        net.comm_timing = True
        for _ in range(2):
            net.zero_grad()
            OF.cross_entropy(net(x), y).backward()
        torch.cuda.synchronize()
        net.comm_timing = False
        recs = net.comm_records()
        rel = ((net.flat.grad - plain).norm() / plain.norm()).item()
        out[name] = (recs, rel)
    return out, len(net.buckets)


def test_ddp_comm_timing_records():
    out, nb = run_world(_rccl_timing_job, 1, (), timeout=600, device=None, backend="nccl",
                        env={"PDNN_FORCE_PG": "1", "PDNN_DDP_FORCE_COMM": "1"})[0]
    for name, (recs, rel) in out.items():
        assert len(recs) == 2, name
        for r in recs:
            assert len(r["bucket_ms"]) == nb and all(0 <= v < 1e3 for v in r["bucket_ms"]), r
            assert all(d >= s for s, d in zip(r["bucket_ready_ms"], r["bucket_done_ms"])), r
            assert r["bwd_end_ms"] > 0 and r["tail_ms"] >= 0 and r["bn_bcast_ms"] is not None, r
        assert rel < (1e-2 if name == "bf16" else 1e-5), (name, rel)
