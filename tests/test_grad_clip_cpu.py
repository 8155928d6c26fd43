"""Global-norm gradient clipping of the fused optimizers on the CPU: the torch-op fallback (CPU arena, loose
tensors) against ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim``, clipping after the DDP average (gloo,
world 2), and the ``--grad-clip`` flag."""
import json
import os

import pytest
import torch

from dist_utils import run_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 3, 3, 3), (64,), (10, 1000), (10,)]


def _tensors(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(*s, generator=g) * 0.1 for s in SHAPES]
    gs = [torch.randn(*s, generator=g) for s in SHAPES]           # norm ~ sqrt(11802) ~ 109 >> 1
    return ps, gs


def _make(opt_name, params):
    from pytorch_distributed_nn_amd import optim as O
    kw = {"sgd": dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4),
          "adam": dict(lr=1e-3, weight_decay=1e-2), "adamw": dict(lr=1e-3, weight_decay=0.1)}[opt_name]
    ours = {"sgd": O.SGD, "adam": O.Adam, "adamw": O.AdamW}[opt_name]
    ref = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[opt_name]
    return ours, ref, kw


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("layout", ["arena", "loose"])
@pytest.mark.parametrize("opt_name", ["sgd", "adam", "adamw"])
def test_fallback_matches_torch_clip(opt_name, layout, grad_scale):
    from pytorch_distributed_nn_amd.optim.flat import FlatParams
    ps, gs = _tensors()
    mine = [torch.nn.Parameter(p.clone()) for p in ps]
    refs = [torch.nn.Parameter(p.clone()) for p in ps]
    fp = FlatParams(mine, device="cpu") if layout == "arena" else None
    ours, ref, kw = _make(opt_name, mine)
    opt, ropt = ours(mine, **kw), ref(refs, **kw)
    opt.grad_scale = grad_scale
    opt.set_grad_clip(1.0)
    assert opt._overlap_ok() is None
    for _ in range(3):
        for p, q, g in zip(mine, refs, gs):
            if fp is not None:
                p.grad.copy_(g)
            else:
                p.grad = g.clone()
            q.grad = g * grad_scale
        before = [p.grad.clone() for p in mine]
        tn = torch.nn.utils.clip_grad_norm_(refs, 1.0)
        ropt.step()
        opt.step()
        assert all(torch.equal(p.grad, b) for p, b in zip(mine, before))      # the gradient is left as it was
        assert abs(float(opt.grad_norm) - float(tn)) <= 1e-5 * float(tn)
        assert float(opt.grad_nonfinite) == 0.0
        for p, q in zip(mine, refs):
            assert torch.allclose(p.detach(), q.detach(), atol=1e-6, rtol=0), (p - q).abs().max()


def test_fallback_nonfinite_and_off():
    ps, gs = _tensors()
    from pytorch_distributed_nn_amd.optim import SGD
    a = [torch.nn.Parameter(p.clone()) for p in ps]
    b = [torch.nn.Parameter(p.clone()) for p in ps]
    oa, ob = SGD(a, lr=0.1, momentum=0.9), SGD(b, lr=0.1, momentum=0.9)
    oa.set_grad_clip(1.0)
    oa.set_grad_clip(None)                      # off again: exactly the unclipped step
    for p, q, g in zip(a, b, gs):
        p.grad, q.grad = g.clone(), g.clone()
    oa.step()
    ob.step()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    oa.set_grad_clip(1.0)
    a[1].grad[3] = float("nan")
    oa.step()
    assert float(oa.grad_nonfinite) == 1.0 and float(oa.grad_norm) != float(oa.grad_norm)


# ---------------------------------------------------------------------------------------------------- DDP, gloo
CLIP = 0.05


def _ddp_clip(rank, world):
    from pytorch_distributed_nn_amd.models import build_model
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.optim import SGD
    from pytorch_distributed_nn_amd.parallel.ddp import DistributedDataParallel
    from pytorch_distributed_nn_amd.trainer import Trainer
    torch.manual_seed(100 + rank)
    m = build_model("mlp2", 10)
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.5, first_bucket_cap_mb=0.05)
    ref_state = {k: v.clone() for k, v in m.state_dict().items()}          # rank 0's weights, after the broadcast
    opt = SGD(m.parameters(), lr=0.1, momentum=0.9)
    tr = Trainer(ddp, opt, OF.cross_entropy, torch.device("cpu"), rank, world, log_interval=1,
                 printer=lambda *a: None, grad_clip=CLIP)
    g = torch.Generator().manual_seed(7)
    batches = [(torch.randn(world * 4, 784, generator=g), torch.randint(0, 10, (world * 4,), generator=g))
               for _ in range(3)]
    norms = []
    for x, y in batches:
        tr.step(x[rank * 4:(rank + 1) * 4], y[rank * 4:(rank + 1) * 4])
        norms.append(float(opt.grad_norm))
    # one process, the concatenated batch, torch's clip and optimizer
    single = build_model("mlp2", 10)
    single.load_state_dict(ref_state)
    sopt = torch.optim.SGD(single.parameters(), lr=0.1, momentum=0.9)
    ref_norms = []
    for x, y in batches:
        sopt.zero_grad()
        OF.cross_entropy(single(x), y).backward()
        ref_norms.append(float(torch.nn.utils.clip_grad_norm_(single.parameters(), CLIP)))
        sopt.step()
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    ref = torch.cat([p.detach().reshape(-1) for p in single.parameters()])
    return flat, ref, norms, ref_norms


def test_ddp_gloo_clips_the_averaged_gradient():
    (f0, r0, n0, rn0), (f1, r1, n1, rn1) = run_world(_ddp_clip, 2)
    assert torch.equal(f0, f1)                                   # both ranks end with identical parameters
    assert min(rn0) > 2 * CLIP                                   # the clip was active in every step
    # clipped updates move a weight by at most lr * CLIP * (1 + momentum + ...) ~ 1e-2 per step: fp32 summation-order
    # differences of the two gradients (~1e-6 relative) stay far below 1e-6 absolute
    assert torch.allclose(f0, r0, atol=1e-6, rtol=0), (f0 - r0).abs().max()
    for a, b in zip(n0, rn0):
        assert abs(a - b) <= 1e-4 * b, (n0, rn0)                 # the norm of the AVERAGED gradient


# ---------------------------------------------------------------------------------------------------- CLI
def test_cli_grad_clip_writes_grad_norm(tmp_path):
    from pytorch_distributed_nn_amd import cli
    m = tmp_path / "metrics.jsonl"
    cli.main(["--no-cuda", "--network", "LeNet", "--synthetic", "--max-steps", "3", "--grad-clip", "0.5",
              "--batch-size", "16", "--log-interval", "1", "--metrics", str(m), "--test-batch-size", "16",
              "--out-dir", str(tmp_path / "out")])
    recs = [json.loads(ln) for ln in open(m) if ln.strip()]
    assert len(recs) == 3
    assert all(r["grad_norm"] > 0 and r["grad_norm"] == r["grad_norm"] for r in recs), recs


def test_cli_grad_clip_flag_default_is_off():
    from pytorch_distributed_nn_amd.cli import parse_args
    assert parse_args([]).grad_clip == 0.0
    assert parse_args(["--grad-clip", "1.0"]).grad_clip == 1.0


def test_cli_refuses_grad_clip_with_overlap(tmp_path):
    from pytorch_distributed_nn_amd.cli import check_mode_flags, parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(["--mode", "ddp", "--comm-type", "AllReduce", "--grad-clip", "1.0", "--opt-overlap"])
    assert "--grad-clip cannot be combined with --opt-overlap" in str(e.value)
    cfg = tmp_path / "c.yaml"
    cfg.write_text("grad-clip: 1.0\nopt-overlap: true\n")          # the same through a YAML config
    with pytest.raises(SystemExit):
        parse_args(["--config", str(cfg)])
    cfg.write_text("grad-clip: 0.25\n")
    assert parse_args(["--config", str(cfg)]).grad_clip == 0.25
    with pytest.raises(SystemExit) as e:                            # the PS master does not clip: never silently
        check_mode_flags(parse_args(["--mode", "ps", "--grad-clip", "1.0"]), "ps", 3)
    assert "--grad-clip" in str(e.value)


def test_trainer_routes_to_the_fused_clip(monkeypatch):
    """Trainer(grad_clip=...) with a fused optimizer never calls torch's clip; any other optimizer still does."""
    from pytorch_distributed_nn_amd.optim import SGD
    from pytorch_distributed_nn_amd.trainer import Trainer
    torch.manual_seed(0)
    x, y = torch.randn(8, 8), torch.randint(0, 4, (8,))
    real = torch.nn.utils.clip_grad_norm_
    calls = []

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", spy)
    m = torch.nn.Linear(8, 4)
    tr = Trainer(m, SGD(m.parameters(), lr=0.1), torch.nn.functional.cross_entropy, log_interval=1,
                 printer=lambda *a: None, grad_clip=0.01)
    hist = tr.train(iter([(x, y)] * 3), epochs=1, max_steps=3, steps_per_epoch=3)
    assert not calls and len(hist) == 3 and all(h["grad_norm"] > 0.01 for h in hist)
    m2 = torch.nn.Linear(8, 4)
    tr2 = Trainer(m2, torch.optim.SGD(m2.parameters(), lr=0.1), torch.nn.functional.cross_entropy, log_interval=1,
                  printer=lambda *a: None, grad_clip=0.01)
    hist2 = tr2.train(iter([(x, y)] * 3), epochs=1, max_steps=3, steps_per_epoch=3)
    assert len(calls) == 3 and all(h["grad_norm"] > 0.01 for h in hist2)
