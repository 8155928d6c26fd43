"""CPU self-check of tests/xent_ls_ref.py (the reference and bounds of the label-smoothing / z-loss cross-entropy
kernels): the float64 reference against torch autograd, the fp32 model inside every bound on every input family (and
the measured errors the bounds' constants are 4x of), planted errors rejected, and the CPU paths of the public
interface (OF.cross_entropy, GPT-2's reference forward, the CLI flags)."""
import json

import pytest
import torch
import torch.nn.functional as F

import xent_ls_ref as L
import xent_ref as X

BF, F32 = X.BF, X.F32


# ------------------------------------------------------------------------------------------ reference vs torch
@pytest.mark.parametrize("ign", [-100, 7])
@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
def test_ref64_matches_torch_float64_at_z0(eps, ign):
    x, y = X.gen_ignored(V=200, R=24)
    y = torch.where((y >= 200) | ((y < 0) & (y != ign)), torch.tensor(ign), y)     # torch refuses out-of-range labels
    x = x.double().requires_grad_()
    ref = L.ref64(x.detach(), y, eps, 0.0, ign)
    for red in ("mean", "sum"):
        x.grad = None
        t = F.cross_entropy(x, y, ignore_index=ign, reduction=red, label_smoothing=eps)
        t.backward()
        den = max(ref.count, 1) if red == "mean" else 1
        assert abs(t.item() - ref.loss.sum().item() / den) <= 1e-12 * max(1.0, abs(t.item()))
        assert (x.grad - ref.grad / den).abs().max().item() <= 1e-14
    rows = F.cross_entropy(x.detach(), y, ignore_index=ign, reduction="none", label_smoothing=eps)
    assert (rows - ref.loss).abs().max().item() <= 1e-12
    assert ref.loss[~ref.valid].abs().max().item() == 0.0 and ref.grad[~ref.valid].abs().max().item() == 0.0


def test_ref64_z_term_matches_autograd():
    x, y = X.gen_ignored(V=200, R=24)
    x = x.double().requires_grad_()
    z = 0.5
    ok = X.valid_rows(y, 200)
    (z * (torch.logsumexp(x, 1) ** 2 * ok).sum()).backward()
    r0, r1 = L.ref64(x.detach(), y, 0.3, 0.0), L.ref64(x.detach(), y, 0.3, z)
    assert ((r1.grad - r0.grad) - x.grad).abs().max().item() <= 1e-12
    want = z * torch.logsumexp(x.detach(), 1) ** 2 * ok
    assert ((r1.loss - r0.loss) - want).abs().max().item() <= 1e-10
    assert r1.grad[~ok].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------ model inside bounds
def _families():
    for V, dt in X.SWEEP:
        yield f"sweep-{V}", X.gen_sweep(V, dt), -100
    for V in X.PLACEMENT_V:
        yield f"placement-{V}", X.gen_placement(V), -100
    for ign in (-100, 7):
        yield f"ignored-{ign}", X.gen_ignored(), ign
    yield "all-ignored", X.gen_all_ignored(), -100
    yield "edges", X.gen_edges(), -100
    for V, _ in X.STRIDED:
        yield f"strided-{V}", X.gen_strided(V), -100
    for V, dt in L.OFFSET_V:
        yield f"offset-{V}", L.gen_offset(V, dt), -100


def test_model32_is_inside_every_bound():
    """Every family, every (eps, z): model32 passes check_grad / check_loss / check_sum, and the errors the constants
    C_G, C_L, C_S are 4x of are measured (printed; the docstring of xent_ls_ref.py quotes them)."""
    meas = {"C_G": 0.0, "C_L": 0.0, "C_S": 0.0}
    ratio = {"grad": 0.0, "loss": 0.0, "sum": 0.0}
    for name, (x, y), ign in _families():
        for eps, z in L.PARAMS:
            ref = L.ref64(x, y, eps, z, ign)
            lse, loss, count, d, g32, xs = L.model32(x, y, eps, z, ign, sc=0.5)
            assert count == ref.count
            X.check_rows(lse, ref.lse)
            ratio["grad"] = max(ratio["grad"], L.check_grad(d, ref, y, 0.5))
            ratio["loss"] = max(ratio["loss"], L.check_loss(loss, ref))
            ratio["sum"] = max(ratio["sum"], L.check_sum(loss.sum(), ref))
            meas["C_G"] = max(meas["C_G"], ((g32.double() - ref.grad).abs() / ref.addends).max().item())
            xd = x.double()
            meas["C_S"] = max(meas["C_S"], ((xs.double() - xd.sum(1)).abs() / xd.abs().sum(1)).max().item())
            le = L.model32(x, y, eps, z, ign, exact_sum=True)[1]
            meas["C_L"] = max(meas["C_L"], ((le.double() - ref.loss).abs() / ref.loss.abs().clamp_min(1.0)).max().item())
    print("model32 worst errors:", {k: f"{v:.3g}" for k, v in meas.items()},
          "worst error / bound:", {k: round(v, 3) for k, v in ratio.items()})
    # the constants are 4x the model's error: neither tighter than the model needs nor wider than 4x (rounded up to
    # one digit: < 8x)
    for k, c in (("C_G", L.C_G), ("C_L", L.C_L), ("C_S", L.C_S)):
        assert 4.0 * meas[k] <= c < 8.0 * meas[k], (k, meas[k], c)


# ------------------------------------------------------------------------------------------ planted errors
def _wrong(kind, x, y, eps, z, ign=-100, ld_pad=None):
    """float64 loss rows and unscaled gradient of a kernel with one planted mistake."""
    xd = x.double()
    R, V = xd.shape
    ref = L.ref64(x, y, eps, z, ign)
    loss, g = ref.loss.clone(), ref.grad.clone()
    ok = ref.valid
    rows, ys = torch.arange(R), y.clamp(0, V - 1)
    p = torch.exp(xd - ref.lse[:, None])
    okf = ok[:, None].double()
    if kind == "spread over V - 1":                 # eps / (V - 1) on the other classes, none on the label
        g = (1 + 2 * z * ref.lse)[:, None] * p - eps / (V - 1)
        g[rows, ys] += eps / (V - 1) - (1 - eps)
        g = g * okf
    elif kind == "no eps / V on the label":
        g[rows, ys] += eps / V * ok.double()
    elif kind == "onehot not scaled":
        g[rows, ys] -= eps * ok.double()
    elif kind == "z on ignored rows":
        loss = loss + (~ok).double() * z * ref.lse ** 2
    elif kind == "no 2 z l":
        g = g - (2 * z * ref.lse)[:, None] * p * okf
    elif kind == "sum over ld":
        loss = loss - ok.double() * eps * ld_pad.double().sum(1) / V
    elif kind == "last chunk twice":
        n8 = V // 8
        dup = xd[:, 8 * (n8 - 1):8 * n8].sum(1)
        loss = loss - ok.double() * eps * dup / V
    else:
        raise KeyError(kind)
    return ref, loss, g


_SHAPES = [(10, F32), (1000, F32), (2056, BF)]
# eps / V missing on the label alone: fp32 shapes only (at V = 2056 in bf16, eps / V = 5e-5 is below the label entry's
# own absolute term of xent_ref.check_grad, 1e-4; there the loss and the other V - 1 entries carry the check)
_PLANTED = ([(k, e, z, V, dt) for k, e, z in [("spread over V - 1", 0.1, 0.0), ("onehot not scaled", 0.1, 0.0),
                                              ("no 2 z l", 0.0, 1e-4), ("no 2 z l", 0.1, 1e-4)] for V, dt in _SHAPES]
            + [("no eps / V on the label", 0.1, 0.0, V, dt) for V, dt in _SHAPES[:2]])


@pytest.mark.parametrize("kind,eps,z,V,dtype", _PLANTED)
def test_planted_gradient_errors_are_rejected(kind, eps, z, V, dtype):
    x, y = X.gen_sweep(V, dtype)
    ref, _, g = _wrong(kind, x, y, eps, z)
    L.check_grad(ref.grad.to(dtype), ref, y)                            # the rounded truth passes
    with pytest.raises(AssertionError):
        L.check_grad(g.to(dtype), ref, y)


def test_planted_loss_errors_are_rejected():
    for V, dtype in [(2056, BF), (50304, BF)]:                          # zero-mean rows: the duplicated last chunk
        x, y = X.gen_sweep(V, dtype)
        ref, loss, _ = _wrong("last chunk twice", x, y, 0.1, 0.0)
        L.check_loss(ref.loss.float(), ref)
        with pytest.raises(AssertionError):
            L.check_loss(loss.float(), ref)
    for V, dtype in L.OFFSET_V[:2]:                                     # the family made for it
        x, y = L.gen_offset(V, dtype)
        ref, loss, _ = _wrong("last chunk twice", x, y, 0.1, 0.0)
        with pytest.raises(AssertionError):
            L.check_loss(loss.float(), ref)
    for V, ld in X.STRIDED:                                             # padding columns of 48: a sum over ld
        x, y = X.gen_strided(V)
        ref, loss, _ = _wrong("sum over ld", x, y, 0.1, 0.0, ld_pad=torch.full((x.shape[0], ld - V), 48.0))
        with pytest.raises(AssertionError):
            L.check_loss(loss.float(), ref)
    x, y = X.gen_ignored()
    ref, loss, _ = _wrong("z on ignored rows", x, y, 0.0, 1e-4)
    with pytest.raises(AssertionError, match="want 0.0"):
        L.check_loss(loss.float(), ref)


def test_mean_over_all_rows_is_rejected():
    """The mean divides by the count of valid rows: a gradient scaled by 1 / R fails check_grad at sc = 1 / count."""
    x, y = X.gen_ignored()
    ref = L.ref64(x, y, 0.1, 1e-4)
    R = x.shape[0]
    assert ref.count < R
    L.check_grad((ref.grad / ref.count).to(BF), ref, y, 1.0 / ref.count)
    with pytest.raises(AssertionError):
        L.check_grad((ref.grad / R).to(BF), ref, y, 1.0 / ref.count)


# ------------------------------------------------------------------------------------------ public interface (CPU)
@pytest.mark.parametrize("red", ["mean", "sum", "none"])
@pytest.mark.parametrize("eps,z", L.PARAMS)
def test_cross_entropy_cpu_branch(eps, z, red):
    from pytorch_distributed_nn_amd.ops import functional as OF
    x, y = X.gen_ignored(V=200, R=24)
    y = torch.where((y >= 200) | ((y < 0) & (y != -100)), torch.tensor(-100), y)
    x = x.float().requires_grad_()
    ref = L.ref64(x.detach(), y, eps, z)
    out = OF.cross_entropy(x, y, reduction=red, label_smoothing=eps, z_loss=z)
    den = max(ref.count, 1) if red == "mean" else 1
    if red == "none":
        assert (out.double() - ref.loss).abs().max().item() <= 1e-5 * ref.loss.abs().max().item()
        out.sum().backward()
    else:
        want = ref.loss.sum().item() / den
        assert abs(out.item() - want) <= 1e-5 * abs(want)
        out.backward()
    assert (x.grad.double() - ref.grad / den).abs().max().item() <= 1e-5 * (1 + 2 * z * 80) / den
    plain = OF.cross_entropy(x.detach(), y, reduction=red)
    assert torch.equal(plain, F.cross_entropy(x.detach(), y, reduction=red))


@pytest.mark.parametrize("bad", [dict(label_smoothing=-0.1), dict(label_smoothing=1.5),
                                 dict(label_smoothing=float("nan")), dict(z_loss=-1.0), dict(z_loss=float("inf"))])
def test_cross_entropy_refuses_bad_coefficients(bad):
    from pytorch_distributed_nn_amd.ops import functional as OF
    with pytest.raises(ValueError):
        OF.cross_entropy(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64), **bad)


def test_gpt2_reference_forward_smoothing_and_evaluation():
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(3)
    m = build_gpt2("gpt2_tiny")
    assert m.config.label_smoothing == 0.0 and m.config.z_loss == 0.0
    idx = torch.randint(0, 512, (2, 16))
    tgt = torch.randint(0, 512, (2, 16))
    tgt[0, :3] = -100
    plain = m(idx, tgt)
    logits = m(idx).detach().view(-1, 512)
    m.config.label_smoothing, m.config.z_loss = 0.1, 1e-2
    loss = m(idx, tgt)
    ref = L.ref64(logits, tgt.view(-1), 0.1, 1e-2)
    want = ref.loss.sum().item() / ref.count
    assert abs(loss.item() - want) <= 1e-5 * want
    assert loss.item() - plain.item() > 1e-3                         # the expected amount is not nothing
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    with torch.no_grad():                                            # evaluation: the plain cross-entropy
        assert torch.equal(m(idx, tgt), plain.detach())


def test_cli_flags(tmp_path):
    from pytorch_distributed_nn_amd import cli
    a = cli.parse_args([])
    assert a.label_smoothing == 0.0 and a.z_loss == 0.0
    a = cli.parse_args(["--label-smoothing", "0.1", "--z-loss", "1e-4"])
    assert a.label_smoothing == 0.1 and a.z_loss == 1e-4
    for bad in (["--label-smoothing", "1.5"], ["--label-smoothing", "-0.1"], ["--label-smoothing", "nan"],
                ["--z-loss", "-1"], ["--z-loss", "inf"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    cfg = tmp_path / "c.yaml"
    cfg.write_text("label-smoothing: 0.2\nz-loss: 0.001\n")
    a = cli.parse_args(["--config", str(cfg)])
    assert a.label_smoothing == 0.2 and a.z_loss == 0.001
    cfg.write_text("label-smoothing: 2.0\n")
    with pytest.raises(SystemExit):
        cli.parse_args(["--config", str(cfg)])
    for mode, world in (("single", 1), ("ddp", 2), ("ps", 3)):       # used in every mode: no refusal
        cli.check_mode_flags(cli.parse_args(["--label-smoothing", "0.1", "--z-loss", "1e-4"]), mode, world)


def test_cli_trains_with_the_smoothed_loss_and_evaluates_plain(tmp_path, monkeypatch):
    """--label-smoothing reaches the Trainer's loss_fn (the first step's loss is the smoothed loss of the untrained
    LeNet, above the plain one by eps (mean_j(l - x_j) - (l - x_y))), evaluation calls the plain loss."""
    from pytorch_distributed_nn_amd import cli
    from pytorch_distributed_nn_amd.ops import functional as OF
    calls = []
    real = OF.cross_entropy

    def spy(*a, **kw):
        calls.append((torch.is_grad_enabled(), kw.get("label_smoothing", 0.0), kw.get("z_loss", 0.0)))
        return real(*a, **kw)

    monkeypatch.setattr(OF, "cross_entropy", spy)
    args = ["--no-cuda", "--network", "LeNet", "--synthetic", "--max-steps", "3", "--batch-size", "16",
            "--log-interval", "1", "--test-batch-size", "16", "--out-dir", str(tmp_path / "out")]
    m = tmp_path / "m.jsonl"
    cli.main(args + ["--label-smoothing", "0.1", "--z-loss", "0.01", "--metrics", str(m)])
    train = [c for c in calls if c[0]]
    ev = [c for c in calls if not c[0]]
    assert len(train) == 3 and all(c[1:] == (0.1, 0.01) for c in train), calls
    assert ev and all(c[1:] == (0.0, 0.0) for c in ev), calls
    smooth0 = json.loads(open(m).readline())["loss"]
    m2 = tmp_path / "m2.jsonl"
    cli.main(args + ["--metrics", str(m2)])
    plain0 = json.loads(open(m2).readline())["loss"]
    # same seed, same first batch, same initial weights: the first losses differ by the smoothing and z terms alone;
    # at initialisation lse ~ log 10 and the logits are small, so the z term is ~ 0.01 * 5.3 and the eps term small
    assert 0.03 < smooth0 - plain0 < 0.2, (smooth0, plain0)
