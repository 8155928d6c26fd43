"""CPU self-check of tests/xent_ref.py: the float64 reference agrees with torch's cross-entropy, and a correct fp32
model of the kernels (same formulas, gradient rounded to bf16) stays inside the bounds of check_grad / check_rows on
every input the GPU tests use.  If the model left a bound, the bound (not a kernel) would be wrong."""
import pytest
import torch
import torch.nn.functional as F

import xent_ref as X

WORST = {}


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("dtype", [X.BF, X.F32], ids=["bf16", "fp32"])
def test_ref64_matches_torch_float64(dtype):
    g = torch.Generator().manual_seed(11)
    R, V = 29, 333
    x = (torch.randn(R, V, generator=g) * 4).to(dtype)
    y = torch.randint(0, V, (R,), generator=g)
    for ign in (-100, 7):
        yy = y.clone()
        yy[2], yy[5], yy[6], yy[20] = ign, ign, 7, 7          # in-range labels only: torch rejects the others
        ref = X.ref64(x, yy, ign)
        xd = x.double().requires_grad_(True)
        none = F.cross_entropy(xd, yy, ignore_index=ign, reduction="none")
        assert torch.allclose(ref.loss, none.detach(), rtol=1e-13, atol=1e-13)
        total = F.cross_entropy(xd, yy, ignore_index=ign, reduction="sum")
        assert abs(ref.loss.sum().item() - total.item()) <= 1e-12 * abs(total.item())
        assert ref.count == int((yy != ign).sum())
        (gsum,) = torch.autograd.grad(total, xd)
        assert torch.allclose(ref.grad, gsum, rtol=1e-12, atol=1e-15)
        mean = F.cross_entropy(xd, yy, ignore_index=ign, reduction="mean")
        assert abs(ref.loss.sum().item() / max(ref.count, 1) - mean.item()) <= 1e-12 * abs(mean.item())
        (gmean,) = torch.autograd.grad(mean, xd)
        assert torch.allclose(ref.grad / max(ref.count, 1), gmean, rtol=1e-12, atol=1e-15)
        assert torch.allclose(ref.lse, torch.logsumexp(x.double(), 1), rtol=1e-14, atol=0)


def test_ref64_out_of_range_labels_are_ignored():
    x, y = X.gen_ignored()
    for ign in (-100, 7):
        ref = X.ref64(x, y, ign)
        bad = (y == ign) | (y < 0) | (y >= x.shape[1])
        assert ref.count == int((~bad).sum()) and 0 < ref.count < len(y)
        assert ref.loss[bad].abs().max().item() == 0.0 and ref.grad[bad].abs().max().item() == 0.0
        assert (ref.loss[~bad] > 0).all()
    ref = X.ref64(*X.gen_all_ignored())
    assert ref.count == 0 and ref.loss.abs().max().item() == 0.0 and ref.grad.abs().max().item() == 0.0


def _model_inside_bounds(x, y, ign=-100):
    ref = X.ref64(x, y, ign)
    kind = "bf16" if x.dtype == X.BF else "fp32"
    for sc in (1.0, 1.0 / max(ref.count, 1)):                   # the sum and the mean scale
        lse, loss, count, d = X.model32(x, y, ign, sc)
        assert count == ref.count
        _note(f"grad {kind}", X.check_grad(d, ref, y, sc))
    _note("lse", X.check_rows(lse, ref.lse))
    _note("loss", X.check_rows(loss, ref.loss))
    _note("sum", X.check_sum(loss.sum(), ref))


@pytest.mark.parametrize("V,dtype", X.SWEEP, ids=[f"{v}-{'bf16' if d == X.BF else 'fp32'}" for v, d in X.SWEEP])
def test_model_inside_bounds_sweep(V, dtype):
    _model_inside_bounds(*X.gen_sweep(V, dtype))


@pytest.mark.parametrize("V", X.PLACEMENT_V)
def test_model_inside_bounds_placement(V):
    x, y = X.gen_placement(V)
    n8 = V // 8
    chunks = [int(l) // 8 for l in y]
    assert y[0] == 0 and y[1] == V - 1
    assert [c % 256 // 64 for c in chunks[2:6]] == [0, 1, 2, 3] and all(c < 256 for c in chunks[2:6])
    assert chunks[6] // 256 == (n8 - 1) // 256 and chunks[6] < n8
    assert 256 <= chunks[7] < 512
    _model_inside_bounds(x, y)


@pytest.mark.parametrize("ign", [-100, 7])
def test_model_inside_bounds_ignored(ign):
    _model_inside_bounds(*X.gen_ignored(), ign)
    _model_inside_bounds(*X.gen_all_ignored(), ign)


def test_model_inside_bounds_edges():
    x, y = X.gen_edges()
    assert x.abs().max().item() <= X.XMAX
    ref = X.ref64(x, y)
    assert ref.loss.max().item() > 20.0                          # the label on the smallest logit
    assert ref.loss[4].item() < 1e-6                             # the saturated row with the label on the peak
    _model_inside_bounds(x, y)


@pytest.mark.parametrize("V,ld", X.STRIDED)
def test_model_inside_bounds_strided(V, ld):
    _model_inside_bounds(*X.gen_strided(V))


@pytest.mark.parametrize("R,V,lo", [(64, 2048, 512), (16, 50304, 0)])
def test_model_inside_bounds_inplace_inputs(R, V, lo):
    """The generator of the in-place comparison, with fewer rows (the GPU test runs 4096 and 256)."""
    x, y = X.gen_inplace(R, V, lo)
    assert int(y.min()) >= lo
    _model_inside_bounds(x, y)


def test_bounds_reject_a_wrong_tail():
    """The bounds see what the max-norm metric cannot: one small softmax entry off by 2%, one ignored row not zero."""
    x, y = X.gen_sweep(4104, X.BF)
    ref = X.ref64(x, y)
    _, _, _, d = X.model32(x, y)
    bad = d.clone()
    bad[7, 4103] = bad[7, 4103].float() * 1.02
    with pytest.raises(AssertionError):
        X.check_grad(bad, ref, y)
    bad = d.clone()
    bad[3, 100] = 1e-20
    with pytest.raises(AssertionError):
        X.check_grad(bad, ref, y)
    X.check_grad(d, ref, y)
