"""A float64 reference of the label-smoothing / z-loss cross-entropy kernels (the pdnn_xent_ls_* entry points of
csrc/kernels/softmax_xent.hip), an fp32 model of a correct kernel, and the per-element bounds the kernels are held to.
Shared by test_xent_ls_gpu.py and the CPU self-check test_xent_ls_ref_cpu.py; the input generators are xent_ref's
(imported, not copied) plus one family of its own (``gen_offset``).

With l = lse(x), a valid label y, V columns, eps = label_smoothing, z = z_loss:

    loss = (1 - eps) (l - x[y]) + eps (l - mean_j x[j]) + z l^2
    dx_j = (1 + 2 z l) softmax(x)_j - (1 - eps) [j == y] - eps / V

and an ignored or out-of-range label gives loss 0 and a gradient row of exact zeros.  ``ref64`` evaluates this in
float64 from the logits exactly as given (already rounded to bf16, or fp32).  ``model32`` evaluates it in fp32 the
way the kernels do (fp32 lse, exp(x - l), the logit sum added up serially per lane of 256 and then across lanes),
with the gradient rounded to the logits' type.

Bounds.  Every constant below is 4x the worst error of ``model32`` over all input families of the tests (xent_ref's
sweep shapes, placement, ignored, edges, strided, and gen_offset; all five (eps, z) pairs of PARAMS), measured on the
CPU by test_xent_ls_ref_cpu.py::test_model32_is_inside_every_bound, which prints them; the measured figure stands
next to each constant.  Nothing is excluded: every element and every row is checked.

* Gradient (``check_grad``).  The kernel forms g = (1 + 2 z l) p - (1 - eps) [j == y] - eps / V in fp32 and rounds
  sc * g to the logits' type.  The fp32 error is relative to the magnitudes of the addends,
  ``A_j = (1 + 2 z |l|) p_j + eps / V`` (+ (1 - eps) at the label), not to g itself: where p_j is near eps / V the
  addends cancel and g_j is arbitrarily small.  The dominant part is exp(x - l): x - l is rounded to fp32 at a
  magnitude of up to ~128, so p carries a relative error of up to |x - l| 2^-25 ~ 4e-6.
      fp32 part:  C_G |sc| A_j,  C_G = 1.1e-5  (model32's worst |g32 - g64| / A: 2.53e-6)
  Rounding the result to bf16 (round to nearest, 2^-9 relative to the computed value) is bounded as in xent_ref by
  twice that, 2^-8 |want|: the number format's precision, no measured constant; an fp32 gradient gets 2^-22 |want|
  for the product with sc.  At the label's own entry the absolute term of xent_ref.check_grad is added, 1e-4 |sc|
  (bf16) or 1e-6 |sc| (fp32).
* Per-row loss (``check_loss``).  ``|loss - ref| <= C_L max(1, |ref|) + eps C_S mean_j |x_j|``: the first term
  covers lse, the products and z l^2, the second is what the fp32 sum of the V logits contributes to eps * mean x.
      C_L = 1.2e-6  (model32 with an exact logit sum: 2.93e-7 of max(1, |ref|))
      C_S = 6e-7  (model32's lane-serial fp32 sum: |sum32 - sum64| / sum_j |x_j| = 1.49e-7 at worst)
  With xent_ref's loss bound (1e-4 max(1, |ref|)) a logit sum over ld instead of V columns, or with the last chunk
  counted twice, passes on zero-mean rows: at V = 50304 one extra chunk of values ~3 moves eps * mean by 5e-5.
* lse is the plain log-sum-exp and keeps xent_ref.check_rows.

The derivation needs |logit| <= 64 (xent_ref.XMAX), z <= 0.5."""
from collections import namedtuple

import torch

import xent_ref as X

BF, F32 = X.BF, X.F32

Ref = namedtuple("Ref", "lse loss count grad valid addends xabs_mean eps z")

C_G = 1.1e-5
C_L = 1.2e-6
C_S = 6e-7

# (eps, z): smoothing alone, z-loss alone, both, eps = 1 (no onehot term at all), z terms dominating
PARAMS = [(0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4), (1.0, 0.0), (0.3, 0.5)]


def _formulas(x, labels, eps, z, ignore_index, xsum=None):
    """lse, loss, valid, gradient, addend magnitudes and the logit sum in x's dtype."""
    R, V = x.shape
    ok = X.valid_rows(labels, V, ignore_index)
    ys = labels.clamp(0, V - 1)
    rows = torch.arange(R, device=x.device)
    lse = torch.logsumexp(x, 1)
    if xsum is None:
        xsum = x.sum(1)
    nll = lse - x.gather(1, ys[:, None])[:, 0]
    loss = (1.0 - eps) * nll + eps * (lse - xsum / V) + z * lse * lse
    loss = torch.where(ok, loss, torch.zeros_like(loss))
    p = torch.exp(x - lse[:, None])
    g = (1.0 + 2.0 * z * lse)[:, None] * p
    g[rows, ys] -= 1.0 - eps
    g = g - eps / V
    g = g * ok[:, None].to(g.dtype)
    add = (1.0 + 2.0 * z * lse.abs())[:, None] * p + eps / V
    add[rows, ys] += 1.0 - eps
    return lse, loss, ok, g, add, xsum


def ref64(logits, labels, eps, z, ignore_index=-100):
    """float64 lse, per-row loss (0 on ignored / out-of-range labels), count of valid rows, UNSCALED gradient (zero
    rows for ignored labels), and what the bounds need: the addend magnitudes and mean |x| per row."""
    x = logits.double()
    lse, loss, ok, g, add, _ = _formulas(x, labels, eps, z, ignore_index)
    return Ref(lse, loss, int(ok.sum().item()), g, ok, add, x.abs().mean(1), eps, z)


def lane_serial_sum(x):
    """The fp32 logit sum in the kernels' order: lane t of 256 adds x[t], x[t + 256], ... one after the other (the
    scalar path; the vector path adds 8 at a time, no worse), then the 256 partial sums are added."""
    R, V = x.shape
    n = -(-V // 256)
    xp = torch.zeros(R, n * 256, dtype=F32, device=x.device)
    xp[:, :V] = x.float()
    xp = xp.view(R, n, 256)
    acc = torch.zeros(R, 256, dtype=F32, device=x.device)
    for k in range(n):
        acc = acc + xp[:, k]
    return acc.sum(1)


def model32(logits, labels, eps, z, ignore_index=-100, sc=1.0, exact_sum=False):
    """The formulas in fp32 with the kernels' summation order, the gradient ``sc * g`` rounded to the logits' type: a
    stand-in for a correct kernel.  Returns (lse, loss, count, grad, grad before scaling and rounding, logit sum).
    ``exact_sum``: the logit sum taken from float64 (separates C_L from C_S)."""
    x = logits.float()
    xsum = logits.double().sum(1).float() if exact_sum else lane_serial_sum(x)
    lse, loss, ok, g, _, xsum = _formulas(x, labels, eps, z, ignore_index, xsum)
    d = (g * torch.tensor(sc, dtype=F32, device=g.device)).to(logits.dtype)
    return lse, loss, int(ok.sum().item()), d, g, xsum


def grad_bound(ref, labels, dtype, sc=1.0):
    R, V = ref.grad.shape
    want = ref.grad * sc
    rows = torch.arange(R, device=want.device)
    ys = labels.clamp(0, V - 1)
    bound = C_G * abs(sc) * ref.addends + want.abs() * (2.0 ** -8 if dtype == BF else 2.0 ** -22) + 1e-30
    bound[rows, ys] += (1e-4 if dtype == BF else 1e-6) * abs(sc)
    return want, bound


def check_grad(d, ref, labels, sc=1.0):
    """Assert ``d`` (bf16 or fp32, [R][V]) against ``sc * ref.grad`` on every element; rows with an ignored label
    must be exactly zero.  Returns the worst error / bound ratio."""
    R, V = d.shape
    want, bound = grad_bound(ref, labels, d.dtype, sc)
    ratio = (d.double() - want).abs() / bound
    worst = ratio.max().item()
    if not worst <= 1.0:
        r, c = divmod(int(ratio.argmax().item()), V)
        raise AssertionError(f"gradient [{r}][{c}] (label {int(labels[r])}, eps {ref.eps}, z {ref.z}): got "
                             f"{d[r, c].item()!r}, want {want[r, c].item()!r}, error / bound = {worst:.3g}")
    ign = ~ref.valid
    if bool(ign.any()):
        assert d[ign].abs().max().item() == 0.0, "gradient rows of ignored labels must be exactly zero"
    return worst


def loss_bound(ref):
    return C_L * ref.loss.abs().clamp_min(1.0) + ref.eps * C_S * ref.xabs_mean


def check_loss(loss, ref):
    """Assert the per-row fp32 loss on every row; rows with an ignored label must be exactly zero.  Returns the worst
    error / bound ratio."""
    assert loss.shape == ref.loss.shape, (loss.shape, ref.loss.shape)
    ratio = (loss.double() - ref.loss).abs() / loss_bound(ref)
    worst = ratio.max().item()
    if not worst <= 1.0:
        r = int(ratio.argmax().item())
        raise AssertionError(f"loss row {r} (eps {ref.eps}, z {ref.z}): got {loss[r].item()!r}, want "
                             f"{ref.loss[r].item()!r}, error / bound = {worst:.3g}")
    ign = ~ref.valid
    if bool(ign.any()):
        assert loss[ign].abs().max().item() == 0.0, "losses of ignored labels must be exactly zero"
    return worst


def check_sum(acc0, ref):
    """acc[0], the fp32 sum of the per-row losses (one 1024-lane block: a serial part of <= ceil(R / 1024) terms and
    a tree), against the float64 sum: the rows' own bounds add up, plus 2^-20 of the sum of |loss| for the adds."""
    want = ref.loss.sum().item()
    got = float(acc0)
    bound = loss_bound(ref).sum().item() + 2.0 ** -20 * ref.loss.abs().sum().item()
    ratio = abs(got - want) / bound if bound > 0.0 else (0.0 if got == want else float("inf"))
    assert ratio <= 1.0, f"loss sum: got {got!r}, want {want!r}, error / bound = {ratio:.3g}"
    return ratio


# ------------------------------------------------------------------------------------------------ inputs
OFFSET_V = [(2056, BF), (50304, BF), (1000, F32)]
OFFSET_R = 9


def gen_offset(V, dtype, R=OFFSET_R):
    """Rows with a mean of about +5 (and one of -7) and values of 40 in the row's last 8 columns, the last 16-byte
    chunk: a logit sum that misses, repeats or overruns the end of the row moves eps * mean x by far more than the
    loss bound, which it does not on xent_ref's zero-mean rows."""
    g = X._gen(7000 + V)
    x = torch.randn(R, V, generator=g) * 2.0 + 5.0
    x[1] -= 12.0
    x[:, V - 8:] = 40.0
    y = torch.randint(0, V, (R,), generator=g)
    y[0], y[2], y[4] = V - 1, -100, V - 8
    return x.clamp_(-X.XMAX, X.XMAX).to(dtype), y
