"""A float64 reference of the cross-entropy kernels, the elementwise bounds they are held to, and the seeded inputs
shared by the GPU tests (test_xent_gpu.py) and the CPU self-check of the reference (test_xent_ref_cpu.py).

The kernels (csrc/kernels/softmax_xent.hip) read bf16 or fp32 logits, keep fp32 inside, and write per-row ``lse``
and ``loss`` in fp32 and the gradient ``sc * (softmax - onehot)`` in the logits' type.  ``ref64`` computes the same
from the logits exactly as given (already rounded to bf16, or fp32), in float64.

Bounds (``check_grad``, ``check_rows``): bf16 round-to-nearest is 2^-9 relative, and the fp32 error of
``exp(v - l)`` for ``|v|, |l| <= 64`` is about 1e-5 relative, so a bf16 gradient entry is held to twice the bf16
rounding, ``|d - ref| <= 2^-8 |ref| + 1e-30``.  At the label's own entry ``p - 1`` cancels, so there the absolute
part is ``1e-4 |sc|``.  fp32 gradients (fp32 logits) get ``1e-5 |ref| + 1e-6 |sc|``.  Per-row ``lse`` and ``loss``:
``|x - ref| <= 1e-4 max(1, |ref|)`` on every row.  The derivation needs ``|logit| <= 64``; every generator here stays
inside that."""
from collections import namedtuple

import torch

BF = torch.bfloat16
F32 = torch.float32

Ref = namedtuple("Ref", "lse loss count grad valid")

XMAX = 64.0


def valid_rows(labels, V, ignore_index=-100):
    return (labels != ignore_index) & (labels >= 0) & (labels < V)


def _formulas(x, labels, ignore_index):
    """lse, loss, valid, softmax - onehot in x's dtype (float64: the reference; float32: the model)."""
    R, V = x.shape
    ok = valid_rows(labels, V, ignore_index)
    ys = labels.clamp(0, V - 1)                                # ignored rows index something harmless
    lse = torch.logsumexp(x, 1)
    loss = torch.where(ok, lse - x.gather(1, ys[:, None])[:, 0], torch.zeros_like(lse))
    g = torch.exp(x - lse[:, None])
    g[torch.arange(R, device=x.device), ys] -= 1.0
    g = g * ok[:, None].to(g.dtype)
    return lse, loss, ok, g


def ref64(logits, labels, ignore_index=-100):
    """float64 per-row lse, per-row loss (0 for ignored / out-of-range labels), count of valid rows, and the
    unscaled gradient softmax - onehot (zero rows for ignored labels).  The mean scale is g / max(count, 1)."""
    lse, loss, ok, g = _formulas(logits.double(), labels, ignore_index)
    return Ref(lse, loss, int(ok.sum().item()), g, ok)


def model32(logits, labels, ignore_index=-100, sc=1.0):
    """The same formulas in fp32 with the gradient ``sc * (softmax - onehot)`` rounded to the logits' type: a
    stand-in for a correct kernel.  Returns (lse, loss, count, grad)."""
    lse, loss, ok, g = _formulas(logits.float(), labels, ignore_index)
    return lse, loss, int(ok.sum().item()), (g * torch.tensor(sc, dtype=F32, device=g.device)).to(logits.dtype)


def check_grad(d, ref, labels, sc=1.0):
    """Assert ``d`` (bf16 or fp32, [R][V]) against ``sc * ref.grad`` elementwise; rows with an ignored label must be
    exactly zero.  Returns the worst error / bound ratio."""
    R, V = d.shape
    want = ref.grad * sc
    err = (d.double() - want).abs()
    rows = torch.arange(R, device=d.device)
    ys = labels.clamp(0, V - 1)
    if d.dtype == BF:
        bound = want.abs() * 2.0 ** -8 + 1e-30
        bound[rows, ys] = want[rows, ys].abs() * 2.0 ** -8 + 1e-4 * abs(sc)
    else:
        bound = want.abs() * 1e-5 + 1e-6 * abs(sc)
    ratio = err / bound
    worst = ratio.max().item()
    if not worst <= 1.0:
        r, c = divmod(int(ratio.argmax().item()), V)
        raise AssertionError(f"gradient [{r}][{c}] (label {int(labels[r])}): got {d[r, c].item()!r}, want "
                             f"{want[r, c].item()!r}, error / bound = {worst:.3g}")
    ign = ~ref.valid
    if bool(ign.any()):
        assert d[ign].abs().max().item() == 0.0, "gradient rows of ignored labels must be exactly zero"
    return worst


def check_rows(x, ref):
    """Assert a per-row fp32 vector (lse or loss) against its float64 reference on every row.  Returns the worst
    error / bound ratio."""
    assert x.shape == ref.shape, (x.shape, ref.shape)
    ratio = (x.double() - ref).abs() / (1e-4 * ref.abs().clamp_min(1.0))
    worst = ratio.max().item()
    if not worst <= 1.0:
        r = int(ratio.argmax().item())
        raise AssertionError(f"row {r}: got {x[r].item()!r}, want {ref[r].item()!r}, error / bound = {worst:.3g}")
    return worst


def check_sum(acc0, ref):
    """acc[0] (fp32 sum of the per-row losses) against the float64 sum at 1e-4 relative."""
    want = ref.loss.sum().item()
    got = float(acc0)
    ratio = abs(got - want) / (1e-4 * abs(want)) if want != 0.0 else (0.0 if got == 0.0 else float("inf"))
    assert ratio <= 1.0, f"loss sum: got {got!r}, want {want!r}, error / bound = {ratio:.3g}"
    return ratio


# ------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _logits(R, V, dtype, g, scale=3.0, shift=0.0):
    return (torch.randn(R, V, generator=g) * scale + shift).clamp_(-XMAX, XMAX).to(dtype)


# (V, dtype) of the sweep; what each size exercises is listed with the test that runs it
SWEEP = [(8, BF), (2048, BF), (2056, BF), (4096, BF), (4104, BF), (50304, BF), (51200, BF), (51208, BF),
         (50257, BF), (10, BF), (10, F32), (1000, F32)]
SWEEP_R = 37


def gen_sweep(V, dtype, R=SWEEP_R):
    """Random rows, random labels with the first and the last class and one ignored row among them."""
    g = _gen(1000 + V)
    x = _logits(R, V, dtype, g)
    y = torch.randint(0, V, (R,), generator=g)
    y[0], y[1], y[3] = 0, V - 1, -100
    return x, y


def placement_labels(V):
    """Labels that land in each part of the kernels' lane layout (256 lanes, 16-byte chunks of 8, chunk i held by
    lane i % 256 as its register chunk i / 256): the first and the last element, one chunk of each of the four
    waves at register chunk 0, one in the last register chunk, one in the second load (chunk i + 256) of the
    two-load loop."""
    n8 = V // 8
    last_c = (n8 - 1) // 256
    return ([0, V - 1] + [8 * (64 * w + 5) + 3 for w in range(4)]
            + [8 * (256 * last_c + ((n8 - 1) % 256) // 2) + 1, 8 * (256 + 100) + 6])


PLACEMENT_V = [50304, 4104]


def gen_placement(V):
    y = torch.tensor(placement_labels(V))
    return _logits(len(y), V, BF, _gen(2000 + V)), y


def gen_ignored(V=2056, R=24):
    """Labels for the ignore rules: -100, 7 (a valid class unless it is the ignore_index), V, V + 5, 2^40, -1, and
    valid ones in between.  Used with ignore_index -100 and 7."""
    g = _gen(3000 + V)
    x = _logits(R, V, BF, g)
    y = torch.randint(0, V, (R,), generator=g)
    y[1], y[2], y[4], y[5], y[8], y[9], y[11], y[R - 1] = -100, 7, V, V + 5, 2 ** 40, -1, 7, -100
    return x, y


def gen_all_ignored(V=2056, R=19):
    return _logits(R, V, BF, _gen(3500 + V)), torch.full((R,), -100, dtype=torch.int64)


EDGE_V = 4096


def gen_edges(V=EDGE_V):
    """Value edges, all within |x| <= 64: equal logits; one logit 60 above the rest with the label on it and off it;
    the label on the smallest logit; all-negative rows around -60."""
    g = _gen(4000 + V)
    rows, labels = [], []
    for c in (0.0, 64.0, -64.0, 1.25):                                   # flat rows
        rows.append(torch.full((V,), c))
        labels.append(17)
    for on in (True, False):                                            # saturated rows
        r = torch.randn(V, generator=g)
        r[1234] = r.max() + 60.0
        rows.append(r)
        labels.append(1234 if on else 99)
    r = torch.randn(V, generator=g) * 8.0                                # label on the smallest logit: large loss
    rows.append(r)
    labels.append(int(r.argmin()))
    for _ in range(2):                                                  # all-negative rows around -60
        rows.append(torch.randn(V, generator=g) * 0.75 - 60.0)
        labels.append(int(torch.randint(0, V, (1,), generator=g)))
    x = torch.stack(rows).clamp_(-XMAX, XMAX).to(BF)
    return x, torch.tensor(labels)


# (V, ld) of the column-slice layouts
STRIDED = [(1000, 1024), (2048, 2056)]
STRIDED_R = 21


def gen_strided(V):
    g = _gen(5000 + V)
    x = _logits(STRIDED_R, V, BF, g)
    y = torch.randint(0, V, (STRIDED_R,), generator=g)
    y[2] = -100
    return x, y


def gen_inplace(R, V, lo):
    """Rows for the in-place / out-of-place comparison, every label drawn from [lo, V)."""
    g = _gen(6000 + V)
    return _logits(R, V, BF, g), torch.randint(lo, V, (R,), generator=g)
