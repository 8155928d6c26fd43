"""A float64 reference of Muon (optim.fused.Muon, newton_schulz): the iteration and one whole step of a matrix parameter,
on the bf16 / fp32 values the torch-op path sees, rounding to bf16 at the three store points only.

Errors compound over the five iterations and the polynomial amplifies a flipped bf16 rounding, so the iteration is
compared by relative Frobenius error per matrix: NS_MEASURED is the worst such error of the fp32 torch-op path against
ns_ref over ns_inputs() (test_muon_cpu.py asserts it to 5% both ways); a path with another summation order is allowed
NS_ALLOW = 4x that, the project's margin (gemm_ref.py)."""
import math

import torch
from gemm_ref import f32

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NS_COEF = (3.4445, -4.7750, 2.0315)
NS_MEASURED = 0.00648
NS_ALLOW = 4.0 * NS_MEASURED
NS_SHAPES = [(40, 72), (136, 136), (33, 50), (160, 264)]


def rbf(t):
    return t.to(F32).to(BF).double()


def ns_ref(x0, s, steps):
    """the iteration in float64 with the three bf16 store points: x0 bf16 [m, n], s the fp32 value of 1 / (|u| + eps)"""
    a, b, c = (f32(v) for v in NS_COEF)
    s = f32(s)
    x = x0.detach().cpu().double()
    for it in range(steps):
        al, o = (f32(s * s), s) if it == 0 else (1.0, 1.0)
        A = rbf(al * (x @ x.mT))
        B = rbf(c * (A @ A) + b * A)
        x = rbf(o * (a * x + B @ x))
    return x


def ns_inputs():
    """seeded (x0 bf16 [m, n], s) per NS_SHAPES: gradients-like gauss matrices at the scale 0.02"""
    g = torch.Generator().manual_seed(20)
    out = []
    for m, n in NS_SHAPES:
        x0 = (torch.randn(m, n, generator=g) * 0.02).to(BF)
        out.append((x0, (1.0 / (x0.double().norm() + 1e-7)).float().item()))
    return out


def rel_fro(got, ref):
    return ((got.detach().cpu().double() - ref).norm() / ref.norm()).item()


def muon_step_ref(w, g, buf, lr, momentum, nesterov, ns_steps, weight_decay, eps, gs=1.0):
    """one matrix parameter w [rows][cols] in float64 from its fp32 weight, gradient and momentum buffer -> dict:
    buf, u, A_u (|.| of u's expression), s, x0 (bf16, [min side][max side]), x (float64) and w"""
    w, g, b0 = w.detach().cpu().double(), g.detach().cpu().double() * gs, buf.detach().cpu().double()
    b = momentum * b0 + g
    u = g + momentum * b if nesterov else b
    ab = momentum * b0.abs() + g.abs()
    rows, cols = w.shape
    s = 1.0 / (u.norm().item() + eps)
    x0 = u.to(F32).to(BF)
    x0 = x0.t().contiguous() if rows > cols else x0
    x = ns_ref(x0, s, ns_steps)
    xw = x.t() if rows > cols else x
    return dict(buf=b, u=u, A_u=g.abs() + momentum * ab if nesterov else ab, A_buf=ab, s=s, x0=x0, x=x,
                w=w * (1 - lr * weight_decay) - lr * math.sqrt(max(1.0, rows / cols)) * xw)
