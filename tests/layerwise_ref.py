"""fp64 per-parameter reference of the layer-wise optimizers (optim/fused.py LARS / LAMB, optim_layerwise.hip).

Plain torch in float64, one parameter at a time, exactly the formulas the kernels document:

LARS    g' = gs * g                                             (gs: every scale the update applies to the gradient)
        r  = eta * |w| / (|g'| + wd * |w| + eps)                 r = 1: excluded, |w| == 0 or |g'| == 0
        d  = r * (g' + wd * w)
        b  = d (first step)  or  mom * b + (1 - damp) * d;       step = d + mom * b (Nesterov)  or  b  (or d: mom == 0)
        w -= lr * step

LAMB    m  = b1 * m + (1 - b1) * g';   v = b2 * v + (1 - b2) * g'^2
        u  = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd * w
        r  = |w| / |u|                                           r = 1: excluded, |w| == 0 or |u| == 0
        w -= lr * r * u

An excluded parameter has wd = 0 and r = 1; ``clamp`` caps r at 1.  ``decay_excluded`` is a switch for the tests
that anchor this file to torch.optim: it gives excluded parameters the weight decay back, so that with everything
excluded LARS is torch's SGD and LAMB is torch's AdamW.

Both functions take ``(params, grads, state)`` as lists (``state[i]`` a dict, empty before the first step) and return
``(new_params, new_state, info)`` without modifying their inputs.  ``info`` holds per parameter the ``ratio``, ``wnorm``
and ``unorm`` (Python floats) and ``A``: per element, the expression the parameter moves by, with every term replaced
by its absolute value and the factor ``lr * r`` taken out, so that ``lr * r * A`` bounds the magnitude of what the
roundings of the update chain are relative to.  ``A_buf`` (LARS) is the same for the momentum buffer (factor ``r``),
``A_m`` / ``A_v`` (LAMB) the absolute-valued moment expressions.
"""
import math

import torch

F64 = torch.float64


def exclude_1d(p):
    return p.ndim <= 1


def _ratio(r, wn, un, adapt, clamp):
    if not adapt or wn == 0.0 or un == 0.0:
        return 1.0
    if clamp and r > 1.0:
        return 1.0
    return r


def lars_step_ref(params, grads, state, lr, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False,
                  trust_coef=1e-3, eps=1e-8, clamp=False, exclude=exclude_1d, gs=1.0, decay_excluded=False):
    out_p, out_s = [], []
    info = dict(ratio=[], wnorm=[], unorm=[], A=[], A_buf=[])
    for p, g, st in zip(params, grads, state):
        ex = exclude is not None and bool(exclude(p))
        wd = weight_decay if (not ex or decay_excluded) else 0.0
        w, g = p.detach().to(F64), g.detach().to(F64) * gs
        wn, un = w.norm().item(), g.norm().item()
        r = _ratio(trust_coef * wn / (un + wd * wn + eps), wn, un, not ex, clamp)
        d = r * (g + wd * w)
        a = g.abs() + wd * w.abs()                         # |d| / r
        new = {}
        if momentum != 0:
            if "momentum_buffer" not in st:
                b, ab = d.clone(), a.clone()
            else:
                b0 = st["momentum_buffer"].detach().to(F64)
                b = momentum * b0 + (1 - dampening) * d
                ab = momentum * b0.abs() / r + abs(1 - dampening) * a
            new["momentum_buffer"] = b
            step, astep = (d + momentum * b, a + momentum * ab) if nesterov else (b, ab)
            info["A_buf"].append(ab)
        else:
            step, astep = d, a
            info["A_buf"].append(None)
        out_p.append(w - lr * step)
        out_s.append(new)
        info["ratio"].append(r)
        info["wnorm"].append(wn)
        info["unorm"].append(un)
        info["A"].append(astep)
    return out_p, out_s, info


def lamb_step_ref(params, grads, state, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, clamp=False,
                  exclude=exclude_1d, gs=1.0, decay_excluded=False):
    b1, b2 = betas
    out_p, out_s = [], []
    info = dict(ratio=[], wnorm=[], unorm=[], A=[], A_m=[], A_v=[])
    for p, g, st in zip(params, grads, state):
        ex = exclude is not None and bool(exclude(p))
        wd = weight_decay if (not ex or decay_excluded) else 0.0
        w, g = p.detach().to(F64), g.detach().to(F64) * gs
        t = st.get("step", 0) + 1
        m0 = st["exp_avg"].detach().to(F64) if "exp_avg" in st else torch.zeros_like(w)
        v0 = st["exp_avg_sq"].detach().to(F64) if "exp_avg_sq" in st else torch.zeros_like(w)
        m = b1 * m0 + (1 - b1) * g
        v = b2 * v0 + (1 - b2) * g * g
        am = b1 * m0.abs() + (1 - b1) * g.abs()
        av = b2 * v0.abs() + (1 - b2) * g * g
        denom = (v / (1 - b2 ** t)).sqrt() + eps
        u = (m / (1 - b1 ** t)) / denom + wd * w
        a = (m.abs() / (1 - b1 ** t)) / denom + wd * w.abs()
        wn, un = w.norm().item(), u.norm().item()
        r = _ratio(wn / un if un != 0.0 else math.inf, wn, un, not ex, clamp)
        out_p.append(w - lr * r * u)
        out_s.append(dict(step=t, exp_avg=m, exp_avg_sq=v))
        info["ratio"].append(r)
        info["wnorm"].append(wn)
        info["unorm"].append(un)
        info["A"].append(a)
        info["A_m"].append(am)
        info["A_v"].append(av)
    return out_p, out_s, info
