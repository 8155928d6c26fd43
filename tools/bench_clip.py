#!/usr/bin/env python
"""What gradient clipping costs an optimizer step on one GPU, at the flagship arena sizes.

Three routes over a flat arena filled with random gradients (25.6 M elements = ResNet-50 with fused SGD, 124 M =
GPT-2 small with fused AdamW), each timed with HIP events around the whole route, alternating between the routes
inside every repeat, median of the repeats after a warm-up:

  (a) the fused step without clipping;
  (b) the fused step with ``set_grad_clip``: two norm launches, the coefficient applied by the update kernel;
  (c) ``torch.nn.utils.clip_grad_norm_`` over the per-parameter views, then the fused step (the former route);

plus the norm pass of (b) on its own (partials + coefficient), whose bytes are one read of the gradient (4 n).
The table goes to stdout and to ``--out`` (default profiles/grad_clip.txt).  There is no CPU mode: a timing taken
without the GPU would say nothing.

    python tools/bench_clip.py [--repeats 30] [--warmup 5] [--out profiles/grad_clip.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("ResNet-50 / SGD", 25.6e6, 160, "sgd"), ("GPT-2 small / AdamW", 124e6, 150, "adamw")]


def make(n_total, n_tensors, opt_name, seed):
    """A flat CUDA arena of about ``n_total`` elements in ``n_tensors`` equal parameters, with its fused optimizer."""
    from pytorch_distributed_nn_amd.optim import SGD, AdamW
    from pytorch_distributed_nn_amd.optim.flat import FlatParams
    per = int(n_total) // n_tensors // 64 * 64
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(per, device="cuda", generator=gen) * 0.02) for _ in range(n_tensors)]
    fp = FlatParams(ps)
    fp.grad.copy_(torch.randn(fp.numel, device="cuda", generator=gen) * 1e-2)       # norm >> 1
    opt = (SGD(ps, lr=1e-4, momentum=0.9, weight_decay=5e-5) if opt_name == "sgd"
           else AdamW(ps, lr=1e-5, weight_decay=0.1))
    return fp, ps, opt


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def run(name, n_total, n_tensors, opt_name, repeats, warmup, max_norm):
    from pytorch_distributed_nn_amd.ops import kernels as K
    fp, ps, opt = make(n_total, n_tensors, opt_name, 0)
    g0 = fp.grad.clone()
    opt.set_grad_clip(max_norm)          # allocates the workspace; toggled per route below
    ws, out = opt._clip_ws, opt._clip_out

    def plain():
        opt.set_grad_clip(None)
        opt.step()

    def fused():
        opt.set_grad_clip(max_norm)
        opt.step()

    def torch_route():
        opt.set_grad_clip(None)
        torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=True)
        opt.step()

    def norm_only():
        K.clip_coef(ws, K.sumsq_partials(fp.grad, ws), max_norm, out)

    routes = [("a", plain), ("b", fused), ("c", torch_route), ("norm", norm_only)]
    evs = {k: [] for k, _ in routes}
    for it in range(warmup + repeats):
        for k, fn in routes:
            pair = timed(fn)
            if k == "c":
                fp.grad.copy_(g0)        # torch's clip scaled the gradient in place: every route sees the same one
            if it >= warmup:
                evs[k].append(pair)
    torch.cuda.synchronize()
    med = {k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in evs.items()}
    lo = {k: min(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in evs.items()}
    n = fp.numel
    gb = 4.0 * n / 1e9
    rows = [f"{name}: {n} fp32 elements ({gb:.3f} GB of gradient), {n_tensors} parameters, norm "
            f"{float(opt.grad_norm):.3f}, max_norm {max_norm}",
            f"  (a) fused step, no clipping            {med['a']:10.1f} us   (min {lo['a']:.1f})",
            f"  (b) fused step, fused clipping         {med['b']:10.1f} us   (min {lo['b']:.1f})",
            f"  (c) torch clip_grad_norm_ + fused step {med['c']:10.1f} us   (min {lo['c']:.1f})",
            f"  (b) - (a)                              {med['b'] - med['a']:10.1f} us   = "
            f"{gb / max(med['b'] - med['a'], 1e-3) * 1e6:.0f} GB/s for one read of the gradient",
            f"  norm pass alone (2 launches)           {med['norm']:10.1f} us   = "
            f"{gb / med['norm'] * 1e6:.0f} GB/s effective",
            f"  (c) - (b)                              {med['c'] - med['b']:10.1f} us   "
            f"((b) is {'faster' if med['b'] < med['c'] else 'NOT faster'} than (c))"]
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "grad_clip.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py needs a GPU: a CPU timing says nothing about the clipped step")
    lines = [f"tools/bench_clip.py --repeats {a.repeats} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, "
             "HIP events around each route, routes alternated inside every repeat, median (min) of the repeats"]
    for name, n_total, n_tensors, opt_name in CONFIGS:
        lines += run(name, n_total, n_tensors, opt_name, a.repeats, a.warmup, a.max_norm)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
