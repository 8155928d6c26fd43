#!/usr/bin/env python
"""What label smoothing and z-loss cost the cross-entropy kernels on one GPU.

The plain entry points (pdnn_xent_*) against the smoothed ones (pdnn_xent_ls_*, eps = 0.1, z = 1e-4) on the same
logits, at 8192 x 50304 bf16 (the GPT-2 small head: the fused forward+gradient, and forward + backward) and at
256 x 1000 (a ResNet-50 head, bf16 and fp32).  Each route is timed with HIP events around its launches, the routes
alternate inside every repeat, and the table gives the median (10th / 90th percentile) of the repeats after a
warm-up, with the achieved GB/s for the bytes the route must move.  The plain route is timed twice per repeat (A and
B): the difference of those two medians is the run-to-run spread the smoothed route is to be read against.  No
threshold is applied: the table states the difference and the spread.

The table goes to stdout and to ``--out`` (default profiles/xent_smoothing.txt).  There is no CPU mode.

    python tools/bench_xent.py [--repeats 50] [--warmup 10] [--out profiles/xent_smoothing.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS, Z = 0.1, 1e-4
# (rows, V, dtype, fused forward+gradient as well)
CONFIGS = [(8192, 50304, torch.bfloat16, True), (256, 1000, torch.bfloat16, True), (256, 1000, torch.float32, False)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def run(R, V, dtype, with_fused, repeats, warmup):
    from pytorch_distributed_nn_amd.ops import kernels as K
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.randn(R, V, device="cuda", generator=gen) * 3.0).to(dtype)
    y = torch.randint(0, V, (R,), device="cuda", generator=gen)
    gs = torch.ones(1, device="cuda")
    out = torch.empty_like(x)
    ls = dict(label_smoothing=EPS, z_loss=Z)
    state = {}

    def fb(**kw):
        _, lse, acc = K.xent_fwd(x, y, **kw)
        state["d"] = K.xent_bwd(x, y, lse, gs, 1.0, count=acc[1:2], **kw)

    routes = [("fwd + bwd, plain A", lambda: fb(), 3), ("fwd + bwd, smoothed", lambda: fb(**ls), 3),
              ("fwd + bwd, plain B", lambda: fb(), 3)]
    if with_fused:
        routes += [("fused fwd+grad, plain A", lambda: K.xent_fwd_grad(x, y, out=out), 2),
                   ("fused fwd+grad, smoothed", lambda: K.xent_fwd_grad(x, y, out=out, **ls), 2),
                   ("fused fwd+grad, plain B", lambda: K.xent_fwd_grad(x, y, out=out), 2)]
    evs = {k: [] for k, _, _ in routes}
    for it in range(warmup + repeats):
        for k, fn, _ in routes:
            pair = timed(fn)
            if it >= warmup:
                evs[k].append(pair)
    torch.cuda.synchronize()
    us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in evs.items()}
    med = {k: statistics.median(v) for k, v in us.items()}
    esz = x.element_size()
    name = f"{R} x {V} {'bf16' if dtype == torch.bfloat16 else 'fp32'}"
    rows = [f"{name}: one pass over the logits = {R * V * esz / 1e6:.1f} MB"]
    for k, _, passes in routes:
        gb = passes * R * V * esz / 1e9
        rows.append(f"  {k:26s} {med[k]:10.1f} us   (p10 {pct(us[k], 0.1):.1f}, p90 {pct(us[k], 0.9):.1f})   "
                    f"{gb / med[k] * 1e6:7.0f} GB/s for {passes} passes")
    for what in (["fwd + bwd"] + (["fused fwd+grad"] if with_fused else [])):
        a, b, s = med[f"{what}, plain A"], med[f"{what}, plain B"], med[f"{what}, smoothed"]
        base = 0.5 * (a + b)
        rows.append(f"  {what}: smoothed - plain = {s - base:+.1f} us ({(s - base) / base * 100:+.2f}%); "
                    f"plain A - plain B = {a - b:+.1f} us ({abs(a - b) / base * 100:.2f}%)")
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "xent_smoothing.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_xent.py needs a GPU: a CPU timing says nothing about the kernels")
    lines = [f"tools/bench_xent.py --repeats {a.repeats} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, "
             f"label_smoothing {EPS}, z_loss {Z}; HIP events around each route (its launches and output "
             "allocations), routes alternated inside every repeat, median (p10, p90) of the repeats"]
    for R, V, dtype, with_fused in CONFIGS:
        lines += run(R, V, dtype, with_fused, a.repeats, a.warmup)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
