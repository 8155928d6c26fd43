#!/usr/bin/env python
"""What the layer-wise optimizers cost an optimizer step on one GPU, at the flagship arenas.

Two arenas with the real parameter shapes (ResNet-50: 161 parameters, 25.6 M elements, 107 of them 1-D; GPT-2 small:
148 parameters, 124 M elements, the 38.6 M-element token embedding among them), filled with random weights and
gradients.  Four routes per arena, each timed with HIP events around the whole route, alternating between the routes
inside every repeat, median of the repeats after a warm-up:

  ResNet-50   (a) fused SGD (momentum, weight decay)     (b) fused LARS     (c) LARS, per-parameter torch ops
  GPT-2       (a) fused AdamW                            (b) fused LAMB     (c) LAMB, per-parameter torch ops

(c) is the optimizer's own torch-op path (the one CPU arenas and loose tensors take) on GPU tensors that are not in
an arena: the same formulas, a handful of launches per parameter.  The byte counts beside the times are those of the
kernels' code (fp32 p, g, state; bf16 shadow), not measurements.  The table goes to stdout and to ``--out`` (default
profiles/layerwise_optim.txt).  There is no CPU mode: a timing taken without the GPU would say nothing.

    python tools/bench_layerwise.py [--repeats 20] [--warmup 3] [--out profiles/layerwise_optim.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resnet50_shapes():
    from pytorch_distributed_nn_amd.models import build_model
    return [tuple(p.shape) for p in build_model("resnet50").parameters() if p.requires_grad]


def gpt2_shapes(n_layer=12, d=768, vocab=50257, ctx=1024):
    shapes = [(vocab, d), (ctx, d)]
    for _ in range(n_layer):
        shapes += [(d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (4 * d, d), (4 * d,), (d, 4 * d), (d,)]
    return shapes + [(d,), (d,)]


def make(shapes, seed, arena=True):
    from pytorch_distributed_nn_amd.optim.flat import FlatParams
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, device="cuda", generator=gen) * 0.02) for s in shapes]
    if arena:
        fp = FlatParams(ps)
        fp.grad.copy_(torch.randn(fp.numel, device="cuda", generator=gen) * 1e-2)
        return fp, ps
    for p in ps:
        p.grad = torch.randn(*p.shape, device="cuda", generator=gen) * 1e-2
    return None, ps


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def run(name, shapes, kind, repeats, warmup):
    from pytorch_distributed_nn_amd.optim import LAMB, LARS, SGD, AdamW
    if kind == "lars":
        mk_base = lambda ps: SGD(ps, lr=1e-4, momentum=0.9, weight_decay=5e-5)                      # noqa: E731
        mk_lw = lambda ps: LARS(ps, lr=1e-2, momentum=0.9, weight_decay=5e-5)                       # noqa: E731
        base_name, lw_name = "fused SGD", "fused LARS"
        base_bytes, lw_bytes = 22, 30          # SGD: r p,g,buf w p,buf,shadow; LARS: + r p,g in the norm pass
    else:
        mk_base = lambda ps: AdamW(ps, lr=1e-5, weight_decay=0.1)                                   # noqa: E731
        mk_lw = lambda ps: LAMB(ps, lr=1e-5, weight_decay=0.1)                                      # noqa: E731
        base_name, lw_name = "fused AdamW", "fused LAMB"
        base_bytes, lw_bytes = 30, 42          # AdamW: r p,g,m,v w p,m,v,shadow; LAMB: r p,g,m,v w m,v | r p,m,v w p,shadow
    fa, pa = make(shapes, 0)
    fb, pb = make(shapes, 0)
    _, pc = make(shapes, 0, arena=False)
    oa, ob, oc = mk_base(pa), mk_lw(pb), mk_lw(pc)
    assert ob._group_flat(0, ob.param_groups[0])[0] is fb and oc._group_flat(0, oc.param_groups[0])[0] is None
    routes = [("a", oa.step), ("b", ob.step), ("c", oc.step)]
    evs = {k: [] for k, _ in routes}
    for it in range(warmup + repeats):
        for k, fn in routes:
            pair = timed(fn)
            if it >= warmup:
                evs[k].append(pair)
    torch.cuda.synchronize()
    med = {k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in evs.items()}
    lo = {k: min(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in evs.items()}
    n = sum(p.numel() for p in pb)
    tab = ob._lw[0]["tab"]
    r = ob.trust_ratios()
    gbs = lambda b, us: b * n / us / 1e3                                                            # noqa: E731
    return [f"{name}: {n} fp32 elements in {len(shapes)} parameters ({sum(len(s) <= 1 for s in shapes)} of them 1-D), "
            f"arena {fb.numel}; {tab.nseg} segments in {tab.nchunk} chunks; trust ratios "
            f"{r.min().item():.3g} .. {r.max().item():.3g}",
            f"  (a) {base_name:<34} {med['a']:10.1f} us   (min {lo['a']:.1f})   {base_bytes} B/element = "
            f"{gbs(base_bytes, med['a']):.0f} GB/s",
            f"  (b) {lw_name + ', 3 launches':<34} {med['b']:10.1f} us   (min {lo['b']:.1f})   {lw_bytes} B/element = "
            f"{gbs(lw_bytes, med['b']):.0f} GB/s",
            f"  (c) {'same formulas, torch ops per tensor':<34} {med['c']:10.1f} us   (min {lo['c']:.1f})",
            f"  (b) / (a)                              {med['b'] / med['a']:10.2f} x    (by bytes "
            f"{lw_bytes / base_bytes:.2f} x)",
            f"  (c) / (b)                              {med['c'] / med['b']:10.2f} x"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "layerwise_optim.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_layerwise.py needs a GPU: a CPU timing says nothing about the fused step")
    lines = [f"tools/bench_layerwise.py --repeats {a.repeats} --warmup {a.warmup}: {torch.cuda.get_device_name(0)}, "
             "HIP events around each route, routes alternated inside every repeat, median (min) of the repeats"]
    for name, shapes, kind in (("ResNet-50 / LARS", resnet50_shapes(), "lars"),
                               ("GPT-2 small / LAMB", gpt2_shapes(), "lamb")):
        lines += run(name, shapes, kind, a.repeats, a.warmup)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
