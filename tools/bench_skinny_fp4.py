#!/usr/bin/env python3
"""Weight-only MXFP4 decode against the bf16 and fp8 paths (the record behind profiles/gemm_skinny_fp4.txt).

  1. per linear: ops.kernels.gemm_skinny (bf16 shadow), gemm_skinny_fp8 (e4m3 codes + row scales) and gemm_skinny_fp4
     (e2m1 codes + block scales; the kernel's rule, and one and two 16-row groups per wave forced) at M in {1, 8, 16, 64}
     on the GPT-2 small and medium shapes with their real epilogues.  us per call inside one captured graph of
     back-to-back calls that rotate over copies of the weight (the same number of copies in every arm, enough for the
     fp8 copies to exceed the 256 MiB Infinity Cache, at most 64: the small weights stay cache-resident in every arm, as
     between the steps of a real decode loop); the arms' graphs are replayed in turn, median over the rounds;
  2. per token: GPT2.generate(graph=True, sampler="device") ms per token at B in {1, 8} with decode_weights bf16, fp8
     and mxfp4 for gpt2_small and gpt2_medium (random init), the arms alternating in this process; ms per token is the
     difference of a 96- and a 32-token call over 64 tokens, which cancels the prefill, the capture and the quantisation;
  3. random-init gpt2_tiny: relative L2 of the logits of the first decode steps against the bf16 weights (not a measure of
     quality on a trained model).

    python tools/bench_skinny_fp4.py [--out profiles/gemm_skinny_fp4.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_skinny_fp8 import CACHE_BYTES, shapes  # noqa: E402

BF = torch.bfloat16
MS = (1, 8, 16, 64)


def graph_of(calls):
    for f in calls[:4]:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in calls:
            f()
    return g


def alternate_us(graphs, ncalls, rounds, warm=3):
    """{arm: median us per call}: the arms' graphs replayed in turn, event-timed, ``rounds`` times after ``warm``"""
    t = {k: [] for k in graphs}
    for r in range(warm + rounds):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            if r >= warm:
                t[k].append(a.elapsed_time(b) * 1e3 / ncalls)
    return {k: statistics.median(v) for k, v in t.items()}


def bench_linears(lines, rounds):
    from pytorch_distributed_nn_amd.ops import kernels as K
    lines.append("1. per linear, us per call in captured graphs of calls rotating over weight copies, arms replayed in turn;")
    lines.append("   fp4 = the kernel's rule of (N, K, MT); rg1 / rg2 = one / two 16-row groups per wave forced (rg2: M <= 32)")
    lines.append("   shape        N      K   M  copies   bf16 us    fp8 us    fp4 us    rg1 us    rg2 us   fp4 / fp8   fp4 / bf16   fp4 GB/s")
    for D in (768, 1024):
        for name, N, Kd, ep in shapes(D):
            copies = max(2, min(64, -(-CACHE_BYTES // (N * Kd))))
            w = [(torch.randn(N, Kd, device="cuda") * 0.02).to(BF) for _ in range(copies)]
            p8 = [K.quant_rows_e4m3(t) for t in w]
            p4 = [K.quant_blocks_mxfp4(t) for t in w]
            bias = torch.randn(N, device="cuda") if ep.get("bias") else None
            n = max(copies, 32) // copies * copies
            for M in MS:
                x = torch.randn(M, Kd, device="cuda").to(BF)
                res = torch.randn(M, N, device="cuda").to(BF) if ep.get("res") else None
                out = torch.empty(M, N, device="cuda", dtype=BF)
                kw = dict(bias=bias, act=ep.get("act", 0), res=res, out=out)
                arms = {"bf16": [lambda i=i: K.gemm_skinny(x, w[i % copies], **kw) for i in range(n)],
                        "fp8": [lambda i=i: K.gemm_skinny_fp8(x, *p8[i % copies], **kw) for i in range(n)]}
                for arm, rg in (("fp4", 0), ("rg1", 1), ("rg2", 2)):
                    if rg < 2 or M <= 32:
                        arms[arm] = [lambda i=i, rg=rg: K.gemm_skinny_fp4(x, *p4[i % copies], groups=rg, **kw) for i in range(n)]
                t = alternate_us({k: graph_of(v) for k, v in arms.items()}, n, rounds)
                rg2 = f"{t['rg2']:8.2f}" if "rg2" in t else "       -"
                lines.append(f"   {name:8s} {N:6d}  {Kd:5d}  {M:2d}  {copies:6d}  {t['bf16']:8.2f}  {t['fp8']:8.2f}  {t['fp4']:8.2f}  "
                             f"{t['rg1']:8.2f}  {rg2}   {t['fp4'] / t['fp8']:9.2f}   {t['fp4'] / t['bf16']:10.2f}   "
                             f"{N * Kd * 17 / 32 / t['fp4'] / 1e3:8.0f}")
            del w, p8, p4
            torch.cuda.empty_cache()


def bench_tokens(lines, rounds):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    arms = ("bf16", "fp8", "mxfp4")
    lines.append("")
    lines.append("2. generate(graph=True, sampler='device', temperature 0.8, top_k 50), ms per token = (t(96 tokens) - t(32 tokens)) / 64,")
    lines.append(f"   median of {rounds} alternating rounds")
    lines.append("   model         B   bf16 ms/token   fp8 ms/token   mxfp4 ms/token   mxfp4 / fp8   mxfp4 / bf16")
    for name in ("gpt2_small", "gpt2_medium"):
        torch.manual_seed(0)
        model = build_gpt2(name).cuda().eval()

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for B in (1, 8):
            idx = torch.randint(0, 50257, (B, 16), device="cuda")
            ms = {a: [] for a in arms}
            for r in range(rounds + 1):                                  # round 0 warms every shape up
                for arm in arms:
                    t = [wall(lambda n=n: model.generate(idx, n, graph=True, sampler="device", seed=1, temperature=0.8,
                                                         top_k=50, decode_weights=arm)) for n in (32, 96)]
                    if r:
                        ms[arm].append((t[1] - t[0]) / 64)
            m = {a: statistics.median(v) for a, v in ms.items()}
            lines.append(f"   {name:12s} {B:2d}   {m['bf16']:12.4f}   {m['fp8']:12.4f}   {m['mxfp4']:14.4f}   "
                         f"{m['mxfp4'] / m['fp8']:11.3f}   {m['mxfp4'] / m['bf16']:12.3f}")
        del model
        torch.cuda.empty_cache()


def bench_logits(lines):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(0)
    model = build_gpt2("gpt2_tiny").cuda().eval()
    idx = torch.randint(0, 512, (8, 16), generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(temperature=0.0, return_logits=True)
    seq, base = model.generate(idx, 4, **kw)
    lines.append("")
    lines.append("3. gpt2_tiny, RANDOM INIT (says nothing about a trained model): relative L2 of the logits against the bf16 weights,")
    lines.append("   worst of 8 rows over the decode steps whose token prefix equals the bf16 run's")
    for arm in ("fp8", "mxfp4"):
        s, lg = model.generate(idx, 4, decode_weights=arm, **kw)
        same = torch.cat([torch.ones(8, 1, device="cuda"), (s[:, 16:19] == seq[:, 16:19]).float().cumprod(1)], 1).bool()
        rel = (lg - base).norm(dim=-1) / base.norm(dim=-1)
        lines.append(f"   {arm:6s} {rel[same].max().item():.3f}   ({int(same.sum())} of {same.numel()} (row, step) pairs compared)")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--rounds", type=int, default=15, help="timed replays per arm of section 1")
    ap.add_argument("--token-rounds", type=int, default=5)
    ap.add_argument("--linears-only", action="store_true", help="section 1 only")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skinny_fp4: needs a GPU (a CPU timing says nothing about the kernels)")
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]         # gfx950: the MI355X
    lines = [f"weight-only MXFP4 decode vs fp8 and bf16 on {torch.cuda.get_device_name(0)} ({arch})", ""]
    bench_linears(lines, args.rounds)
    if not args.linears_only:
        bench_tokens(lines, args.token_rounds)
        bench_logits(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
