#!/usr/bin/env python3
"""Quantised-weight prefill against the bf16 path (the record behind profiles/gemm_wq.txt).

  1. per linear: ops.linear.linear_fwd (the bf16 shadow on the GEMM engines), ops.kernels.gemm_wq_fp8 and gemm_wq_fp4
     (the kernel's rule of (M, N)), and gemm_wq_fp8 with the 64- and the 128-row tile forced, at M in {64, 128, 1024, 8192}
     on the four block linears of GPT-2 small and medium with their real epilogues.  us per call inside one captured
     graph per arm of back-to-back calls rotating over four copies of the weight; the arms' graphs are replayed in turn
     in this process, median over the rounds, and the spread (max - min) / median of each arm's rounds is reported;
  2. per prefill: GPT2.generate(max_new_tokens=1) wall ms at B in {1, 8}, P in {128, 1023} (1023 + the one new token is
     the block size; the prefill pads to 1024 rows per sequence) with decode_weights bf16, fp8 and mxfp4, the quantised
     ones with prefill_weights both ways on a DecodeWeights made once, the arms alternating in this process.

    python tools/bench_wq.py [--out profiles/gemm_wq.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_skinny_fp4 import graph_of  # noqa: E402
from bench_skinny_fp8 import shapes  # noqa: E402

BF = torch.bfloat16
MS = (64, 128, 1024, 8192)
COPIES = 4


def alternate(graphs, ncalls, rounds, warm=3):
    """{arm: (median us per call, (max - min) / median over the rounds)}: the arms' graphs replayed in turn, event-timed"""
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
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in t.items()}


def bench_linears(lines, rounds):
    from pytorch_distributed_nn_amd.ops import kernels as K
    from pytorch_distributed_nn_amd.ops import linear as BL
    from pytorch_distributed_nn_amd.ops._backend import lib
    lines.append("1. per linear, us per call in captured graphs of calls rotating over weight copies, arms replayed in turn;")
    lines.append("   fp8 / fp4 = the kernel's tile rule of (M, N); t64 / t128 = gemm_wq_fp8 with that tile forced; spread = the")
    lines.append("   largest (max - min) / median of an arm's rounds in the row")
    lines.append("   shape        N      K      M  tile   bf16 us    fp8 us    fp4 us    t64 us   t128 us   fp8 / bf16   fp4 / bf16   spread")
    for D in (768, 1024):
        for name, N, Kd, ep in shapes(D)[:4]:
            w = [(torch.randn(N, Kd, device="cuda") * 0.02).to(BF) for _ in range(COPIES)]
            p8 = [K.quant_rows_e4m3(t) for t in w]
            p4 = [K.quant_blocks_mxfp4(t) for t in w]
            bias = torch.randn(N, device="cuda")
            for M in MS:
                x = torch.randn(M, Kd, device="cuda").to(BF)
                res = torch.randn(M, N, device="cuda").to(BF) if ep.get("res") else None
                out = torch.empty(M, N, device="cuda", dtype=BF)
                kw = dict(bias=bias, act=ep.get("act", 0), res=res)
                n = 8 if M >= 1024 else 32
                arms = {"bf16": [lambda i=i: BL.linear_fwd(x, w[i % COPIES], **kw) for i in range(n)],
                        "fp8": [lambda i=i: K.gemm_wq_fp8(x, *p8[i % COPIES], out=out, **kw) for i in range(n)],
                        "fp4": [lambda i=i: K.gemm_wq_fp4(x, *p4[i % COPIES], out=out, **kw) for i in range(n)],
                        "t64": [lambda i=i: K.gemm_wq_fp8(x, *p8[i % COPIES], out=out, tile=64, **kw) for i in range(n)],
                        "t128": [lambda i=i: K.gemm_wq_fp8(x, *p8[i % COPIES], out=out, tile=128, **kw) for i in range(n)]}
                t = alternate({k: graph_of(v) for k, v in arms.items()}, n, rounds)
                us = {k: v[0] for k, v in t.items()}
                lines.append(f"   {name:8s} {N:6d}  {Kd:5d}  {M:5d}  {lib().pdnn_gemm_wq_plan(M, N):4d}  {us['bf16']:8.2f}  {us['fp8']:8.2f}  "
                             f"{us['fp4']:8.2f}  {us['t64']:8.2f}  {us['t128']:8.2f}   {us['fp8'] / us['bf16']:10.2f}   "
                             f"{us['fp4'] / us['bf16']:10.2f}   {max(v[1] for v in t.values()):6.3f}")
            del w, p8, p4
            torch.cuda.empty_cache()


def bench_prefill(lines, rounds):
    from pytorch_distributed_nn_amd.generation import DecodeWeights
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    arms = [("bf16", "bf16"), ("fp8", "bf16"), ("fp8", "decode"), ("mxfp4", "bf16"), ("mxfp4", "decode")]
    lines.append("")
    lines.append(f"2. generate(max_new_tokens=1, temperature 0), wall ms per call, median of {rounds} alternating rounds;")
    lines.append("   columns: decode_weights / prefill_weights; the last two: prefill on the codes over prefill on the shadows")
    lines.append("   model         B     P   bf16/bf16   fp8/bf16   fp8/decode   mxfp4/bf16   mxfp4/decode   fp8 ratio   mxfp4 ratio")
    for name in ("gpt2_small", "gpt2_medium"):
        torch.manual_seed(0)
        model = build_gpt2(name).cuda().eval()
        dec = {"bf16": "bf16", "fp8": DecodeWeights(model, "fp8"), "mxfp4": DecodeWeights(model, "mxfp4")}
        for B in (1, 8):
            for P in (128, 1023):
                idx = torch.randint(0, 50257, (B, P), device="cuda")
                ms = {a: [] for a in arms}
                for r in range(rounds + 1):                                  # round 0 warms every shape up
                    for a in arms:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        model.generate(idx, 1, temperature=0.0, decode_weights=dec[a[0]], prefill_weights=a[1])
                        torch.cuda.synchronize()
                        if r:
                            ms[a].append((time.perf_counter() - t0) * 1e3)
                m = {a: statistics.median(v) for a, v in ms.items()}
                lines.append(f"   {name:12s} {B:2d}  {P:4d}   {m[arms[0]]:9.3f}  {m[arms[1]]:9.3f}   {m[arms[2]]:10.3f}   {m[arms[3]]:10.3f}   "
                             f"{m[arms[4]]:12.3f}   {m[arms[2]] / m[arms[1]]:9.3f}   {m[arms[4]] / m[arms[3]]:11.3f}")
        del model, dec
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--rounds", type=int, default=10, help="timed replays per arm of section 1")
    ap.add_argument("--prefill-rounds", type=int, default=5)
    ap.add_argument("--linears-only", action="store_true", help="section 1 only")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wq: needs a GPU (a CPU timing says nothing about the kernels)")
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]         # gfx950: the MI355X
    lines = [f"quantised-weight prefill (weight-only fp8 / MXFP4 GEMM for many rows) vs bf16 on {torch.cuda.get_device_name(0)} ({arch})", ""]
    bench_linears(lines, args.rounds)
    if not args.linears_only:
        bench_prefill(lines, args.prefill_rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
