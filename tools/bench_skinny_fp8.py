#!/usr/bin/env python3
"""Weight-only fp8 decode against the bf16 path (the record behind profiles/gemm_skinny_fp8.txt).

  1. per linear: ops.kernels.gemm_skinny (bf16 shadow) against gemm_skinny_fp8 (e4m3 codes + row scales) at M in {1, 8}
     on the GPT-2 small and medium shapes with their real epilogues; us per call inside one captured graph of
     back-to-back calls that rotate over copies of the weight (the same number of copies in both arms, enough for the
     fp8 copies to exceed the 256 MiB Infinity Cache, at most 64: the small weights then stay cache-resident in both
     arms, as they do between the steps of a real decode loop), and the achieved bytes/s over the weights;
  2. per token: GPT2.generate(graph=True, sampler="device") ms per token at B in {1, 8} with decode_weights bf16 against
     fp8 for gpt2_small and gpt2_medium (random init), both arms alternating in this process; ms per token is the
     difference of a 96- and a 32-token call over 64 tokens, which cancels the prefill, the capture and the quantisation;
  3. the one-off cost of quantising a model (generation.DecodeWeights).

    python tools/bench_skinny_fp8.py [--out profiles/gemm_skinny_fp8.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_decode import graph_us  # noqa: E402

BF = torch.bfloat16
CACHE_BYTES = 300 << 20


def shapes(D):
    return [("qkv", 3 * D, D, dict(bias=True)), ("proj", D, D, dict(bias=True, res=True)),
            ("fc", 4 * D, D, dict(bias=True, act=2)), ("fc2", D, 4 * D, dict(bias=True, res=True)),
            ("lm_head", 50304, D, dict())]


def bench_linears(lines, reps):
    from pytorch_distributed_nn_amd.ops import kernels as K
    lines.append("1. per linear, us per call in a captured graph of calls rotating over weight copies; GB/s over the weight bytes")
    lines.append("   shape        N      K   M  copies   bf16 us   GB/s    fp8 us   GB/s   fp8 / bf16 time")
    for D in (768, 1024):
        for name, N, Kd, ep in shapes(D):
            copies = max(2, min(64, -(-CACHE_BYTES // (N * Kd))))
            w = [(torch.randn(N, Kd, device="cuda") * 0.02).to(BF) for _ in range(copies)]
            pairs = [K.quant_rows_e4m3(t) for t in w]
            bias = torch.randn(N, device="cuda") if ep.get("bias") else None
            for M in (1, 8):
                x = torch.randn(M, Kd, device="cuda").to(BF)
                res = torch.randn(M, N, device="cuda").to(BF) if ep.get("res") else None
                out = torch.empty(M, N, device="cuda", dtype=BF)
                kw = dict(bias=bias, act=ep.get("act", 0), res=res, out=out)
                n = max(copies, 32) // copies * copies
                t16 = graph_us([lambda i=i: K.gemm_skinny(x, w[i % copies], **kw) for i in range(n)], reps, 3)
                t8 = graph_us([lambda i=i: K.gemm_skinny_fp8(x, *pairs[i % copies], **kw) for i in range(n)], reps, 3)
                lines.append(f"   {name:8s} {N:6d}  {Kd:5d}  {M:2d}  {copies:6d}  {t16:8.2f}  {2 * N * Kd / t16 / 1e3:5.0f}  "
                             f"{t8:8.2f}  {N * Kd / t8 / 1e3:5.0f}   {t8 / t16:6.2f}")
            del w, pairs
            torch.cuda.empty_cache()


def bench_tokens(lines, rounds):
    from pytorch_distributed_nn_amd.generation import DecodeWeights
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    lines.append("")
    lines.append("2. generate(graph=True, sampler='device', temperature 0.8, top_k 50), ms per token = (t(96 tokens) - t(32 tokens)) / 64,")
    lines.append(f"   median of {rounds} alternating rounds; 3. quantising the model once (median of 3)")
    lines.append("   model         B   bf16 ms/token   fp8 ms/token   fp8 / bf16   quantise ms")
    for name in ("gpt2_small", "gpt2_medium"):
        torch.manual_seed(0)
        model = build_gpt2(name).cuda().eval()

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        tq = statistics.median(wall(lambda: DecodeWeights(model)) for _ in range(3))
        for B in (1, 8):
            idx = torch.randint(0, 50257, (B, 16), device="cuda")
            ms = {"bf16": [], "fp8": []}
            for r in range(rounds + 1):                                  # round 0 warms every shape up
                for arm in ("bf16", "fp8"):
                    t = [wall(lambda n=n: model.generate(idx, n, graph=True, sampler="device", seed=1, temperature=0.8,
                                                         top_k=50, decode_weights=arm)) for n in (32, 96)]
                    if r:
                        ms[arm].append((t[1] - t[0]) / 64)
            a, b = statistics.median(ms["bf16"]), statistics.median(ms["fp8"])
            lines.append(f"   {name:12s} {B:2d}   {a:12.4f}   {b:12.4f}   {b / a:10.3f}   {tq:10.2f}")
        del model
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--linears-only", action="store_true", help="section 1 only")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skinny_fp8: needs a GPU (a CPU timing says nothing about the kernels)")
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]         # gfx950: the MI355X
    lines = [f"weight-only fp8 decode vs bf16 on {torch.cuda.get_device_name(0)} ({arch})", ""]
    bench_linears(lines, args.reps)
    if not args.linears_only:
        bench_tokens(lines, args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
