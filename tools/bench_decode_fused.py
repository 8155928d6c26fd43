#!/usr/bin/env python3
"""decode_fused against the unfused decode step (the record behind profiles/decode_fused.txt).

  1. per call, the LayerNorm sites (qkv, fc, LM head): ops.kernels.layernorm_fwd + gemm_skinny[_fp8] against the one
     gemm_skinny_ln, at M in {1, 8, 16}, GPT-2 small and medium widths, bf16 and fp8 weights; us per (pair of) call(s)
     inside one captured graph of back-to-back calls that rotate over copies of the weight (as tools/bench_skinny_fp8.py);
     the LM head is not part of decode_fused (it lost here), the kernel still takes its shape;
  2. per token: GPT2.generate(graph=True, sampler="device") ms per token at B in {1, 8}, decode_fused off against on,
     bf16 weights with a bf16 cache and fp8 weights with an fp8 cache, gpt2_small and gpt2_medium (random init), prompts
     of 16 and of 400 tokens.  Both arms alternate in this process; ms per token is the difference of a 96- and a
     32-token call over 64 tokens, which cancels the prefill and the capture.  The spread of the unfused arm (its
     rounds' range) is the margin the option is judged by.

    python tools/bench_decode_fused.py [--out profiles/decode_fused.txt]
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
EPS = 1e-5


def bench_ln_sites(lines, reps):
    from pytorch_distributed_nn_amd.ops import kernels as K
    lines.append("1. LayerNorm sites, us per call in a captured graph of calls rotating over weight copies")
    lines.append("   site       N      D   M  weights   LN + GEMM us   fused us   fused / pair")
    for D in (768, 1024):
        for name, N, ep in (("qkv", 3 * D, dict(bias=True)), ("fc", 4 * D, dict(bias=True, act=2)), ("lm_head", 50304, dict())):
            copies = max(2, min(64, -(-CACHE_BYTES // (N * D))))
            w = [(torch.randn(N, D, device="cuda") * 0.02).to(BF) for _ in range(copies)]
            pairs = [K.quant_rows_e4m3(t) for t in w]
            bias = torch.randn(N, device="cuda") if ep.get("bias") else None
            gam, bet = torch.rand(D, device="cuda") + 0.5, torch.randn(D, device="cuda")
            n = max(copies, 32) // copies * copies
            for M in (1, 8, 16):
                x = torch.randn(M, D, device="cuda").to(BF)
                out = torch.empty(M, N, device="cuda", dtype=BF)
                kw = dict(bias=bias, act=ep.get("act", 0), out=out)
                for fmt, ws in (("bf16", w), ("fp8", pairs)):
                    def pair(i, ws=ws, fmt=fmt):
                        xn = K.layernorm_fwd(x, gam, bet, EPS)[0]
                        return K.gemm_skinny(xn, ws[i], **kw) if fmt == "bf16" else K.gemm_skinny_fp8(xn, *ws[i], **kw)
                    t0 = graph_us([lambda i=i: pair(i % copies) for i in range(n)], reps, 3)
                    t1 = graph_us([lambda i=i, ws=ws: K.gemm_skinny_ln(x, gam, bet, EPS, ws[i % copies], **kw) for i in range(n)],
                                  reps, 3)
                    lines.append(f"   {name:8s} {N:6d}  {D:5d}  {M:2d}  {fmt:5s}   {t0:12.2f}  {t1:9.2f}   {t1 / t0:10.2f}")
            del w, pairs
            torch.cuda.empty_cache()


def bench_tokens(lines, rounds):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    lines.append("")
    lines.append("2. generate(graph=True, sampler='device', temperature 0.8, top_k 50), ms per token = (t(96 tokens) - t(32 tokens)) / 64,")
    lines.append(f"   median of {rounds} alternating rounds; spread = the range of the unfused arm's rounds")
    lines.append("   model         weights/cache  B  prompt   unfused    spread     fused   fused / unfused")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for name in ("gpt2_small", "gpt2_medium"):
        torch.manual_seed(0)
        model = build_gpt2(name).cuda().eval()
        for fmt in ("bf16", "fp8"):
            for B, P in ((1, 16), (8, 16), (1, 400), (8, 400)):
                idx = torch.randint(0, 50257, (B, P), device="cuda")
                ms = {False: [], True: []}
                for r in range(rounds + 1):                              # round 0 warms every shape up
                    for on in (False, True):
                        t = [wall(lambda n=n: model.generate(idx, n, graph=True, sampler="device", seed=1, temperature=0.8,
                                                             top_k=50, decode_weights=fmt, kv_cache=fmt, decode_fused=on))
                             for n in (32, 96)]
                        if r:
                            ms[on].append((t[1] - t[0]) / 64)
                a, b = statistics.median(ms[False]), statistics.median(ms[True])
                lines.append(f"   {name:12s}  {fmt:5s}/{fmt:5s}   {B:2d}  {P:4d}   {a:7.4f}   {max(ms[False]) - min(ms[False]):7.4f}   "
                             f"{b:7.4f}   {b / a:15.3f}")
        del model
        torch.cuda.empty_cache()


class _Report(list):
    """the report's lines, each printed as it is measured"""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls-only", action="store_true", help="section 1 only")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_fused: needs a GPU (a CPU timing says nothing about the kernels)")
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]         # gfx950: the MI355X
    lines = _Report()
    lines.append(f"decode_fused vs the unfused decode step on {torch.cuda.get_device_name(0)} ({arch})")
    lines.append("")
    bench_ln_sites(lines, args.reps)
    if not args.calls_only:
        bench_tokens(lines, args.rounds)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
