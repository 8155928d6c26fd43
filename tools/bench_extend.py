#!/usr/bin/env python3
"""Extend-attention timings on one GPU (the record in profiles/attn_extend.txt):

1. kv_cache_append + attn_extend alone (csrc/kernels/attention_extend.hip), H = 12, Tmax = 1024, at (B, Tq, cached) in
   {1, 8} x {64, 128} x {0, 512, 896}: us per call pair, the blocks of the grid and the MFMA TFLOP/s over the visible
   (query, key) pairs.
2. GPT-2 small, second-turn latency: a 64-token turn plus ``--tokens`` greedy tokens behind 512 and 896 cached tokens,
   through generate(resume=True) on the kept cache, against the only way without it: generate on the concatenated
   history (prefill of everything, padded to 128).  Both end with the same number of decode steps.

One process, warm-up first, medians of event timings.  Nothing here is a pass/fail gate.
    python tools/bench_extend.py [--out profiles/attn_extend.txt] [--iters 200] [--tokens 16] [--reps 10]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup):
    """median ms of fn() over ``iters`` event-timed calls after ``warmup`` untimed ones"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def bench_kernel(lines, iters):
    from pytorch_distributed_nn_amd.ops import kernels as K
    H, Tmax = 12, 1024
    lines.append(f"1. kv_cache_append + attn_extend, H = {H}, Tmax = {Tmax}, tile = {K.EXTEND_TILE} queries per block "
                 f"(median of {iters} call pairs, 50 warm-up)")
    lines.append("    B    Tq  cached  blocks  append us  extend us  TFLOP/s (visible pairs)")
    for B in (1, 8):
        kc = torch.randn(B, H, Tmax, 64, device="cuda").to(torch.bfloat16)
        vc = torch.randn(B, H, Tmax, 64, device="cuda").to(torch.bfloat16)
        for Tq in (64, 128):
            qkv = torch.randn(B * Tq, 3 * H * 64, device="cuda").to(torch.bfloat16)
            out = torch.empty(B * Tq, H * 64, device="cuda", dtype=torch.bfloat16)
            for n in (0, 512, 896):
                lens = torch.full((B,), n, device="cuda", dtype=torch.int32)
                ta = timed(lambda: K.kv_cache_append(qkv, kc, vc, lens), iters, 50)
                te = timed(lambda: K.attn_extend(qkv, kc, vc, lens, out=out), iters, 50)
                pairs = B * H * (Tq * n + Tq * (Tq + 1) // 2)
                lines.append(f"   {B:2d}  {Tq:4d}  {n:6d}  {B * H * Tq // K.EXTEND_TILE:6d}  {ta * 1e3:9.1f}  {te * 1e3:9.1f}  "
                             f"{4 * 64 * pairs / (te * 1e-3) / 1e12:7.2f}")
    lines.append("")


def bench_turn(lines, tokens, reps):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    from pytorch_distributed_nn_amd.ops import transformer as TX
    torch.manual_seed(0)
    model = build_gpt2("gpt2_small").cuda().eval()
    turn = 64
    lines.append(f"2. GPT-2 small, one sequence: a {turn}-token turn + {tokens} greedy tokens behind a cached history "
                 f"(median ms of {reps} calls, 2 warm-up; eager loop, torch sampler)")
    lines.append("   cached   resume ms   full-history generate ms   full / resume")
    for n in (512, 896):
        hist = torch.randint(0, 50000, (1, n + turn), device="cuda")
        cache = TX.KVCache(model, 1, 1024, "cuda")
        model.generate(hist[:, :n], 1, temperature=0.0, cache=cache)          # fills slots 0..n-1 (and runs one step)

        def resumed():
            cache.truncate(n)
            model.generate(hist[:, n:], tokens, temperature=0.0, cache=cache, resume=True)

        def full():
            model.generate(hist, tokens, temperature=0.0, cache=cache)
        tr, tf = timed(resumed, reps, 2), timed(full, reps, 2)
        lines.append(f"   {n:6d}   {tr:9.2f}   {tf:24.2f}   {tf / tr:12.2f}x")
    lines.append("")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tokens", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    lines = ["Extend attention (csrc/kernels/attention_extend.hip) and resumed GPT-2 generation: tools/bench_extend.py on one "
             f"{torch.cuda.get_device_name(0)}.", ""]
    bench_kernel(lines, args.iters)
    bench_turn(lines, args.tokens, args.reps)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
