#!/usr/bin/env python3
"""Decode-path timings on one GPU (the record behind ops.kernels.DECODE_CHUNK, profiles/attention_decode.txt):

  1. attn_decode alone at H = 12, B in {1, 8}, lens in {127, 1023}, chunk in {64, 128, 256}: us per call and the
     achieved bytes/s over the K + V bytes the call must read (2 * B * H * (lens + 1) * 128 bytes);
  2. ms per token of GPT-2 small at B in {1, 8}: generate() eager and graph=True, and the uncached loop that re-runs the
     full forward (padded to 128) per token;
  3. the share of one eager decode step spent in the M = B linears (the case for a skinny-M GEMM).

One process, warm-up first, many iterations, medians of per-iteration event timings.  Nothing here is a pass/fail gate.
    python tools/bench_decode.py [--out profiles/attention_decode.txt] [--iters 200] [--tokens 64]"""
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
    lines.append("attn_decode alone, H = 12, Tmax = 1024 (median of %d calls, 50 warm-up)" % iters)
    lines.append("   B   lens  chunk      us    GB/s over K+V")
    best = {}
    for B in (1, 8):
        qkv = torch.randn(B, 3 * H * 64, device="cuda").to(torch.bfloat16)
        kc = torch.randn(B, H, Tmax, 64, device="cuda").to(torch.bfloat16)
        vc = torch.randn(B, H, Tmax, 64, device="cuda").to(torch.bfloat16)
        out = torch.empty(B, H * 64, device="cuda", dtype=torch.bfloat16)
        for n in (127, 1023):
            lens = torch.full((B,), n, device="cuda", dtype=torch.int32)
            for chunk in K.DECODE_CHUNKS:
                part = torch.empty(K.attn_decode_ws(B, H, Tmax, chunk), device="cuda")
                ms = timed(lambda: K.attn_decode(qkv, kc, vc, lens, chunk=chunk, out=out, part=part), iters, 50)
                nbytes = 2 * B * H * (n + 1) * 128
                lines.append(f"  {B:2d}  {n:5d}  {chunk:5d}  {ms * 1e3:6.1f}  {nbytes / (ms * 1e-3) / 1e9:8.1f}")
                best.setdefault((B, n), []).append((ms, chunk))
    # the chunk whose time, relative to the best chunk of each (B, lens), is smallest in total
    rel = {c: sum(dict((c2, m) for m, c2 in v)[c] / min(v)[0] for v in best.values()) for c in K.DECODE_CHUNKS}
    pick = min(rel, key=rel.get)
    lines.append(f"fastest chunk per (B, lens): {dict((k, min(v)[1]) for k, v in best.items())}")
    lines.append("sum over (B, lens) of time / best time: " + ", ".join(f"chunk {c}: {r:.3f}" for c, r in rel.items()))
    lines.append(f"chosen chunk: {pick}; ops.kernels.DECODE_CHUNK = {K.DECODE_CHUNK}")
    lines.append("")


def bench_model(lines, tokens):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    from pytorch_distributed_nn_amd.ops import linear as BL
    torch.manual_seed(0)
    m = build_gpt2("gpt2_small").cuda().eval()
    P = 128
    lines.append(f"GPT-2 small, prompt {P}, {tokens} new tokens, greedy (ms per token = whole call / tokens, median of 3 calls)")
    lines.append("   B   cached eager   cached graph   uncached full forward")
    for B in (1, 8):
        idx = torch.randint(0, 50257, (B, P), device="cuda")

        def cached(graph):
            def run():
                m.generate(idx, tokens, temperature=0.0, graph=graph)
            return run

        def uncached():
            row = idx
            with torch.no_grad():
                for _ in range(tokens):
                    T = row.shape[1]
                    Tp = (T + 127) // 128 * 128
                    lg = m(torch.nn.functional.pad(row, (0, Tp - T)))[:, T - 1]
                    row = torch.cat([row, lg.argmax(-1, keepdim=True)], 1)
        res = [timed(f, 3, 1) / tokens for f in (cached(False), cached(True), uncached)]
        lines.append(f"  {B:2d}   {res[0]:10.3f}   {res[1]:12.3f}   {res[2]:12.3f}")
    # share of the M = B linears in one eager decode step: time the step's GEMMs alone on the same shapes
    lines.append("")
    lines.append("M = B linears of one decode step (12 x qkv, proj, fc, fc2 + the LM head), timed alone, eager:")
    for B in (1, 8):
        blk = m.transformer.h[0]
        params, sh = blk.fused_params()
        from pytorch_distributed_nn_amd.ops import functional as OF
        wte = OF.weight_bf16(m.transformer.wte.weight)
        x = torch.randn(B, 768, device="cuda").to(torch.bfloat16)
        h = torch.randn(B, 3072, device="cuda").to(torch.bfloat16)

        def gemms():
            for _ in range(12):
                BL.linear_fwd(x, sh[0], bias=params[3])
                BL.linear_fwd(x, sh[1], bias=params[5], res=x)
                BL.linear_fwd(x, sh[2], bias=params[9], act=2)
                BL.linear_fwd(h, sh[3], bias=params[11], res=x)
            BL.linear_fwd(x, wte)
        g = timed(gemms, 20, 5)
        idx = torch.randint(0, 50257, (B, P), device="cuda")
        step = timed(lambda: m.generate(idx, tokens, temperature=0.0), 3, 1) / tokens
        lines.append(f"  B = {B}: linears {g:.3f} ms of an eager step of {step:.3f} ms = {100 * g / step:.0f}%")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode needs a GPU"
    lines = [f"tools/bench_decode.py on {torch.cuda.get_device_name(0)}", ""]
    bench_kernel(lines, a.iters)
    if not a.skip_model:
        bench_model(lines, a.tokens)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
