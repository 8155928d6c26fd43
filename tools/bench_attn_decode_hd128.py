#!/usr/bin/env python3
"""The head-dim-128 decode attention kernels against the head-dim-64 ones at equal cache bytes (the record behind
profiles/attn_decode_hd128.txt).

  calls:  ops.kernels.attn_decode and attn_decode_multi (S = 4) at head dim 128 with H = 8 against head dim 64 with
          H = 16 (the same K and V bytes), Tmax = 1024, B in {1, 8}, 128 / 512 / 1008 cached tokens, for each chunk size;
          us per call inside one captured graph of back-to-back calls that rotate over 12 caches, both arms captured in
          this process and replayed in alternating rounds; median over the rounds and their spread (max - min) / median.
  tokens: GPT2.generate(graph=True, sampler="device") on a 12-layer n_embd = 1024 model (random init) with n_head = 8
          (head dim 128) against its n_head = 16 twin (head dim 64), alternating; ms per token = the difference of a 24-
          and an 8-token call over 16 tokens, which cancels the prefill and the capture.

Each section runs in a child process of its own under a time limit, and a failed section ends the run.

    python tools/bench_attn_decode_hd128.py [--out profiles/attn_decode_hd128.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_decode import timed  # noqa: E402

BF = torch.bfloat16
TMAX, LAYERS, S = 1024, 12, 4
ARMS = ((128, 8), (64, 16))                     # (head dim, heads): 1024 columns both
CACHED = (128, 512, 1008)
LIMIT = {"calls": 300, "tokens": 300}          # seconds per section


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def bench_calls(lines, reps, rounds):
    from pytorch_distributed_nn_amd.ops import kernels as K
    lines.append(f"calls: head dim 128, H = 8 against head dim 64, H = 16; Tmax = {TMAX}; us per call in a captured graph of "
                 f"{2 * LAYERS} calls rotating")
    lines.append(f"   over {LAYERS} caches, median of {rounds} alternating rounds of {reps} replays (+- spread = (max - min) / median)")
    lines.append("   entry    B  cached  chunk    d128 us  spread    d64 us  spread   d128 / d64")
    n = 2 * LAYERS
    for B in (1, 8):
        cs = {d: [[torch.randn(B, H, TMAX, d, device="cuda").to(BF) for _ in range(2)] for _ in range(LAYERS)] for d, H in ARMS}
        for name, rows in (("single", B), ("multi", B * S)):
            qkv = {d: torch.randn(rows, 3 * H * d, device="cuda").to(BF) for d, H in ARMS}
            for cached in CACHED:
                lens = torch.full((B,), cached, dtype=torch.int32, device="cuda")
                for chunk in K.DECODE_CHUNKS:
                    graphs = {}
                    for d, H in ARMS:
                        out = torch.empty(rows, H * d, device="cuda", dtype=BF)
                        part = torch.empty(K.attn_decode_multi_ws(B, S, H, TMAX, chunk, d=d), device="cuda")
                        kw = dict(chunk=chunk, out=out, part=part)
                        if name == "single":
                            calls = [lambda i=i, d=d, kw=kw: K.attn_decode(qkv[d], *cs[d][i % LAYERS], lens, **kw) for i in range(n)]
                        else:
                            calls = [lambda i=i, d=d, kw=kw: K.attn_decode_multi(qkv[d], *cs[d][i % LAYERS], lens, S, **kw)
                                     for i in range(n)]
                        calls[0]()
                        torch.cuda.synchronize()
                        graphs[d] = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graphs[d]):
                            for f in calls:
                                f()
                    t = {d: [] for d, _ in ARMS}
                    for _ in range(rounds):
                        for d, _ in ARMS:
                            t[d].append(timed(graphs[d].replay, reps, 3) * 1e3 / n)
                    (a, sa), (b, sb) = med_spread(t[128]), med_spread(t[64])
                    lines.append(f"   {name:6s}  {B:2d}  {cached:6d}  {chunk:5d}   {a:8.2f}  {sa:5.1%}  {b:8.2f}  {sb:5.1%}   {a / b:8.2f}")
        del cs
        torch.cuda.empty_cache()


def bench_tokens(lines, rounds):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    lines.append("tokens: 12 layers, n_embd = 1024, generate(graph=True, sampler='device', temperature 0.8, top_k 50), prompt = cached - 8")
    lines.append(f"   tokens, ms per token = (t(24 tokens) - t(8 tokens)) / 16, median of {rounds} alternating rounds (+- spread)")
    lines.append("    B  cached   n_head 8 (d128)  spread   n_head 16 (d64)  spread   d128 / d64")
    torch.manual_seed(0)
    models = {h: build_gpt2("gpt2_small", n_embd=1024, n_head=h).cuda().eval() for h in (8, 16)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for B in (1, 8):
        for cached in CACHED:
            idx = torch.randint(0, 50257, (B, cached - 8), device="cuda")
            ms = {h: [] for h in models}
            for r in range(rounds + 1):                                  # round 0 warms every shape up
                for h, m in models.items():
                    t = [wall(lambda n=n: m.generate(idx, n, graph=True, sampler="device", seed=1, temperature=0.8, top_k=50))
                         for n in (8, 24)]
                    if r:
                        ms[h].append((t[1] - t[0]) / 16)
            (a, sa), (b, sb) = med_spread(ms[8]), med_spread(ms[16])
            lines.append(f"   {B:2d}  {cached:6d}   {a:15.4f}  {sa:5.1%}   {b:15.4f}  {sb:5.1%}   {a / b:8.3f}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--section", choices=sorted(LIMIT), default=None, help="run this section here (the driver starts these)")
    args = ap.parse_args(argv)
    if args.section:                            # a child: the only process that opens the GPU
        if not torch.cuda.is_available():
            raise SystemExit("bench_attn_decode_hd128: needs a GPU (a CPU timing says nothing about the kernels)")
        lines = []
        if args.section == "calls":
            arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
            lines += [f"decode attention at head dim 128 vs head dim 64 on {torch.cuda.get_device_name(0)} ({arch})", ""]
            bench_calls(lines, args.reps, args.rounds)
        else:
            bench_tokens(lines, args.rounds)
        print("\n".join(lines))
        return
    text = ""
    for section in ("calls", "tokens"):         # each under its own limit; a failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", section, "--reps", str(args.reps),
                            "--rounds", str(args.rounds)], stdout=subprocess.PIPE, text=True, timeout=LIMIT[section])
        if r.returncode != 0:
            raise SystemExit(f"bench_attn_decode_hd128: section {section} ended with status {r.returncode}")
        text += r.stdout + "\n"
        print(r.stdout)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
