#!/usr/bin/env python3
"""The fp8 (e4m3) key/value cache against the bf16 cache (the record behind profiles/attn_decode_fp8.txt).

  1. per call: ops.kernels.attn_decode against attn_decode_fp8 at H = 12, Tmax = 1024, B in {1, 8}, 128 / 512 / 1008
     cached tokens, for each chunk size; us per call inside one captured graph of back-to-back calls that rotate over
     12 caches (the layers of GPT-2 small: the same number in both arms, as a real step walks them), and the achieved
     bytes/s over the visible K and V rows (128 bytes per row in bf16, 68 with codes and scale);
  2. the append + extend pair (kv_cache_append + attn_extend against their fp8 twins), Tq = 64 behind the same caches;
  3. per token: GPT2.generate(graph=True, sampler="device") on gpt2_small (random init) with kv_cache bf16 / fp8 and
     decode_weights bf16 / fp8, all four arms alternating in this process; a prompt of cached - 8 tokens, ms per token =
     the difference of a 24- and an 8-token call over 16 tokens, which cancels the prefill, the capture and the
     quantisation: the 16 tokens run at cached .. cached + 16 cached tokens.

    python tools/bench_kv_fp8.py [--out profiles/attn_decode_fp8.txt]
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
H, TMAX, LAYERS = 12, 1024, 12
CACHED = (128, 512, 1008)


def caches(B):
    """LAYERS (bf16 cache, fp8 cache) pairs of Gaussian K / V, every slot quantised by the fill kernel"""
    from pytorch_distributed_nn_amd.ops import kernels as K
    out = []
    for _ in range(LAYERS):
        qkv = torch.randn(B * TMAX, 3 * H * 64, device="cuda").to(BF)
        c16 = [torch.empty(B, H, TMAX, 64, device="cuda", dtype=BF) for _ in range(2)]
        c8 = [torch.empty(B, H, TMAX, 64, device="cuda", dtype=torch.uint8) for _ in range(2)] + \
             [torch.empty(B, H, TMAX, device="cuda") for _ in range(2)]
        K.kv_cache_fill(qkv, *c16, B, TMAX)
        K.kv_cache_fill_fp8(qkv, *c8, B, TMAX)
        out.append((c16, c8))
    return out


def bench_calls(lines, reps):
    from pytorch_distributed_nn_amd.ops import kernels as K
    lines.append(f"1. attn_decode vs attn_decode_fp8, H = {H}, Tmax = {TMAX}; us per call in a captured graph of calls rotating over")
    lines.append(f"   {LAYERS} caches; GB/s over the visible K and V rows (bf16 128 B / row, fp8 68 B / row)")
    lines.append("    B  cached  chunk   bf16 us   GB/s    fp8 us   GB/s   fp8 / bf16 time")
    ext = ["", "2. kv_cache_append + attn_extend vs their fp8 twins, Tq = 64 behind the cached tokens, us per pair",
           "    B  cached   bf16 us    fp8 us   fp8 / bf16 time"]
    for B in (1, 8):
        cs = caches(B)
        qkv = torch.randn(B, 3 * H * 64, device="cuda").to(BF)
        qext = torch.randn(B * 64, 3 * H * 64, device="cuda").to(BF)
        n = 2 * LAYERS
        for cached in CACHED:
            lens = torch.full((B,), cached, dtype=torch.int32, device="cuda")
            rows = 2 * B * H * cached
            for chunk in K.DECODE_CHUNKS:
                out = torch.empty(B, H * 64, device="cuda", dtype=BF)
                part = torch.empty(K.attn_decode_ws(B, H, TMAX, chunk), device="cuda")
                kw = dict(chunk=chunk, out=out, part=part)
                t16 = graph_us([lambda i=i: K.attn_decode(qkv, *cs[i % LAYERS][0], lens, **kw) for i in range(n)], reps, 3)
                t8 = graph_us([lambda i=i: K.attn_decode_fp8(qkv, *cs[i % LAYERS][1], lens, **kw) for i in range(n)], reps, 3)
                lines.append(f"   {B:2d}  {cached:6d}  {chunk:5d}  {t16:8.2f}  {rows * 128 / t16 / 1e3:5.0f}  {t8:8.2f}  "
                             f"{rows * 68 / t8 / 1e3:5.0f}   {t8 / t16:6.2f}")
            if cached + 64 > TMAX:
                continue
            out = torch.empty(B * 64, H * 64, device="cuda", dtype=BF)

            def pair(append, extend, c):
                append(qext, *c, lens)
                extend(qext, *c, lens, out=out)
            t16 = graph_us([lambda i=i: pair(K.kv_cache_append, K.attn_extend, cs[i % LAYERS][0]) for i in range(n)], reps, 3)
            t8 = graph_us([lambda i=i: pair(K.kv_cache_append_fp8, K.attn_extend_fp8, cs[i % LAYERS][1]) for i in range(n)],
                          reps, 3)
            ext.append(f"   {B:2d}  {cached:6d}  {t16:8.2f}  {t8:8.2f}   {t8 / t16:6.2f}")
        del cs
        torch.cuda.empty_cache()
    lines.extend(ext)


def bench_tokens(lines, rounds):
    from pytorch_distributed_nn_amd.generation import DecodeWeights
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    arms = [(kv, dw) for dw in ("bf16", "fp8") for kv in ("bf16", "fp8")]
    lines.append("")
    lines.append("3. gpt2_small generate(graph=True, sampler='device', temperature 0.8, top_k 50), prompt = cached - 8 tokens,")
    lines.append(f"   ms per token = (t(24 tokens) - t(8 tokens)) / 16, median of {rounds} alternating rounds; columns kv_cache / decode_weights")
    lines.append("    B  cached   " + "   ".join(f"{kv:>4s} / {dw:<4s}" for kv, dw in arms) + "   fp8 kv / bf16 kv (bf16 w, fp8 w)")
    torch.manual_seed(0)
    model = build_gpt2("gpt2_small").cuda().eval()
    dec = {"bf16": "bf16", "fp8": DecodeWeights(model)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for B in (1, 8):
        for cached in CACHED:
            idx = torch.randint(0, 50257, (B, cached - 8), device="cuda")
            ms = {a: [] for a in arms}
            for r in range(rounds + 1):                                  # round 0 warms every shape up
                for kv, dw in arms:
                    t = [wall(lambda n=n: model.generate(idx, n, graph=True, sampler="device", seed=1, temperature=0.8,
                                                         top_k=50, decode_weights=dec[dw], kv_cache=kv)) for n in (8, 24)]
                    if r:
                        ms[(kv, dw)].append((t[1] - t[0]) / 16)
            m = {a: statistics.median(v) for a, v in ms.items()}
            lines.append(f"   {B:2d}  {cached:6d}   " + "   ".join(f"{m[a]:11.4f}" for a in arms) +
                         f"   {m[('fp8', 'bf16')] / m[('bf16', 'bf16')]:.3f}, {m[('fp8', 'fp8')] / m[('bf16', 'fp8')]:.3f}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls-only", action="store_true", help="sections 1 and 2 only")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_fp8: needs a GPU (a CPU timing says nothing about the kernels)")
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]         # gfx950: the MI355X
    lines = [f"fp8 (e4m3) key/value cache vs bf16 on {torch.cuda.get_device_name(0)} ({arch})", ""]
    bench_calls(lines, args.reps)
    if not args.calls_only:
        bench_tokens(lines, args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
