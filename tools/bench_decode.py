#!/usr/bin/env python3
"""Decode-path timings on one GPU (the record behind ops.kernels.DECODE_CHUNK, profiles/attention_decode.txt):

  1. attn_decode alone at H = 12, B in {1, 8}, lens in {127, 1023}, chunk in {64, 128, 256}: us per call and the
     achieved bytes/s over the K + V bytes the call must read (2 * B * H * (lens + 1) * 128 bytes);
  2. ms per token of GPT-2 small at B in {1, 8}: generate() eager and graph=True, and the uncached loop that re-runs the
     full forward (padded to 128) per token;
  3. the share of one eager decode step spent in the M = B linears (the case for a skinny-M GEMM).

With --skinny (the record behind ops.kernels.SKINNY_MAX_M, profiles/gemm_skinny.txt) instead:

  1. gemm_skinny against gemm_nt_ex (the path before it) on the five linears of GPT-2 small with their real epilogues,
     M in {1, 2, 4, 8, 16, 32, 64}: us per call and GB/s over the weight bytes.  A call is timed inside a captured graph
     of back-to-back calls that rotate over enough copies of the weight to exceed the 256 MiB Infinity Cache, so the
     weights come from HBM as in a decode step and the figure includes the kernel boundary, not the host's launch cost;
  2. the largest M of that list up to which the skinny kernel is faster on all five shapes (SKINNY_MAX_M);
  3. the model section at tuning decode_skinny = 1 and = 0 (0 is the path before the kernel, bit for bit: a same-process
     A/B), and the linears' share of the eager step at both.

With --sample (profiles/sample_decode.txt) instead:

  (a) one call of GPT2._sample (eager torch: topk, masked_fill, sort, softmax, multinomial) against one launch of
      sample_logits at V = 50 304, B in {1, 8}, (k, p) in {(None, None), (50, None), (None, 0.9), (50, 0.9)}, both logits
      dtypes (the torch sampler needs fp32: its bf16 figure includes the fp32 copy generate() makes); median us per call;
  (b) ms per token of GPT-2 small, prompt 128, top_k = 50, top_p = 0.9: sampler="torch" eager and graph=True,
      sampler="device" graph=True, and the greedy graph=True figure (the path of the parent commit) as the floor.

One process, warm-up first, many iterations, medians of per-iteration event timings.  Nothing here is a pass/fail gate.
    python tools/bench_decode.py [--out profiles/attention_decode.txt] [--iters 200] [--tokens 64]
    python tools/bench_decode.py --skinny [--out profiles/gemm_skinny.txt]
    python tools/bench_decode.py --sample [--out profiles/sample_decode.txt]"""
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


SKINNY_SHAPES = [("qkv", 2304, 768, dict(bias=True)), ("proj", 768, 768, dict(bias=True, res=True)),
                 ("fc", 3072, 768, dict(bias=True, act=2)), ("fc2", 768, 3072, dict(bias=True, res=True)),
                 ("lm_head", 50304, 768, dict())]
SKINNY_MS = [1, 2, 4, 8, 16, 32, 64]
HBM_GBS, BOUNDARY_US = 6300.0, (1.2, 1.45)            # the achievable HBM rate and the kernel-boundary floor


def graph_us(calls, reps, warm):
    """median us per call of a captured graph of ``calls`` (a list of thunks, run back to back on one stream)"""
    for f in calls[:4]:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in calls:
            f()
    return timed(g.replay, reps, warm) * 1e3 / len(calls)


def bench_skinny(lines, reps):
    from pytorch_distributed_nn_amd.ops import kernels as K
    bf = torch.bfloat16
    lines.append("1. gemm_skinny vs gemm_nt_ex, the five linears of GPT-2 small with their epilogues; us per call inside a")
    lines.append("   captured graph of calls rotating over > 256 MiB of weight copies (HBM-resident weights, boundary included;")
    lines.append(f"   median of {reps} replays); GB/s over the weight bytes.  For scale: {HBM_GBS / 1e3:.1f} TB/s achievable HBM rate,")
    lines.append(f"   {BOUNDARY_US[0]}-{BOUNDARY_US[1]} us kernel-boundary floor per call.")
    lines.append("   shape      N      K    M   skinny us   GB/s   nt_ex us   GB/s   speed-up   floor us (bytes / 6.3 TB/s)")
    faster = {M: True for M in SKINNY_MS}
    for name, N, Kd, ep in SKINNY_SHAPES:
        nbytes = 2 * N * Kd
        ncopy = max(2, -(-320 * 2 ** 20 // nbytes))
        ws = [(torch.randn(N, Kd, device="cuda") * 0.02).to(bf) for _ in range(ncopy)]
        bias = torch.randn(N, device="cuda") if ep.get("bias") else None
        for M in SKINNY_MS:
            x = torch.randn(M, Kd, device="cuda").to(bf)
            res = torch.randn(M, N, device="cuda").to(bf) if ep.get("res") else None
            out = torch.empty(M, N, device="cuda", dtype=bf)
            act = ep.get("act", 0)
            t = {}
            for kind, fn in (("skinny", K.gemm_skinny), ("nt_ex", K.gemm_nt_ex)):
                calls = [(lambda w=w, fn=fn: fn(x, w, bias=bias, act=act, res=res, out=out)) for w in ws]
                t[kind] = graph_us(calls, reps, 3)
            faster[M] = faster[M] and t["skinny"] < t["nt_ex"]
            lines.append(f"   {name:8s} {N:5d}  {Kd:5d}  {M:3d}   {t['skinny']:9.2f}  {nbytes / t['skinny'] / 1e3:5.0f}   "
                         f"{t['nt_ex']:8.2f}  {nbytes / t['nt_ex'] / 1e3:5.0f}   {t['nt_ex'] / t['skinny']:7.2f}x   "
                         f"{nbytes / HBM_GBS / 1e3:6.2f}")
        del ws
    lines.append("")
    pick = 0
    for M in SKINNY_MS:
        if not faster[M]:
            break
        pick = M
    lines.append("2. skinny faster than gemm_nt_ex on all five shapes: " + ", ".join(f"M={M}: {'yes' if faster[M] else 'no'}" for M in SKINNY_MS))
    lines.append(f"   largest M up to which it is faster on all five: {pick}; ops.kernels.SKINNY_MAX_M = {K.SKINNY_MAX_M}")
    lines.append("")


def bench_model_ab(lines, tokens):
    """the model section at decode_skinny = 1 and 0 (0 = the path before gemm_skinny, bit for bit)"""
    from pytorch_distributed_nn_amd import tuning
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    from pytorch_distributed_nn_amd.ops import functional as OF
    from pytorch_distributed_nn_amd.ops import linear as BL
    torch.manual_seed(0)
    m = build_gpt2("gpt2_small").cuda().eval()
    P = 128
    lines.append(f"3. GPT-2 small, prompt {P}, {tokens} new tokens, greedy; ms per token = whole call / tokens, median of 5 calls;")
    lines.append("   decode_skinny = 0 is the path before the kernel (same process, same box)")
    lines.append("   B   decode_skinny   cached eager   cached graph   graph / eager   linears alone (eager)   share of eager step")
    old = tuning.get("decode_skinny")
    res = {}
    for B in (1, 8):
        idx = torch.randint(0, 50257, (B, P), device="cuda")
        params, sh = m.transformer.h[0].fused_params()
        wte = OF.weight_bf16(m.transformer.wte.weight)
        x = torch.randn(B, 768, device="cuda").to(torch.bfloat16)
        h = torch.randn(B, 3072, device="cuda").to(torch.bfloat16)

        def gemms():
            for _ in range(12):
                BL.linear_fwd_decode(x, sh[0], bias=params[3])
                BL.linear_fwd_decode(x, sh[1], bias=params[5], res=x)
                BL.linear_fwd_decode(x, sh[2], bias=params[9], act=2)
                BL.linear_fwd_decode(h, sh[3], bias=params[11], res=x)
            BL.linear_fwd_decode(x, wte)
        for v in (1, 0, 1, 0):                                     # interleaved rounds; the second round is reported too
            tuning.set("decode_skinny", v)
            e = timed(lambda: m.generate(idx, tokens, temperature=0.0), 5, 1) / tokens
            g = timed(lambda: m.generate(idx, tokens, temperature=0.0, graph=True), 5, 1) / tokens
            lin = timed(gemms, 20, 5)
            res.setdefault((B, v), []).append((e, g))
            lines.append(f"  {B:2d}   {v:13d}   {e:12.3f}   {g:12.3f}   {g / e:13.2f}   {lin:21.3f}   {100 * lin / e:18.0f}%")
    tuning.set("decode_skinny", old)
    for B in (1, 8):
        e1, g1 = (min(r[i] for r in res[(B, 1)]) for i in (0, 1))
        e0, g0 = (min(r[i] for r in res[(B, 0)]) for i in (0, 1))
        lines.append(f"   B = {B}: eager {e0:.3f} -> {e1:.3f} ms / token ({e0 / e1:.2f}x), graph {g0:.3f} -> {g1:.3f} ({g0 / g1:.2f}x); "
                     f"graph=True vs eager with the kernel: {e1 / g1:.2f}x")
    lines.append("")


def bench_sample(lines, iters, tokens, skip_model):
    from pytorch_distributed_nn_amd.models.gpt2 import GPT2, build_gpt2
    from pytorch_distributed_nn_amd.ops import kernels as K
    V = 50304
    lines.append(f"(a) one sampling call at V = {V}, temperature 0.8: GPT2._sample (eager torch) against sample_logits (one launch);")
    lines.append(f"    median us per call of {iters} event-timed calls, 20 warm-up; torch on bf16 logits includes its fp32 copy")
    lines.append("   B   top_k   top_p   dtype   torch us   device us   torch / device")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for B in (1, 8):
        x32 = torch.randn(B, V, device="cuda") * 3
        tok = torch.zeros(B, dtype=torch.int64, device="cuda")
        state = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
        for k, p in ((None, None), (50, None), (None, 0.9), (50, 0.9)):
            for dt in (torch.bfloat16, torch.float32):
                x = x32.to(dt)
                t = timed(lambda: GPT2._sample(x.float() if dt != torch.float32 else x, 0.8, k, gen, p), iters, 20) * 1e3
                d = timed(lambda: K.sample_logits(x, tok, state, temperature=0.8, top_k=k, top_p=p), iters, 20) * 1e3
                lines.append(f"  {B:2d}   {str(k):>5s}   {str(p):>5s}   {'bf16' if dt == torch.bfloat16 else 'fp32'}   {t:8.1f}   "
                             f"{d:9.1f}   {t / d:14.2f}")
    lines.append("")
    if skip_model:
        return
    torch.manual_seed(0)
    m = build_gpt2("gpt2_small").cuda().eval()
    P = 128
    lines.append(f"(b) GPT-2 small, prompt {P}, {tokens} new tokens, temperature 0.8, top_k = 50, top_p = 0.9; ms per token = whole")
    lines.append("    call / tokens (prefill included), median of 5 calls; greedy graph is the path of the parent commit")
    lines.append("   B   torch eager   torch graph   device graph   greedy graph (floor)")
    for B in (1, 8):
        idx = torch.randint(0, 50257, (B, P), device="cuda")
        kw = dict(temperature=0.8, top_k=50, top_p=0.9)
        te = timed(lambda: m.generate(idx, tokens, generator=gen, **kw), 5, 1) / tokens
        tg = timed(lambda: m.generate(idx, tokens, generator=gen, graph=True, **kw), 5, 1) / tokens
        dg = timed(lambda: m.generate(idx, tokens, sampler="device", seed=1, graph=True, **kw), 5, 1) / tokens
        gg = timed(lambda: m.generate(idx, tokens, temperature=0.0, graph=True), 5, 1) / tokens
        lines.append(f"  {B:2d}   {te:11.3f}   {tg:11.3f}   {dg:12.3f}   {gg:12.3f}")
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
    ap.add_argument("--skinny", action="store_true", help="the gemm_skinny sections (profiles/gemm_skinny.txt)")
    ap.add_argument("--sample", action="store_true", help="the sampling sections (profiles/sample_decode.txt)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode needs a GPU"
    lines = [f"tools/bench_decode.py{' --skinny' if a.skinny else ' --sample' if a.sample else ''} on "
             f"{torch.cuda.get_device_name(0)}", ""]
    if a.sample:
        bench_sample(lines, a.iters, a.tokens, a.skip_model)
    elif a.skinny:
        bench_skinny(lines, min(a.iters, 30))
        if not a.skip_model:
            bench_model_ab(lines, a.tokens)
    else:
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
