#!/usr/bin/env python3
"""Speculative decoding timings on one GPU (the record in profiles/speculate_decode.txt): GPT-2 small, random
initialisation, prompt 128, graph=True, sampler="device", B in {1, 8}, S in {2, 4, 8} with B * S <= 64.

  1. ms per verify unit at each S against ms per plain device-sampler step (``speculate=None``: the code path of the
     commit before speculation, unchanged by it) in the same process, the calls of one repetition interleaved;
  2. new tokens / s with table drafts whose tokens are right with probability 0, 0.5 and 1 (independently, seeded), and
     with the n-gram draft on a prompt that repeats (greedy, where a random model soon loops);
  3. the mean number of tokens a verify unit must emit for S to break even with the plain step, and the per-token
     draft correctness p that gives it when drafts are right independently: E[tokens] = (1 - p^S) / (1 - p).

A figure is the difference of two whole generate() calls, N = 256 and N = 64 new tokens, over the difference of their
step (or token) counts: the prefill, the warm-up unit and the graph capture are in both and cancel.  Wall clock around a
device synchronise, median of --reps repetitions after one untimed pass.  Nothing here is a pass/fail gate.
    python tools/bench_speculate.py [--out profiles/speculate_decode.txt] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P, N_LONG, N_SHORT, SEED = 128, 256, 64, 7
SAMPLED = dict(temperature=0.8, top_k=40)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def break_even_p(S, need):
    """p with (1 - p^S) / (1 - p) = need, by bisection; None when even p = 1 (S tokens a unit) is not enough"""
    if need > S:
        return None
    if need <= 1:
        return 0.0
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = (lo + hi) / 2
        if sum(mid ** i for i in range(S)) < need:
            lo = mid
        else:
            hi = mid
    return hi


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_speculate.py needs a GPU")
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    from pytorch_distributed_nn_amd.ops.transformer import KVCache
    torch.manual_seed(0)
    model = build_gpt2("gpt2_small").cuda().eval()
    V = model.config.vocab_size
    lines = [f"Speculative decoding, GPT-2 small (random init), P = {P}, graph=True, sampler='device' on "
             f"{torch.cuda.get_device_name(0)}",
             f"(tools/bench_speculate.py: (generate N = {N_LONG}) - (generate N = {N_SHORT}), wall clock, median of "
             f"{args.reps} interleaved repetitions after one warm-up pass)", ""]
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        idx = torch.randint(0, V, (B, P), generator=g).cuda()
        rep_idx = torch.randint(0, V, (B, 16), generator=g).repeat(1, P // 16).cuda()
        cache = KVCache(model, B, model.kv_cache_len(P, N_LONG + 8), "cuda", S=8)
        common = dict(sampler="device", seed=SEED, graph=True, cache=cache)
        truth = model.generate(idx, N_LONG, **SAMPLED, **common)[:, P:]
        Ss = [S for S in (2, 4, 8) if B * S <= 64]
        tables = {}
        for pc in (0.0, 0.5, 1.0):
            ok = torch.rand(B, N_LONG, generator=torch.Generator().manual_seed(int(pc * 10))).cuda() < pc
            tables[pc] = torch.where(ok, truth, (truth + 1) % V).contiguous()
        # name -> N -> callable returning (tokens, stats or None)
        runs = {"plain": lambda n: (model.generate(idx, n, **SAMPLED, **common), None),
                "plain greedy, repeating prompt": lambda n: (model.generate(rep_idx, n, temperature=0.0, **common), None)}
        for S in Ss:
            for pc, tab in tables.items():
                runs[f"S={S} table {int(pc * 100)}%"] = (
                    lambda n, S=S, tab=tab: model.generate(idx, n, speculate=S, draft=tab[:, :n].contiguous(),
                                                           return_stats=True, **SAMPLED, **common))
            runs[f"S={S} ngram, repeating prompt"] = (
                lambda n, S=S: model.generate(rep_idx, n, temperature=0.0, speculate=S, draft="ngram", ngram=3,
                                              return_stats=True, **common))
        times = {k: {N_LONG: [], N_SHORT: []} for k in runs}
        units = {}
        ref = {}
        for rep in range(args.reps + 1):                    # pass 0 is the warm-up
            for name, fn in runs.items():
                for n in (N_LONG, N_SHORT):
                    ms, (tok, st) = wall(lambda: fn(n))
                    if rep:
                        times[name][n].append(ms)
                    units[(name, n)] = st["verify_steps"] if st else n - 1
                    base = ref.setdefault(("rep" in name, n), tok)          # same tokens as the plain run: checked
                    if not torch.equal(tok, base):
                        raise SystemExit(f"B={B} {name} N={n}: tokens differ from the plain loop")
        med = {k: {n: statistics.median(v[n]) for n in v} for k, v in times.items()}
        dtok = B * (N_LONG - N_SHORT)
        lines.append(f"B = {B}")
        lines.append(f"  {'run':38s} {'ms/unit':>8s} {'tokens/unit/row':>16s} {'new tokens/s':>13s}   (N={N_LONG}: ms total, units)")
        plain_ms = None
        for name in runs:
            dms = med[name][N_LONG] - med[name][N_SHORT]
            du = units[(name, N_LONG)] - units[(name, N_SHORT)]
            per_unit = dms / du
            if name == "plain":
                plain_ms = per_unit
            lines.append(f"  {name:38s} {per_unit:8.3f} {(N_LONG - N_SHORT) / du:16.2f} {dtok / dms * 1e3:13.0f}   "
                         f"({med[name][N_LONG]:.1f}, {units[(name, N_LONG)]})")
        lines.append("  break-even against the plain step (tokens a verify unit must emit per row; per-token draft "
                     "correctness p if independent):")
        for S in Ss:
            name = f"S={S} table 0%"
            unit_ms = (med[name][N_LONG] - med[name][N_SHORT]) / (units[(name, N_LONG)] - units[(name, N_SHORT)])
            need = unit_ms / plain_ms
            p = break_even_p(S, need)
            lines.append(f"    S={S}: unit {unit_ms:.3f} ms / plain {plain_ms:.3f} ms = {need:.2f} tokens per unit"
                         + (f", p = {p:.2f}" if p is not None else f": more than S = {S}, never breaks even"))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
