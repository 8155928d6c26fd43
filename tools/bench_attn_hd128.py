"""Time the head-dim-128 flash kernels (csrc/kernels/attention_hd128.hip) against what ran at this head dim before them
and against the d = 64 kernels at the same FLOPs.

    python tools/bench_attn_hd128.py [--rounds 7] [--iters 200]       # one JSON line per case

Cases: B = 8, T = 1024, causal, D = 768 (H = 6) and D = 1024 (H = 8), forward and backward.  Three arms alternate in one
process, ROUNDS times:
    hd128   K.flash_attn_fwd / _bwd at head dim 128
    chain   ops.transformer.attention_fwd / attention_bwd, the materialised S / P chain (two batched GEMMs + a row softmax
            forward, four GEMMs + a softmax backward): what use_flash sent this shape to before
    hd64    K.flash_attn_fwd / _bwd at head dim 64 with 2 H heads: the same D, the same FLOPs
Every call is timed by its own pair of device events after three warm-up calls; the chain's backward writes dS over P, so
its P is restored from a copy before each call, outside the timed window.  Reported per arm: the median over the rounds of
the mean call time, min / max over the rounds, and spread = (max - min) / median.  ``hd128_wins`` is true when the chain's
median exceeds the new kernels' by more than the chain's own spread.  ``max_abs_diff`` compares the new kernels' out and
dqkv with the chain's on the same inputs (both round P and dS to bf16; unit-scale values).  ``chain_sp_bytes`` is the
fp32 S + bf16 P the chain keeps per layer until the backward and the flash path never allocates."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pytorch_distributed_nn_amd.ops import kernels as K  # noqa: E402
from pytorch_distributed_nn_amd.ops import transformer as TX  # noqa: E402


def timeit(fn, iters, prep=None):
    """mean device time of one call, us"""
    for _ in range(3):
        if prep:
            prep()
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        if prep:
            prep()
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sum(s.elapsed_time(e) for s, e in ev) / iters * 1e3


def case(B, T, H, rounds, iters):
    D = H * 128
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = (torch.randn(B * T, 3 * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    do = torch.randn(B * T, D, device="cuda", generator=g).to(torch.bfloat16)
    s128, s64 = 1 / math.sqrt(128), 1 / math.sqrt(64)
    out, lse = K.flash_attn_fwd(qkv, B, T, H, s128)
    dqkv = K.flash_attn_bwd(qkv, out, do, lse, B, T, H, s128)
    out64, lse64 = K.flash_attn_fwd(qkv, B, T, 2 * H, s64)
    y, P, S = TX.attention_fwd(qkv, B, T, H)
    P0 = P.clone()
    dchain = TX.attention_bwd(do, qkv, P, B, T, H, dS_buf=S)
    diff = {"out": (out.float() - y.float()).abs().max().item(), "dqkv": (dqkv.float() - dchain.float()).abs().max().item()}
    del y, dchain
    arms = {"hd128_fwd": (lambda: K.flash_attn_fwd(qkv, B, T, H, s128), None),
            "chain_fwd": (lambda: TX.attention_fwd(qkv, B, T, H), None),
            "hd64_fwd": (lambda: K.flash_attn_fwd(qkv, B, T, 2 * H, s64), None),
            "hd128_bwd": (lambda: K.flash_attn_bwd(qkv, out, do, lse, B, T, H, s128), None),
            "chain_bwd": (lambda: TX.attention_bwd(do, qkv, P, B, T, H, dS_buf=S), lambda: P.copy_(P0)),
            "hd64_bwd": (lambda: K.flash_attn_bwd(qkv, out64, do, lse64, B, T, 2 * H, s64), None)}
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, prep) in arms.items():
            times[k].append(timeit(fn, iters, prep))
    r = {"B": B, "T": T, "H": H, "D": D, "causal": True, "rounds": rounds, "iters": iters,
         "chain_sp_bytes": 6 * B * H * T * T, "max_abs_diff": diff}
    fl = 4 * B * H * T * T * 128 * 0.5
    for d, mult in (("fwd", 1.0), ("bwd", 2.5)):
        st = {}
        for arm in ("hd128", "chain", "hd64"):
            v = sorted(times[f"{arm}_{d}"])
            st[arm] = {"us": v[len(v) // 2], "min_max_us": [v[0], v[-1]], "spread": (v[-1] - v[0]) / v[len(v) // 2]}
        st["hd128_tflops"] = mult * fl / st["hd128"]["us"] / 1e6
        st["chain_over_hd128"] = st["chain"]["us"] / st["hd128"]["us"]
        st["hd64_over_hd128"] = st["hd64"]["us"] / st["hd128"]["us"]
        st["hd128_wins"] = st["chain"]["us"] - st["hd128"]["us"] > st["chain"]["min_max_us"][1] - st["chain"]["min_max_us"][0]
        r[d] = st
    rnd = lambda v: round(v, 3) if isinstance(v, float) else ([rnd(x) for x in v] if isinstance(v, list) else  # noqa: E731
                                                              ({k: rnd(x) for k, x in v.items()} if isinstance(v, dict) else v))
    print(json.dumps(rnd(r)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_hd128: no GPU")
    for H in (6, 8):
        case(8, 1024, H, a.rounds, a.iters)


if __name__ == "__main__":
    main()
