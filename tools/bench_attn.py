"""Time the fused attention kernels (attention.hip) alone at GPT-2 shapes vs torch SDPA (reference point).

    python tools/bench_attn.py            # one JSON line per config
    python tools/bench_attn.py --doc-len 256 [--rounds 7]
        packed documents of N tokens at B8 / T1024 / H12: the DOC kernels and the plain causal ones alternate in one
        process, ROUNDS times; medians, the plain kernel's own spread across the rounds, and the ratio beside the work
        ratio sum(len^2) / T^2
    python tools/bench_attn.py --dropout 0.1 [--seq-len 4096] [--doc-len 256] [--bwd-wide 1] [--rounds 7]
        dropout P on the probabilities (the DROP kernels) against the kernels without it, at B8 / T / H12, the pairs
        alternating in one process; with --doc-len both sides run under the packed-document mask
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch_distributed_nn_amd.ops import kernels as K  # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3       # us


def doc_main(doc_len, rounds):
    B, T, H = 8, 1024, 12
    sc = 1 / math.sqrt(64)
    qkv = (torch.randn(B * T, 3 * H * 64, device="cuda") * 0.5).to(torch.bfloat16)
    t = torch.arange(T, device="cuda", dtype=torch.int32)
    ds = (t // doc_len * doc_len).expand(B, T).contiguous()
    de = (ds + doc_len).clamp_max(T).contiguous()
    out, lse = K.flash_attn_fwd(qkv, B, T, H, sc, True)
    outd, lsed = K.flash_attn_fwd(qkv, B, T, H, sc, doc=(ds, de))
    do = torch.randn_like(out)
    fns = {"plain_fwd": lambda: K.flash_attn_fwd(qkv, B, T, H, sc, True),
           "doc_fwd": lambda: K.flash_attn_fwd(qkv, B, T, H, sc, doc=(ds, de)),
           "plain_bwd": lambda: K.flash_attn_bwd(qkv, out, do, lse, B, T, H, sc, True),
           "doc_bwd": lambda: K.flash_attn_bwd(qkv, outd, do, lsed, B, T, H, sc, doc=(ds, de))}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timeit(fn, iters=50))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lens = [min(doc_len, T - s) for s in range(0, T, doc_len)]
    r = {"B": B, "T": T, "H": H, "doc_len": doc_len, "rounds": rounds, "work_ratio": sum(n * n for n in lens) / (T * T)}
    for d in ("fwd", "bwd"):
        p, q = times["plain_" + d], times["doc_" + d]
        r[d] = {"plain_us": med["plain_" + d], "doc_us": med["doc_" + d], "ratio": med["doc_" + d] / med["plain_" + d],
                "plain_min_max_us": [min(p), max(p)], "doc_min_max_us": [min(q), max(q)],
                "plain_spread": (max(p) - min(p)) / med["plain_" + d]}
    rnd = lambda v: round(v, 3) if isinstance(v, float) else ([rnd(x) for x in v] if isinstance(v, list) else  # noqa: E731
                                                              ({k: rnd(x) for k, x in v.items()} if isinstance(v, dict) else v))
    print(json.dumps(rnd(r)), flush=True)


def drop_main(p, T, doc_len, rounds, bwd_wide):
    B, H = 8, 12
    sc = 1 / math.sqrt(64)
    if bwd_wide is not None:
        K.tune_set("attn_bwd_wide", bwd_wide)
    qkv = (torch.randn(B * T, 3 * H * 64, device="cuda") * 0.5).to(torch.bfloat16)
    doc = None
    if doc_len:
        t = torch.arange(T, device="cuda", dtype=torch.int32)
        ds = (t // doc_len * doc_len).expand(B, T).contiguous()
        doc = (ds, (ds + doc_len).clamp_max(T).contiguous())
    st = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
    out, lse = K.flash_attn_fwd(qkv, B, T, H, sc, doc=doc, drop=(0.0, st, 0))          # p = 0: the plain / DOC kernels
    outd, lsed = K.flash_attn_fwd(qkv, B, T, H, sc, doc=doc, drop=(p, st, 0))
    do = torch.randn_like(out)
    fns = {"base_fwd": lambda: K.flash_attn_fwd(qkv, B, T, H, sc, doc=doc, drop=(0.0, st, 0)),
           "drop_fwd": lambda: K.flash_attn_fwd(qkv, B, T, H, sc, doc=doc, drop=(p, st, 0)),
           "base_bwd": lambda: K.flash_attn_bwd(qkv, out, do, lse, B, T, H, sc, doc=doc, drop=(0.0, st, 0)),
           "drop_bwd": lambda: K.flash_attn_bwd(qkv, outd, do, lsed, B, T, H, sc, doc=doc, drop=(p, st, 0))}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timeit(fn, iters=50 if T <= 1024 else 10))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    r = {"B": B, "T": T, "H": H, "p": p, "p_eff": K.dropout_p_eff(p), "doc_len": doc_len, "rounds": rounds,
         "attn_bwd_wide": K.tune_get("attn_bwd_wide")}
    for d in ("fwd", "bwd"):
        a, b = times["base_" + d], times["drop_" + d]
        r[d] = {"base_us": med["base_" + d], "drop_us": med["drop_" + d], "ratio": med["drop_" + d] / med["base_" + d],
                "base_min_max_us": [min(a), max(a)], "drop_min_max_us": [min(b), max(b)],
                "base_spread": (max(a) - min(a)) / med["base_" + d]}
    rnd = lambda v: round(v, 3) if isinstance(v, float) else ([rnd(x) for x in v] if isinstance(v, list) else  # noqa: E731
                                                              ({k: rnd(x) for k, x in v.items()} if isinstance(v, dict) else v))
    print(json.dumps(rnd(r)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dropout", type=float, default=0.0, metavar="P", help="the DROP kernels at P vs the ones without")
    ap.add_argument("--seq-len", type=int, default=1024, help="--dropout: T (a multiple of 128)")
    ap.add_argument("--bwd-wide", type=int, default=None, help="--dropout: attn_bwd_wide of both sides (default: tuning)")
    ap.add_argument("--doc-len", type=int, default=0, help="packed documents of N tokens vs the plain causal kernels")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.dropout:
        if not 0.0 < a.dropout < 1.0 or a.seq_len % 128 or a.doc_len < 0:
            raise SystemExit("--dropout must be in (0, 1), --seq-len a multiple of 128")
        return drop_main(a.dropout, a.seq_len, a.doc_len, a.rounds, a.bwd_wide)
    if a.doc_len:
        if a.doc_len < 1:
            raise SystemExit("--doc-len must be >= 1")
        return doc_main(a.doc_len, a.rounds)
    for B, T, H, causal in [(8, 1024, 12, True), (8, 1024, 12, False), (2, 4096, 12, True), (32, 1024, 12, True)]:
        D = H * 64
        qkv = (torch.randn(B * T, 3 * D, device="cuda") * 0.5).to(torch.bfloat16)
        sc = 1 / math.sqrt(64)
        out, lse = K.flash_attn_fwd(qkv, B, T, H, sc, causal)
        do = torch.randn_like(out)
        fl = 4 * B * H * T * T * 64 * (0.5 if causal else 1.0)
        r = {"B": B, "T": T, "H": H, "causal": causal}
        r["fwd_us"] = timeit(lambda: K.flash_attn_fwd(qkv, B, T, H, sc, causal))
        r["bwd_us"] = timeit(lambda: K.flash_attn_bwd(qkv, out, do, lse, B, T, H, sc, causal))
        r["fwd_tf"] = fl / r["fwd_us"] / 1e6
        r["bwd_tf"] = 2.5 * fl / r["bwd_us"] / 1e6
        q, k, v = (qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4))
        try:
            r["sdpa_fwd_us"] = timeit(lambda: F.scaled_dot_product_attention(q, k, v, is_causal=causal))
        except Exception as ex:      # noqa: BLE001
            r["sdpa_err"] = repr(ex)[:100]
        print(json.dumps({k2: (round(v2, 2) if isinstance(v2, float) else v2) for k2, v2 in r.items()}), flush=True)


if __name__ == "__main__":
    main()
