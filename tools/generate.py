#!/usr/bin/env python3
"""Generate token ids from a GPT-2 checkpoint written by the trainer (utils.observability.save_checkpoint), or from a
random initialisation, with GPT2.generate (key/value cache; on a GPU the decode-attention kernel).

    python tools/generate.py --network gpt2_small --checkpoint ckpt.pt --prompt-ids 1,2,3 --max-new-tokens 32
    python tools/generate.py --network gpt2_tiny --random-init --prompt-ids prompt.npy --top-k 40 --seed 1
    python tools/generate.py --network gpt2_small --random-init --prompt-ids 1,2,3,1,2,3 --sampler device --speculate 4
    python tools/generate.py --network gpt2_small --random-init --prompt-ids prompt.npy --chunk 256

The prompt is a list of token ids (``1,2,3``) or a .npy file holding an integer vector [P] or matrix [B][P]; there is no
tokenizer here.  Prints one line of comma-separated ids per row: the prompt followed by the new tokens."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_prompt(spec):
    """'1,2,3' or a .npy path -> int64 tensor [B][P]"""
    if spec.endswith(".npy"):
        a = np.load(spec)
        if a.dtype.kind not in "iu" or a.ndim not in (1, 2) or a.size == 0:
            raise ValueError(f"--prompt-ids {spec}: expected a non-empty integer vector or matrix, got {a.dtype} {a.shape}")
        t = torch.from_numpy(a.astype(np.int64))
    else:
        try:
            t = torch.tensor([int(v) for v in spec.split(",") if v.strip() != ""], dtype=torch.int64)
        except ValueError:
            raise ValueError(f"--prompt-ids {spec!r}: expected comma-separated integers or a .npy file") from None
        if t.numel() == 0:
            raise ValueError("--prompt-ids: empty prompt")
    return t.view(1, -1) if t.dim() == 1 else t


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--network", default="gpt2_small", help="a gpt2_* config name (models.gpt2.CONFIGS)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--checkpoint", help="checkpoint file written by the trainer")
    src.add_argument("--random-init", action="store_true", help="no checkpoint: the seeded initialisation")
    ap.add_argument("--prompt-ids", required=True, help="'1,2,3' or a .npy file ([P] or [B][P] integers)")
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--temperature", type=float, default=1.0, help="0 = greedy")
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--top-p", type=float, default=None, help="nucleus sampling: keep the most probable tokens up to this mass")
    ap.add_argument("--sampler", choices=["torch", "device"], default="torch",
                    help="device: the sampling kernel and its counter-based generator, seeded by --seed")
    ap.add_argument("--eos-token", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--graph", action="store_true", help="replay one captured decode step (GPU)")
    ap.add_argument("--speculate", type=int, default=None, metavar="S",
                    help="speculative decoding: verify S tokens per step (2..8, needs --sampler device); the tokens are "
                         "those of the plain loop, and the acceptance statistics go to stderr")
    ap.add_argument("--draft-ngram", type=int, default=3, metavar="n", help="longest n-gram of the prompt-lookup draft")
    ap.add_argument("--chunk", type=int, default=None, metavar="C",
                    help="ingest the prompt in pieces of C tokens through generate(resume=True) on a kept cache before "
                         "sampling (GPU; the CPU path keeps no cache and runs the prompt in one piece)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from pytorch_distributed_nn_amd.models.gpt2 import CONFIGS, build_gpt2
    name = args.network.lower()
    if not name.startswith("gpt2") or name not in CONFIGS:
        raise SystemExit(f"--network {args.network}: expected one of {sorted(CONFIGS)}")
    try:
        idx = parse_prompt(args.prompt_ids)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))
    torch.manual_seed(args.seed)
    model = build_gpt2(name)
    if args.checkpoint:
        from pytorch_distributed_nn_amd.utils.observability import load_checkpoint
        load_checkpoint(args.checkpoint, model, restore_rng=False)
    V = model.config.vocab_size
    if int(idx.min()) < 0 or int(idx.max()) >= V:
        raise SystemExit(f"--prompt-ids: token ids must be in [0, {V}), got {int(idx.min())}..{int(idx.max())}")
    dev = torch.device(args.device)
    model = model.to(dev).eval()
    if args.sampler == "device":
        draw = dict(sampler="device", seed=args.seed)
    else:
        draw = dict(generator=torch.Generator(device=dev).manual_seed(args.seed))
    if args.speculate is not None:
        draw.update(speculate=args.speculate, ngram=args.draft_ngram, return_stats=True)
    if args.chunk is not None and args.chunk < 1:
        raise SystemExit(f"--chunk {args.chunk}: expected a positive number of tokens")
    kw = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, eos_token=args.eos_token,
              graph=args.graph and dev.type == "cuda", **draw)
    idx = idx.to(dev)
    try:
        if args.chunk is not None and dev.type == "cuda":
            from pytorch_distributed_nn_amd.ops.transformer import KVCache
            S = args.speculate or 1
            cache = KVCache(model, idx.shape[0], idx.shape[1] + args.max_new_tokens + (S if S > 1 else 0), dev, S=S)
            pieces = list(idx.split(args.chunk, dim=1))
            for piece in pieces[:-1]:
                model.generate(piece, 0, cache=cache, resume=True)
            out = model.generate(pieces[-1], args.max_new_tokens, cache=cache, resume=True, **kw)
            head = idx[:, :idx.shape[1] - pieces[-1].shape[1]]
            out = (torch.cat([head, out[0]], 1), out[1]) if args.speculate is not None else torch.cat([head, out], 1)
        else:
            if args.chunk is not None:
                print("--chunk: no cache is kept on the CPU, the prompt runs in one piece", file=sys.stderr)
            out = model.generate(idx, args.max_new_tokens, **kw)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.speculate is not None:
        out, stats = out
        emitted = sum(e * n for e, n in enumerate(stats["stats"]))
        print(f"speculate {args.speculate}: {stats['verify_steps']} verify steps, tokens emitted per (row, step) "
              f"{stats['stats']} (mean {emitted / max(sum(stats['stats']), 1):.2f})", file=sys.stderr)
    for row in out.cpu().tolist():
        print(",".join(map(str, row)))
    return out


if __name__ == "__main__":
    main()
