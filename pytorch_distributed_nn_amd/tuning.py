"""Python-side entries of the dispatch table (the kernel-side table is csrc/kernels/tuning.h).

One environment variable overrides either side for A/B runs: ``PDNN_TUNE="key=value,key=value"`` (keys of
both tables; the kernel library reports unknown ones when it loads).  Each default is the measured optimum:

=================  =======  ===========================================================================
key                default  meaning (measurement)
=================  =======  ===========================================================================
side_wgrad         1        conv weight gradients on a second HIP stream beside the data-gradient chain
                            (ResNet-50 +8.3%, profiles/resnet50_bs256_side_stream_r2.txt); 0 = one stream
wide1x1_dgrad      1        1x1 / stride-1 data gradients with K >= 512 and >= 1024 outputs (ResNet-50 stage-4 conv1) on
                            the long-reduction streaming kernel (conv1x1_wide.hip): 81 vs 102 us per layer (r4_02)
a2_fold            1        Bottleneck conv3 reads relu(bn2(t2)) through the A-stationary kernel's operand prologue
                            instead of a materialised a2: 0 never, 1 where its weight gradient already runs on the
                            implicit-GEMM engine (more than 200,704 pixels: ResNet-50 stage 1 at bs 256), 2 wherever
                            the kernel takes the shape (the weight gradient then leaves the ping-pong engine)
wt_prefetch        0        GPT-2 data-gradient GEMMs' transposed weight copies: 0 one transpose launch per weight at
                            its first backward use, 1 all of them in one launch at forward start (compute stream),
                            2 that launch on the side stream beside the forward (544.7k / 542.3k / 537.0k tok/s,
                            gpurun_out/r5_10: the eager backward has launch gaps the small transposes fill)
wt_layer_batch     1        those transposes (wt_prefetch 0) batched per transformer block: the four weights of a block
                            in one launch at the start of its backward (592.8k vs 590.1k tok/s, r5_28)
colsum_atomic      1        accumulating bias-gradient column sums in one launch with fp32 atomics (0: two-level
                            deterministic partial rows + level-2 launch; GPT-2 542.3k vs 538.0k tok/s, r5_10)
bias_in_wgrad      1        GPT-2 linear bias gradients as fused row sums inside the weight-gradient GEMM (0: a
                            column-sum pass over the output gradient)
wgrad1x1_pp_pix    200704   1x1 / stride-1 weight gradients without an operand prologue on the ping-pong engine up to
                            this many pixels (ResNet-50 stages 2-4 at bs 256; stage 1 stays on the implicit-GEMM
                            engine's split-K atomics: tools/bench_wgrad1x1.py, gpurun_out/r3_38-40)
gpt2_side_wgrad    1        GPT-2 linear weight gradients on the weight-gradient side stream beside the data-gradient
                            chain, the compute stream at high priority (0: one stream): DDP path 636.3k / 636.9k ->
                            664.5k / 665.9k tok/s, plain eager 680k vs 646k graphed (gpurun_out/r6_35); the tied LM
                            head's weight gradient there too measured no better (r6_34) and stays on the compute stream
wgrad_plan_cus     128      CUs the tile-width / K-split plan of a GPT-2 weight gradient on the side stream assumes
                            (kernels.pp_wgrad plan_cus; 0: the device's): fewer splits (fc / fc2 7 -> 3, qkv 8 -> 4)
                            mean less fp32 slab traffic beside the data-gradient chain: 671k -> 680k tok/s same box
                            (gpurun_out/r6_40 / r6_41).  Compute-stream weight gradients (the tied LM head) plan for
                            the whole chip
xent_fused         1        GPT-2 training forward writes the unscaled cross-entropy gradient over the logits in the same
                            pass (ops/transformer.py LMHeadLossFn; 0: separate forward and backward passes)
decode_skinny      1        GPT-2 decode linears (M = batch rows, up to ops.kernels.SKINNY_MAX_M) on the weight-streaming
                            skinny-M kernel (csrc/kernels/gemm_skinny.hip; profiles/gemm_skinny.txt); 0 = the training
                            GEMM engines, bit for bit the path before that kernel
ds_sub             1        stride-2 1x1 shortcut convs read a contiguous copy of their input's even pixels (one
                            subsample pass): the forward then runs as a stride-1 1x1 conv, the weight gradient as a
                            plain GEMM on the ping-pong engine (0: the implicit-GEMM engine's strided gathers)
s2_halo            3        3x3 / stride-2 convs on the half-resolution halo kernels (csrc/kernels/conv_s2.hip), a bit
                            mask: 1 data gradient (ResNet-50 bs 256: 210 / 135 / 126 vs 320 / 228 / 205 us per stage on
                            the implicit-GEMM engine), 2 forward where its grid fills the chip (stage 2: 111 vs 139 us;
                            32 forces it everywhere), 16 the data gradient's BN2-backward operand prologue (+45-55 us
                            per call: slower than the separate apply pass), 8 weight gradient on the direct kernel over
                            the input's parity planes (conv3x3_wgrad.hip: 372-389 vs 158-159 us -- four halo stagings
                            per tile for 1-4 taps each), 4 forward reads t1 through the BN1 + ReLU prologue (a1 not
                            materialised; the weight gradient then takes the prologue: 292-296 vs 158-159 us on the
                            implicit-GEMM engine), 64 that prologue writes a1 as a by-product where the forward runs
                            on the halo kernel (no bn_apply pass; measured neutral: 11,822 / 11,826 vs 11,810 / 11,842
                            img/s, r6_06), 128 the data gradient on two parity classes per block (neutral to worse:
                            223 / 161 / 143 vs 225 / 141 / 125 us per stage).  Step A/B (gpurun_out/r6_02): 3 -> 11,650 img/s, 0 11,602, 11 11,452,
                            15 11,416.  0 = implicit GEMM everywhere
=================  =======  ===========================================================================

Every other former switch is fixed at its measured optimum where it is used, with the measurement cited there
(round 4 cut the table from 37 entries: VERDICT r3 weak #5).
"""
from __future__ import annotations

import os

DEFAULTS = {"side_wgrad": 1, "wide1x1_dgrad": 1, "a2_fold": 1, "wt_prefetch": 0, "wt_layer_batch": 1, "colsum_atomic": 1, "bias_in_wgrad": 1, "s2_halo": 3, "ds_sub": 1, "wgrad1x1_pp_pix": 200704, "gpt2_side_wgrad": 1, "xent_fused": 1, "wgrad_plan_cus": 128, "decode_skinny": 1}

_VALUES = dict(DEFAULTS)


def _parse(s: str) -> dict:
    out = {}
    for item in filter(None, (p.strip() for p in s.split(","))):
        if "=" not in item:
            raise ValueError(f"PDNN_TUNE: {item!r} is not key=value")
        k, v = item.split("=", 1)
        out[k.strip()] = int(v)
    return out


for _k, _v in _parse(os.environ.get("PDNN_TUNE", "")).items():
    if _k in _VALUES:
        _VALUES[_k] = _v


def get(key: str) -> int:
    return _VALUES[key]


def set(key: str, value: int) -> int:        # noqa: A001 - mirrors pdnn_tune_set
    """Set a Python-side entry; returns the previous value."""
    if key not in _VALUES:
        raise KeyError(f"unknown tuning key {key!r} (kernel-side keys: ops.kernels.tune_set)")
    old = _VALUES[key]
    _VALUES[key] = int(value)
    return old
