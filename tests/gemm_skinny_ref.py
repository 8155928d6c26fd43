"""The skinny-M weight-streaming GEMM (csrc/kernels/gemm_skinny.hip, ops.kernels.gemm_skinny) against the float64
reference of tests/gemm_ref.py: the case list, an fp32 model of the kernel's own summation order (a stand-in for a
correct kernel and the carrier of planted errors) and the checks shared by test_gemm_skinny_gpu.py and the CPU self-check
test_gemm_skinny_ref_cpu.py.  ``make``, ``reference``, ``check_elem``, ``check_exact``, the bounds, the GELU terms and the
five input families are gemm_ref's, unchanged: y = act(x w^T + bias) (+ res) is its ``nt_ex`` entry point with alpha = 1.

The kernel's partition of K, mirrored here (``partition``; the GPU test compares it with pdnn_gemm_skinny_plan):
    UNIT = 64    reduction elements of one load pair: a lane reads 32 contiguous bytes of its row, the four lanes of a row
                 128; the two MFMAs of a unit take the 8-element pieces {16 g + 8 h + j} (h = 0, 1: MFMA, g = 0..3: lane
                 group, j = 0..7), so an MFMA's 32 reduction indices are not contiguous and a tail of K ends both MFMAs
                 of the last unit early, 8 elements (one 16-byte load) at a time
    STEP         128 (64 with four row tiles, M > 32): what a wave loads ahead; no effect on the order of the sum
    slices       a block has NW waves, NW from (N, K) only: the first of 4, 6, 8, 12 with ceil(N / 16) NW >= 1024 that
                 divides the units of K, else the first with >= 1024 waves and NW <= units, else the largest NW <= units,
                 else 4.  Wave v sums the slice [v SL, min((v + 1) SL, K)), SL = ceil(units / NW) * 64, MFMA after MFMA
                 into one fp32 accumulator; the NW partial sums are added in wave order, then bias, GELU of the
                 bf16-rounded value, res, round to nearest even.  Nothing depends on M.
``model_skinny`` follows exactly that; the sum of one MFMA (<= 32 exact products) is formed in float64 and rounded once,
as gemm_ref._acc does for its slices.

Shapes: the smallest at which the kernel can go wrong.  M: one row, the edges of the 16-row tiles and of the three
instantiations (MT = 1 | 2 | 4 at M <= 16 | 32 | 64).  N: one ragged group (8), one full, ragged second (24, 40), nine
groups (136).  K: 8 .. 72 in 8-element steps around the MFMA piece and the unit, 120 / 128 / 136 the step, 248 / 256 / 264
(units 4 -> 5: SL 64 -> 128, a one-piece slice and an empty wave), 376 / 384 / 392 (NW 4 | 6), 520 (NW 8), 760 / 768 / 776
(NW 12, SL 64 -> 128); rotated, not crossed.  BIG: the grid-filling rule of the plan (NW = 12, 6, 12 with SL = 256, 4 with
a ragged last group) at the real GPT-2 shapes.  Every (shape, variant) runs with contiguous and with padded ldx / ldc.

The constant of the bound.  test_gemm_skinny_ref_cpu.py measures the model's worst error / (u S) with the bf16 rounding
off over every case: 2.68 at worst, below gemm_ref.MEASURED["acc"] = 7.6 (a slice of these cases has at most 8 MFMA
roundings and a block adds at most 12 slices, against 48 roundings of the whole sum there), so gemm_ref.acc_const is used unchanged (the CPU test asserts
the inequality for every case), capped by K + 3 as there.

Recorded worst error / bound (both test files print them):
  fp32 model (test_gemm_skinny_ref_cpu.py): y_bf16 0.995, gelu_y_noaux 0.931
  kernel on an MI355X (test_gemm_skinny_gpu.py): y_bf16 0.995, gelu_y_noaux 0.931; the integer family exact.  Both reach
    ~1 only through the bf16 rounding of the result itself, as in gemm_ref.
"""
import torch

import gemm_ref as A

BF, F32, F64 = A.BF, A.F32, A.F64

# ------------------------------------------------------------------------------------------------ the kernel's partition
UNIT = 64                     # SK_UNIT
PIECE = 8                     # one 16-byte load
MIN_WAVES = 1024              # SK_MIN_WAVES
WAVES = (4, 6, 8, 12)
MAX_M = 64


def step_of(M):
    return 64 if M > 32 else 128


def partition(N, K):
    """-> (waves per block, slice length) of pdnn_gemm_skinny for (N, K)"""
    groups, units = -(-N // 16), -(-K // UNIT)
    nw = next((c for c in WAVES if groups * c >= MIN_WAVES and units % c == 0), None)
    if nw is None:
        nw = next((c for c in WAVES if groups * c >= MIN_WAVES and c <= units), None)
    if nw is None:
        nw = next((c for c in reversed(WAVES) if c <= units), 4)
    return nw, -(-units // nw) * UNIT


def slices(N, K):
    nw, sl = partition(N, K)
    return [(min(v * sl, K), min(v * sl + sl, K)) for v in range(nw)]


# ------------------------------------------------------------------------------------------------ cases
MS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64]
NS = [8, 16, 24, 40, 136]
KS = [8, 32, 72, 136, 520,                                  # the issue's list
      16, 24, 40, 56, 64,                                   # MFMA piece and unit
      120, 128, 192,                                        # step
      248, 256, 264, 376, 384, 392, 760, 768, 776]          # slices: SL and NW change
SHAPES = [(M, N, KS[(i * len(NS) + j) % len(KS)]) for i, M in enumerate(MS) for j, N in enumerate(NS)]
BIG = [(3, 2304, 768), (17, 3072, 768), (33, 768, 3072), (2, 4104, 200)]
VARIANTS = [("plain", dict()), ("bias", dict(bias=True)), ("bias_gelu", dict(bias=True, act=2)),
            ("bias_res", dict(bias=True, res=True)), ("bias_gelu_res", dict(bias=True, act=2, res=True))]


def cases(shapes=None):
    """[(id, make-arguments, options)]: families rotate against (shape, variant); both paddings"""
    out = []
    for si, (M, N, K) in enumerate(SHAPES + BIG):
        if shapes is not None and (M, N, K) not in shapes:
            continue
        for vi, (name, opt) in enumerate(VARIANTS):
            fam = A.FAMILIES[(si + vi) % 5]
            if fam == "integer" and opt.get("act"):          # the integer family skips GELU (gemm_ref)
                fam = "gauss"
            for pad in (0, 8):
                out.append((f"{name}-{fam}-{M}x{N}x{K}-pad{pad}", ("skinny", fam, M, N, K, si + vi), dict(opt, pad=pad)))
    return out


def build(args, opt):
    return A.make(*args, **opt)


reference = A.reference


# ------------------------------------------------------------------------------------------------ fp32 model
MUTATIONS = ["k_tail_dropped", "wave_slice_skipped", "wave_slice_twice", "perm_mismatch", "row_tile_swapped",
             "rows_past_M_stored", "ragged_n_bias_shift", "res_before_act", "bias_skipped", "bf16_trunc"]
_G = torch.arange(4)[:, None]
_J = torch.arange(PIECE)[None, :]


def _mfma_idx(u, h):
    """the reduction indices of MFMA h of the unit starting at u (before the slice end cuts them)"""
    return (u + 16 * _G + PIECE * h + _J).reshape(-1)


def _slice_sum(a, b, k0, k1, mut):
    """fp32 accumulator of one wave: its MFMAs in unit order, each sum in float64 rounded once"""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=F32, device=a.device)
    if mut == "k_tail_dropped":
        k1 = k0 + (k1 - k0) // UNIT * UNIT
    for u in range(k0, k1, UNIT):
        for h in (0, 1):
            iw = _mfma_idx(u, h).to(a.device)
            ix = iw
            if mut == "perm_mismatch" and u + UNIT <= k1:       # x fragment in the natural order of the MFMA
                ix = (u + 32 * h + PIECE * _G + _J).reshape(-1).to(a.device)
            keep = iw < k1
            if keep.any():
                acc = acc + (a[:, ix[keep]].double() @ b[iw[keep], :].double()).float()
    return acc


def model_skinny(c, mut=None, rnd=True):
    """ops.kernels.gemm_skinny in fp32 -> {"y", "tail_rows"}: tail_rows = rows >= M the call stored (0 when correct)"""
    a, b = c.a.float(), c.b.float()
    M, N, K = c.M, c.N, c.K
    dev = a.device
    sl = slices(N, K)
    live = [v for v, (k0, k1) in enumerate(sl) if k1 > k0]
    parts = []
    for v, (k0, k1) in enumerate(sl):
        if mut == "wave_slice_skipped" and len(live) > 1 and v == live[1]:
            parts.append(torch.zeros(M, N, dtype=F32, device=dev))
            continue
        p = _slice_sum(a, b, k0, k1, mut)
        parts.append(p)
        if mut == "wave_slice_twice" and len(live) > 1 and v == live[1]:
            parts.append(p)
    v = parts[0]
    for p in parts[1:]:
        v = v + p
    if c.bias is not None and mut != "bias_skipped":
        bias = c.bias
        if mut == "ragged_n_bias_shift" and N % 16:
            n = torch.arange(N, device=dev)
            bias = torch.where(n >= N // 16 * 16, c.bias[(n + 4).clamp_max(N - 1)], c.bias)
        v = v + bias
    early = mut == "res_before_act" and c.res is not None and c.act == 2
    if early:
        v = v + c.res.float()
    if c.act == 2:
        v = A.model_gelu((v.to(BF) if rnd else v).float())
    if c.res is not None and not early:
        v = v + c.res.float()
    if mut == "row_tile_swapped" and M > 16:
        m = torch.arange(M, device=dev)
        src = torch.where((m < 32) & ((m ^ 16) < M), m ^ 16, m)
        v = v[src]
    if rnd:
        v = A.trunc_bf16(v) if mut == "bf16_trunc" else v.to(BF)
    tail = (-(-M // 16) * 16 - M) if mut == "rows_past_M_stored" else 0
    return {"y": v, "tail_rows": tail}


def check(c, outs, ref=None):
    """outputs {"y", "tail_rows"} of the kernel or the model against the reference -> {name: worst error / bound}"""
    assert outs.get("tail_rows", 0) == 0, f"{outs['tail_rows']} rows >= M were stored"
    return A.check(c, {"y": outs["y"]}, ref if ref is not None else reference(c))
