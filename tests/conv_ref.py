"""A float64 reference of the direct convolution kernels (csrc/kernels/conv3x3.hip: the LDS-halo 3x3 kernel at
the 64- and 128-wide tile, the weight-resident 64 -> 64 kernel and the A-stationary 1x1 kernel; conv1x1_wide.hip: the
long-reduction 1x1 kernel; conv_direct.h: their shared epilogues and operand prologues), the elementwise bounds they are
held to, fp32 models of them (a stand-in for a correct kernel, and the carrier of planted errors) and the seeded inputs
and case lists shared by the GPU tests (test_conv_gpu.py) and the CPU self-check (test_conv_ref_cpu.py).  Everything
here runs on CPU and GPU tensors alike.  Also covered: the stride-2 halo kernels (conv_s2.hip; kind "s2", forward by
strided slices of the padded input, data gradient by scattering dy W into the parity classes of dx, pro_out (a1)
checked on its own with bn_ref's bound and y then against the conv of the kernel's own a1), the implicit-GEMM fallback
of conv_fwd / conv_dgrad (kind "gen": any R, stride, pad through the same gather / scatter) and the weight gradients
on every route (the section at the end of this module).

A case holds what the kernel receives.  x [P][Ci] bf16 (P = Nimg H W pixels, NHWC) and the weight in the KERNEL's layout
wk [Co][taps][Ci] bf16 (taps = 9, tap = 3 r + s, or 1).  A forward is y = conv(x, wk).  A data gradient (dgrad) is the
same kernel on dy with the tap-flipped transposed weight: the layer's weight is W[k][tap][c] = wk[c][8 - tap][k]
(``layer_weight``), the GPU test hands W to conv3x3_flip / transpose_bf16 and the reference computes dx from W by the
transposed-conv formula dx[y][x] = sum_{r,s} dy[y - (r - 1)][x - (s - 1)] . W[:, r, s, :], so a flip that is omitted
or wrong shows.  Convolutions are nine shifted float64 matmuls over a zero-padded image (no F.conv2d in double); the
same routine on absolute values gives the magnitude S.

Operand stage.  pro = (sc, sh): the operand is a = bf16(relu(fma(x, sc, sh))), bn_apply's formula; the reference operand
is bn_ref.ref_apply in float64, unrounded, and y carries the Lipschitz term sum |w| e_a with e_a = 2^-8 |a| + C_Y u S_y
(bn_ref's bound of that stage), as gemm_ref does for GELU without aux.  pre = (t, mean, invstd, gamma, dgamma, dbeta,
dt_out?): the operand is dt = bn_bwd_apply(gm = x, t) mode 0 with L = P; dt_out is checked on its own with bn_ref's bound
(C_DX) and y against the float64 conv of the kernel's OWN dt_out; without dt_out, against the reference dt with the same
Lipschitz term (e_a = 2^-8 |dt| + C_DX u S_dt).

Epilogues (conv_direct.h c3_epilogue_rows), acc the fp32 sum:
    plain    y = bf16(acc)                      stats   the same + slab of sum r, sum r^2 over r = the stored bf16 y
    res      y = bf16(acc + res)                resmask y = bf16(acc + res * bit), bit c & 7 of byte [p][c >> 3]
    bnb      gm = bf16(acc) * [z > 0], z = fma(t, msc, msh); slab of sum gm and (sum gm t - mean sum gm) invstd
The mask: fmaf rounds the exact t msc + msh once, and rounding neither crosses nor reaches zero, so its sign is the sign of
the exact value, which float64 holds exactly (8 x 24 significant bits in the product).  The mask must therefore match
everywhere except where 0 < |z| <= 2^-40 (|t msc| + |msh|) (float64's own rounding of the sum); test_conv_ref_cpu.py
asserts that no element of any case lies there, so no element is left out.  Every bnb case plants exact zeros (t = 1,
msc = 0.5, msh = -0.5 on channels c % 8 == 3, a quarter of their pixels), where gm must be +0 ('>' against '>=').

Notation.  u = 2^-24, S = sum |a| |w| (+ |res|), terms = taps Ci.
    bf16 outputs:  |got - ref| <= A + c u S + (u + 2^-8) |ref| + TINY      (gemm_ref.bound_of; A the Lipschitz term)
    where the mask is off: got must be +0 exactly
    slab totals (float64 sum over the 64 bins of the fp32 slab) against float64 sums of the kernel's own bf16 output:
        |got - ref| <= K_SLAB u T + u |ref|,  T = sum |r|, sum r^2, sum |gm|, invstd (sum |gm t| + |mean| sum |gm|)
        (the last is what cancels inside the kernel's (sum gm t - mean sum gm) invstd, not the smaller sum |gm xhat|)
c and K_SLAB are not picked: ``model`` accumulates in fp32 in the kernels' order (64-channel chunk outer, tap inner,
32-deep MFMA steps; a step's own 32 products summed in float64 and rounded once, as gemm_ref._acc) with the result's
rounding switched off, ``model_slab`` sums like the epilogue (4 rows per lane, a 16-lane tree, 64-row partials added to
bin (row / 64) % 64 in order), and test_conv_ref_cpu.py measures their worst error / (u S) over every case of this
module and asserts MEASURED to 2% both ways.  The constants are 4x the measurement (the project's margin for the GPU's
summation order: the MFMA's internal order and the order of the atomics), c capped at terms + 3 as gemm_ref.acc_const.
Up to 9 x 256 terms (72 steps) the measured accumulation constant is 9.89 (positive family, the stride-2 forward at
256 channels; the stride-1 cases alone measure 7.26).  That exceeds gemm_ref.MEASURED["acc"] = 7.6, so it is not
reused: c = min(39.6, terms + 3).  The K = 8192 cases of the long-reduction kernel (256 steps) measure 13.42 and get
their own c = 53.7; K_SLAB = 4 x 0.928 = 3.71 (a stride-2 data gradient's partial holds one parity class).

Input families (gemm_ref's).  gauss.  positive: every operand > 0, so a dropped tap or chunk shows at full size.
cancelling: the second half of the channels repeats the first with the weight negated and slightly perturbed.
poisoned: gauss; the GPU test stores x (and pre's t) with NaN rows before the first and after the last pixel, everything
else with the finite 777: the halo kernels read "row -1" and "row H" only through the zero pixel, so the result must be
finite and inside the bound.  integer: operands are integers in [-4, 4] (res in [-8, 8], pro sc in {1, 2, -1} and sh in
[-2, 2], pre gamma in {1, 2, -1} with invstd = 1 and dgamma = dbeta = 0, so operands stay integers <= 10), 9 Ci max|a|
max|w| < 2^24: every order of summation is exact and y / dx / gm must equal the round-to-nearest-even bf16 of the
reference bit for bit; drawn until no two taps of the weight and no two pixels of x are equal, so a swapped tap or a
shifted pixel cannot cancel.  The slab totals of this family are held to the bound only.

Launch geometry mirrored here (asserted against the library's predicates in test_conv_gpu.py): c3_halo_max, c3_smem,
halo_supported, halo_nb (the silent 128 -> 64 fallback), resident_ok, areg_plan (block groups g and weight steps).

Recorded worst error / bound (both test files print them; the bf16 outputs reach ~1 because the rounding of the result
alone reaches 2^-8 |ref| just above a power of two, and model and kernel then share the worst element):
  fp32 models (test_conv_ref_cpu.py): y 0.996, gm 0.995, dt 0.996, a1 0.996, y_pre2 0.589, y_pro 0.680, slab_s 0.044,
    slab_q 0.366 (0.081 / 0.401 with the implicit-GEMM cases), dW 0.25 (fp32 part 2.88 of c = 11.5)
  kernels on an MI355X (test_conv_gpu.py; the halo kernel under nb auto / 1 / 64 / 128, the A-stationary kernel at
    steps == 1 and steps > 1 and with 513 pixel tiles, the long-reduction kernel up to K = 8192, the stride-2 kernels
    per class and per class pair, the implicit-GEMM fallback): the same figures in all eight kinds; dW direct 0.343,
    direct stride 2 0.587, ping-pong 0.064, implicit GEMM 0.857 (split-K atomics, fp32 output: the accumulation shows).  The integer family is exact on every route.
    Why the same: y / gm / dt / a1 are set by the result's own rounding; the slab's worst cases have one add per bin
    (nothing for the atomics to reorder); and in y_pro / y_pre2 the Lipschitz term of the unseen operand rounding
    (2^-8 of the magnitude) swamps the accumulation error (c u S ~ 2^-19 S), so these two kinds say nothing about the
    accumulation order: there the positive and integer families guard the sum (a dropped term is of full size, or the
    result exact), and the pre == 1 / pro_out forms of the same kernels check it from the kernel's own operand.
The kernel's nb = 128 -> 64 fallback (conv3x3.hip, "c3_smem<128>(W) > 80 KB") cannot be reached by a supported shape:
pdnn_conv3x3_supported already asks for that size when Co % 128 == 0.  Only its Co % 128 != 0 half runs, here and anywhere.
"""
import functools
from types import SimpleNamespace

import torch

import bn_ref as B
from gemm_ref import BF, F32, F64, U, TINY, Elem, FAMILIES, bits_equal, check_elem, check_exact, trunc_bf16
import gemm_ref as G

# worst error / (u S) of the fp32 models with the result's rounding off (test_conv_ref_cpu.py asserts them to 2%, both
# ways).  "acc": reductions up to LONG_TERMS terms; "acc_long": the K = 8192 long-reduction cases (256 steps)
MEASURED = {"acc": 9.89, "acc_long": 13.42, "slab": 0.928, "wgrad": 2.88}
LONG_TERMS = 9 * 256
C_ACC = 4.0 * MEASURED["acc"]              # above gemm_ref.MEASURED["acc"] = 7.6: not reused
C_ACC_LONG = 4.0 * MEASURED["acc_long"]
K_SLAB = 4.0 * MEASURED["slab"]
BM = 256
PAD_FILL = G.PAD_FILL

EPIS = ["plain", "stats", "res", "resmask", "bnb"]
MUTATIONS = ["tap_drop_border", "no_flip", "left_wrap", "skip_last8", "bf16_trunc", "stats_lastrow_twice", "bit_order",
             "mask_ge", "wstep_next"]


def acc_const(terms):
    return min(C_ACC if terms <= LONG_TERMS else C_ACC_LONG, terms + 3.0)


# ------------------------------------------------------------------------------------------ launch geometry
def c3_halo_max(W):
    return ((BM - 1 + W - 1) // W + 3) * W


def c3_smem(nb, W):
    return (c3_halo_max(W) + 1) * 128 + 2 * nb * 128


def halo_supported(P, W, Ci, Co, force=True):
    """pdnn_conv3x3_supported (force: tuning conv3x3_force, which also takes W < 12)"""
    if Ci % 64 or Co % 64 or Ci < 64 or Co < 64 or (W < 12 and not force) or P >= 2 ** 30:
        return False
    return c3_smem(128 if Co % 128 == 0 else 64, W) <= 80 * 1024


def halo_nb(Co, W, nb=0):
    """the column tile pdnn_conv3x3 runs for a requested nb (0 / 1: automatic): 128 falls back to 64 silently"""
    if nb in (0, 1):
        nb = 128 if Co % 128 == 0 else 64
    if nb == 128 and (Co % 128 or c3_smem(128, W) > 80 * 1024):
        nb = 64
    return nb


def resident_ok(Ci, Co, W, pre, pro):
    """nb = 1 runs the weight-resident persistent kernel"""
    return (not pre and not pro and Ci == 64 and Co == 64 and c3_halo_max(W) * 8 <= 16 * 256
            and (c3_halo_max(W) + 1) * 128 + 9 * 64 * 128 <= 160 * 1024)


def widest(pred):
    return max(W for W in range(1, 1025) if pred(W))


W_MAX64 = widest(lambda W: c3_smem(64, W) <= 80 * 1024)             # 85 (six halo rows); 73 is the widest with seven
W_MAX128 = widest(lambda W: c3_smem(128, W) <= 80 * 1024)           # 38
W_MAXRES = widest(lambda W: resident_ok(64, 64, W, False, False))   # 85


def areg_plan(P, K, N):
    """areg_run: (nb, block groups g, weight steps per block)"""
    nb = 32 if K == 256 else 64
    chunks, tiles, g = N // nb, -(-P // BM), 1
    while g < chunks and tiles * g < 512 and chunks % (2 * g) == 0:
        g *= 2
    return nb, g, chunks // g


# ------------------------------------------------------------------------------------------------ cases
# variant: (name, dgrad, epi, pre (0 none, 1 with dt_out, 2 without), pro)
V_HALO = [("fwd_plain", 0, "plain", 0, 0), ("fwd_stats", 0, "stats", 0, 0), ("fwd_pro_plain", 0, "plain", 0, 1),
          ("fwd_pro_stats", 0, "stats", 0, 1), ("dg_plain", 1, "plain", 0, 0), ("dg_res", 1, "res", 0, 0),
          ("dg_resmask", 1, "resmask", 0, 0), ("dg_bnb", 1, "bnb", 0, 0), ("dg_pre1_plain", 1, "plain", 1, 0),
          ("dg_pre2_resmask", 1, "resmask", 2, 0), ("dg_pre1_bnb", 1, "bnb", 1, 0), ("dg_pre2_stats", 1, "stats", 2, 0),
          ("dg_pre1_res", 1, "res", 1, 0)]
V_AREG = V_HALO[:12]
# stride 2 (conv_s2.hip): pro == 2 also asks for pro_out (a1); every dgrad variant without pre runs on the per-class
# kernel and on the class-pair kernel (tuning s2_halo bit 128)
V_S2 = [("fwd_plain", 0, "plain", 0, 0), ("fwd_stats", 0, "stats", 0, 0), ("fwd_pro_plain", 0, "plain", 0, 1),
        ("fwd_pro_stats", 0, "stats", 0, 1), ("fwd_pro2_stats", 0, "stats", 0, 2), ("fwd_pro2_plain", 0, "plain", 0, 2),
        ("dg_plain", 1, "plain", 0, 0), ("dg_bnb", 1, "bnb", 0, 0), ("dg_pre1_plain", 1, "plain", 1, 0),
        ("dg_pre2_bnb", 1, "bnb", 2, 0), ("dg_pre1_bnb", 1, "bnb", 1, 0), ("dg_pre2_plain", 1, "plain", 2, 0)]
V_WIDE = [v for v in V_HALO if not v[4]]
VARIANT = {v[0]: v for v in V_HALO + V_S2}

# (Nimg, H, W), Ci, Co: pixel counts 1 / 255 / 256 / 257 / 513; image boundaries inside a tile and tile boundaries
# mid-row; W = 1; H = 1 at the widest seven-row W; the widest W of the 64 tile / resident kernel and of the 128 tile;
# W = 56 (ResNet-50 stage 1) on the 64 tile; Ci != Co; Ci = 256 (four chunks).  Co = 128 at W = 56 is NOT a halo shape:
# pdnn_conv3x3_supported itself asks for c3_smem<128>(W) <= 80 KB when Co % 128 == 0, so the kernel's silent
# 128 -> 64 fallback is reached only by a forced nb = 128 at Co % 128 != 0 (the (64, 192) shapes under nb = 128)
HALO = [((1, 1, 1), 64, 64), ((1, 15, 17), 64, 128), ((1, 16, 16), 128, 64), ((257, 1, 1), 64, 64),
        ((1, 27, 19), 128, 128), ((3, 9, 11), 64, 192), ((7, 3, 3), 128, 64), ((2, 5, 6), 64, 64),
        ((1, 300, 1), 64, 128), ((5, 1, 73), 64, 64), ((1, 4, W_MAX64), 64, 64), ((1, 7, W_MAX128), 128, 128),
        ((1, 5, 56), 64, 64), ((2, 9, 11), 256, 128)]
HALO_NB = [0, 1, 64, 128]


def s2_halo_max(Wo):
    return ((BM - 1 + Wo - 1) // Wo + 2) * Wo


def s2_supported(H, W, Ci, Co):
    """pdnn_conv3x3s2_supported: even H, W, channels in 128s, halo + weights within 80 KB"""
    if H % 2 or W % 2 or H < 2 or W < 2 or Ci % 128 or Co % 128 or Ci < 128 or Co < 128:
        return False
    return (s2_halo_max(W // 2) + 1) * 128 + 2 * 128 * 128 <= 80 * 1024


W_MAXS2 = 2 * widest(lambda Wo: s2_supported(2, 2 * Wo, 128, 128))          # 108: Wo = 54, seven halo rows
# full-resolution (Nimg, H, W), input channels, output channels of the LAYER (a data gradient maps Co -> Ci):
# Ho = Wo = 1; a 9-pixel tile of three images; 255 / 256 / 510 half-resolution pixels; images straddling a tile and
# tile boundaries mid-row (3 x 9 x 11 = 297 half-resolution pixels); the widest W
# the implicit-GEMM fallback (pdnn_conv_fwd / pdnn_conv_dgrad): (Nimg, H, W) of the layer's input, (R, stride, pad), Ci, Co.
# 3x3 stride 1 at C = 72; 3x3 stride 2 with odd H, W; 1x1 stride 2; 1x1 stride 1 at C = 72 / 192 (panel mode off)
GEN = [((2, 5, 6), (3, 1, 1), 72, 72), ((1, 7, 9), (3, 2, 1), 72, 64), ((2, 6, 6), (1, 2, 0), 72, 128),
       ((1, 1, 300), (1, 1, 0), 72, 72), ((1, 1, 300), (1, 1, 0), 192, 192)]
V_GEN = ["fwd_plain", "fwd_stats", "fwd_pro_plain", "fwd_pro_stats", "dg_plain", "dg_res", "dg_resmask", "dg_bnb"]
V_GEN_S2 = ["fwd_plain", "fwd_stats", "fwd_pro_stats", "dg_plain"]
S2 = [((1, 2, 2), 128, 128), ((3, 2, 6), 128, 256), ((1, 34, 30), 256, 128), ((1, 32, 32), 128, 128),
      ((2, 34, 30), 128, 128), ((3, 18, 22), 256, 256), ((1, 4, W_MAXS2), 128, 128)]
AREG_KN = [(64, 192), (64, 320), (128, 192), (128, 320), (256, 192), (64, 64), (128, 128), (256, 64)]
AREG_P = [1, 255, 256, 257, 600]
AREG_BIG = (131200, 64, 128)               # >= 512 pixel tiles: the production branch g = 1
WIDE_KN = [(512, 64), (512, 192), (576, 64), (576, 192)]
WIDE_P = [1, 255, 257]
WIDE_LONG = (257, 8192, 64)                # 96 KB of PRE coefficients in LDS
WIDE_DGRAD = (255, 512, 1024)              # conv_dgrad routes here (K >= 512, N >= 1024)


def _cid(kind, img, Ci, Co, vname, fam):
    return f"{kind}-{vname}-{fam}-{img[0]}x{img[1]}x{img[2]}-{Ci}to{Co}"


@functools.lru_cache(maxsize=None)
def all_cases():
    """{group: [(id, (kind, img, Ci, Co, variant name, family))]}: everything test_conv_gpu.py runs"""
    halo, areg, wide = [], [], []
    for si, (img, Ci, Co) in enumerate(HALO):
        for vi, v in enumerate(V_HALO):
            fam = FAMILIES[(si + vi) % 5]
            halo.append((_cid("c3", img, Ci, Co, v[0], fam), ("c3", img, Ci, Co, v[0], fam)))
    si = 0
    for K, N in AREG_KN:
        for P in AREG_P:
            for j in range(4):
                vi = (si * 4 + j) % 12
                fam = FAMILIES[(si + vi + j) % 5]
                img = (1, 1, P)
                areg.append((_cid("p1", img, K, N, V_AREG[vi][0], fam), ("p1", img, K, N, V_AREG[vi][0], fam)))
            si += 1
    P, K, N = AREG_BIG
    for vn, fam in (("fwd_stats", "positive"), ("dg_bnb", "gauss"), ("dg_pre1_plain", "integer"), ("fwd_pro_plain", "gauss")):
        areg.append((_cid("p1", (1, 1, P), K, N, vn, fam), ("p1", (1, 1, P), K, N, vn, fam)))
    si = 0
    for K, N in WIDE_KN:
        for P in WIDE_P:
            for j in range(3):
                vi = (si * 3 + j) % len(V_WIDE)
                fam = FAMILIES[(si + vi + j) % 5]
                wide.append((_cid("p1", (1, 1, P), K, N, V_WIDE[vi][0], fam), ("p1", (1, 1, P), K, N, V_WIDE[vi][0], fam)))
            si += 1
    P, K, N = WIDE_LONG
    for vn, fam in (("dg_pre1_plain", "positive"), ("dg_pre2_resmask", "integer"), ("dg_pre1_bnb", "gauss")):
        wide.append((_cid("p1", (1, 1, P), K, N, vn, fam), ("p1", (1, 1, P), K, N, vn, fam)))
    P, K, N = WIDE_DGRAD
    for vn, fam in (("dg_plain", "integer"), ("dg_resmask", "positive"), ("dg_pre1_plain", "cancelling"), ("dg_bnb", "poisoned")):
        wide.append((_cid("p1", (1, 1, P), K, N, vn, fam), ("p1", (1, 1, P), K, N, vn, fam)))
    s2 = []
    for si, (img, Ci, Co) in enumerate(S2):
        for vi, v in enumerate(V_S2):
            fam = FAMILIES[(si + vi) % 5]
            ci, co = (Co, Ci) if v[1] else (Ci, Co)            # a data gradient's operand has the layer's Co channels
            s2.append((_cid("s2", img, ci, co, v[0], fam), ("s2", img, ci, co, v[0], fam)))
    gen = []
    for si, (img, geo, Ci, Co) in enumerate(GEN):
        for vi, vn in enumerate(V_GEN if geo[1] == 1 else V_GEN_S2):
            v = VARIANT[vn]
            fam = FAMILIES[(si + vi) % 5]
            ci, co = (Co, Ci) if v[1] else (Ci, Co)
            cid = _cid("gen", img, ci, co, vn, fam) + f"-r{geo[0]}s{geo[1]}"
            gen.append((cid, ("gen", img, ci, co, vn, fam, geo)))
    return {"halo": halo, "areg": areg, "wide": wide, "s2": s2, "gen": gen}


def by_id():
    return {cid: args for group in all_cases().values() for cid, args in group}


# ------------------------------------------------------------------------------------------------ inputs
def _distinct_rows(m):
    return torch.unique(m, dim=0).shape[0] == m.shape[0]


def gen_xw(family, P, T, Ci, Co, g):
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)        # noqa: E731
    if family == "integer":
        assert 9 * Ci * 10 * 4 < 2 ** 24
        for _ in range(32):
            x = torch.randint(-4, 5, (P, Ci), generator=g).double()
            w = torch.randint(-4, 5, (Co, T, Ci), generator=g).double()
            if _distinct_rows(x) and _distinct_rows(w.permute(1, 0, 2).reshape(T, -1)):
                return x, w
        raise AssertionError("integer family: no distinct draw")
    if family == "positive":
        x = torch.rand(P, Ci, generator=g, dtype=F64) * 1.5 + 0.25
        w = torch.rand(Co, T, Ci, generator=g, dtype=F64) * 1.5 + 0.25
    elif family == "cancelling":
        h = Ci // 2
        x1, w1 = rn(P, h).to(BF).double(), rn(Co, T, h).to(BF).double()
        x = torch.cat([x1, x1], -1)
        w = torch.cat([w1, -w1 + 2.0 ** -5 * rn(Co, T, h)], -1)
    else:
        x, w = rn(P, Ci), rn(Co, T, Ci) * 0.25
    return x.to(BF).double(), w.to(BF).double()


def make(kind, img, Ci, Co, vname, family, geo=None):
    """A seeded case on the CPU.  geo = (R, st, pad) of kind "gen" (the implicit-GEMM fallback)"""
    _, dgrad, epi, pre, pro = VARIANT[vname]
    Nimg, H, W = img
    R, st, pad = geo if geo else ((1, 1, 0) if kind == "p1" else (3, 2, 1) if kind == "s2" else (3, 1, 1))
    P, T = Nimg * H * W, R * R
    Po = P
    if kind in ("s2", "gen"):              # forward: full -> output resolution; data gradient: the other way
        Ho, Wo = out_hw(img, R, st, pad)
        P, Po = (Nimg * Ho * Wo, P) if dgrad else (P, Nimg * Ho * Wo)
    g = torch.Generator().manual_seed(G._seed(kind, vname, family, Nimg, H, W, Ci, Co, *(geo or ())))
    integer = family == "integer"
    x, w = gen_xw(family, P, T, Ci, Co, g)
    c = SimpleNamespace(kind=kind, img=img, R=R, st=st, pad=pad, P=P, Po=Po, T=T, Ci=Ci, Co=Co, vname=vname, family=family, dgrad=bool(dgrad), epi=epi,
                        pre=pre, pro=pro, poison=family == "poisoned", x=x.to(BF), wk=w.to(BF), res=None, keep=None,
                        bn=None, pre_ops=None, pro_ops=None)
    rnd, rand = (lambda *s: torch.randn(*s, generator=g)), (lambda *s: torch.rand(*s, generator=g))
    pick = lambda vals, n: torch.tensor(vals, dtype=F32)[torch.randint(0, len(vals), (n,), generator=g)]    # noqa: E731
    if epi in ("res", "resmask"):
        c.res = (torch.randint(-8, 9, (Po, Co), generator=g).float() if integer else rnd(Po, Co) * 2.0).to(BF)
        if epi == "resmask":
            c.keep = rand(Po, Co) > 0.5
    if epi == "bnb":
        t = rnd(Po, Co)
        msc = (rand(Co) + 0.5) * pick([1.0, -1.0], Co)
        msh = rnd(Co) * 0.3
        zc = torch.arange(Co) % 8 == 3                     # planted exact zeros of t msc + msh
        msc[zc], msh[zc] = 0.5, -0.5
        t = torch.where(zc[None, :] & (rand(Po, Co) < 0.25), torch.ones_like(t), t).to(BF)
        c.bn = (t, rnd(Co) * 0.1, rand(Co) + 0.5, msc, msh)
    if pre:
        if integer:
            c.pre_ops = (rnd(P, Ci).to(BF), rnd(Ci) * 0.1, torch.ones(Ci), pick([1.0, 2.0, -1.0], Ci), torch.zeros(Ci),
                         torch.zeros(Ci))
        else:
            c.pre_ops = (rnd(P, Ci).to(BF), rnd(Ci) * 0.1, rand(Ci) + 0.5, rand(Ci) + 0.5, rnd(Ci) * 0.5 * P, rnd(Ci) * 0.5 * P)
    if pro:
        if integer:
            c.pro_ops = (pick([1.0, 2.0, -1.0], Ci), torch.randint(-2, 3, (Ci,), generator=g).float())
        else:
            c.pro_ops = ((rand(Ci) + 0.5) * pick([1.0, 1.0, -1.0], Ci), rnd(Ci) * 0.5)
    return c


def case_to(c, device):
    mv = lambda v: (v.to(device) if torch.is_tensor(v) else tuple(mv(e) for e in v) if isinstance(v, tuple) else v)   # noqa: E731
    return SimpleNamespace(**{k: (mv(v) if k != "img" else v) for k, v in vars(c).items()})


def layer_weight(c):
    """the layer's weight of a data gradient, W[k = Ci][tap][c = Co] = wk[c][T - 1 - tap][k] (bf16)"""
    return c.wk.flip(1).permute(2, 1, 0).contiguous()


# ------------------------------------------------------------------------------------------------ reference
def tap_operand(a, img, tap, T, transposed=False):
    """[P][Ci] -> the operand of one tap: pixel (y + r - 1, x + s - 1) (transposed: (y - r + 1, x - s + 1)), zero outside"""
    if T == 1:
        return a
    Nimg, H, W = img
    r, s = tap // 3, tap % 3
    if transposed:
        r, s = 2 - r, 2 - s
    xp = torch.zeros(Nimg, H + 2, W + 2, a.shape[1], dtype=a.dtype, device=a.device)
    xp[:, 1:H + 1, 1:W + 1] = a.reshape(Nimg, H, W, -1)
    return xp[:, r:r + H, s:s + W].reshape(Nimg * H * W, -1)


def out_hw(img, R=3, st=2, pad=1):
    return (img[1] + 2 * pad - R) // st + 1, (img[2] + 2 * pad - R) // st + 1


def s2_gather(a, img, tap, R=3, st=2, pad=1):
    """strided forward operand of one tap: x[st i + r - pad][st j + s - pad] over the output grid, zero outside"""
    Nimg, H, W = img
    Ho, Wo = out_hw(img, R, st, pad)
    r, s = tap // R, tap % R
    xp = torch.zeros(Nimg, H + 2 * pad, W + 2 * pad, a.shape[1], dtype=a.dtype, device=a.device)
    xp[:, pad:H + pad, pad:W + pad] = a.reshape(Nimg, H, W, -1)
    return xp[:, r:r + st * Ho:st, s:s + st * Wo:st].reshape(Nimg * Ho * Wo, -1)


def s2_scatter(acc, v, img, tap, R=3, st=2, pad=1):
    """strided data gradient: dx[st i + r - pad][st j + s - pad] += v[i][j] on the zero-padded accumulator"""
    Nimg, H, W = img
    Ho, Wo = out_hw(img, R, st, pad)
    r, s = tap // R, tap % R
    acc[:, r:r + st * Ho:st, s:s + st * Wo:st] += v.view(Nimg, Ho, Wo, -1)


def _geo(c):
    return (c.R, c.st, c.pad)


def _s2_dgrad(c, a, wl):
    """a [Ph][Ci] float64, wl [Ci][T][Co]: the transposed strided conv -> [P full][Co]"""
    Nimg, H, W = c.img
    pad = c.pad
    acc = torch.zeros(Nimg, H + 2 * pad, W + 2 * pad, c.Co, dtype=a.dtype, device=a.device)
    for t in range(c.T):
        s2_scatter(acc, a @ wl[:, t, :], c.img, t, *_geo(c))
    return acc[:, pad:H + pad, pad:W + pad].reshape(-1, c.Co)


def conv64(c, a):
    """float64 conv of operand a [P][Ci] (float64): forward from wk, data gradient from the layer's weight W"""
    if c.kind in ("s2", "gen"):
        if c.dgrad:
            return _s2_dgrad(c, a, layer_weight(c).double())
        wk = c.wk.double()
        return sum(s2_gather(a, c.img, t, *_geo(c)) @ wk[:, t, :].t() for t in range(c.T))
    if c.dgrad:
        Wl = layer_weight(c).double()                                      # [Ci][T][Co]
        return sum(tap_operand(a, c.img, t, c.T, True) @ Wl[:, t, :] for t in range(c.T))
    wk = c.wk.double()
    return sum(tap_operand(a, c.img, t, c.T) @ wk[:, t, :].t() for t in range(c.T))


def conv_abs(c, a_abs):
    """sum over taps of |operand| |w|: the magnitude S, and the Lipschitz term of an operand error"""
    wk = c.wk.double().abs()
    if c.kind in ("s2", "gen"):
        if c.dgrad:
            return _s2_dgrad(c, a_abs, layer_weight(c).double().abs())
        return sum(s2_gather(a_abs, c.img, t, *_geo(c)) @ wk[:, t, :].t() for t in range(c.T))
    return sum(tap_operand(a_abs, c.img, t, c.T) @ wk[:, t, :].t() for t in range(c.T))


def ref_operand(c):
    """-> (operand in float64, its error bound e_a or None if exact, dt Elem parts (ref, S) for pre)"""
    x = c.x.double()
    if c.pro:
        a, S = B.ref_apply(c.x, *c.pro_ops)
        ea = None if c.family == "integer" else 2.0 ** -8 * a.abs() + B.C_Y * U * S
        return a, ea, (a, S)
    if c.pre:
        t, mean, inv, gamma, dg, db = c.pre_ops
        dt, S = B.ref_bwd_apply(c.x, t, mean, inv, gamma, dg, db, None)
        ea = None if c.family == "integer" else 2.0 ** -8 * dt.abs() + B.C_DX * U * S
        return dt, ea, (dt, S)
    return x, None, None


def mask_parts(c):
    """-> (mask z > 0, ambiguity band 0 < |z| <= 2^-40 (|t msc| + |msh|), exact zeros z == 0)"""
    t, _, _, msc, msh = c.bn
    p, h = t.double() * msc.double(), msh.double()
    z = p + h
    return z > 0, (z != 0) & (z.abs() <= 2.0 ** -40 * (p.abs() + h.abs())), z == 0


def reference(c, dt_own=None):
    """-> {"y": Elem (bnb: the unmasked dx), "mask"?, "dt"?: (ref, S)}.  dt_own: the kernel's own dt_out (pre == 1):
    the operand is then exact"""
    a, ea, dt = ref_operand(c)
    if dt_own is not None:
        a, ea = dt_own.double(), None
    y, S = conv64(c, a), conv_abs(c, a.abs())
    A = conv_abs(c, ea) if ea is not None else torch.zeros_like(y)
    if c.res is not None:
        r = c.res.double() * (c.keep.double() if c.keep is not None else 1.0)
        y, S = y + r, S + r.abs()
    out = {"y": Elem(y, A, S, acc_const(c.T * c.Ci))}
    if dt is not None:
        out["a1" if c.pro else "dt"] = dt
    if c.bn is not None:
        out["mask"] = mask_parts(c)[0]
    return out


def ref_slab(c, y_own):
    """-> {"slab_s": (ref, bound), "slab_q": (ref, bound)} [Co] from the kernel's own bf16 output"""
    r = y_own.double()
    if c.epi == "stats":
        s, q, Ts, Tq = r.sum(0), (r * r).sum(0), r.abs().sum(0), (r * r).sum(0)
    else:
        t, mean, inv = c.bn[0].double(), c.bn[1].double(), c.bn[2].double()
        s, q = r.sum(0), (r * (t - mean) * inv).sum(0)
        Ts = r.abs().sum(0)
        Tq = inv * ((r * t).abs().sum(0) + mean.abs() * Ts)
    return {"slab_s": (s, K_SLAB * U * Ts + U * s.abs() + TINY), "slab_q": (q, K_SLAB * U * Tq + U * q.abs() + TINY)}


def slab_totals(slab, Co):
    """the [2 * bins][Co] fp32 slab -> float64 column totals [2][Co]"""
    return slab.view(-1, 2, Co).double().sum(0)


# ------------------------------------------------------------------------------------------------ checks
def check(c, outs, ref=None):
    """a kernel's (or model's) outputs {"y", "dt"?, "slab"? ([2][Co] float64 totals)} -> {kind: worst error / bound}"""
    r = {}
    if c.pre == 1:
        dref, dS = (ref or reference(c))["dt"]
        if c.family == "integer":
            r["dt"] = check_exact(outs["dt"], Elem(dref, None, None, None), "dt_out")
        else:
            r["dt"] = B.check_elem(outs["dt"], dref, dS, B.C_DX, "dt_out")
        ref = reference(c, dt_own=outs["dt"])
    if c.pro == 2:
        aref, aS = (ref or reference(c))["a1"]
        if c.family == "integer":
            r["a1"] = check_exact(outs["a1"], Elem(aref, None, None, None), "pro_out")
        else:
            r["a1"] = B.check_elem(outs["a1"], aref, aS, B.C_Y, "pro_out")
        ref = reference(c, dt_own=outs["a1"])
    ref = ref or reference(c)
    one = check_exact if c.family == "integer" else check_elem
    y, e = outs["y"], ref["y"]
    if c.poison:
        assert torch.isfinite(y.float()).all(), "a NaN outside the image reached the result"
    if c.epi == "bnb":
        m = ref["mask"]
        off = torch.where(m, torch.zeros_like(y), y)
        assert bits_equal(off, torch.zeros_like(y)), \
            f"gm must be +0 where t msc + msh <= 0 ({int((off.view(torch.int16) != 0).sum())} elements are not)"
        r["gm"] = one(y, e, "gm", m)
    else:
        r["y_pro" if c.pro == 1 else "y_pre2" if c.pre == 2 else "y"] = one(y, e, "y")
    if c.epi in ("stats", "bnb"):
        for k, (sref, sb) in ref_slab(c, y).items():
            r[k] = _check_vec64(outs["slab"][0 if k == "slab_s" else 1], sref, sb, k)
    return r


def _check_vec64(got, ref, bound, what):
    ratio = (got.double() - ref).abs() / bound
    worst = ratio.max().item()
    if not worst <= 1.0:
        G._fail(what, ratio, got, ref)
    return worst


def fp32_part(got, e):
    return G.fp32_part(got, e)


# ------------------------------------------------------------------------------------ fp32 models of the kernels
def _tree16(v):
    """[.., 16, N] -> [.., N]: row16_sum's butterfly (lanes 1, 2, 4, 8 apart)"""
    for _ in range(4):
        v = v[..., 0::2, :] + v[..., 1::2, :]
    return v[..., 0, :]


def model_partials(terms):
    """[P][N] fp32 -> [groups of 64 rows][N] fp32: a lane adds its 4 rows (16 apart) in order, then the 16-lane tree"""
    P, N = terms.shape
    Gn = -(-P // 64)
    t = torch.zeros(Gn * 64, N, dtype=F32, device=terms.device)
    t[:P] = terms
    t = t.view(Gn, 4, 16, N)
    lane = t[:, 0].clone()
    for fm in range(1, 4):
        lane = lane + t[:, fm]
    return _tree16(lane)


def _bins(part):
    """64-row partials -> bins (row group % 64) added in order -> float64 total"""
    Gn, N = part.shape
    n = -(-Gn // 64)
    p = torch.zeros(n * 64, N, dtype=F32, device=part.device)
    p[:Gn] = part
    p = p.view(n, 64, N)
    b = p[0].clone()
    for i in range(1, n):
        b = b + p[i]
    return b.double().sum(0)


def model_slab(c, y, mut=None):
    """the slab totals [2][Co] (float64) the epilogue leaves for its own bf16 output y"""
    order = (lambda v: v)
    if c.kind == "s2" and c.dgrad:
        # a partial holds 64 half-resolution pixels of ONE parity class: rows regrouped (64-pixel group, class, pixel)
        Nimg, H, W = c.img

        def order(v):
            v = v.view(Nimg, H // 2, 2, W // 2, 2, -1).permute(0, 1, 3, 2, 4, 5).reshape(c.P, 4, -1)
            Gn = -(-c.P // 64)
            pad = torch.zeros(Gn * 64, 4, v.shape[-1], dtype=v.dtype, device=v.device)
            pad[:c.P] = v
            return pad.view(Gn, 64, 4, -1).permute(0, 2, 1, 3).reshape(Gn * 256, -1)
    r = order(y.float())
    if mut == "stats_lastrow_twice":
        r = torch.cat([r, y.float()[-1:]], 0)
    if c.epi == "stats":
        return torch.stack([_bins(model_partials(r)), _bins(model_partials(r * r))])
    t, mean, inv = order(c.bn[0].float()), c.bn[1], c.bn[2]
    if mut == "stats_lastrow_twice":
        t = torch.cat([t, t[-1:]], 0)
    s = model_partials(r)
    q = (model_partials(r * t) - mean * s) * inv
    return torch.stack([_bins(s), _bins(q)])


def model(c, mut=None, rnd=True):
    """The kernels in fp32: operand prologue (bn_ref's models, rounded to bf16), accumulation in the kernels' order
    (64-channel chunk outer, tap inner, 32-deep steps), the epilogue, round to nearest even.  ``mut``: one of MUTATIONS (a
    planted error where the case has the feature it breaks, else the correct result).  rnd=False keeps y in fp32.
    -> {"y", "dt"? (pre == 1), "slab"? (from the rounded y)}"""
    dev = c.x.device
    out = {}
    a = c.x
    if c.pro:
        a = B.model_apply(c.x, *c.pro_ops)[0]
        if c.pro == 2:
            out["a1"] = a
    elif c.pre:
        t, mean, inv, gamma, dg, db = c.pre_ops
        a = B.model_bwd_apply(c.x, t, mean, inv, gamma, dg, db, None)
        if c.pre == 1:
            out["dt"] = a
    a = a.float()
    wk = c.wk.float()
    if mut == "no_flip" and c.dgrad and c.T == 9 and c.kind != "gen":      # (the implicit-GEMM engine takes W as is)
        wk = wk.flip(1)
    if mut == "skip_last8":
        a = a.clone()
        a[:, -8:] = 0
    if mut == "wstep_next" and c.kind == "p1" and c.Ci <= 256:
        nb, g, steps = areg_plan(c.P, c.Ci, c.Co)
        if steps > 1:          # step s reads the image of step s + 1 (the last one its own)
            ch = torch.arange(c.Co, device=dev) // nb
            nxt = torch.where((ch % steps) + 1 < steps, ch + 1, ch)
            wk = wk[nxt * nb + torch.arange(c.Co, device=dev) % nb]
    Nimg, H, W = c.img
    acc = torch.zeros(c.Po, c.Co, dtype=F32, device=dev)
    strided = c.kind in ("s2", "gen")
    if strided and c.dgrad:
        accp = torch.zeros(Nimg, H + 2 * c.pad, W + 2 * c.pad, c.Co, dtype=F32, device=dev)
    for c0 in range(0, c.Ci, 64):
        for tap in range(c.T):
            if strided:
                for k0 in range(c0, min(c0 + 64, c.Ci), 32):
                    if c.dgrad:          # layer tap ``tap`` is the kernel's tap T - 1 - tap
                        s2_scatter(accp, (a[:, k0:k0 + 32].double() @ wk[:, c.T - 1 - tap, k0:k0 + 32].double().t()).float(),
                                   c.img, tap, *_geo(c))
                    else:
                        acc = acc + (s2_gather(a[:, k0:k0 + 32], c.img, tap, *_geo(c)).double()
                                     @ wk[:, tap, k0:k0 + 32].double().t()).float()
                continue
            op = tap_operand(a[:, c0:c0 + 64], c.img, tap, c.T)
            if c.T == 9:
                if mut == "tap_drop_border" and tap == 4:
                    op = op.clone()
                    op[0] = 0
                if mut == "left_wrap" and tap % 3 == 0 and W > 1:
                    # x == 0 reads flat pixel p + (r - 1) W - 1 (the previous row's last) where that row is in the image
                    p = torch.arange(c.P, device=dev)
                    yy = p // W % H + tap // 3 - 1
                    src = p + (tap // 3 - 1) * W - 1
                    bad = (p % W == 0) & (yy >= 0) & (yy < H) & (src >= 0)
                    op = torch.where(bad[:, None], a[src.clamp(0, c.P - 1), c0:c0 + 64], op)
            for k0 in range(0, 64, 32):
                acc = acc + (op[:, k0:k0 + 32].double() @ wk[:, tap, c0 + k0:c0 + k0 + 32].double().t()).float()
    v = accp[:, c.pad:H + c.pad, c.pad:W + c.pad].reshape(-1, c.Co) if (strided and c.dgrad) else acc
    if c.res is not None:
        keep = c.keep
        if keep is not None and mut == "bit_order":
            keep = keep.view(c.Po, c.Co // 8, 8).flip(-1).reshape(c.Po, c.Co)
        v = v + (c.res.float() if keep is None else torch.where(keep, c.res.float(), torch.zeros_like(v)))
    rb = (lambda t: trunc_bf16(t) if mut == "bf16_trunc" else t.to(BF))
    if c.bn is not None:
        # the kernel's own mask: fmaf(t, msc, msh) > 0 in fp32, the fma as an exact (float64) product and sum rounded once
        z32 = (c.bn[0].double() * c.bn[3].double() + c.bn[4].double()).float()
        m, zero = z32 > 0, z32 == 0
        if mut == "mask_ge":
            m = m | zero
        v = torch.where(m, rb(v).float() if rnd else v, torch.zeros_like(v))
    y = rb(v) if rnd else v
    out["y"] = y
    if c.epi in ("stats", "bnb") and rnd:
        out["slab"] = model_slab(c, y, mut)
    return out


def slab_fp32_part(c, y, slab):
    """worst |slab - ref| / (u T) of the slab model (what MEASURED["slab"] records)"""
    worst = 0.0
    for i, (k, (ref, bound)) in enumerate(ref_slab(c, y).items()):
        T = (bound - U * ref.abs() - TINY) / (K_SLAB * U)
        worst = max(worst, (((slab[i] - ref).abs() - U * ref.abs()).clamp_min(0.0) / (U * T + 1e-300)).max().item())
    return worst


# =================================================================================================== weight gradients
# conv_wgrad(x, dy, R, S, st, pad, pro=, out=): fp32 dW[ko][tap][c] = old + sum over output pixels p of dy[p][ko] a[p @ tap][c],
# a = x or bf16(relu(fma(x, sc, sh))) (pro=).  Routes (kernels.conv_wgrad, mirrored by ``wg_route``): the direct 3x3
# stride-1 kernel (conv3x3_wgrad.hip; W in 7 / 14 / 28 / 56), the direct stride-2 kernel (Wo in 7 / 14 / 28, tuning
# s2_halo bit 8), the ping-pong 1x1 route (P % 32 == 0, no pro) and the implicit-GEMM fallback (everything else).
# Reference: float64 dy^T . gather(a) per tap; S = |dy|^T . gather|a| + |old|; with pro= the Lipschitz term
# |dy|^T . gather(e_a).  Bound: fp32, |got - ref| <= A + c u S + u |ref| + TINY, c = min(4 MEASURED["wgrad"], P + G + 3).
# The model: w3_plan's split (G blocks per 64 x 64 chunk pair, block ``part`` owns tiles [part tiles / G, (part + 1)
# tiles / G) of 256 pixels), a block's partial accumulated in fp32 over 32-pixel MFMA steps, then the reduce kernel's
# order (PG groups, group pg adds partials pg, pg + PG, ... in order; the groups in order; old + sum).  The ping-pong
# and implicit-GEMM routes sum split-K slabs / atomics instead; the same model with G = 8 stands in for them, the 4x
# margin covering their order.
WG_MUTATIONS = ["wg_overwrite", "wg_skip_last_tile", "wg_tap_swap", "wg_partial_twice"]
# (Nimg, H, W), (R, st, pad), C, Ko, pro.  Direct stride 1: W = 7 / 14 / 28 / 56; pixel counts either side of one tile
# (126, 252 | 266); C != Ko; odd H; H = 1 (no direct shape: w3_smem needs two bracket rows per image, so the
# fallback runs).  w3_plan's boundaries: G = min(ceil(128 / pairs), tiles): with 16 chunk pairs (256 -> 256) G = 8, so
# 2016 pixels (8 tiles: one tile per block, G == tiles) against 2072 (9 tiles: the first block with two, uneven
# split); with 8 pairs G = 16 = the reduce kernel's first PG threshold, 4144 pixels (17 tiles).
WGRAD = [((2, 9, 7), (3, 1, 1), 64, 128, 0), ((4, 9, 7), (3, 1, 1), 64, 64, 1), ((1, 19, 14), (3, 1, 1), 128, 64, 0),
         ((2, 9, 28), (3, 1, 1), 64, 64, 1), ((1, 5, 56), (3, 1, 1), 64, 192, 0), ((8, 9, 28), (3, 1, 1), 256, 256, 0),
         ((1, 37, 56), (3, 1, 1), 256, 256, 1), ((2, 37, 56), (3, 1, 1), 256, 128, 0), ((30, 1, 14), (3, 1, 1), 64, 64, 0),
         # direct stride 2 at Wo = 7 / 14 / 28
         ((1, 6, 14), (3, 2, 1), 64, 64, 0), ((2, 10, 28), (3, 2, 1), 128, 64, 1), ((1, 6, 56), (3, 2, 1), 64, 128, 0),
         # 1x1: ping-pong at P % 32 == 0, the fallback at P % 32 != 0 and with pro=
         ((1, 1, 256), (1, 1, 0), 64, 128, 0), ((1, 1, 250), (1, 1, 0), 64, 128, 0), ((1, 1, 256), (1, 1, 0), 128, 64, 1),
         # implicit-GEMM fallback: 3x3 at C = 72, 3x3 stride 2 with odd H, W, 1x1 stride 2
         ((2, 5, 6), (3, 1, 1), 72, 72, 1), ((1, 7, 9), (3, 2, 1), 72, 64, 0), ((2, 6, 6), (1, 2, 0), 72, 128, 0)]


def w3_supported(H, W, C, Ko):
    """pdnn_conv3x3_wgrad_supported"""
    if C % 64 or Ko % 64 or C < 64 or Ko < 64 or H < 1 or W not in (7, 14, 28, 56):
        return False
    Rr = (255 + W - 1) // W + 3
    if Rr * W > 512:
        return False
    hrows = Rr + 2 * ((Rr + H - 1) // H + 1) + 1
    return 256 * 64 * 2 + hrows * (W + 2) * 160 <= 160 * 1024


def w3_plan(P, C, Ko):
    """-> (tiles, G)"""
    tiles, pairs = -(-P // 256), (Ko // 64) * (C // 64)
    return tiles, max(1, min(-(-128 // pairs), tiles))


def wg_route(img, geo, C, Ko, pro, s2_bit8=True):
    Nimg, H, W = img
    if geo == (3, 1, 1) and w3_supported(H, W, C, Ko):
        return "direct"
    if geo == (3, 2, 1) and s2_bit8 and H % 2 == 0 and W % 2 == 0 and w3_supported(H // 2, W // 2, C, Ko):
        return "direct_s2"
    if geo == (1, 1, 0) and not pro and (Nimg * H * W) % 32 == 0:
        return "pp"
    return "gemm"


def wgrad_cases():
    out = []
    for i, (img, geo, C, Ko, pro) in enumerate(WGRAD):
        for j in range(2):
            fam = FAMILIES[(i + 3 * j) % 5] if j == 0 else ("integer" if FAMILIES[i % 5] != "integer" else "positive")
            cid = f"wg-{fam}-{img[0]}x{img[1]}x{img[2]}-r{geo[0]}s{geo[1]}-{C}to{Ko}-pro{pro}"
            out.append((cid, (img, geo, C, Ko, pro, fam)))
    return out


def wg_make(img, geo, C, Ko, pro, family):
    Nimg, H, W = img
    R, st, pad = geo
    Ho, Wo = out_hw(img, R, st, pad)
    P, Po, T = Nimg * H * W, Nimg * Ho * Wo, R * R
    g = torch.Generator().manual_seed(G._seed("wg", family, Nimg, H, W, C, Ko, pro, *geo))
    integer = family == "integer"
    if integer:
        assert Po * 10 * 4 < 2 ** 24
        x = torch.randint(-4, 5, (P, C), generator=g).double()
        dy = torch.randint(-4, 5, (Po, Ko), generator=g).double()
    elif family == "positive":
        x = torch.rand(P, C, generator=g, dtype=F64) * 1.5 + 0.25
        dy = torch.rand(Po, Ko, generator=g, dtype=F64) * 1.5 + 0.25
    elif family == "cancelling":          # the second half of the pixels cancels the first (1x1: exactly paired)
        x = torch.randn(P, C, generator=g, dtype=F64)
        dy = torch.randn(Po, Ko, generator=g, dtype=F64)
        if Po > 1:
            h = Po // 2
            dy[h:2 * h] = -dy[:h] + 2.0 ** -5 * torch.randn(h, Ko, generator=g, dtype=F64)
            if P == Po:
                x[h:2 * h] = x[:h]
    else:
        x, dy = torch.randn(P, C, generator=g, dtype=F64), torch.randn(Po, Ko, generator=g, dtype=F64)
    old = (torch.randint(-8, 9, (Ko, T, C), generator=g).float() if integer else torch.randn(Ko, T, C, generator=g) * 2.0)
    c = SimpleNamespace(kind="wg", img=img, R=R, st=st, pad=pad, P=P, Po=Po, T=T, Ci=C, Co=Ko, family=family, pro=pro,
                        poison=family == "poisoned", x=x.to(BF), dy=dy.to(BF), old=old, pro_ops=None)
    if pro:
        pick = lambda vals, n: torch.tensor(vals, dtype=F32)[torch.randint(0, len(vals), (n,), generator=g)]    # noqa: E731
        c.pro_ops = ((pick([1.0, 2.0, -1.0], C), torch.randint(-2, 3, (C,), generator=g).float()) if integer else
                     ((torch.rand(C, generator=g) + 0.5) * pick([1.0, 1.0, -1.0], C), torch.randn(C, generator=g) * 0.5))
    return c


def _wg_gather_all(c, a):
    """[P][C] -> [Po][T C]: every tap's operand side by side"""
    return torch.cat([s2_gather(a, c.img, t, c.R, c.st, c.pad) for t in range(c.T)], 1)


def wg_reference(c):
    """-> Elem over dW [Ko][T][C]"""
    dy = c.dy.double()
    if c.pro:
        a, Sa = B.ref_apply(c.x, *c.pro_ops)
        ea = None if c.family == "integer" else 2.0 ** -8 * a.abs() + B.C_Y * U * Sa
    else:
        a, ea = c.x.double(), None
    shp = (c.Co, c.T, c.Ci)
    ref = (dy.t() @ _wg_gather_all(c, a)).view(shp) + c.old.double()
    S = (dy.abs().t() @ _wg_gather_all(c, a.abs())).view(shp) + c.old.double().abs()
    A = (dy.abs().t() @ _wg_gather_all(c, ea)).view(shp) if ea is not None else torch.zeros_like(ref)
    tiles, Gp = w3_plan(c.Po, c.Ci, c.Co)
    return Elem(ref, A, S, min(4.0 * MEASURED["wgrad"], c.Po + Gp + 3.0))


def wg_model(c, mut=None):
    """fp32 dW of the direct kernels' structure (see above) -> [Ko][T][C] fp32"""
    a = (B.model_apply(c.x, *c.pro_ops)[0] if c.pro else c.x).float()
    g = _wg_gather_all(c, a)
    if mut == "wg_tap_swap" and c.T == 9:
        g = g.view(c.Po, 9, c.Ci)[:, [1, 0, 2, 3, 4, 5, 6, 7, 8]].reshape(c.Po, -1)
    dyt = c.dy.float().t()
    tiles, Gp = w3_plan(c.Po, c.Ci, c.Co)
    if wg_route(c.img, (c.R, c.st, c.pad), c.Ci, c.Co, c.pro) in ("pp", "gemm"):
        Gp = min(8, tiles)
    parts = []
    for part in range(Gp):
        t0, t1 = part * tiles // Gp, (part + 1) * tiles // Gp
        if mut == "wg_skip_last_tile" and part == Gp - 1 and c.Po > 32:
            t1 = t1 - 1 if tiles > 1 else t1
        acc = torch.zeros(c.Co, c.T * c.Ci, dtype=F32, device=a.device)
        p1 = min(t1 * 256, c.Po)
        if mut == "wg_skip_last_tile" and tiles == 1:
            p1 = (c.Po - 1) // 32 * 32
        for p0 in range(t0 * 256, p1, 32):
            e = min(p0 + 32, p1)
            acc = acc + (dyt[:, p0:e].double() @ g[p0:e].double()).float()
        parts.append(acc)
    if mut == "wg_partial_twice" and Gp > 0:
        parts.append(parts[-1])
    PG = 32 if Gp >= 256 else 16 if Gp >= 128 else 8 if Gp >= 64 else 4 if Gp >= 32 else 2 if Gp >= 16 else 1
    groups = []
    for pg in range(PG):
        sg = torch.zeros_like(parts[0])
        for b in range(pg, len(parts), PG):
            sg = sg + parts[b]
        groups.append(sg)
    tot = groups[0]
    for sg in groups[1:]:
        tot = tot + sg
    old = torch.zeros_like(c.old) if mut == "wg_overwrite" else c.old
    return old + tot.view(c.Co, c.T, c.Ci)


def wg_check(c, got, e=None):
    e = e or wg_reference(c)
    if c.poison:
        assert torch.isfinite(got).all()
    return (check_exact if c.family == "integer" else check_elem)(got, e, "dW")
