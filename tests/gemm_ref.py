"""A float64 reference of the GEMM engines (csrc/kernels/gemm_mfma.hip: the register-staged 128-row kernel;
gemm_glds.h: the 256-row engine; gemm_pp.hip: the ping-pong engine with its split-K slabs), the elementwise bounds they
are held to, fp32 models of every entry point (a stand-in for a correct kernel, and the carrier of planted errors) and
the seeded inputs and case lists shared by the GPU tests (test_gemm_gpu.py) and the CPU self-check
(test_gemm_ref_cpu.py).  Everything here runs on CPU and GPU tensors alike.  The fp8 GEMM and the convolutions are out
of scope (test_fp8_gpu.py, test_conv*_gpu.py keep them).

Entry points: gemm_nt (bias, relu, out_f32, alpha, out), gemm_nn, gemm_tn_acc, gemm_nt_ex (act 0/1/2, aux, res, dgelu,
w_kn), gemm_batched (three operand-mode pairs, both output types, res, alpha, causal 0-3, padded batch strides),
pp_wgrad (alpha, rowsum, splits, bn) and gemm_nt_splitk.  A case holds the LOGICAL operands a [.., M, K] and b [.., K, N]
(bf16); each entry point's storage layout (transposed, strided, padded, poisoned) is made from them by the caller.

Every reference is float64 arithmetic on exactly what the kernel receives: the bf16 operands, the fp32 bias, alpha as
the fp32 value the C entry point receives (``f32``), the bf16 residual / dGELU operand and the old contents of an
accumulated output.  Epilogue order, the same in all three engines:
    v = acc * alpha;  v += bias;  ReLU, or GELU(bf16(v)) with aux = bf16(v);  v *= gelu'(u);  v += res;  round.
GELU is the tanh form through a sigmoid, x / (1 + exp2(-2 log2(e) x (c0 + c1 x^2))) (gelu_sig in gemm_common.h), evaluated
on the bf16-rounded pre-activation.  So ``aux`` is checked against the float64 pre-activation and ``y`` against the
float64 GELU of the kernel's OWN aux: each on its own.  Without aux, y carries the Lipschitz term of the unseen rounding.

Notation.  u = 2^-24.  S = |alpha| sum_k |a_k b_k| + |bias| + |res| + |old|: the magnitudes that enter the fp32 sum.
    fp32 outputs:   |got - ref| <= C u S + u |ref| + TINY
    bf16 outputs:   the same + 2^-8 |ref|  (half an ulp of bf16 just above a power of two; a truncating conversion
                    errs by up to 2^-7 |ref| and is caught here and, exactly, by the integer family)
    row sums:       S = |alpha| sum_k |a_k| + |old|
    GELU from aux:  x = aux exactly, so |got - x s(x) - res| <= 2^-8 |ref| + (C_gelu + HW) u (|x| + |res|) + u |ref|:
                    C_gelu u is the fp32 evaluation of s(x) (argument polynomial, exp2, reciprocal), measured below, and
                    HW = 4 allows v_exp_f32 / v_rcp_f32 their ulp each and the denormal flush of exp2
    GELU, no aux:   + LIP (2^-8 |pre| + C u S), LIP = 1.13 >= max |gelu'|: the input moves by its bf16 rounding and
                    its fp32 error
    dGELU:          ref = pre gelu'(u) + res, u given exactly: C u S |gelu'(u)| + (C_dgelu + HW) u |pre| G(u), with
                    G = s (1 + |2 u p(u)|) (1 + 2 |arg|): the magnitudes inside gelu_tanh_grad, see gelu_grad64
The constants.  None is picked in advance: the fp32 models below (fp32 accumulation in 32- or 64-deep slices, the
split-K slab sum, the epilogue order above) run without the bf16 rounding of the result, test_gemm_ref_cpu.py measures
their worst error / (u S) over every family and case of this module, and C is 4x that (the project's margin for the
GPU's different summation order): MEASURED and C below; the CPU test asserts both.  The worst case of the sum is the
positive family at K = 1536 in 32-deep slices (48 roundings of a partial sum that is all of S); C = 30.4 would exceed
the analytic worst case of ANY summation order at small K, (K + 4) u S (K exact bf16 x bf16 products, K - 1 additions,
alpha, bias, the slab sum), and a constant above that asserts nothing.  So a K-term sum is held to
acc_const(K) = min(C, K + 3), and the CPU test asserts that this is below K + 4 for every case.

Input families.  gauss.  positive: every operand > 0 (no cancellation: a dropped slice shows at full size).
cancelling: the second half of K repeats the first with b negated and slightly perturbed, so ref is near 0 while S is
large.  poisoned: gauss whose storage has NaN in every pad column of a strided operand and NaN rows after its last row
(the callers place them; the other families pad with the finite value 777).  integer: operands are integers in [-4, 4],
drawn until no two rows and no two columns (of length >= 8) of an operand are equal; bias, res and old are integers in
[-8, 8]; alpha in {1, 2, -0.5}.  K max|a| max|b| = 16 K < 2^24, so every partial sum is exact in any order: fp32
outputs must equal the reference bit for bit and bf16 outputs its round-to-nearest-even (which also rejects truncation).
The only normalisation is the sign of zero (+0.0 is added to both).  The integer family skips GELU and dGELU.

Causal modes of gemm_batched (square T x T structure): 1: output tiles wholly above the diagonal are not written, so
only k <= q is compared.  2: A is exactly lower triangular and holds NaN at k >= roundup(q + 1, 256): the reduction of a
row tile stops at its last row's diagonal, rounded up to the engines' tile heights (128, 256), so a correct kernel never
reads them; 3: the mirror image (A upper triangular over [m][k], NaN at k < rounddown(m, 256)).  Results must be finite.

Measured fp32 parts (MEASURED; worst error / (u S) of the models without the result's bf16 rounding; the CPU test asserts
the match to 2% both ways): acc 7.6 (positive, 136 x 136 x 1536, 32-deep slices; the gauss family stays below 1),
rowsum 0.298, gelu 2.02, dgelu 2.40 (s(x) and gelu'(x) over every bf16 x with |x| <= 16).  So C = 30.4, 1.19, 8.1, 9.6.

Recorded worst error / bound (both test files print them; the bf16 outputs reach ~1 because the rounding of the result
alone reaches 2^-8 |ref| just above a power of two, and model and kernel then share the worst element):
  fp32 models (test_gemm_ref_cpu.py): y_bf16 0.996, y_f32 0.274, aux 0.996, gelu_y 0.996, gelu_y_noaux 0.944,
    dgelu_y 0.995, rowsum 0.592
  kernels on an MI355X (test_gemm_gpu.py, every engine, tile width and epilogue form, one and several work items per
    block): y_bf16 0.996, y_f32 0.529, aux 0.996, gelu_y 0.996, gelu_y_noaux 0.944, dgelu_y 0.995, rowsum 0.603.  The
    integer family is exact on every engine.  Within 10% of a bound: only the bf16 outputs, by their own rounding (the
    fp32 outputs, which show the accumulation alone, stay near half of theirs).
"""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

U = 2.0 ** -24
TINY = 2.0 ** -115            # fp32 underflow floor of a sum of <= 2^11 terms, as in attn_ref
HW = 4.0                      # ulps allowed to v_exp_f32 / v_rcp_f32 on top of the modelled fp32 evaluation
LIP = 1.13                    # >= max |gelu'(x)| = 1.1289
PAD_FILL = 777.0              # finite filler of pad columns / tail rows outside the poisoned family
G0, G1, G2 = 0.7978845608028654, 0.035677408136300125, 0.10703222440890037
NEG2LOG2E = -2.885390081777927

# worst error / (u S) of the fp32 models with the result's bf16 rounding off (test_gemm_ref_cpu.py asserts it to 2%,
# both ways), and 4x that
MEASURED = {"acc": 7.6, "rowsum": 0.298, "gelu": 2.02, "dgelu": 2.40}
C = {k: 4.0 * v for k, v in MEASURED.items()}
MIN_K = 8

Elem = namedtuple("Elem", "ref A S c")        # float64 reference, absolute slack, fp32 magnitude and its constant
FAMILIES = ["gauss", "positive", "cancelling", "poisoned", "integer"]
INT_ALPHA = [1.0, 2.0, -0.5]
REAL_ALPHA = [1.0, 0.37, -1.5]


def f32(v):
    """a Python float rounded to fp32, as the C entry points receive alpha"""
    return torch.tensor(v, dtype=F32).item()


# ------------------------------------------------------------------------------------------------ shapes
def _cycle(Ms, Ns, Ks):
    return [(M, N, Ks[(i + j) % len(Ks)]) for i, M in enumerate(Ms) for j, N in enumerate(Ns)]


MINIMAL = [(1, 8, 8), (16, 16, 32), (8, 8, 64)]
# row-tile edges of the 128- and 256-row tiles x column-tile edges of the 64 / 128 / 256-wide tiles; K = 72: partial
# 64-deep tile, 96 / 160: K % 64 != 0 (the sk64 fallback), 128: K % 64 == 0
EDGE = _cycle([127, 128, 129, 255, 256, 257], [56, 64, 72, 120, 128, 136, 264], [72, 96, 128, 160])
KSTEPS = [(300, 296, 64), (136, 136, 1536), (136, 136, 1600)]       # half-LDS single step; 24 | 25 steps: kLowKBn64
MULTI = [(520, 776, 96)]                                             # several work items per block, ragged edges
GLDS_BN = [(264, N, 64) for N in (504, 520, 1016, 1032)]             # glds_bn: 64 | 128 | 256 wide
NT_SHAPES = MINIMAL + EDGE + KSTEPS + MULTI + GLDS_BN
F32_SHAPES = [(M, N, K) for N in (1, 3, 13, 20, 68) for M, K in ((129, 72), (16, 32))]   # out_f32, N % 8 != 0 allowed
PP_BN = [96, 128, 192, 256, 257, 288]


def pp_bn_shapes(w):
    """N either side of tile width w (257 = the 256-wide tile with the deeper ring), M one and two row tiles"""
    w = 256 if w == 257 else w
    return [(M, N, K) for N, K in ((w - 8, 128), (w, 96), (w + 8, 128)) for M in (16, 264)]


EPI_SHAPES = [(264, 136, 96), (520, 776, 96)]                        # pp_epi_slack x pp_epi_pair
WGRAD_K = [96, 160, 544, 1056]
WGRAD_SPLITS = [1, 2, 3, 5, 16, 17, 40]
WGRAD_MN = [(8, 8), (8, 136), (264, 8), (264, 136)]
TN_SHAPES = [(72, 200, 136), (8, 8, 8), (264, 136, 2048)]
CAUSAL_T = [8, 136, 256, 264, 512, 520]       # 256, 512: K = T % 64 == 0, what glds accepts; 512: two of its row tiles
CAUSAL_D = [8, 64]
BATCHES = [(1, 1), (2, 3)]


# ------------------------------------------------------------------------------------------------ inputs
def _seed(*parts):
    s = 17
    for p in parts:
        s = (s * 1000003 + (hash(p) if not isinstance(p, str) else sum(ord(ch) * (i + 7) for i, ch in enumerate(p)))) % (2 ** 31 - 1)
    return s


def _distinct(t):
    """no two rows and no two columns of the last two dims equal (vectors shorter than 8 cannot be told apart)"""
    m = t.reshape(-1, *t.shape[-2:])
    for x in m:
        R, Cc = x.shape
        if Cc >= 8 and torch.unique(x, dim=0).shape[0] != R:
            return False
        if R >= 8 and torch.unique(x, dim=1).shape[1] != Cc:
            return False
    return True


def gen_ab(family, M, N, K, g, batch=()):
    """logical a [*batch, M, K], b [*batch, K, N], float64 values that bf16 holds exactly"""
    rn = lambda *s: torch.randn(*batch, *s, generator=g, dtype=F64)        # noqa: E731
    if family == "integer":
        assert 16 * K < 2 ** 24
        for _ in range(32):
            a = torch.randint(-4, 5, (*batch, M, K), generator=g).double()
            b = torch.randint(-4, 5, (*batch, K, N), generator=g).double()
            if _distinct(a) and _distinct(b):
                return a, b
        raise AssertionError("integer family: no distinct draw")
    if family == "positive":
        a = torch.rand(*batch, M, K, generator=g, dtype=F64) * 1.5 + 0.25
        b = torch.rand(*batch, K, N, generator=g, dtype=F64) * 1.5 + 0.25
    elif family == "cancelling":
        h = K // 2
        a1, b1 = rn(M, h).to(BF).double(), rn(h, N).to(BF).double()
        a = torch.cat([a1, a1], -1)
        b = torch.cat([b1, -b1 + 2.0 ** -5 * rn(h, N)], -2)
    else:
        a, b = rn(M, K), rn(K, N)
    return a.to(BF).double(), b.to(BF).double()


def make(ep, family, M, N, K, idx=0, batch=(), **opt):
    """A seeded case on the CPU.  ``opt``: alpha, bias, act (0/1/2), out_f32, res, aux, dgelu, w_kn, old, rowsum,
    splits, bn, pad (strided operands and ldc > N), amode, bmode, causal.  ``idx`` picks alpha and the seed."""
    g = torch.Generator().manual_seed(_seed(ep, family, M, N, K, idx, *batch))
    integer = family == "integer"
    a, b = gen_ab(family, M, N, K, g, batch)
    c = SimpleNamespace(ep=ep, family=family, M=M, N=N, K=K, idx=idx, batch=tuple(batch), a=a.to(BF), b=b.to(BF),
                        alpha=1.0, bias=None, act=0, out_f32=False, res=None, aux=False, du=None, w_kn=False, old=None,
                        rowsum_old=None, splits=0, bn=0, pad=0, amode=0, bmode=0, causal=0, poison=family == "poisoned")
    small = lambda *s: (torch.randint(-8, 9, (*batch, *s), generator=g).double() if integer      # noqa: E731
                        else torch.randn(*batch, *s, generator=g, dtype=F64) * 2.0)
    if opt.get("alpha"):
        c.alpha = (INT_ALPHA if integer else REAL_ALPHA)[idx % 3] if opt["alpha"] is True else opt["alpha"]
    if opt.get("bias"):
        c.bias = small(N).float()
    if opt.get("res"):
        c.res = small(M, N).to(BF)
    if opt.get("dgelu"):
        c.du = (torch.randn(*batch, M, N, generator=g, dtype=F64) * 1.5).to(BF)
    if opt.get("old"):
        c.old = small(M, N).float()
    if opt.get("rowsum"):
        c.rowsum_old = small(M).float()
    for k in ("act", "out_f32", "aux", "w_kn", "splits", "bn", "pad", "amode", "bmode", "causal"):
        if k in opt:
            setattr(c, k, opt[k])
    if c.causal in (2, 3):
        # A exactly triangular over [m][k]; NaN where no engine's row tile reaches (module docstring)
        assert M == K
        q, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
        av = c.a.double()
        if c.causal == 2:
            av = torch.where(k <= q, av, torch.zeros_like(av))
            av = torch.where(k >= (q + 256) // 256 * 256, torch.full_like(av, float("nan")), av)
        else:
            av = torch.where(k >= q, av, torch.zeros_like(av))
            av = torch.where(k < q // 256 * 256, torch.full_like(av, float("nan")), av)
        c.a = av.to(BF)
    return c


def case_to(c, device):
    return SimpleNamespace(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(c).items()})


def nt_variants(family, N):
    """the option sets every (family, shape) of NT_SHAPES runs: (name, entry point, options).  Odd ``idx`` pads."""
    if N % 8:
        return [("nt_f32_bias_relu", "nt", dict(out_f32=True, bias=True, act=1, alpha=True)),
                ("nt_f32_plain", "nt", dict(out_f32=True, alpha=True))]
    v = [("nt_bias", "nt", dict(bias=True, alpha=True)),
         ("nt_f32_bias_relu", "nt", dict(out_f32=True, bias=True, act=1, alpha=True)),
         ("nn", "nn", dict(alpha=True)),
         ("nn_f32", "nn", dict(alpha=True, out_f32=True)),
         ("ex_relu_res", "nt_ex", dict(act=1, bias=True, res=True)),
         ("ex_res_kn", "nt_ex", dict(res=True, w_kn=True))]
    if family != "integer":
        v += [("ex_gelu_aux_res", "nt_ex", dict(act=2, bias=True, aux=True, res=True)),
              ("ex_gelu", "nt_ex", dict(act=2, bias=True)),
              ("ex_dgelu_res_kn", "nt_ex", dict(dgelu=True, res=True, w_kn=True)),
              ("ex_dgelu", "nt_ex", dict(dgelu=True, bias=True))]
    return v


def nt_cases(shapes, families=FAMILIES):
    """[(id, make-arguments)] of the plain-GEMM entry points over ``shapes``"""
    out = []
    for si, (M, N, K) in enumerate(shapes):
        for fi, fam in enumerate(families):
            for vi, (name, ep, opt) in enumerate(nt_variants(fam, N)):
                idx = si + fi + vi
                out.append((f"{name}-{fam}-{M}x{N}x{K}", (ep, fam, M, N, K, idx), dict(opt, pad=8 * (idx % 2))))
    return out


def wgrad_cases():
    """pp_wgrad: every K x splits, the (M, N) corners, bn, alpha and rowsum rotating so each value meets each split"""
    out = []
    i = 0
    for K in WGRAD_K:
        for sp in WGRAD_SPLITS:
            M, N = WGRAD_MN[i % 4]
            fam = FAMILIES[i % 5]
            alpha = (INT_ALPHA[i % 3] if fam == "integer" else (1.0, 0.5)[i % 2])
            opt = dict(splits=sp, bn=(0, 128, 256)[i % 3], alpha=alpha, rowsum=i % 2 == 0, old=True, pad=4 * (i // 2 % 2))
            out.append((f"wgrad-{fam}-{M}x{N}x{K}-s{sp}", ("wgrad", fam, M, N, K, i), opt))
            i += 1
    # the rest of the cross at the uneven, ragged corner: every family, every bn, rowsum on and off
    for fam in FAMILIES:
        for bn in (0, 128, 256):
            for rs in (False, True):
                alpha = INT_ALPHA[i % 3] if fam == "integer" else 0.5
                out.append((f"wgrad-{fam}-264x136x544-s5-bn{bn}-rs{int(rs)}", ("wgrad", fam, 264, 136, 544, i),
                            dict(splits=5, bn=bn, alpha=alpha, rowsum=rs, old=True, pad=4 * (i % 2))))
                i += 1
    return out


def splitk_cases():
    out = []
    i = 0
    for K in WGRAD_K:
        for sp in WGRAD_SPLITS:
            M, N = WGRAD_MN[(i + 1) % 4]
            fam = FAMILIES[(i + 2) % 5]
            out.append((f"splitk-{fam}-{M}x{N}x{K}-s{sp}", ("splitk", fam, M, N, K, i), dict(splits=sp, pad=8 * (i % 2))))
            i += 1
    return out


def tn_cases():
    out = []
    for si, (M, N, K) in enumerate(TN_SHAPES):
        for fi, fam in enumerate(FAMILIES):
            i = si + fi
            alpha = INT_ALPHA[i % 3] if fam == "integer" else (1.0, -0.5)[i % 2]
            out.append((f"tn-{fam}-{M}x{N}x{K}", ("tn", fam, M, N, K, i), dict(alpha=alpha, old=True, pad=4 * (i % 2))))
    return out


MODE_PAIRS = [(0, 0), (0, 1), (1, 1)]


def batched_cases():
    """dense: every mode pair x output type x batch, res and alpha = 0.125; causal: the attention chain's five forms"""
    out = []
    i = 0
    for (M, N, K) in [(72, 136, 64), (136, 72, 72), (264, 264, 128)]:
        for am, bm in MODE_PAIRS:
            for f32o in (False, True):
                for nb in BATCHES:
                    fam = FAMILIES[i % 5]
                    alpha = INT_ALPHA[i % 3] if fam == "integer" else 0.125
                    opt = dict(amode=am, bmode=bm, out_f32=f32o, alpha=alpha, res=not f32o and i % 2 == 0, pad=8 * (i % 2))
                    out.append((f"bat-{fam}-{M}x{N}x{K}-a{am}b{bm}-f{int(f32o)}-nb{nb[0]}x{nb[1]}",
                                ("batched", fam, M, N, K, i, nb), opt))
                    i += 1
    for T in CAUSAL_T:
        for d in CAUSAL_D:
            for form, (M, N, K, am, bm, f32o, mode) in enumerate([(T, T, d, 0, 0, True, 1), (T, d, T, 0, 1, False, 2),
                                                                  (T, d, T, 1, 1, False, 3)]):
                for nb in BATCHES:
                    fam = FAMILIES[i % 5]
                    alpha = INT_ALPHA[i % 3] if fam == "integer" else 0.125
                    opt = dict(amode=am, bmode=bm, out_f32=f32o, alpha=alpha, causal=mode, pad=8 * (i % 2))
                    out.append((f"causal{mode}-{fam}-T{T}-d{d}-nb{nb[0]}x{nb[1]}", ("batched", fam, M, N, K, i, nb), opt))
                    i += 1
    return out


def pp_bn_all():
    seen, out = set(), []
    for w in PP_BN:
        for s in pp_bn_shapes(w):
            if s not in seen:
                seen.add(s)
                out.append(s)
    return out


# the shapes of the GPU lists the planted errors are run on: ragged in M (two and three row tiles) and N, K % 64 != 0
MUT_SHAPES = [(257, 264, 160), (127, 56, 72), (129, 120, 96), (520, 776, 96)]
MUT_F32_SHAPES = [(129, 13, 72), (16, 3, 32)]


def all_cases():
    """{group: [(id, make-arguments, options)]}: everything test_gemm_gpu.py runs"""
    return {"nt": nt_cases(NT_SHAPES + F32_SHAPES + [s for s in pp_bn_all() + EPI_SHAPES if s not in NT_SHAPES]),
            "wgrad": wgrad_cases(), "splitk": splitk_cases(), "tn": tn_cases(), "batched": batched_cases()}


def build(args, opt):
    ep, fam, M, N, K, idx = args[:6]
    c = make(ep, fam, M, N, K, idx, batch=args[6] if len(args) > 6 else (), **opt)
    if ep in ("wgrad", "tn"):
        c.out_f32 = True
    return c


# ------------------------------------------------------------------------------------------------ GELU
def gelu_parts64(x):
    """float64 gelu_sig with the kernel's fp32 constants -> s, polynomial derivative p = u'(x), argument u"""
    u = x * (f32(G0) + f32(G1) * x * x)
    s = 1.0 / (1.0 + torch.exp2(f32(NEG2LOG2E) * u))
    return s, f32(G0) + f32(G2) * x * x, u


def gelu64(x):
    return x * gelu_parts64(x)[0]


def gelu_grad64(x):
    """-> gelu'(x) and G(x) = s (1 + |2 x p|) (1 + 2 |u|): the magnitudes inside gelu_tanh_grad, its 1 - s taken at full
    size (the error of s passes through the cancelling 1 - s unreduced); s itself carries the relative error of its
    exponent's argument, ~ 2 |u| roundings, which matters where s is tiny"""
    s, p, u = gelu_parts64(x)
    return s + 2.0 * x * s * (1.0 - s) * p, s * (1.0 + (2.0 * x * p).abs()) * (1.0 + 2.0 * u.abs())


def model_gelu_sig(x):
    """fp32 gelu_sig; exp2 is taken in float64 and rounded once (a correctly rounded fp32 exp2), so the model does not
    depend on the host's vector math library"""
    u = x * (G0 + torch.tensor(G1, dtype=F32) * x * x)
    return 1.0 / (1.0 + torch.exp2((torch.tensor(NEG2LOG2E, dtype=F32) * u).double()).float())


def model_gelu(x):
    return x * model_gelu_sig(x)


def model_gelu_grad(x):
    s = model_gelu_sig(x)
    return s + 2.0 * x * s * (1.0 - s) * (G0 + torch.tensor(G2, dtype=F32) * x * x)


# ------------------------------------------------------------------------------------------------ reference
def acc_const(name, K):
    """the constant of a K-term sum: C, or below K = C - 3 the analytic bound of any summation order, K + 3 (the K
    products of bf16 factors are exact in fp32; K - 1 additions, alpha, bias, one more for the slab sum)"""
    return min(C[name], K + 3.0)


def _clean(c):
    a = c.a.double()
    return torch.nan_to_num(a, nan=0.0) if c.causal in (2, 3) else a


def reference(c):
    """-> {"y": Elem, "aux": Elem (GELU with aux), "rowsum": Elem (pp_wgrad with rowsum), "pre": (ref, S)}.
    With act == 2, "y" is the float64 GELU of the float64 pre-activation carrying the Lipschitz slack; a kernel that
    also returned aux is checked through ``reference_gelu_from_aux`` instead."""
    a, b = _clean(c), c.b.double()
    al = f32(c.alpha)
    pre, S = al * (a @ b), abs(al) * (a.abs() @ b.abs())
    if c.bias is not None:
        pre, S = pre + c.bias.double(), S + c.bias.double().abs()
    out = {"pre": (pre, S)}
    A = torch.zeros_like(pre)
    y, cacc = pre, acc_const("acc", c.K)
    if c.act == 1:
        y = pre.clamp_min(0.0)
    elif c.act == 2:
        out["aux"] = Elem(pre, A, S, cacc)
        y = gelu64(pre)
        A = LIP * (2.0 ** -8 * pre.abs() + cacc * U * S) + (C["gelu"] + HW) * U * pre.abs()
        S = torch.zeros_like(S)
    if c.du is not None:
        gp, G = gelu_grad64(c.du.double())
        y, S = y * gp, S * gp.abs()
        A = A + (C["dgelu"] + HW) * U * pre.abs() * G
    if c.res is not None:
        y, S = y + c.res.double(), S + c.res.double().abs()
    if c.old is not None:
        y, S = y + c.old.double(), S + c.old.double().abs()
    out["y"] = Elem(y, A, S, cacc)
    if c.rowsum_old is not None:
        r = al * a.sum(-1) + c.rowsum_old.double()
        out["rowsum"] = Elem(r, torch.zeros_like(r), abs(al) * a.abs().sum(-1) + c.rowsum_old.double().abs(),
                             acc_const("rowsum", c.K))
    return out


def reference_gelu_from_aux(c, aux):
    """y of an act == 2 call from the kernel's own bf16 aux: x is exact, only s(x), the product, res and the rounding"""
    x = aux.double()
    y, S = gelu64(x), x.abs()
    if c.res is not None:
        y, S = y + c.res.double(), S + c.res.double().abs()
    return Elem(y, HW * U * x.abs(), S, C["gelu"])


# ------------------------------------------------------------------------------------------------ checks
def _fail(what, ratio, got, ref):
    i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax().item())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    raise AssertionError(f"{what} {list(idx)}: got {got.reshape(-1)[i].item()!r}, want {ref.reshape(-1)[i].item()!r}, "
                         f"error / bound = {ratio.reshape(-1)[i].item():.3g}")


def bound_of(e, bf16):
    return e.A + e.c * U * e.S + (U + (2.0 ** -8 if bf16 else 0.0)) * e.ref.abs() + TINY


def check_elem(got, e, what, mask=None):
    """every element of ``got`` (bf16 or fp32) against an Elem (``mask``: the causal-1 triangle).  -> worst error / bound"""
    assert got.dtype in (BF, F32) and got.shape == e.ref.shape, (what, got.dtype, got.shape, e.ref.shape)
    ratio = (got.double() - e.ref).abs() / bound_of(e, got.dtype == BF)
    if mask is not None:
        ratio = torch.where(mask, ratio, torch.zeros_like(ratio))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not worst <= 1.0:
        _fail(what, ratio, got, e.ref)
    return worst


def bits(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def check_exact(got, e, what, mask=None):
    """integer family: fp32 equal to the reference bit for bit, bf16 to its round-to-nearest-even (sign of zero aside)"""
    want = e.ref.to(got.dtype)
    assert torch.equal(want.double(), e.ref) or got.dtype == BF, (what, "reference not exact in fp32")
    g, w = got + 0.0, want + 0.0
    if mask is not None:
        g, w = torch.where(mask, g, torch.zeros_like(g)), torch.where(mask, w, torch.zeros_like(w))
    if not bits_equal(g, w):
        _fail(what + " (integer family: exact)", (g.double() - w.double()).abs() * 1e30, got, e.ref)
    return 0.0


def causal1_mask(c, device):
    return (torch.arange(c.N, device=device)[None, :] <= torch.arange(c.M, device=device)[:, None]) if c.causal == 1 else None


def check(c, outs, ref=None):
    """a kernel's (or model's) outputs {"y", "aux"?, "rowsum"?} against the reference -> {name: worst error / bound}"""
    ref = ref if ref is not None else reference(c)
    one = check_exact if c.family == "integer" else check_elem
    mask = causal1_mask(c, outs["y"].device)
    r = {}
    if c.act == 2 and outs.get("aux") is not None:
        r["aux"] = check_elem(outs["aux"], ref["aux"], "aux")
        r["gelu_y"] = check_elem(outs["y"], reference_gelu_from_aux(c, outs["aux"]), "y = GELU(aux)")
    else:
        key = "gelu_y_noaux" if c.act == 2 else "dgelu_y" if c.du is not None else ("y_f32" if outs["y"].dtype == F32 else "y_bf16")
        r[key] = one(outs["y"], ref["y"], "y", mask)
    if c.causal in (2, 3):
        assert torch.isfinite(outs["y"].float()).all(), "causal reduction read the NaN outside its triangle"
    if "rowsum" in ref:
        r["rowsum"] = one(outs["rowsum"], ref["rowsum"], "rowsum")
    return r


def fp32_part(got, e):
    """worst |got - ref| / (u S) of a model output without its bf16 rounding (what MEASURED records)"""
    r = ((got.double() - e.ref).abs() - e.A - U * e.ref.abs() - TINY).clamp_min(0.0) / (U * e.S + 1e-300)
    return r.max().item() if r.numel() else 0.0


# ------------------------------------------------------------------------------------ fp32 models of the kernels
MUTATIONS = ["drop_last_slice", "k64_tail", "acc_not_cleared", "alpha_ignored", "alpha_after_bias", "bias_shift4",
             "bias_skipped_n4", "relu_skipped_f32", "res_before_act", "col_swap", "row_low", "overwrite", "split_twice",
             "split_skipped", "rowsum_no_alpha", "rowsum_per_coltile", "causal2_short", "causal3_late", "bf16_trunc"]


def split_ranges(K, splits):
    """slice ranges [k0, k1) of the ping-pong split-K: 32-deep slices, splits clamped to their count, the first
    nsl % splits one slice longer"""
    nsl = K // 32
    s = max(1, min(splits, nsl))
    base, rem = nsl // s, nsl % s
    out = []
    for z in range(s):
        k0 = z * base + min(z, rem)
        out.append((32 * k0, 32 * (k0 + base + (1 if z < rem else 0))))
    return out


def _acc(a, b, k0, k1, sl):
    """fp32 accumulation of a[.., k0:k1] @ b[.., k0:k1, :] in sl-deep slices.  A slice's own sum is formed in float64
    and rounded once (<= 64 products of bf16 factors: exact there), so the model does not depend on the summation order
    of the host's BLAS and MEASURED is the same on every machine."""
    acc = torch.zeros(*a.shape[:-1], b.shape[-1], dtype=F32, device=a.device)
    for s in range(k0, k1, sl):
        e = min(s + sl, k1)
        acc = acc + (a[..., s:e].double() @ b[..., s:e, :].double()).float()
    return acc


def trunc_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def model(c, mut=None, rnd=True, sl=None):
    """Every entry point in fp32: accumulation in ``sl``-deep slices (default: 64 for the register and glds kernels'
    K-steps, 32 for the ping-pong entry points wgrad / splitk), the split-K slab sum in split order, the epilogue
    order of the module docstring, round to nearest even.  ``mut``: one of MUTATIONS (a planted error where the case
    has the feature it breaks, else the correct result).  rnd=False keeps the result (and aux) in fp32.
    -> {"y", "aux"?, "rowsum"?}"""
    a, b = c.a.float(), c.b.float()
    M, N, K = c.M, c.N, c.K
    dev = a.device
    pp = c.ep in ("wgrad", "splitk")
    sl = sl or (32 if pp else 64)
    alpha = torch.tensor(1.0 if mut == "alpha_ignored" else c.alpha, dtype=F32, device=dev)
    Ke = K
    if mut == "k64_tail" and K > 64:
        Ke = K // 64 * 64
    if mut == "drop_last_slice" and K > 32:
        Ke = (K - 1) // 32 * 32
    if c.causal in (2, 3):                     # row tiles of 128: the reduction range is a tile's, not a row's
        acc = torch.zeros(*c.batch, M, N, dtype=F32, device=dev)
        for m0 in range(0, M, 128):
            m1 = min(m0 + 128, M)
            if c.causal == 2:
                k0, k1 = 0, min(K, (m0 + 128 + 63) // 64 * 64 - (64 if mut == "causal2_short" else 0))
            else:
                k0, k1 = m0 // 64 * 64 + (64 if mut == "causal3_late" else 0), K
            acc[..., m0:m1, :] = _acc(a[..., m0:m1, :], b, k0, max(k0, k1), sl)
        slabs = [acc]
    elif pp:
        rng = split_ranges(K, c.splits)
        if mut == "split_twice" and len(rng) > 1 and K // 32 % len(rng):
            rng = rng + [rng[-1]]
        if mut == "split_skipped" and len(rng) > 1 and K // 32 % len(rng):
            rng = rng[:-1]
        slabs = [_acc(a, b, k0, min(k1, Ke), sl) for k0, k1 in rng]
    else:
        slabs = [_acc(a, b, 0, Ke, sl)]
    if mut == "acc_not_cleared" and M > 256:   # the second row tile of a block starts from the first one's sums
        n = min(256, M - 256)
        slabs[0] = slabs[0].clone()
        slabs[0][..., 256:256 + n, :] += slabs[0][..., :n, :].clone()
    out = {}
    if c.rowsum_old is not None:
        ra = torch.tensor(1.0, dtype=F32) if mut == "rowsum_no_alpha" else alpha
        rs = c.rowsum_old.clone()
        tiles = -(-N // (c.bn or 256)) if mut == "rowsum_per_coltile" else 1
        for k0, k1 in split_ranges(K, c.splits):
            for _ in range(tiles):
                rs = rs + _acc(a, torch.ones(*c.batch, K, 1, dtype=F32, device=dev), k0, k1, sl)[..., 0] * ra
        out["rowsum"] = rs
    # ---- epilogue
    if c.ep in ("wgrad", "tn"):                # out (+)= alpha * sum of slabs, added to the old contents first
        v = torch.zeros_like(slabs[0]) if mut == "overwrite" else c.old.clone()
        for s_ in slabs:
            v = v + s_ * alpha
        out["y"] = v
        return out
    acc = slabs[0]
    for s_ in slabs[1:]:
        acc = acc + s_
    bias = None
    if c.bias is not None:
        bias = c.bias.expand(*acc.shape).clone()
        n = torch.arange(N, device=dev)
        if mut == "bias_shift4" and N % 128:   # the last ragged 128-wide column tile reads four columns on
            last = n >= (N - 1) // 128 * 128
            bias = torch.where(last, c.bias[(n + 4).clamp_max(N - 1)], c.bias).expand(*acc.shape).clone()
        if mut == "bias_skipped_n4" and c.out_f32:
            bias = torch.where(n // 4 * 4 + 4 <= N, c.bias, torch.zeros_like(c.bias)).expand(*acc.shape).clone()
    if mut == "alpha_after_bias" and bias is not None:
        v = (acc + bias) * alpha
    else:
        v = acc * alpha
        if bias is not None:
            v = v + bias
    early_res = mut == "res_before_act" and c.res is not None and c.act in (1, 2)
    if early_res:
        v = v + c.res.float()
    if c.act == 1 and not (mut == "relu_skipped_f32" and c.out_f32):
        v = v.clamp_min(0.0)
    elif c.act == 2:
        pre = v.to(BF) if rnd else v
        if c.aux:
            out["aux"] = pre
        v = model_gelu(pre.float())
    if c.du is not None:
        v = v * model_gelu_grad(c.du.float())
    if c.res is not None and not early_res:
        v = v + c.res.float()
    # ---- store
    if mut == "col_swap" and N >= 4:
        n = torch.arange(N, device=dev)
        sw = torch.where((n % 4 == 1) & (n // 4 * 4 + 4 <= N), n + 1, torch.where((n % 4 == 2) & (n // 4 * 4 + 4 <= N), n - 1, n))
        v = v[..., sw]
    if mut == "row_low" and M % 128:           # (the last row's values fall off the end: on the GPU, into the guard)
        m0 = (M - 1) // 128 * 128
        v = torch.cat([v[..., :m0, :], torch.zeros_like(v[..., :1, :]), v[..., m0:M - 1, :]], -2)
    if c.causal == 1:                          # tiles wholly above the diagonal are not written: a marker stays
        m0 = torch.arange(M, device=dev)[:, None] // 128 * 128
        n0 = torch.arange(N, device=dev)[None, :] // 64 * 64
        v = torch.where(n0 >= m0 + 128, torch.full_like(v, 7.0), v)
    if not c.out_f32 and rnd:
        v = trunc_bf16(v) if mut == "bf16_trunc" else v.to(BF)
    out["y"] = v
    return out
