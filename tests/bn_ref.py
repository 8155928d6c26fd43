"""A float64 reference of the BatchNorm kernels (csrc/kernels/batchnorm.hip), the elementwise bounds they are held to,
fp32 models of the kernels (a stand-in for a correct kernel, and the carrier of planted errors), and the seeded inputs
shared by the GPU tests (test_bn_gpu.py) and the CPU self-check (test_bn_ref_cpu.py).  Everything here runs on CPU and
GPU tensors alike.

Every ``ref_*`` function computes, in float64, from exactly what the kernel is given: activations already rounded to
bf16 and per-channel coefficients in fp32 as passed (eps and momentum as the fp32 values the C entry point receives).
So each kernel is tested on its own, not through the error of the kernel before it.

Bounds.  u = 2^-24 is the fp32 unit roundoff; bf16 keeps 8 significant bits, so its round-to-nearest is up to 2^-8
relative (half an ulp just above a power of two).

* bf16 outputs (``check_elem``): ``|got - ref| <= 2^-8 |ref| + c u S`` per element.  2^-8 |ref| is the bf16
  rounding of the result itself; S is the sum of the magnitudes of the fp32 summands that cancel in it, so a near-zero result
  of large summands, or a channel with a large coefficient, gets the slack its fp32 arithmetic needs and no more.
    y  = x*sc + sh + res*rsc + rsh: the kernel forms sh + rsh (one rounding), then two fmas (one rounding each):
         at most 3 roundings of partial sums, each bounded by S_y = |x*sc| + |sh| + |res*rsc| + |rsh|; c = C_Y = 4.
    dx = k*gm + x*A + B with the kernel's per-channel k = gamma*invstd, A = -k*invstd*dgamma/L,
         B = k*(mean*invstd*dgamma/L - dbeta/L): k carries 1 rounding, A 4, the two fmas 2, and B up to 6 roundings of
         its own two summands b1 = k*mean*invstd*dgamma/L and b2 = k*dbeta/L.  B is itself a difference formed in fp32,
         so its slack must come from |b1| + |b2|, not from |B| (which may cancel): S_dx = |k*gm| + |x*A| + |b1| + |b2|
         (>= |k*gm| + |x*A| + |B|); c = C_DX = 8.
  ReLU is monotone and 1-Lipschitz, so the same bound holds after it.
* ``gm``: bitwise, it is g or +0.  Mask bits: exactly (y > 0) of the kernel's own y.
* fp32 sums (``sum x``, ``sum x^2``, ``sum gm``, ``sum gm*xhat``): ``|got - ref| <= k u sum|terms|`` with sum|terms|
  from the float64 reference.  k is not picked in advance: ``blocked_sum32`` models the kernels' summation in fp32
  (sequential per-thread-row sums in the kernel's row order, sequential fp32 adds of a block's thread-rows, fp32 adds
  of the blocks into 64 bins in three different orders, float64 over the bins) and test_bn_ref_cpu.py measures its
  largest error / (u sum|terms|) over every input of this module.  K_SUM is 4x that measurement, because the atomics
  reorder the adds on the GPU; both numbers are below.
  The sums propagate to first order: dmean = dS/L (+ u|mean| for the fp32 store), dvar = dQ/L + 2|mean| dmean + dmean^2,
  dinvstd = 0.5 invstd dvar / (var + eps) + u invstd, scale: |gamma| dinvstd + u|scale|, shift: |scale| dmean +
  |mean gamma| dinvstd + 4u(|mean scale| + |beta|), running stats: momentum times dmean / (L/(L-1)) dvar, + u|ref|.
  dgamma / dbeta are the sums stored to fp32: + u|ref|.

Recorded by test_bn_ref_cpu.py (worst error / bound of the fp32 models over all SHAPES; the test prints them):
  summation model, error / (u sum|terms|): statistics 5.97, backward sums 2.42  ->  K_MEASURED below, K_SUM = 4x
  forward chain 0.749 (run_var), eval coeff 0.373, dgamma / dbeta 0.234, y 0.996, dx / dx2 0.996 (y and dx reach 1
  because the bf16 rounding alone reaches 2^-8 |ref|; the fp32 part c u S is what separates a model from a planted error)
The kernels on an MI355X (test_bn_gpu.py prints them): mean 0.047, invstd 0.084, scale 0.127, shift 0.082, run_mean 0.573,
  run_var 0.749, eval 0.359, dgamma 0.234, dbeta 0.169, y 0.996, dx 0.996, dx2 0.996.  No bound had to be loosened.
"""
from types import SimpleNamespace

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

U = 2.0 ** -24
EPS = 1e-5
STAT_BINS = 64
NT = 256
BN_RMIN = 32

# largest error / (u sum|terms|) of blocked_sum32 over this module's inputs, rounded up: the forward statistics
# (sum x, sum x^2; 5.97, on a far-from-zero channel whose terms all have one sign) and the backward sums (sum gm,
# sum gm*xhat; 2.42), and the bounds' k: 4x the measurement
K_MEASURED = {"stats": 6.0, "backward": 2.5}
K_SUM = {"stats": 24.0, "backward": 10.0}
C_Y = 4.0
C_DX = 8.0

# (L, C): what each reaches is listed in test_bn_gpu.py
SHAPES = [(1, 8), (2, 8), (147, 2048), (1100, 2048), (2500, 2048), (10243, 200), (3137, 24), (32845, 64),
          (131372, 8), (4096, 256)]
ALL_BRANCH_SHAPES = [(1100, 2048), (10243, 200), (1, 8)]


# ------------------------------------------------------------------------------------------ launch geometry
def rpi(C):
    """rows per block iteration: 256 threads / (C/8) channel groups"""
    return NT // (C // 8)


def idle_threads(C):
    return NT - rpi(C) * (C // 8)


def stream_grid(L, C):
    """bn_stream_grid of bn_apply / bn_bwd_apply"""
    return max(1, min(512, (L * (C // 8) + NT - 1) // NT))


def reduce_grid(L, C):
    """reduce_grid of bn_stats / bn_bwd_reduce"""
    r = rpi(C) * BN_RMIN
    return max(1, min(512, (L + r - 1) // r))


def row_iters(L, C, grid):
    """(fewest, most) rows any thread-row of a ``grid``-block launch visits"""
    T = grid * rpi(C)
    return L // T, (L + T - 1) // T


# ------------------------------------------------------------------------------------------------ inputs
def f32(v):
    """a Python float rounded to fp32, as the C entry points receive eps and momentum"""
    return torch.tensor(v, dtype=F32).item()


def gen_case(L, C):
    """Seeded inputs of one shape, on the CPU.  Channel means run from 0 to 8 sigma with alternating sign; gamma has a
    zero, a negative and a large entry; channel CONST is constant (var = 0); gy has a per-channel mean and a component
    proportional to xhat, so dbeta/L and xhat*dgamma/L are order-one parts of dx; mscale is +-{0.5, 1, 2} and mshift a
    multiple of 2^-6 (x*mscale + mshift is exact in fp32) and about 5% of x's entries (a fifth of those of the channels
    with a mean within 2 sigma) sit exactly on the zero of x*mscale + mshift."""
    g = torch.Generator().manual_seed(7000 + 31 * L + C)
    ch = torch.arange(C, dtype=F64)
    sgn = 1.0 - 2.0 * (torch.arange(C) % 2).double()
    mu = 8.0 * ch / (C - 1) * sgn
    sig = 2.0 ** torch.randint(-2, 2, (C,), generator=g).double()
    pick = torch.tensor([0.5, 1.0, 2.0, -0.5, -1.0, -2.0], dtype=F64)
    mscale = pick[torch.randint(0, 6, (C,), generator=g)]
    mshift = torch.randint(-8, 9, (C,), generator=g).double() / 64.0
    x = torch.randn(L, C, generator=g, dtype=F64) * sig + mu * sig
    plant = (torch.rand(L, C, generator=g) < 0.2) & (mu.abs() <= 2.0)      # only near-zero-mean channels: the far
    x = torch.where(plant, (-mshift / mscale).expand(L, C), x)             # ones keep their 8 sigma
    x[:, CONST] = 1.5
    x = x.to(BF)
    mean, var = stats64(x)
    xhat = (x.double() - mean) / torch.sqrt(var + EPS)
    gamma = (torch.rand(C, generator=g, dtype=F64) * 1.5 + 0.5) * sgn.roll(1)
    gamma[0], gamma[1], gamma[2] = 0.0, -1.5, 24.0
    gmean = (torch.rand(C, generator=g, dtype=F64) + 0.5) * sgn.roll(3)
    gslope = 0.75 * (1.0 - 2.0 * (torch.arange(C) % 3 == 0).double())
    gy = (torch.randn(L, C, generator=g, dtype=F64) + gmean + gslope * xhat).to(BF)
    x2 = (torch.randn(L, C, generator=g, dtype=F64) * sig.flip(0) + (mu * sig).flip(0)).to(BF)
    gamma2 = (torch.rand(C, generator=g, dtype=F64) * 1.5 + 0.5) * sgn.roll(2)
    gamma2[5] = 0.0
    c = SimpleNamespace(
        L=L, C=C, x=x, gy=gy, x2=x2,
        res=(torch.randn(L, C, generator=g, dtype=F64) * 1.5 + 0.5).to(BF),
        gamma=gamma.float(), beta=torch.randn(C, generator=g), gamma2=gamma2.float(),
        rm=torch.randn(C, generator=g) * 0.5, rv=torch.rand(C, generator=g) + 0.5,
        rscale=((torch.rand(C, generator=g, dtype=F64) * 1.5 + 0.5) * sgn.roll(5)).float(),
        rshift=torch.randn(C, generator=g), mscale=mscale.float(), mshift=mshift.float())
    return c


CONST = 3                  # the constant channel of gen_case


def case_to(c, device):
    return SimpleNamespace(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(c).items()})


def given_coeffs(c):
    """The fp32 coefficients the apply / backward kernels are handed, from the float64 statistics of c.x and c.x2
    rounded to fp32: mean, invstd, scale, shift (and the second BN's), added to the case."""
    for sfx, x, gamma, beta in (("", c.x, c.gamma, c.beta), ("2", c.x2, c.gamma2, None)):
        mean, var = stats64(x)
        inv = (1.0 / torch.sqrt(var + f32(EPS))).float()
        setattr(c, "mean" + sfx, mean.float())
        setattr(c, "invstd" + sfx, inv)
        setattr(c, "scale" + sfx, gamma * inv)
        setattr(c, "shift" + sfx, (beta if beta is not None else 0.0) - mean.float() * gamma * inv)
    return c


# --------------------------------------------------------------------------------------- float64 reference
def stats64(x):
    xd = x.double()
    mean = xd.mean(0)
    var = ((xd * xd).mean(0) - mean * mean).clamp_min(0.0)
    return mean, var


def ref_forward(x, gamma, beta, rm, rv, momentum, eps=EPS):
    """bn_stats -> bn_finalize: {name: (reference, bound)} for mean, invstd, scale, shift, run_mean, run_var (the last
    two only when rm / rv are given; they are the values BEFORE the update)."""
    L, C = x.shape
    xd = x.double()
    eps, mom = f32(eps), f32(momentum)
    S, Q = xd.sum(0), (xd * xd).sum(0)
    dS, dQ = K_SUM["stats"] * U * xd.abs().sum(0), K_SUM["stats"] * U * Q
    mean = S / L
    var = (Q / L - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    g = gamma.double() if gamma is not None else torch.ones_like(mean)
    b = beta.double() if beta is not None else torch.zeros_like(mean)
    dmean = dS / L
    dvar = dQ / L + 2.0 * mean.abs() * dmean + dmean * dmean
    dinv = 0.5 * inv * dvar / (var + eps) + U * inv
    scale = g * inv
    shift = b - mean * scale
    out = {"mean": (mean, dmean + U * mean.abs()), "invstd": (inv, dinv),
           "scale": (scale, g.abs() * dinv + U * scale.abs()),
           "shift": (shift, scale.abs() * dmean + (mean * g).abs() * dinv + 4.0 * U * ((mean * scale).abs() + b.abs()))}
    if rm is not None:
        unb = L / (L - 1.0) if L > 1 else 1.0
        r_m = (1.0 - mom) * rm.double() + mom * mean
        r_v = (1.0 - mom) * rv.double() + mom * var * unb
        out["run_mean"] = (r_m, mom * dmean + U * r_m.abs())
        out["run_var"] = (r_v, mom * unb * dvar + U * r_v.abs())
    return out


def ref_eval_coeff(eps, gamma, beta, rm, rv):
    """{name: (reference, bound)}: rsqrtf is good to a few ulp (4u), then one rounding per product / difference"""
    eps = f32(eps)
    inv = 1.0 / torch.sqrt(rv.double() + eps)
    g = gamma.double() if gamma is not None else torch.ones_like(inv)
    b = beta.double() if beta is not None else torch.zeros_like(inv)
    scale = g * inv
    shift = b - rm.double() * scale
    return {"scale": (scale, 6.0 * U * scale.abs()),
            "shift": (shift, 8.0 * U * (rm.double() * scale).abs() + 2.0 * U * (b.abs() + shift.abs()))}


def ref_apply(x, scale, shift, res=None, rscale=None, rshift=None, relu=True):
    """-> (y, S_y) in float64"""
    a = x.double() * scale.double()
    y = a + shift.double()
    S = a.abs() + shift.double().abs()
    if res is not None:
        r = res.double() * (rscale.double() if rscale is not None else 1.0)
        y = y + r
        S = S + r.abs()
        if rshift is not None:
            y = y + rshift.double()
            S = S + rshift.double().abs()
    return (y.clamp_min(0.0) if relu else y), S


def unpack_bits(bits, C):
    """uint8 [L][C/8] sign bits -> bool [L][C]"""
    sh = torch.arange(8, device=bits.device)
    return ((bits.to(torch.int32)[:, :, None] >> sh) & 1).bool().reshape(bits.shape[0], C)


def pack_bits(mask):
    """bool [L][C] -> uint8 [L][C/8], bit j of byte [row][c/8] = mask[row][c + j]"""
    L, C = mask.shape
    sh = torch.arange(8, device=mask.device)
    return (mask.view(L, C // 8, 8).to(torch.int32) << sh).sum(-1).to(torch.uint8)


def ref_mask(mode, x, msrc=None, mscale=None, mshift=None, strict=True):
    """The backward's mask per mode, or None for mode 0.  strict=False is the planted error '>= 0'."""
    if mode == 0:
        return None
    if mode == 3:
        return unpack_bits(msrc, x.shape[1])
    v = msrc.double() if mode == 1 else x.double() * mscale.double() + mshift.double()
    return v > 0 if strict else v >= 0


def ref_gm(g, mask):
    """bf16, bitwise what the kernels' gm is"""
    return g if mask is None else torch.where(mask, g, torch.zeros_like(g))


def ref_bwd_reduce(g, x, mean, invstd, mask):
    """-> {"dbeta": (sum gm, bound), "dgamma": (sum gm*xhat, bound)}, bounds for the fp32 values bn_bwd_finalize
    stores"""
    gm = ref_gm(g, mask).double()
    t = gm * (x.double() - mean.double()) * invstd.double()
    s, q = gm.sum(0), t.sum(0)
    return {"dbeta": (s, K_SUM["backward"] * U * gm.abs().sum(0) + U * s.abs()),
            "dgamma": (q, K_SUM["backward"] * U * t.abs().sum(0) + U * q.abs())}


def ref_bwd_apply(g, x, mean, invstd, gamma, dgamma, dbeta, mask):
    """-> (dx, S_dx) in float64 from the dgamma / dbeta passed in"""
    L = x.shape[0]
    gm = ref_gm(g, mask).double()
    inv = invstd.double()
    k = (gamma.double() if gamma is not None else 1.0) * inv
    dg, db = dgamma.double() / L, dbeta.double() / L
    A = -k * inv * dg
    b1, b2 = k * mean.double() * inv * dg, k * db
    xa = x.double() * A
    kg = k * gm
    return kg + xa + (b1 - b2), kg.abs() + xa.abs() + b1.abs() + b2.abs()


# ------------------------------------------------------------------------------------------------ checks
def _fail(what, ratio, got, ref, shape):
    i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax().item())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), shape))
    raise AssertionError(f"{what} {list(idx)}: got {got.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r}, "
                         f"error / bound = {ratio.flatten()[i].item():.3g}")


def check_elem(got, ref, S, c, what):
    """bf16 ``got`` against float64 ``ref`` elementwise: |got - ref| <= 2^-8 |ref| + c u S.  -> worst error / bound"""
    assert got.dtype == BF and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bound = ref.abs() * 2.0 ** -8 + c * U * S + 1e-300
    ratio = (got.double() - ref).abs() / bound
    worst = ratio.max().item()
    if not worst <= 1.0:
        _fail(what, ratio, got, ref, ref.shape)
    return worst


def check_vec(got, ref_bound, what):
    """fp32 per-channel ``got`` against (float64 reference, bound).  -> worst error / bound"""
    ref, bound = ref_bound
    assert got.dtype == F32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    ratio = (got.double() - ref).abs() / (bound + 1e-300)
    worst = ratio.max().item()
    if not worst <= 1.0:
        _fail(what, ratio, got, ref, ref.shape)
    return worst


def check_bits(bits, y):
    assert bits.dtype == torch.uint8 and bits.shape == (y.shape[0], y.shape[1] // 8)
    assert torch.equal(bits, pack_bits(y > 0)), "mask bits must be (y > 0) of the kernel's own y"


def check_gm(gm, g, mask):
    assert gm.dtype == BF and torch.equal(gm.view(torch.int16), ref_gm(g, mask).view(torch.int16)), \
        "gm must be bitwise g where the mask is set and +0 elsewhere"


# ------------------------------------------------------------------------------------ fp32 models of the kernels
def blocked_sum32(terms, C, order=0):
    """fp32 model of the kernels' per-channel sum of ``terms`` ([L][C] fp32): thread-row (block b, row slot k) sums
    rows (b*RPI + k) + i*grid*RPI for i = 0, 1, ... sequentially; a block adds its RPI thread-rows sequentially; block
    b adds into bin b % 64 (order 0: ascending blocks, 1: descending, 2: a fixed permutation); float64 over the bins."""
    L = terms.shape[0]
    R, G = rpi(C), reduce_grid(L, C)
    T = R * G
    n = (L + T - 1) // T
    t = torch.zeros(n * T, C, dtype=F32, device=terms.device)
    t[:L] = terms
    t = t.view(n, G, R, C)
    acc = torch.zeros(G, R, C, dtype=F32, device=terms.device)
    for i in range(n):
        acc += t[i]
    blk = torch.zeros(G, C, dtype=F32, device=terms.device)
    for k in range(R):
        blk += acc[:, k]
    ids = list(range(G))
    if order == 1:
        ids.reverse()
    elif order == 2:
        ids = torch.randperm(G, generator=torch.Generator().manual_seed(G)).tolist()
    bins = torch.zeros(STAT_BINS, C, dtype=F32, device=terms.device)
    for b in ids:
        bins[b % STAT_BINS] += blk[b]
    return bins.double().sum(0)


def model_forward(x, gamma, beta, rm, rv, momentum, eps=EPS, order=0, biased=False, no_eps=False):
    """bn_stats + bn_finalize: fp32 sums (blocked_sum32), then the finalize's float64 arithmetic with its fp32 stores.
    -> dict like ref_forward's, values only.  Planted errors: biased running var, eps omitted."""
    L, C = x.shape
    xf = x.float()
    s, q = blocked_sum32(xf, C, order), blocked_sum32(xf * xf, C, order)
    eps, mom = (0.0 if no_eps else f32(eps)), f32(momentum)
    mean = s / L
    var = (q / L - mean * mean).clamp_min(0.0)
    inv = (1.0 / torch.sqrt(var + eps)).float()
    g = gamma if gamma is not None else torch.ones_like(inv)
    b = beta if beta is not None else torch.zeros_like(inv)
    out = {"mean": mean.float(), "invstd": inv, "scale": g * inv, "shift": b - mean.float() * g * inv}
    if rm is not None:
        unb = var * L / (L - 1.0) if (L > 1 and not biased) else var
        out["run_mean"] = ((1.0 - mom) * rm.double() + mom * mean).float()
        out["run_var"] = ((1.0 - mom) * rv.double() + mom * unb).float()
    return out


def model_eval_coeff(eps, gamma, beta, rm, rv):
    inv = torch.rsqrt(rv + torch.tensor(eps, dtype=F32, device=rv.device))
    g = gamma if gamma is not None else torch.ones_like(inv)
    b = beta if beta is not None else torch.zeros_like(inv)
    return g * inv, b - rm * g * inv


def _row_mutate(out, mut):
    """planted store errors: the last row left unwritten (it keeps a buffer's old content, here zeros), or row L-1
    written from row L-2's data"""
    if mut == "last_row_unwritten":
        out[-1] = 0
    elif mut == "last_row_stale" and out.shape[0] > 1:
        out[-1] = out[-2]
    return out


def model_apply(x, scale, shift, res=None, rscale=None, rshift=None, relu=True, mut=None):
    """bn_apply in fp32, rounded to bf16.  -> (y, bits).  Planted errors: rshift not added, the row errors."""
    sh = shift + rshift if (rshift is not None and mut != "no_rshift") else shift
    v = x.float() * scale
    if res is not None:
        v = v + (res.float() * rscale + sh if rscale is not None else res.float() + sh)
    else:
        v = v + sh
    if relu:
        v = v.clamp_min(0.0)
    y = _row_mutate(v.to(BF), mut)
    return y, pack_bits(v > 0)


def model_bwd_reduce(g, x, mean, invstd, mask, order=0):
    """bn_bwd_reduce + bn_bwd_finalize in fp32: -> (dgamma, dbeta) as stored"""
    C = x.shape[1]
    gm = ref_gm(g, mask).float()
    q = blocked_sum32(gm * (x.float() - mean) * invstd, C, order)
    s = blocked_sum32(gm, C, order)
    return q.float(), s.float()


def model_bwd_apply(g, x, mean, invstd, gamma, dgamma, dbeta, mask, mut=None):
    """bn_bwd_apply in fp32 with the kernel's k, A, B, rounded to bf16.  Planted errors: the dbeta/L term dropped, the
    dgamma term dropped, invL off by one row, the row errors."""
    L = x.shape[0]
    invL = torch.tensor(1.0 / (L + 1 if mut == "invL" else L), dtype=F32, device=x.device)
    k = (gamma if gamma is not None else torch.ones_like(invstd)) * invstd
    dg = torch.zeros_like(dgamma) if mut == "no_dgamma" else dgamma * invL
    db = torch.zeros_like(dbeta) if mut == "no_dbeta" else dbeta * invL
    A = -k * invstd * dg
    B = k * (mean * invstd * dg - db)
    gm = ref_gm(g, mask).float()
    return _row_mutate((k * gm + (x.float() * A + B)).to(BF), mut)
