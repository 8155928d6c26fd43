"""A float64 reference of the attention and LayerNorm kernels (csrc/kernels/attention.hip, transformer.hip), the
elementwise bounds they are held to, fp32 models of the kernels (a stand-in for a correct kernel, and the carrier of
planted errors) and the seeded inputs shared by the GPU tests (test_attn_gpu.py, test_tuning_gpu.py) and the CPU
self-check (test_attn_ref_cpu.py).  Everything here runs on CPU and GPU tensors alike.

Every ``ref_*`` function computes, in float64, from exactly what the kernel is handed: qkv / x / dO already rounded to
bf16, the forward's O (bf16) and lse2 / mean / rstd (fp32) as passed to the backward, scale and eps as the fp32 values
the C entry points receive.  So each kernel is tested on its own, not through the error of the kernel before it.

Notation.  u = 2^-24 (fp32 unit roundoff); bf16 rounding is up to 2^-8 relative.  c = scale * log2(e); scores are in
log2 units c*s.  P = exp2(c*s - lse2).  Every check is per element, over every element (nothing is excluded).

bf16 outputs that are a sum over bf16-rounded factors (``check_bf16``):

    |got - ref| <= 2^-8 |ref| + 2^-8 A + C u S

  2^-8 |ref| is the rounding of the stored result.  A is the float64 sum of magnitudes of the terms whose factor the
  kernel rounds to bf16 before the second product (each term moves by up to 2^-8 of itself): sum_k P|V| for O,
  sum_q P|dO| for dV, scale sum_k |dS||K| for dQ, scale sum_q |dS||Q| for dK.  S collects the fp32 error, to first
  order:
    the exponent argument c*s - m is formed from a 64-term fp32 accumulation (error ~ u c sum_i |q_i k_i|), the fp32
    constant c (u |c s|) and one fma rounding (u |c s - m|, |m| ~ |lse2|); exp2 turns an argument error e into a
    relative error ln2 e of P, and v_exp_f32 adds about one ulp of its own.  So P carries the relative error u w,
        w[q][k] = 1 + ln2 (c sum_i |q_i||k_i| + |lse2[q]|),
    and the forward's normaliser l = sum_k p carries their P-weighted mean wbar[q] = sum_k P w.
    O:  S = sum_k P (w + wbar) |V|         (w >= 1 also covers the fp32 accumulation of the product itself)
    dV: S = sum_q P w |dO|
    dS = P (dP - delta) is a difference of two fp32 64-term sums, so its error is u times
        E = |dS| w + P (sum_i |dO_i V_ki| + sum_i |dO_i O_i|)      (the second part is what cancels behind dP - delta)
    dQ: S = scale sum_k E |K|,  dK: S = scale sum_q E |Q|.
  The softmax kernels and the unfused chain use the same form with natural-log weights (below).

fp32 outputs (``check_f32``): |got - ref| <= k u (sum of term magnitudes) + u |ref|:
    lse2:  magnitudes = sum_k P c sum_i|q_i||k_i| (the P-weighted argument errors) + |lse2| + RESC + log2 T (|m| and
           |log2 l| of m + log2 l: l <= T 2^RESC under the lazy rescale)
    lse (softmax kernel): sum_k P |s scale| + |lse| + 1
    mean:  sum|x| / D.   rstd: through the variance as in BatchNorm: dvar = k u var + dmean^2 (the kernel's variance is
           two-pass, so the mean's error enters only squared), drstd = 0.5 rstd dvar / (var + eps) + 4 u rstd (rsqrtf).
    dgamma / dbeta: sum_r |dy xhat|, sum_r |dy|; with ``acc`` the old gradient adds u (|old| + |ref|).
  LayerNorm y = xhat g + b from the kernel's own statistics: 2^-8|ref| + |g| (rstd dmean + |x - mean| drstd) + C u
  (|xhat g| + |b|).  dx = rstd (gg - s1 - xhat s2) + dres: S = rstd (|gg| + sum|gg|/D + |xhat| sum|gg xhat|/D) + |dres|.

Exact by construction, asserted bitwise: causal row 0 has O[0] = V[0]; a query row whose dO is all zero has dQ = 0;
dS above the diagonal is 0; masked P is 0.

The constants.  None is picked in advance: the fp32 models below (flash: 64-key tiles, online softmax with the lazy
rescale past RESC = 8 decided per 16-query fragment, P and dS rounded to bf16 before the second product, fp32
accumulation) run with the bf16 roundings switched off, and test_attn_ref_cpu.py measures their worst
error / (u S) over every family and shape of this module.  Each constant is 4x that measurement rounded up (the GPU sums
in another order and v_exp_f32 / v_log_f32 / rsqrtf are a few ulp): MEASURED and C below; the CPU test asserts both.

Measured fp32 parts (MEASURED, worst error / (u S) of the models without bf16 roundings, rounded up): O 3.2, lse2 5.1,
dV 6.7, dQ 6.4, dK 6.1; softmax kernels P 0.6, lse 0.4, dS 5.7; unfused chain y 0.4, dV 0.4, dQ 0.2, dK 0.2;
LayerNorm mean 0.5, variance 6.3, y 3.6, dx 3.6, column sums 3.3.

Recorded worst error / bound (bf16 roundings on; both test files print them; the bf16 outputs reach ~1 because the
rounding of the result alone reaches 2^-8 |ref|, and model and kernel then share the worst element):
  fp32 models (test_attn_ref_cpu.py): O 0.896, lse2 0.263, dQ 0.848, dK 0.848, dV 0.927; softmax P 0.995, lse 0.465,
    dS 0.996; chain y 0.805, dV 0.781, dQ 0.472, dK 0.535; LayerNorm y 0.996, mean 0.477, rstd 0.232, dx 0.996,
    dgamma 0.464, dbeta 0.470
  kernels on an MI355X (test_attn_gpu.py, all eight backward variants): O 0.896, lse2 0.133, dQ 0.848, dK 0.848,
    dV 0.927; softmax P 0.995, lse 0.753, dS 0.996; chain y 0.805, dV 0.781, dQ 0.472, dK 0.535; LayerNorm y 0.996,
    mean 0.443, rstd 0.298, dx 0.996, dgamma 0.464, dbeta 0.470.  No bound had to be loosened and no kernel changed.
Every bound also carries the absolute floor TINY for fp32 underflow (see below).
"""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

U = 2.0 ** -24
HD = 64
RESC = 8.0
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
EPS = 1e-5
# underflow: a term below the fp32 normal range (2^-126) may be flushed to zero, and a sum here has at most 2^11 terms
# (T = 1028 keys, D = 2048 channels), so every bound carries this absolute floor
TINY = 2.0 ** -115

# worst error / (u S) of the fp32 models with the bf16 roundings off (test_attn_ref_cpu.py asserts <=), and 4x that
MEASURED = {"O": 3.2, "lse2": 5.1, "dV": 6.7, "dQ": 6.4, "dK": 6.1, "sm_P": 0.6, "sm_lse": 0.4, "sm_dS": 5.7,
            "ch_y": 0.4, "ch_dV": 0.4, "ch_dQ": 0.2, "ch_dK": 0.2,
            "ln_mean": 0.5, "ln_var": 6.3, "ln_y": 3.6, "ln_dx": 3.6, "ln_sum": 3.3}
C = {k: 4.0 * v for k, v in MEASURED.items()}

Elem = namedtuple("Elem", "ref A S")          # bf16 output: float64 reference, bf16-factor magnitude, fp32 magnitude
Vec = namedtuple("Vec", "ref bound")          # fp32 output: float64 reference, absolute bound

FAMILIES = ["gauss", "next_key", "self_key", "growing", "shrinking", "far_masked", "flat"]
FLASH_SHAPES = [(1, 128, 1), (1, 256, 3), (3, 128, 2), (2, 384, 1), (1, 640, 2), (1, 1024, 2)]
CROSS_SHAPES = [(1, 128, 1), (1, 256, 3), (1, 640, 2)]            # the full backward-variant cross runs on these
SOFTMAX_T = [4, 12, 252, 256, 260, 1028]
CHAIN_SHAPES = [(1, 8, 1, 8), (2, 72, 3, 32), (1, 200, 2, 64), (1, 264, 1, 64)]
LN_D = [8, 504, 512, 520, 1024, 1032, 2048]
LN_R = [1, 3, 16, 17, 33, 8209]


def ln_cases():
    """every D at every small R; the 8209-row case (clamp to 512 blocks, ragged last stride) at one D per template"""
    return [(R, D) for D in LN_D for R in LN_R if R < 8209 or D in (8, 520, 2048)]


def f32(v):
    """a Python float rounded to fp32, as the C entry points receive scale and eps"""
    return torch.tensor(v, dtype=F32).item()


# ------------------------------------------------------------------------------------------------ layout
def split_heads(qkv, B, T, H, d=HD):
    """packed [B*T][3*H*d] -> q, k, v views [B][H][T][d]"""
    x = qkv.view(B, T, 3, H, d).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def heads(o, B, T, H, d=HD):
    """[B*T][H*d] -> [B][H][T][d]"""
    return o.view(B, T, H, d).permute(0, 2, 1, 3)


def merge(o):
    """[B][H][T][d] -> [B*T][H*d]"""
    B, H, T, d = o.shape
    return o.permute(0, 2, 1, 3).reshape(B * T, H * d)


def pack(q, k, v):
    """three [B][H][T][d] -> [B*T][3*H*d]"""
    B, H, T, d = q.shape
    return torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * d)


def above_diag(T, device, shift=0, ge=False):
    """bool [T(query)][T(key)]: key > query + shift (ge: >=)"""
    i = torch.arange(T, device=device)
    return (i[None, :] >= i[:, None] + shift) if ge else (i[None, :] > i[:, None] + shift)


# ------------------------------------------------------------------------------------------------ inputs
def _dim01(level_log2, c):
    """(ka, kb) bf16 with 16 ka + kb = level / c up to 2^-6: a key whose dims 0, 1 are (ka, kb) scores ``level`` (log2
    units) against a query whose dims 0, 1 are (16, 1)"""
    raw = level_log2 / c
    ka = torch.round(raw / 16.0).to(BF).double()
    kb = (raw - 16.0 * ka).to(BF).double()
    return ka, kb


def growing_levels(n):
    """tile levels in log2 units: +7.5 (under RESC: the maximum stays stale), +8.5 (16 over the stale maximum: moves),
    +13 (moves), repeated"""
    inc = [7.5, 8.5, 13.0]
    lv = [0.0]
    for j in range(1, n):
        lv.append(lv[-1] + inc[(j - 1) % 3])
    return torch.tensor(lv, dtype=F64)


def gen_flash(family, B, T, H, scale=0.125):
    """Seeded qkv [B*T][3*H*64] and dO [B*T][H*64], bf16, on the CPU.  Families (scores in log2 units c*s):
    gauss: unit Gaussian.  next_key / self_key: key t+1 / key t scores >= 12 above every other key of query t.
    growing / shrinking / far_masked: every query's score profile over the keys is a staircase (dims 0, 1 carry it):
    growing_levels per 64-key tile; 0 in tile 0 and <= -160 after it; +2.2 per key (a masked key 64 ahead is > 130
    above the row's lse2).  flat: Gaussian with every 7th q row and every 5th dO row all zero."""
    g = torch.Generator().manual_seed(9000 + 97 * FAMILIES.index(family) + 13 * B + T + 7 * H)
    c = f32(scale) * LOG2E
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)        # noqa: E731
    q, k, v = rn(B, H, T, HD), rn(B, H, T, HD), rn(B, H, T, HD)
    dO = rn(B, H, T, HD)
    if family in ("next_key", "self_key"):
        E = torch.randint(0, 2, (B, H, T, HD), generator=g).double() * 2.0 - 1.0
        k = 2.5 * E + 0.25 * k
        q = 2.5 * (E.roll(-1, 2) if family == "next_key" else E) + 0.25 * q
    elif family in ("growing", "shrinking", "far_masked"):
        t = torch.arange(T, dtype=F64)
        if family == "growing":
            lv = growing_levels(T // 64 + 1)[(t // 64).long()]
        elif family == "shrinking":
            lv = torch.where(t < 64, torch.zeros_like(t), -160.0 - 5.0 * (t // 64))
        else:
            lv = 2.2 * t
        ka, kb = _dim01(lv, c)
        q, k = 0.125 * q, 0.125 * k
        q[..., 0], q[..., 1] = 16.0, 1.0
        k[..., 0], k[..., 1] = ka, kb
    elif family == "flat":
        t = torch.arange(T)
        q[:, :, t % 7 == 3] = 0.0
        dO[:, :, t % 5 == 1] = 0.0
    return pack(q, k, v).to(BF).contiguous(), merge(dO).to(BF).contiguous()


def gen_softmax(T, causal):
    """S fp32 [rows][T] (row r is query r % T), dP fp32 with NaN above the diagonal when causal; rows = 2T + 3 (T + 3
    at T = 1028): not a multiple of 4.  Rows alternate a unit-logit Gaussian, a sharply peaked and a constant row."""
    rows = (2 * T if T < 1000 else T) + 3
    g = torch.Generator().manual_seed(4000 + 2 * T + int(causal))
    S = torch.randn(rows, T, generator=g, dtype=F64) * 8.0
    r = torch.arange(rows)
    S[r % 3 == 1] *= 12.0
    S[r % 3 == 2] = 40.0
    S[:, -1] += 64.0                                  # the last key, in the 256-stride tail, dominates a full row
    dP = torch.randn(rows, T, generator=g, dtype=F64) * 2.0 + 0.5
    S, dP = S.float(), dP.float()
    if causal:
        nan = above_diag(T, S.device)[r % T]
        S = torch.where(nan, torch.full_like(S, float("nan")), S)      # never written by the causal GEMMs
        dP = torch.where(nan, torch.full_like(dP, float("nan")), dP)
    return S.contiguous(), dP.contiguous()


def gen_chain(B, T, H, d):
    g = torch.Generator().manual_seed(5000 + 11 * T + d + B)
    qkv = torch.randn(B * T, 3 * H * d, generator=g, dtype=F64)
    qkv[:, :2 * H * d] *= 1.5
    return qkv.to(BF).contiguous(), torch.randn(B * T, H * d, generator=g, dtype=F64).to(BF).contiguous()


def gen_ln(R, D):
    """Rows cycle through: unit Gaussian; mean 100 sigma; constant 1.5 (variance 0); Gaussian scaled 2^-3; Gaussian
    with mean -3.  gamma has a zero, a negative and a large (24) entry.  Existing gradients for ``acc`` are non-zero."""
    g = torch.Generator().manual_seed(6000 + 31 * R + D)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)        # noqa: E731
    kind = torch.arange(R) % 5
    x = rn(R, D)
    x[kind == 1] += 100.0
    x[kind == 2] = 1.5
    x[kind == 3] *= 0.125
    x[kind == 4] -= 3.0
    sgn = 1.0 - 2.0 * (torch.arange(D) % 2).double()
    gamma = (torch.rand(D, generator=g, dtype=F64) * 1.5 + 0.5) * sgn
    gamma[0], gamma[1], gamma[2] = 0.0, -1.5, 24.0
    xb = x.to(BF)
    mean = xb.double().mean(1, keepdim=True)
    xh = (xb.double() - mean) / torch.sqrt(xb.double().var(1, unbiased=False, keepdim=True) + EPS)
    dy = rn(R, D) + 0.5 + 0.75 * xh                                # mean(gg) and mean(gg xhat) are order one
    return SimpleNamespace(R=R, D=D, x=xb.contiguous(), gamma=gamma.float(), beta=rn(D).float(), dy=dy.to(BF).contiguous(),
                           dres=(rn(R, D) * 1.5).to(BF).contiguous(), old_dg=rn(D).float() * 3.0, old_db=rn(D).float() * 3.0)


def case_to(c, device):
    return SimpleNamespace(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(c).items()})


# --------------------------------------------------------------------------------------- float64 reference: flash
def _flash64(qkv, B, T, H, scale, causal):
    q, k, v = (t.double() for t in split_heads(qkv, B, T, H))
    c = f32(scale) * LOG2E
    s2 = c * (q @ k.transpose(-1, -2))
    aqk = c * (q.abs() @ k.abs().transpose(-1, -2))
    mask = above_diag(T, qkv.device) if causal else None
    return q, k, v, s2, aqk, mask


def ref_flash_fwd(qkv, B, T, H, scale, causal):
    """-> O: Elem over [B*T][H*64], lse2: Vec over [B][H][T] (base 2, scaled-score domain)"""
    q, k, v, s2, aqk, mask = _flash64(qkv, B, T, H, scale, causal)
    if causal:
        s2 = s2.masked_fill(mask, float("-inf"))
    m = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - m)
    lse2 = (m + torch.log2(e.sum(-1, keepdim=True)))
    P = torch.exp2(s2 - lse2)
    w = 1.0 + LN2 * (aqk + lse2.abs())
    wbar = (P * w).sum(-1, keepdim=True)
    O = Elem(merge(P @ v), merge(P @ v.abs()), merge((P * (w + wbar)) @ v.abs()))
    mag = (P * aqk).sum(-1) + lse2.squeeze(-1).abs() + RESC + math.log2(T)
    return O, Vec(lse2.squeeze(-1), C["lse2"] * U * mag + U * lse2.squeeze(-1).abs())


def ref_flash_bwd(qkv, O_given, dO, lse2_given, B, T, H, scale, causal):
    """-> {"dQ" | "dK" | "dV": Elem over [B][H][T][64]}; dqkv_parts() splits a kernel's packed dqkv the same way"""
    q, k, v, s2, aqk, mask = _flash64(qkv, B, T, H, scale, causal)
    sc = f32(scale)
    l2 = lse2_given.double().unsqueeze(-1)
    P = torch.exp2(s2 - l2)
    if causal:
        P = P.masked_fill(mask, 0.0)
    w = 1.0 + LN2 * (aqk + l2.abs())
    o, do = heads(O_given, B, T, H).double(), heads(dO, B, T, H).double()
    delta = (do * o).sum(-1, keepdim=True)
    adelta = (do * o).abs().sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    adP = do.abs() @ v.abs().transpose(-1, -2)
    dS = P * (dP - delta)
    E = dS.abs() * w + P * (adP + adelta)
    Pt, dSt, Et = P.transpose(-1, -2), dS.transpose(-1, -2), E.transpose(-1, -2)
    return {"dV": Elem(Pt @ do, Pt @ do.abs(), (P * w).transpose(-1, -2) @ do.abs()),
            "dQ": Elem(sc * (dS @ k), sc * (dS.abs() @ k.abs()), sc * (E @ k.abs())),
            "dK": Elem(sc * (dSt @ q), sc * (dSt.abs() @ q.abs()), sc * (Et @ q.abs()))}


def dqkv_parts(dqkv, B, T, H, d=HD):
    q, k, v = split_heads(dqkv, B, T, H, d)
    return {"dQ": q, "dK": k, "dV": v}


# ----------------------------------------------------------------------------- float64 reference: softmax kernels
def _row_mask(rows, T, causal, device, shift=0):
    if not causal:
        return None
    return above_diag(T, device, shift)[torch.arange(rows, device=device) % T]


def ref_softmax_fwd(S, scale, causal, mask_shift=0):
    """S fp32 [rows][T] -> P: Elem, lse: Vec (natural log).  Weights as for flash with natural-log arguments: the
    kernel forms a*scale (u |a scale|), subtracts m (u |a scale - m|), and __expf multiplies by log2(e) first."""
    rows, T = S.shape
    x = S.double() * f32(scale)
    mask = _row_mask(rows, T, causal, S.device, mask_shift)
    if causal:
        x = x.masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(x, -1, keepdim=True)
    P = torch.exp(x - lse)
    ax = torch.where(P > 0, x.abs(), torch.zeros_like(x)) if causal else x.abs()
    w = 1.0 + ax + lse.abs()
    wbar = (P * w).sum(-1, keepdim=True)
    mag = (P * ax).sum(-1) + lse.squeeze(-1).abs() + 1.0
    return Elem(P, torch.zeros_like(P), P * (w + wbar)), Vec(lse.squeeze(-1), C["sm_lse"] * U * mag + U * lse.squeeze(-1).abs())


def ref_softmax_bwd(P, dP, scale, causal):
    """P bf16, dP fp32 (NaN allowed where masked) -> dS: Elem; exactly 0 above the diagonal"""
    rows, T = P.shape
    mask = _row_mask(rows, T, causal, P.device)
    p, g = P.double(), dP.double()
    if causal:
        p, g = p.masked_fill(mask, 0.0), g.masked_fill(mask, 0.0)
    sc = f32(scale)
    delta = (p * g).sum(-1, keepdim=True)
    adelta = (p * g).abs().sum(-1, keepdim=True)
    return Elem(sc * p * (g - delta), torch.zeros_like(p), sc * p * (g.abs() + adelta))


# ------------------------------------------------------------------------------- float64 reference: unfused chain
def ref_chain(qkv, dO, B, T, H, d, causal):
    """attention_fwd / attention_bwd end to end: y = softmax(scale Q K^T) V and its gradients, float64 from qkv and dO.
    The chain rounds P to bf16 once and uses that P for y, dV, delta and dS, then rounds dS: with
    adel = sum_k P |dP| the bf16 magnitudes are A_y = sum P|V|, A_dV = sum P|dO|, and for dQ / dK
    scale sum (2 |dS| + P adel) |K| (P's rounding moves dS by 2^-8 |dS| directly and by 2^-8 P adel through delta, and
    dS is rounded again).  The fp32 parts are those of the flash kernels with natural-log weights."""
    q, k, v = (t.double() for t in split_heads(qkv, B, T, H, d))
    sc = f32(1.0 / math.sqrt(d))
    x = sc * (q @ k.transpose(-1, -2))
    ax = sc * (q.abs() @ k.abs().transpose(-1, -2))
    if causal:
        x = x.masked_fill(above_diag(T, qkv.device), float("-inf"))
    lse = torch.logsumexp(x, -1, keepdim=True)
    P = torch.exp(x - lse)
    w = 1.0 + ax + lse.abs()
    wbar = (P * w).sum(-1, keepdim=True)
    W = P * (w + wbar)
    do = heads(dO, B, T, H, d).double()
    dP = do @ v.transpose(-1, -2)
    adP = do.abs() @ v.abs().transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    adel = (P * dP.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    A = 2.0 * dS.abs() + P * adel
    E = W * (dP - delta).abs() + P * (adP + (W * dP.abs()).sum(-1, keepdim=True) + adel)
    tr = lambda t: t.transpose(-1, -2)                               # noqa: E731
    return {"y": Elem(P @ v, P @ v.abs(), W @ v.abs()),
            "dV": Elem(tr(P) @ do, tr(P) @ do.abs(), tr(W) @ do.abs()),
            "dQ": Elem(sc * (dS @ k), sc * (A @ k.abs()), sc * (E @ k.abs())),
            "dK": Elem(sc * (tr(dS) @ q), sc * (tr(A) @ q.abs()), sc * (tr(E) @ q.abs()))}


# ----------------------------------------------------------------------------------- float64 reference: LayerNorm
def ref_layernorm_fwd(x, g, b, eps=EPS):
    """-> y: (ref, bound) with the statistics' propagated error in the bound, mean: Vec, rstd: Vec"""
    R, D = x.shape
    xd, gd, bd = x.double(), g.double(), b.double()
    eps = f32(eps)
    mean = xd.mean(1, keepdim=True)
    dmean = C["ln_mean"] * U * xd.abs().mean(1, keepdim=True) + U * mean.abs()
    dev = xd - mean
    var = (dev * dev).mean(1, keepdim=True)
    dvar = C["ln_var"] * U * var + dmean * dmean
    rstd = 1.0 / torch.sqrt(var + eps)
    drstd = 0.5 * rstd * dvar / (var + eps) + 4.0 * U * rstd
    y = dev * rstd * gd + bd
    ybound = (y.abs() * 2.0 ** -8 + gd.abs() * (rstd * dmean + dev.abs() * drstd)
              + C["ln_y"] * U * ((dev * rstd * gd).abs() + bd.abs()))
    return (y, ybound), Vec(mean.squeeze(1), dmean.squeeze(1)), Vec(rstd.squeeze(1), drstd.squeeze(1))


def ref_layernorm_bwd(dy, x, g, mean_given, rstd_given, dres=None, old=None):
    """-> dx: Elem (A = 0), dgamma: Vec, dbeta: Vec; ``old`` = (dgamma, dbeta) already in the accumulators"""
    R, D = x.shape
    rs = rstd_given.double().unsqueeze(1)
    xh = (x.double() - mean_given.double().unsqueeze(1)) * rs
    dyd = dy.double()
    gg = dyd * g.double()
    s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    a1, a2 = gg.abs().mean(1, keepdim=True), (gg * xh).abs().mean(1, keepdim=True)
    dx = rs * (gg - s1 - xh * s2)
    S = rs * (gg.abs() + a1 + xh.abs() * a2)
    if dres is not None:
        dx, S = dx + dres.double(), S + dres.double().abs()
    out = {"dx": Elem(dx, torch.zeros_like(dx), S)}
    for name, t, o in (("dgamma", dyd * xh, old[0] if old else None), ("dbeta", dyd, old[1] if old else None)):
        ref = t.sum(0)
        bound = C["ln_sum"] * U * t.abs().sum(0)
        if o is not None:
            bound = bound + U * o.double().abs()
            ref = ref + o.double()
        out[name] = Vec(ref, bound + U * ref.abs())
    return out


# ------------------------------------------------------------------------------------------------ checks
def _fail(what, ratio, got, ref):
    i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax().item())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    raise AssertionError(f"{what} {list(idx)}: got {got.reshape(-1)[i].item()!r}, want {ref.reshape(-1)[i].item()!r}, "
                         f"error / bound = {ratio.reshape(-1)[i].item():.3g}")


def _ratio(got, ref, bound, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = (got.double() - ref).abs() / (bound + TINY)
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not worst <= 1.0:
        _fail(what, ratio, got, ref)
    return worst


def check_bf16(got, e, c, what):
    """bf16 ``got`` against an Elem, every element: |got - ref| <= 2^-8 |ref| + 2^-8 A + c u S.  -> worst error / bound"""
    assert got.dtype == BF, (what, got.dtype)
    return _ratio(got, e.ref, (e.ref.abs() + e.A) * 2.0 ** -8 + c * U * e.S, what)


def check_f32(got, v, what):
    assert got.dtype == F32, (what, got.dtype)
    return _ratio(got, v.ref, v.bound, what)


def check_bound(got, ref_bound, what, dtype=BF):
    assert got.dtype == dtype, (what, got.dtype)
    return _ratio(got, ref_bound[0], ref_bound[1], what)


def fp32_part(got, e):
    """worst |got - ref| / (u S) of a model run without bf16 roundings (what MEASURED records)"""
    r = ((got.double() - e.ref).abs() - TINY).clamp_min(0.0) / (U * e.S + 1e-300)
    return r.max().item()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8).reshape(-1),
                                                                     b.contiguous().view(torch.uint8).reshape(-1))


def check_flash_fwd(qkv, O, lse2, B, T, H, scale, causal, ref=None):
    """a kernel's (or model's) forward against the reference (``ref``: ref_flash_fwd's result, if already computed)
    -> {"O": ratio, "lse2": ratio}"""
    eO, vl = ref if ref is not None else ref_flash_fwd(qkv, B, T, H, scale, causal)
    out = {"O": check_bf16(O, eO, C["O"], "O"), "lse2": check_f32(lse2, vl, "lse2")}
    if causal:
        v0 = split_heads(qkv, B, T, H)[2][:, :, 0]
        assert torch.equal(heads(O, B, T, H)[:, :, 0], v0), "causal row 0: O[0] must be V[0] bitwise"
    return out


def check_flash_bwd(qkv, O_given, dO, lse2_given, dqkv, B, T, H, scale, causal, ref=None):
    if ref is None:
        ref = ref_flash_bwd(qkv, O_given, dO, lse2_given, B, T, H, scale, causal)
    got = dqkv_parts(dqkv, B, T, H)
    out = {n: check_bf16(got[n], ref[n], C[n], n) for n in ("dQ", "dK", "dV")}
    zero = (heads(dO, B, T, H) == 0).all(-1)                         # [B][H][T]: all-zero dO rows
    assert (got["dQ"][zero] == 0).all(), "a query row with dO = 0 must have dQ = 0 exactly"
    return out


def forward_given(qkv, B, T, H, scale, causal):
    """the float64 forward rounded as the backward receives it: O bf16 [B*T][H*64], lse2 fp32 [B][H][T]"""
    eO, vl = ref_flash_fwd(qkv, B, T, H, scale, causal)
    return eO.ref.to(BF).contiguous(), vl.ref.float().contiguous()


# ------------------------------------------------------------------------------------ fp32 models of the kernels
def _rb(t, rnd):
    return t.to(BF).float() if rnd else t


def model_flash_fwd(qkv, B, T, H, scale, causal, mut=None, rnd=True):
    """attn_fwd_kernel in fp32: 64-key tiles, a wave's 32 queries skip tiles wholly above their diagonal, the running
    maximum moves only when some query of a 16-query fragment exceeds it by more than RESC, P rounded to bf16 before
    P V.  rnd=False keeps P and O in fp32.  -> O ([B*T][D] bf16 or fp32), lse2 fp32.  Planted errors (``mut``):
    mask_ge, mask_shift, frag_unmasked, no_alpha_o, no_alpha_l, lse_base_e, stale_tile."""
    dev = qkv.device
    q, k, v = (t.float() for t in split_heads(qkv, B, T, H))
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    rows = torch.arange(T, device=dev)
    wave0 = rows // 32 * 32
    stale_rows = ((rows % 128) // 32 == 1)[:, None]
    m = torch.full((B, H, T), float("-inf"), dtype=F32, device=dev)
    l = torch.zeros(B, H, T, dtype=F32, device=dev)
    o = torch.zeros(B, H, T, HD, dtype=F32, device=dev)
    for kb in range(T // 64):
        k0 = kb * 64
        live = (k0 <= wave0) if causal else torch.ones(T, dtype=torch.bool, device=dev)
        if not live.any():
            break
        kt, vt = k[:, :, k0:k0 + 64], v[:, :, k0:k0 + 64]
        s = q @ kt.transpose(-1, -2)
        if mut == "stale_tile" and kb >= 1:
            s = torch.where(stale_rows, q @ k[:, :, k0 - 64:k0].transpose(-1, -2), s)
        keys = k0 + torch.arange(64, device=dev)
        if causal:
            if mut == "mask_ge":
                masked = keys[None, :] >= rows[:, None]
            elif mut == "mask_shift":
                masked = keys[None, :] > rows[:, None] + 1
            else:
                masked = keys[None, :] > rows[:, None]
            if mut == "frag_unmasked":
                masked = masked & ~((k0 + 63 > wave0)[:, None] & (keys >= k0 + 48)[None, :] & (rows[:, None] >= k0))
            s = s.masked_fill(masked, float("-inf"))
        mt = s.max(-1).values * c
        gt = (mt > m + RESC) & live
        moved = gt.view(B, H, T // 16, 16).any(-1, keepdim=True).expand(B, H, T // 16, 16).reshape(B, H, T) & live
        mn = torch.where(moved, torch.maximum(m, mt), m)
        alpha = torch.where(moved, torch.exp2(m - mn), torch.ones_like(m))
        p = torch.exp2((s.double() * c - mn.double().unsqueeze(-1)).float())
        pv = _rb(p, rnd) @ vt
        if mut == "stale_tile" and kb >= 1:
            pv = torch.where(stale_rows, _rb(p, rnd) @ v[:, :, k0 - 64:k0], pv)
        al = torch.ones_like(alpha) if mut == "no_alpha_l" else alpha
        ao = torch.ones_like(alpha) if mut == "no_alpha_o" else alpha
        l = torch.where(live, l * al + p.sum(-1), l)
        o = torch.where(live[:, None], o * ao.unsqueeze(-1) + pv, o)
        m = torch.where(live, mn, m)
    O = merge(o * (1.0 / l).unsqueeze(-1))
    lse2 = m + torch.log2(l)
    if mut == "lse_base_e":
        lse2 = lse2 * LN2
    return (O.to(BF) if rnd else O), lse2


def model_flash_bwd(qkv, O_given, dO, lse2_given, B, T, H, scale, causal, mut=None, rnd=True):
    """the backward kernels in fp32: P recomputed from lse2 (exp2 may overflow to inf above the diagonal before the mask
    zeroes it), delta from dO . O, P and dS rounded to bf16 before the second products.  -> packed dqkv.  Planted
    errors: mask_ge, mask_shift, frag_unmasked, delta_neighbour, dk_no_scale."""
    dev = qkv.device
    q, k, v = (t.float() for t in split_heads(qkv, B, T, H))
    o, do = heads(O_given, B, T, H).float(), heads(dO, B, T, H).float()
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    sc = f32(scale)
    s = q @ k.transpose(-1, -2)
    p = torch.exp2((s.double() * c - lse2_given.double().unsqueeze(-1)).float())
    if causal:
        masked = above_diag(T, dev, shift=1 if mut == "mask_shift" else 0, ge=mut == "mask_ge")
        if mut == "frag_unmasked":
            i = torch.arange(T, device=dev)
            masked = masked & ~((i[None, :] % 64 >= 48) & (i[None, :] // 64 == i[:, None] // 64))
        p = torch.where(masked, torch.zeros_like(p), p)
    delta = (do * o).sum(-1, keepdim=True)
    if mut == "delta_neighbour":
        delta = delta.roll(1, 2)
    ds = p * (do @ v.transpose(-1, -2) - delta)
    pb, dsb = _rb(p, rnd), _rb(ds, rnd)
    dv = pb.transpose(-1, -2) @ do
    dq = (dsb @ k) * sc
    dk = (dsb.transpose(-1, -2) @ q) * (1.0 if mut == "dk_no_scale" else sc)
    out = pack(dq, dk, dv)
    return out.to(BF) if rnd else out


def model_softmax_fwd(S, scale, causal, mut=None, rnd=True):
    """attn_softmax_fwd_kernel in fp32.  Planted errors: lim_off_by_one (one more key visible), tail_skipped (the keys
    past the last whole stride of 256 are left out)"""
    rows, T = S.shape
    r = torch.arange(rows, device=S.device)
    lim = (r % T + 1) if causal else torch.full_like(r, T)
    if mut == "lim_off_by_one":
        lim = (lim + 1).clamp_max(T)
    kk = torch.arange(T, device=S.device)
    vis = kk[None, :] < lim[:, None]
    if mut == "tail_skipped" and T > 256:
        vis = vis & (kk < T // 256 * 256)[None, :]
    sc = torch.tensor(scale, dtype=F32, device=S.device)
    x = torch.where(vis, S * sc, torch.full_like(S, float("-inf")))
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    tot = e.sum(-1, keepdim=True)
    P = e * (1.0 / tot)
    return (P.to(BF) if rnd else P), (m + torch.log(tot)).squeeze(-1)


def model_softmax_bwd(P, dP, scale, causal, rnd=True):
    rows, T = P.shape
    mask = _row_mask(rows, T, causal, P.device)
    p, g = P.float(), dP
    if causal:
        p, g = p.masked_fill(mask, 0.0), g.masked_fill(mask, 0.0)
    d = (p * g).sum(-1, keepdim=True)
    dS = torch.tensor(scale, dtype=F32, device=P.device) * p * (g - d)
    return dS.to(BF) if rnd else dS


def model_chain(qkv, dO, B, T, H, d, causal, rnd=True):
    """attention_fwd + attention_bwd in fp32 with the chain's bf16 roundings -> {"y", "dQ", "dK", "dV"} [B][H][T][d]"""
    q, k, v = (t.float() for t in split_heads(qkv, B, T, H, d))
    sc = 1.0 / math.sqrt(d)
    S = (q @ k.transpose(-1, -2)).reshape(B * H * T, T)
    P, _ = model_softmax_fwd(S, sc, causal, rnd=rnd)
    Pf = P.float().view(B, H, T, T)
    do = heads(dO, B, T, H, d).float()
    dP = (do @ v.transpose(-1, -2)).reshape(B * H * T, T)
    dS = model_softmax_bwd(P, dP, sc, causal, rnd=rnd).float().view(B, H, T, T)
    out = {"y": Pf @ v, "dV": Pf.transpose(-1, -2) @ do, "dQ": dS @ k, "dK": dS.transpose(-1, -2) @ q}
    return {n: (t.to(BF) if rnd else t) for n, t in out.items()}


def ln_blocks(R):
    return max(1, min(512, R // 16))


def ln_sum32(terms, order=0):
    """fp32 model of layernorm_bwd's column sums: wave (block b, w) adds rows 4b + w + i * 4 * blocks sequentially, a
    block adds its 4 waves, block b adds into bin b % 64 (order 0 ascending, 1 descending), float64 over the bins"""
    R, D = terms.shape
    nb = ln_blocks(R)
    st = 4 * nb
    n = (R + st - 1) // st
    t = torch.zeros(n * st, D, dtype=F32, device=terms.device)
    t[:R] = terms
    t = t.view(n, nb, 4, D)
    acc = torch.zeros(nb, 4, D, dtype=F32, device=terms.device)
    for i in range(n):
        acc += t[i]
    blk = torch.zeros(nb, D, dtype=F32, device=terms.device)
    for w in range(4):
        blk += acc[:, w]
    bins = torch.zeros(64, D, dtype=F32, device=terms.device)
    for b in (range(nb) if order == 0 else reversed(range(nb))):
        bins[b % 64] += blk[b]
    return bins.double().sum(0)


def model_layernorm_fwd(x, g, b, eps=EPS, mut=None, rnd=True):
    """layernorm_fwd_kernel in fp32 (two-pass variance).  Planted error: unbiased (divides by D - 1)"""
    R, D = x.shape
    xf = x.float()
    mu = xf.sum(1, keepdim=True) / D
    dev = xf - mu
    var = (dev * dev).sum(1, keepdim=True) / ((D - 1) if mut == "unbiased" else D)
    rs = torch.rsqrt(var + torch.tensor(eps, dtype=F32, device=x.device))
    y = dev * rs * g + b
    return (y.to(BF) if rnd else y), mu.squeeze(1), rs.squeeze(1), var.squeeze(1)


def model_layernorm_bwd(dy, x, g, mean, rstd, dres=None, old=None, mut=None, rnd=True, order=0):
    """layernorm_bwd_kernel + the bins' finalize in fp32.  Planted errors: no_dres, s2_sign"""
    R, D = x.shape
    rs = rstd.unsqueeze(1)
    xh = (x.float() - mean.unsqueeze(1)) * rs
    gv = dy.float()
    gg = gv * g
    s1, s2 = gg.sum(1, keepdim=True) / D, (gg * xh).sum(1, keepdim=True) / D
    dx = rs * ((gg - s1 + xh * s2) if mut == "s2_sign" else (gg - s1 - xh * s2))
    if dres is not None and mut != "no_dres":
        dx = dx + dres.float()
    dg, db = ln_sum32(gv * xh, order), ln_sum32(gv, order)
    if old is not None:
        dg, db = dg + old[0].double(), db + old[1].double()
    return (dx.to(BF) if rnd else dx), dg.float(), db.float()
