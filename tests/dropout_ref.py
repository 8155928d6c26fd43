"""The dropout generator of csrc/kernels/dropout_rng.h re-implemented line for line in numpy integers, float64 references
of the kernels that drop (the row kernels of dropout.hip, the DROP variants of the flash-attention kernels), fp32 models
of the dropped attention kernels (a stand-in for a correct kernel, and the carrier of planted errors) and the bounds they
are held to.  Shared by test_dropout_ref_cpu.py and test_dropout_gpu.py; Elem, check_bf16, check_f32, gen_flash and the
document layouts are attn_ref's and attn_doc_ref's, unchanged.

Generator.  state = (seed, step); key(seed, step, site, stream) -> (k0, k1) by two splitmix64 finalisers; the word of
granule idx is the lowbias32 hash of idx + k0 with k1 added between its two multiplies; element j of the granule (4
consecutive keys of a query, 4 consecutive columns of a row) is kept iff byte j of the word >= thr = floor(256 p + 1/2)
(at most 255).  p_eff = thr / 256, scale = 256 / (256 - thr).

Attention with dropout.  The softmax is untouched: lse2 and P are those of attn_ref / attn_doc_ref (documents composed
in through their masks).  O = (P o keep) V s with s = 1 / (1 - p_eff);  dV = (P o keep)^T dO s;
dS = P (keep s dP - delta), delta = rowsum(dO o O) with the dropped O;  dQ = scale dS K, dK = scale dS^T Q.
Bounds: attn_ref's form, term by term.  A dropped term is exactly 0 in kernel and reference alike and a kept one is
the undropped term times s (one more fp32 rounding, covered by w >= 1), so
    O:  A = sum_k Pd |V|,  S = sum_k Pd (w + wbar) |V|      with Pd = P keep s
    dV: A = sum_q Pd |dO|, S = sum_q Pd w |dO|
    dS: E = |dS| w + P (keep s sum_i |dO_i V_ki| + sum_i |dO_i O_i|);  dQ: S = scale sum_k E |K|, dK likewise over q
and lse2's bound is the undropped one (the kernel computes it from the undropped P).

Constants.  attn_ref's rule: MEASURED is the worst error / (u S) of the fp32 models of this file with the bf16
roundings off, over SHAPES x FAMILIES x PS, plain and under LAYOUTS, rounded up; C = 4 x MEASURED;
test_dropout_ref_cpu.py asserts both.  Measured on the CPU (worst case: the growing family every time): plain O 1.93,
lse2 2.21, dQ 3.48, dK 4.46, dV 4.78; documents O 1.95, lse2 2.73, dQ 3.48, dK 4.56, dV 5.20; MEASURED rounds them up.
They sit below attn_ref's and attn_doc_ref's own (3.2 .. 9.1), whose worst cases are families this file does not run
(far_masked, next_key, far_masked_before); attn_ref.MEASURED and attn_doc_ref.MEASURED are not used here.
"""
import numpy as np
import torch

import attn_doc_ref as DR
import attn_ref as A

BF, F32, F64 = A.BF, A.F32, A.F64
U, HD, RESC, LOG2E, LN2 = A.U, A.HD, A.RESC, A.LOG2E, A.LN2
SITE_EMBD = 0x7fffffff

SHAPES = [(1, 128, 1), (3, 128, 2), (1, 256, 3), (1, 640, 2)]          # (B, T, H)
CROSS_SHAPES = [(1, 128, 1), (1, 256, 3), (1, 640, 2)]                 # all eight backward variants run on these
ROW_SHAPES = [(1, 8), (3, 72), (130, 768)]
FAMILIES = ["gauss", "flat", "growing"]
PS = [0.1, 0.5]
MASK_PS = [0.1, 0.5, 0.996]
LAYOUTS = ["one", "tile_edges", "off_edges", "skip_lead"]
STATE = (20240607, 3)                                                  # (seed, step) of the shared cases
SITE = 4                                                               # layer 1, attention probabilities
FWD_MUTS = ["head_neighbour", "transposed", "no_scale", "lse_dropped", "flip_bit"]
BWD_MUTS = ["head_neighbour", "transposed", "no_scale", "next_step", "delta_undropped", "flip_bit"]

# worst error / (u S) of the fp32 models below with the bf16 roundings off (asserted <=), and 4x that
MEASURED = {"plain": {"O": 2.0, "lse2": 2.3, "dQ": 3.5, "dK": 4.5, "dV": 4.8},
            "doc": {"O": 2.0, "lse2": 2.8, "dQ": 3.5, "dK": 4.6, "dV": 5.2}}
C = {m: {k: 4.0 * v for k, v in d.items()} for m, d in MEASURED.items()}


# ------------------------------------------------------------------------------------------------ generator
def threshold(p):
    p32 = float(np.float32(p))
    assert 0.0 <= p32 < 1.0, p
    return min(255, int(p32 * 256.0 + 0.5))


def p_eff(p):
    return threshold(p) / 256.0


def scale_of(p):
    return 256.0 / (256 - threshold(p))


def _mix64(z):
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def key(seed, step, site, stream):
    with np.errstate(over="ignore"):
        seed, step = np.uint64(seed & (2 ** 64 - 1)), np.uint64(step & (2 ** 64 - 1))
        z = _mix64(seed + np.uint64(0x9E3779B97F4A7C15) * (step + np.uint64(1)))
        z = _mix64(z ^ ((np.uint64(site) << np.uint64(32)) | np.uint64(stream)))
    return np.uint32(z & np.uint64(0xFFFFFFFF)), np.uint32(z >> np.uint64(32))


def words(k, idx):
    """idx uint32 array -> the 32-bit word of every granule"""
    with np.errstate(over="ignore"):
        x = idx.astype(np.uint32) + k[0]
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x += k[1]
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def _bits(k, n, thr):
    w = words(k, np.arange(n, dtype=np.uint64).astype(np.uint32))
    return ((w[:, None] >> (8 * np.arange(4, dtype=np.uint32))[None, :]) & np.uint32(255)) >= thr


def keep_rows(state, site, p, R, D):
    """bool [R][D]: element (row, col) is byte col & 3 of granule row * (D / 4) + (col >> 2), stream 0"""
    return torch.from_numpy(_bits(key(state[0], state[1], site, 0), R * (D // 4), threshold(p)).reshape(R, D))


def keep_attn(state, site, p, B, H, T):
    """bool [B][H][T(q)][T(k)]: byte k & 3 of granule q * (T / 4) + (k >> 2), stream b * H + h"""
    thr = threshold(p)
    return torch.from_numpy(np.stack([_bits(key(state[0], state[1], site, s), T * (T // 4), thr).reshape(T, T)
                                      for s in range(B * H)]).reshape(B, H, T, T))


# ------------------------------------------------------------------------------------------------ rows
def ref_rows(x, res, keep, p):
    """-> (float64 reference, bound) of dropout_add_fwd / dropout_bwd: y = res + keep x s.  One bf16 rounding of the
    result, the fp32 scale s (u), the product and the add (u each)."""
    t = keep.double() * x.double() * scale_of(p)
    y = t + (res.double() if res is not None else 0.0)
    return y, y.abs() * 2.0 ** -8 + 4.0 * U * (t.abs() + (res.double().abs() if res is not None else 0.0)) + A.TINY


# ------------------------------------------------------------------------------------------------ attention: float64
def _masked(doc, B, T, dev, side):
    if doc is None:
        return A.above_diag(T, dev)
    return DR.masked_by_start(doc[0].to(dev), T) if side == "q" else DR.masked_by_end(doc[1].to(dev), T)


def ref_drop_fwd(qkv, keep, p, B, T, H, scale, doc=None):
    """-> O: Elem, lse2: Vec.  ``doc`` = (doc_start, doc_end) or None"""
    mode = "doc" if doc is not None else "plain"
    q, k, v, s2, aqk, _ = A._flash64(qkv, B, T, H, scale, False)
    s2 = s2.masked_fill(_masked(doc, B, T, qkv.device, "q"), float("-inf"))
    m = s2.max(-1, keepdim=True).values
    lse2 = m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))
    P = torch.exp2(s2 - lse2)
    w = 1.0 + LN2 * (aqk + lse2.abs())
    wbar = (P * w).sum(-1, keepdim=True)
    Pd = P * keep.to(qkv.device).double() * scale_of(p)
    O = A.Elem(A.merge(Pd @ v), A.merge(Pd @ v.abs()), A.merge((Pd * (w + wbar)) @ v.abs()))
    l2 = lse2.squeeze(-1)
    mag = (P * aqk).sum(-1) + l2.abs() + RESC + np.log2(T)
    return O, A.Vec(l2, C[mode]["lse2"] * U * mag + U * l2.abs())


def ref_drop_bwd(qkv, O_given, dO, lse2_given, keep, p, B, T, H, scale, doc=None):
    q, k, v, s2, aqk, _ = A._flash64(qkv, B, T, H, scale, False)
    sc, s = A.f32(scale), scale_of(p)
    l2 = lse2_given.double().unsqueeze(-1)
    w = 1.0 + LN2 * (aqk + l2.abs())
    o, do = A.heads(O_given, B, T, H).double(), A.heads(dO, B, T, H).double()
    delta = (do * o).sum(-1, keepdim=True)
    adelta = (do * o).abs().sum(-1, keepdim=True)
    ks = keep.to(qkv.device).double() * s
    dP = do @ v.transpose(-1, -2)
    adP = do.abs() @ v.abs().transpose(-1, -2)
    Pall = torch.exp2(s2 - l2)

    def side(which):
        P = Pall.masked_fill(_masked(doc, B, T, qkv.device, which), 0.0)
        dS = P * (ks * dP - delta)
        return P, dS, dS.abs() * w + P * (ks * adP + adelta)

    Pq, dSq, Eq = side("q")
    Pk, dSk, Ek = side("k")
    tr = lambda t: t.transpose(-1, -2)                             # noqa: E731
    Pd = Pk * ks
    return {"dV": A.Elem(tr(Pd) @ do, tr(Pd) @ do.abs(), tr(Pd * w) @ do.abs()),
            "dQ": A.Elem(sc * (dSq @ k), sc * (dSq.abs() @ k.abs()), sc * (Eq @ k.abs())),
            "dK": A.Elem(sc * (tr(dSk) @ q), sc * (tr(dSk).abs() @ q.abs()), sc * (tr(Ek) @ q.abs()))}


def drop_forward_given(qkv, keep, p, B, T, H, scale, doc=None):
    eO, vl = ref_drop_fwd(qkv, keep, p, B, T, H, scale, doc)
    return eO.ref.to(BF).contiguous(), vl.ref.float().contiguous()


def check_drop_fwd(O, lse2, ref, doc=None):
    mode = "doc" if doc is not None else "plain"
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse2).all(), "forward output not finite"
    return {"O": A.check_bf16(O, ref[0], C[mode]["O"], "O"), "lse2": A.check_f32(lse2, ref[1], "lse2")}


def check_drop_bwd(dqkv, ref, B, T, H, doc=None):
    mode = "doc" if doc is not None else "plain"
    assert torch.isfinite(dqkv.float()).all(), "backward output not finite"
    got = A.dqkv_parts(dqkv, B, T, H)
    return {n: A.check_bf16(got[n], ref[n], C[mode][n], n) for n in ("dQ", "dK", "dV")}


# ------------------------------------------------------------------------------------------------ attention: fp32 models
def mut_keep(keep, mut):
    if mut == "head_neighbour":
        return keep.flatten(0, 1).roll(1, 0).view_as(keep)
    if mut == "transposed":
        return keep.transpose(-1, -2)
    if mut == "flip_bit":
        keep = keep.clone()
        keep[:, :, 1, 0] = ~keep[:, :, 1, 0]
        return keep
    return keep


def _one_doc(B, T):
    return torch.zeros(B, T, dtype=torch.int32), torch.full((B, T), T, dtype=torch.int32)


def model_drop_fwd(qkv, keep, p, B, T, H, scale, doc=None, mut=None, rnd=True):
    """attn_fwd_kernel<DOC, DROP> in fp32: attn_doc_ref.model_doc_fwd's tile logic (for the plain kernel: one document
    per row, which runs the plain kernel's tiles) with the keep mask on the P that enters P V, the row sum l from the
    undropped P and s on the final 1 / l.  Planted errors: head_neighbour, transposed, no_scale, lse_dropped (l and
    lse2 from the dropped, scaled P), flip_bit (query 1, key 0)."""
    dev = qkv.device
    ds, de = (t.to(dev) for t in (doc if doc is not None else _one_doc(B, T)))
    kp = mut_keep(keep.to(dev), mut).float()
    s = 1.0 if mut == "no_scale" else torch.tensor(scale_of(p), dtype=F32).item()
    q, k, v = (t.float() for t in A.split_heads(qkv, B, T, H))
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    rows = torch.arange(T, device=dev)
    wave0, blk0 = rows // 32 * 32, rows // 128 * 128
    cl = lambda t: t.clamp(0, T)                                   # noqa: E731
    dsl = cl(ds.long())
    kb0 = torch.minimum(cl(DR._at(ds, blk0)) // 64, (blk0 + 128) // 64 - 1)
    ws_first, ws_last = cl(DR._at(ds, wave0)), cl(DR._at(ds, wave0 + 31))
    m = torch.full((B, H, T), DR.M0 if doc is not None else float("-inf"), dtype=F32, device=dev)
    l = torch.zeros(B, H, T, dtype=F32, device=dev)
    o = torch.zeros(B, H, T, HD, dtype=F32, device=dev)
    for kb in range(T // 64):
        k0 = kb * 64
        live = ((k0 <= wave0)[None, :] & (k0 + 63 >= ws_first) & (kb >= kb0))[:, None, :]
        if not live.any():
            continue
        edge = k0 < ws_last
        kt, vt = k[:, :, k0:k0 + 64], v[:, :, k0:k0 + 64]
        sc = q @ kt.transpose(-1, -2)
        keys = k0 + torch.arange(64, device=dev)
        masked = (keys[None, :] > rows[:, None])[None] | (edge[:, :, None] & (keys[None, None, :] < dsl[:, :, None]))
        sc = sc.masked_fill(masked[:, None], float("-inf"))
        mt = sc.max(-1).values * c
        gt = (mt > m + RESC) & live
        moved = gt.view(B, H, T // 16, 16).any(-1, keepdim=True).expand(B, H, T // 16, 16).reshape(B, H, T) & live
        mn = torch.where(moved, torch.maximum(m, mt), m)
        alpha = torch.where(moved, torch.exp2(m - mn), torch.ones_like(m))
        pr = torch.exp2((sc.double() * c - mn.double().unsqueeze(-1)).float())
        pd = pr * kp[:, :, :, k0:k0 + 64]
        pv = A._rb(pd, rnd) @ vt
        rs = (pd * s).sum(-1) if mut == "lse_dropped" else pr.sum(-1)
        l = torch.where(live, l * alpha + rs, l)
        o = torch.where(live[..., None], o * alpha.unsqueeze(-1) + pv, o)
        m = torch.where(live, mn, m)
    O = A.merge(o * (s / l).unsqueeze(-1))
    lse2 = m + torch.log2(l)
    return (O.to(BF) if rnd else O), lse2


def model_drop_bwd(qkv, O_given, dO, lse2_given, keep, p, B, T, H, scale, doc=None, mut=None, rnd=True):
    """the DROP backward kernels in fp32: P recomputed from lse2 and masked (the kernels' visibility is the mask's:
    attn_doc_ref's models carry the tile logic and its planted errors), P o keep rounded to bf16 for dV with s applied
    to the fp32 sum, dS = P (keep s dP - delta) rounded to bf16.  Planted errors: head_neighbour, transposed, no_scale,
    flip_bit; next_step and delta_undropped are planted by the caller through ``keep`` / ``O_given``."""
    dev = qkv.device
    kp = mut_keep(keep.to(dev), mut).float()
    s = 1.0 if mut == "no_scale" else torch.tensor(scale_of(p), dtype=F32).item()
    q, k, v = (t.float() for t in A.split_heads(qkv, B, T, H))
    o, do = A.heads(O_given, B, T, H).float(), A.heads(dO, B, T, H).float()
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    sc = A.f32(scale)
    pall = torch.exp2(((q @ k.transpose(-1, -2)).double() * c - lse2_given.double().unsqueeze(-1)).float())
    delta = (do * o).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)

    def side(which):
        pm = torch.where(_masked(doc, B, T, dev, which), torch.zeros_like(pall), pall)
        dsm = pm * (kp * (dp * s) - delta)
        return A._rb(pm * kp, rnd), A._rb(dsm, rnd)

    _, dsq = side("q")
    pk, dsk = side("k")
    out = A.pack((dsq @ k) * sc, (dsk.transpose(-1, -2) @ q) * sc, (pk.transpose(-1, -2) @ do) * s)
    return out.to(BF) if rnd else out


def cases():
    """(family, (B, T, H), p, layout or None): every shape x family x p plain, and under each layout"""
    return [(f, s, p, lay) for s in SHAPES for f in FAMILIES for p in PS for lay in [None] + LAYOUTS]


def doc_of(layout, B, T):
    return DR.layout_bounds(layout, B, T) if layout is not None else None
