"""The packed-document variants of the flash-attention kernels (csrc/kernels/attention.hip, template parameter DOC): a
float64 reference under an arbitrary (doc_start, doc_end), fp32 models of the DOC kernels, the document layouts, the one
extra input family and a CPU mirror of the bounds kernel.  Shared by test_attn_doc_ref_cpu.py and test_attn_doc_gpu.py;
everything else (Elem, check_bf16, check_f32, the constants C, gen_flash, split_heads ...) is attn_ref's, unchanged.

Mask.  Query q of sequence b sees key k iff doc_start[b][q] <= k <= q.  The forward and dQ are handed doc_start and use
only it; dK / dV use only doc_end (key k is seen by the queries k <= q < doc_end[b][k]).  The reference computes from
exactly that: O, lse2 and dQ under the doc_start mask, dK and dV under the doc_end mask (the same mask for a
consistent pair of arrays).

Bounds.  The bound form is attn_ref's: its derivation bounds each visible term on its own and never uses which keys are
masked (a masked term is exactly 0 in kernel and reference alike), and log2 T still bounds log2 l.  The constants
follow attn_ref's rule (4x the worst error / (u S) of the fp32 models with the bf16 roundings off, rounded up), measured
here over every layout, shape and family of this file, NF = 1 and 2 (test_attn_doc_ref_cpu.py asserts them):
    O 4.0, lse2 8.6, dQ 7.4, dK 7.3, dV 9.1        (attn_ref.MEASURED, plain kernels: 3.2, 5.1, 6.4, 6.1, 6.7)
They are above attn_ref's, every one on far_masked_before: with short documents a row's sum has few terms, each with
|c s| up to 2.2 T log2 units from a 64-term fp32 product sum whose partial sums stay that large, so the error per unit
of S does not average down as it does over a plain causal row (unit layout: lse2 is that one product, O is one term).
attn_ref's constants stay as they are; MEASURED and C below are this file's own.
Recorded worst error / bound of the kernels on an MI355X (test_attn_doc_gpu.py, all eight backward variants):
O 0.893, lse2 0.094, dQ 0.857, dK 0.934, dV 0.935.

Models.  model_doc_fwd / model_doc_bwd follow the kernels' tile logic, not only the mask: the block's first key tile,
the wave's tile skip, the mask applied on "edge" tiles only, the running maximum starting at the finite floor M0 (the
-inf hazard of a fully masked first tile), the lazy rescale per 16-query fragment, the query loop of dK / dV ending at
the block's last doc_end.  ``mut`` plants one error; ``rnd=False`` keeps P, dS and the outputs in fp32.
"""
import math

import torch

import attn_ref as A

BF, F32, F64 = A.BF, A.F32, A.F64
HD, RESC, LOG2E, LN2, U = A.HD, A.RESC, A.LOG2E, A.LN2, A.U
M0 = -3.0e38                                     # the DOC forward's initial running maximum (attention.hip)
# worst error / (u S) of the fp32 models of this file with the bf16 roundings off (asserted <=), and 4x that
MEASURED = {"O": 4.0, "lse2": 8.6, "dQ": 7.4, "dK": 7.3, "dV": 9.1}
C = {k: 4.0 * v for k, v in MEASURED.items()}

SHAPES = [(1, 128, 1), (1, 256, 3), (3, 128, 2), (2, 384, 1), (1, 640, 2)]
CROSS_SHAPES = [(1, 128, 1), (1, 256, 3), (1, 640, 2)]             # all eight backward variants run on these
FAMILIES = ["gauss", "next_key", "growing", "flat", "far_masked_before"]
LAYOUTS = ["one", "unit", "tile_edges", "off_edges", "frag_edges", "late_in_wave", "skip_lead", "last_token",
           "many_in_wave"]
MUTS = ["start_off_by_one", "end_off_by_one", "block_start_for_all_waves", "lead_tile_skipped", "edge_unmasked",
        "no_inf_guard", "bounds_of_batch0"]


# ------------------------------------------------------------------------------------------------ layouts
def layout_starts(name, T):
    """document start indices of one sequence (0 is always one); an entry past T is dropped"""
    if name == "one":
        st = []
    elif name == "unit":
        st = list(range(T))
    elif name == "tile_edges":
        st = list(range(64, T, 64))
    elif name == "off_edges":
        st = [63, 65, 127, 129]
    elif name == "frag_edges":
        st = [15, 16, 17, 31, 32, 33, 47, 48]
    elif name == "late_in_wave":
        st = [60, 100]
    elif name == "skip_lead":
        st = [200]
    elif name == "last_token":
        st = [T - 1]
    elif name == "many_in_wave":
        st = [130, 140, 150, 155]
    else:
        raise KeyError(name)
    return sorted({0, *[s for s in st if 0 < s < T]})


def bounds_of_starts(starts, T):
    """-> doc_start, doc_end int32 [T] of one sequence"""
    ds = torch.zeros(T, dtype=torch.int32)
    de = torch.zeros(T, dtype=torch.int32)
    for s, e in zip(starts, starts[1:] + [T]):
        ds[s:e] = s
        de[s:e] = e
    return ds, de


def layout_bounds(name, B, T):
    """[B][T] bounds: sequence b takes the b-th layout after ``name``, so an array indexed without b fails"""
    i = LAYOUTS.index(name)
    rows = [bounds_of_starts(layout_starts(LAYOUTS[(i + b) % len(LAYOUTS)], T), T) for b in range(B)]
    return torch.stack([r[0] for r in rows]).contiguous(), torch.stack([r[1] for r in rows]).contiguous()


def bounds_from_tokens(idx, eot):
    """CPU mirror of pdnn_doc_bounds: token t starts a document iff t == 0 or token t - 1 is ``eot`` (the EOT token
    belongs to the document it ends).  idx int64 [B][T] -> doc_start, doc_end int32 [B][T]"""
    B, T = idx.shape
    ds = torch.zeros(B, T, dtype=torch.int32)
    de = torch.zeros(B, T, dtype=torch.int32)
    for b in range(B):
        row = idx[b].tolist()
        s = 0
        for t in range(T):
            if t > 0 and row[t - 1] == eot:
                s = t
            ds[b, t] = s
        e = T
        for t in range(T - 1, -1, -1):
            if row[t] == eot:
                e = t + 1
            de[b, t] = e
    return ds, de


# ------------------------------------------------------------------------------------------------ inputs
def gen_doc(family, B, T, H, scale=0.125):
    """attn_ref.gen_flash for its families; far_masked_before: the score falls by 2.2 log2 units per key, so the keys
    before a document start are far above the row's lse2: the backward's exp2 overflows to inf there before the mask
    zeroes it, and the forward's running maximum must never have seen them"""
    if family != "far_masked_before":
        return A.gen_flash(family, B, T, H, scale)
    g = torch.Generator().manual_seed(9700 + 13 * B + T + 7 * H)
    c = A.f32(scale) * LOG2E
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)        # noqa: E731
    q, k, v, dO = 0.125 * rn(B, H, T, HD), 0.125 * rn(B, H, T, HD), rn(B, H, T, HD), rn(B, H, T, HD)
    ka, kb = A._dim01(-2.2 * torch.arange(T, dtype=F64), c)
    q[..., 0], q[..., 1] = 16.0, 1.0
    k[..., 0], k[..., 1] = ka, kb
    return A.pack(q, k, v).to(BF).contiguous(), A.merge(dO).to(BF).contiguous()


# --------------------------------------------------------------------------------------------- float64 reference
def _idx(T, dev):
    i = torch.arange(T, device=dev)
    return i[:, None], i[None, :]                 # query column vector, key row vector


def masked_by_start(ds, T):
    """bool [B][1][T(q)][T(k)]: key k is NOT visible to query q (k > q or k < doc_start[b][q])"""
    q, k = _idx(T, ds.device)
    return ((k > q) | (k < ds.long()[:, :, None])).unsqueeze(1)


def masked_by_end(de, T):
    """the same from the keys' side: q < k or q >= doc_end[b][k]"""
    q, k = _idx(T, de.device)
    return ((k > q) | (q >= de.long()[:, None, :])).unsqueeze(1)


def ref_doc_fwd(qkv, ds, de, B, T, H, scale):
    """-> O: Elem over [B*T][H*64], lse2: Vec over [B][H][T]; attn_ref.ref_flash_fwd under the doc_start mask"""
    q, k, v, s2, aqk, _ = A._flash64(qkv, B, T, H, scale, False)
    s2 = s2.masked_fill(masked_by_start(ds, T), float("-inf"))
    m = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - m)
    lse2 = m + torch.log2(e.sum(-1, keepdim=True))
    P = torch.exp2(s2 - lse2)
    w = 1.0 + LN2 * (aqk + lse2.abs())
    wbar = (P * w).sum(-1, keepdim=True)
    O = A.Elem(A.merge(P @ v), A.merge(P @ v.abs()), A.merge((P * (w + wbar)) @ v.abs()))
    l2 = lse2.squeeze(-1)
    mag = (P * aqk).sum(-1) + l2.abs() + RESC + math.log2(T)
    return O, A.Vec(l2, C["lse2"] * U * mag + U * l2.abs())


def ref_doc_bwd(qkv, O_given, dO, lse2_given, ds, de, B, T, H, scale):
    """-> {"dQ" | "dK" | "dV": Elem over [B][H][T][64]}: dQ under the doc_start mask, dK / dV under the doc_end mask"""
    q, k, v, s2, aqk, _ = A._flash64(qkv, B, T, H, scale, False)
    sc = A.f32(scale)
    l2 = lse2_given.double().unsqueeze(-1)
    w = 1.0 + LN2 * (aqk + l2.abs())
    o, do = A.heads(O_given, B, T, H).double(), A.heads(dO, B, T, H).double()
    delta = (do * o).sum(-1, keepdim=True)
    adelta = (do * o).abs().sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    adP = do.abs() @ v.abs().transpose(-1, -2)
    Pall = torch.exp2(s2 - l2)                                     # inf where a masked key is far above lse2

    def side(masked):
        P = Pall.masked_fill(masked, 0.0)
        dS = P * (dP - delta)
        return P, dS, dS.abs() * w + P * (adP + adelta)

    Pq, dSq, Eq = side(masked_by_start(ds, T))
    Pk, dSk, Ek = side(masked_by_end(de, T))
    tr = lambda t: t.transpose(-1, -2)                             # noqa: E731
    return {"dV": A.Elem(tr(Pk) @ do, tr(Pk) @ do.abs(), tr(Pk * w) @ do.abs()),
            "dQ": A.Elem(sc * (dSq @ k), sc * (dSq.abs() @ k.abs()), sc * (Eq @ k.abs())),
            "dK": A.Elem(sc * (tr(dSk) @ q), sc * (tr(dSk).abs() @ q.abs()), sc * (tr(Ek) @ q.abs()))}


def doc_forward_given(qkv, ds, de, B, T, H, scale):
    eO, vl = ref_doc_fwd(qkv, ds, de, B, T, H, scale)
    return eO.ref.to(BF).contiguous(), vl.ref.float().contiguous()


def check_doc_fwd(qkv, O, lse2, ds, de, B, T, H, scale, ref=None):
    eO, vl = ref if ref is not None else ref_doc_fwd(qkv, ds, de, B, T, H, scale)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse2).all(), "forward output not finite"
    out = {"O": A.check_bf16(O, eO, C["O"], "O"), "lse2": A.check_f32(lse2, vl, "lse2")}
    first = (ds.long() == torch.arange(T, device=ds.device)[None, :])[:, None, :]          # [B][1][T]
    v = A.split_heads(qkv, B, T, H)[2]
    same = (A.heads(O, B, T, H) == v).all(-1)
    assert bool((same | ~first).all()), "the first token of a document: O must be V bitwise"
    return out


def check_doc_bwd(qkv, O_given, dO, lse2_given, dqkv, ds, de, B, T, H, scale, ref=None):
    if ref is None:
        ref = ref_doc_bwd(qkv, O_given, dO, lse2_given, ds, de, B, T, H, scale)
    assert torch.isfinite(dqkv.float()).all(), "backward output not finite"
    got = A.dqkv_parts(dqkv, B, T, H)
    out = {n: A.check_bf16(got[n], ref[n], C[n], n) for n in ("dQ", "dK", "dV")}
    zero = (A.heads(dO, B, T, H) == 0).all(-1)
    assert (got["dQ"][zero] == 0).all(), "a query row with dO = 0 must have dQ = 0 exactly"
    return out


# ------------------------------------------------------------------------------------ fp32 models of the DOC kernels
def _at(arr, pos):
    """arr [B][T] gathered at positions pos [T] (the same positions for every b) -> [B][T] long"""
    return arr.long()[:, pos]


def _mut_bounds(ds, de, mut):
    if mut == "bounds_of_batch0":
        return ds[:1].expand_as(ds), de[:1].expand_as(de)
    return ds, de


def model_doc_fwd(qkv, ds, de, B, T, H, scale, mut=None, rnd=True):
    """attn_fwd_kernel<DOC> in fp32 -> O ([B*T][D] bf16, or fp32 with rnd=False), lse2 fp32.  Planted errors:
    start_off_by_one (one more key visible), block_start_for_all_waves (the wave's first / last doc_start are the
    block's first), lead_tile_skipped (the block's first key tile rounded up), edge_unmasked (the mask runs only on the
    tile that holds the last document start of the wave), no_inf_guard (the maximum starts at -inf), bounds_of_batch0."""
    dev = qkv.device
    ds, de = _mut_bounds(ds.to(dev), de.to(dev), mut)
    q, k, v = (t.float() for t in A.split_heads(qkv, B, T, H))
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    rows = torch.arange(T, device=dev)
    wave0 = rows // 32 * 32
    blk0 = rows // 128 * 128
    cl = lambda t: t.clamp(0, T)                                   # noqa: E731
    dsl = cl(ds.long()) - (1 if mut == "start_off_by_one" else 0)                          # [B][T]
    b_first = cl(_at(ds, blk0))
    kb0 = torch.minimum((b_first + 63) // 64 if mut == "lead_tile_skipped" else b_first // 64, (blk0 + 128) // 64 - 1)
    ws_first, ws_last = cl(_at(ds, wave0)), cl(_at(ds, wave0 + 31))
    if mut == "block_start_for_all_waves":
        ws_first = ws_last = b_first
    m0 = float("-inf") if mut == "no_inf_guard" else M0
    m = torch.full((B, H, T), m0, dtype=F32, device=dev)
    l = torch.zeros(B, H, T, dtype=F32, device=dev)
    o = torch.zeros(B, H, T, HD, dtype=F32, device=dev)
    for kb in range(T // 64):
        k0 = kb * 64
        live = ((k0 <= wave0)[None, :] & (k0 + 63 >= ws_first) & (kb >= kb0))[:, None, :]  # [B][1][T]
        if not live.any():
            continue
        edge = k0 < ws_last
        if mut == "edge_unmasked":
            edge = edge & (k0 + 63 >= ws_last)
        kt, vt = k[:, :, k0:k0 + 64], v[:, :, k0:k0 + 64]
        s = q @ kt.transpose(-1, -2)
        keys = k0 + torch.arange(64, device=dev)
        masked = (keys[None, :] > rows[:, None])[None] | (edge[:, :, None] & (keys[None, None, :] < dsl[:, :, None]))
        s = s.masked_fill(masked[:, None], float("-inf"))
        mt = s.max(-1).values * c
        gt = (mt > m + RESC) & live
        moved = gt.view(B, H, T // 16, 16).any(-1, keepdim=True).expand(B, H, T // 16, 16).reshape(B, H, T) & live
        mn = torch.where(moved, torch.maximum(m, mt), m)
        alpha = torch.where(moved, torch.exp2(m - mn), torch.ones_like(m))
        p = torch.exp2((s.double() * c - mn.double().unsqueeze(-1)).float())
        pv = A._rb(p, rnd) @ vt
        l = torch.where(live, l * alpha + p.sum(-1), l)
        o = torch.where(live[..., None], o * alpha.unsqueeze(-1) + pv, o)
        m = torch.where(live, mn, m)
    O = A.merge(o * (1.0 / l).unsqueeze(-1))
    lse2 = m + torch.log2(l)
    return (O.to(BF) if rnd else O), lse2


def model_doc_bwd(qkv, O_given, dO, lse2_given, ds, de, B, T, H, scale, mut=None, rnd=True, nf=2):
    """attn_bwd_dq_kernel<.., NF, DOC> and attn_bwd_dkdv_kernel<NF, DOC> in fp32 (``nf`` = NF of both): P recomputed
    from lse2 (inf before a document start on far_masked_before, until the mask zeroes it), the tile ranges and the
    edge-tile masks of both kernels.  -> packed dqkv.  Planted errors: start_off_by_one, end_off_by_one (one more query
    sees the key), block_start_for_all_waves, lead_tile_skipped, edge_unmasked, bounds_of_batch0."""
    dev = qkv.device
    ds, de = _mut_bounds(ds.to(dev), de.to(dev), mut)
    q, k, v = (t.float() for t in A.split_heads(qkv, B, T, H))
    o, do = A.heads(O_given, B, T, H).float(), A.heads(dO, B, T, H).float()
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    sc = A.f32(scale)
    s = q @ k.transpose(-1, -2)
    p = torch.exp2((s.double() * c - lse2_given.double().unsqueeze(-1)).float())
    delta = (do * o).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    i = torch.arange(T, device=dev)
    qq, kk = i[:, None], i[None, :]
    tile = i // 64 * 64                                            # first index of the 64-tile of a position
    W, BLK = 16 * nf, 64 * nf
    cl = lambda t: t.clamp(0, T)                                   # noqa: E731
    wave0, blk0 = i // W * W, i // BLK * BLK

    # dQ: rows are queries (wave / block of the query), columns keys (tile of the key)
    dsl = (cl(ds.long()) - (1 if mut == "start_off_by_one" else 0))[:, :, None]            # [B][T][1]
    b_first = cl(_at(ds, blk0))
    kb0 = torch.minimum((b_first + 63) // 64 if mut == "lead_tile_skipped" else b_first // 64, (blk0 + BLK) // 64 - 1)
    ws_first, ws_last = cl(_at(ds, wave0)), cl(_at(ds, wave0 + W - 1))
    if mut == "block_start_for_all_waves":
        ws_first = ws_last = b_first
    k0 = tile[None, None, :]
    run = (k0 <= (wave0 + W - 1)[None, :, None]) & (k0 + 63 >= ws_first[:, :, None]) & (k0 // 64 >= kb0[:, :, None])
    edge = k0 < ws_last[:, :, None]
    if mut == "edge_unmasked":
        edge = edge & (k0 + 63 >= ws_last[:, :, None])
    vis_q = run & ~(kk > qq)[None] & ~(edge & (kk[None] < dsl))                            # [B][T][T]

    # dK / dV: columns are keys (wave / block of the key), rows queries (tile of the query)
    dl = (cl(de.long()) + (1 if mut == "end_off_by_one" else 0))[:, None, :]               # [B][1][T]
    nqe = torch.maximum(torch.minimum((cl(_at(de, blk0 + BLK - 1)) + 63) // 64, torch.tensor(T // 64, device=dev)),
                        blk0 // 64 + 1)
    we_first, we_last = cl(_at(de, wave0)), cl(_at(de, wave0 + W - 1))
    if mut == "block_start_for_all_waves":
        we_first = we_last = cl(_at(de, blk0 + BLK - 1))
    qs = tile[None, :, None]
    run = (qs + 63 >= wave0[None, None, :]) & (qs < we_last[:, None, :]) & (qs // 64 < nqe[:, None, :])
    edge = qs + 63 >= we_first[:, None, :]
    if mut == "edge_unmasked":
        edge = edge & (qs < we_first[:, None, :])
    vis_k = run & ~(kk > qq)[None] & ~(edge & (qq[None] >= dl))

    def side(vis):
        pm = torch.where(vis[:, None], p, torch.zeros_like(p))
        dsm = pm * (dp - delta)
        return A._rb(pm, rnd), A._rb(dsm, rnd)

    _, dsq = side(vis_q)
    pk, dsk = side(vis_k)
    dq = (dsq @ k) * sc
    dk = (dsk.transpose(-1, -2) @ q) * sc
    dv = pk.transpose(-1, -2) @ do
    out = A.pack(dq, dk, dv)
    return out.to(BF) if rnd else out
