"""A float64 reference of one append + extend call (csrc/kernels/attention_extend.hip), the elementwise bound the kernel
is held to, an fp32 model of the kernel (a stand-in for a correct kernel, and the carrier of planted errors) and the seeded
inputs shared by test_attn_extend_gpu.py and the CPU self-check test_attn_extend_ref_cpu.py.  The house pattern of
attn_ref.py / attn_decode_ref.py; everything here runs on CPU and GPU tensors alike.

``ref_extend`` computes, in float64, from exactly what the kernels are handed: the packed qkv rows of the Tq new tokens
per sequence (bf16), the cache as it stands before the call (bf16; slot lens[b] and everything after it may hold
anything), lens and the fp32 scale.  lens is clamped into [0, Tmax] as in the kernels.  Query j of sequence b sits at
position p = lens[b] + j; its keys are the cache slots 0..lens[b]-1 and the new keys 0..j.  A row whose position is
>= Tmax has no slot of its own: it is left unchecked (``checked`` of the result marks the others).

Bound.  Notation of attn_ref: u = 2^-24, c = scale * log2(e), scores in log2 units t = c*s, P = exp2(t - lse2), and

    |got - ref| <= 2^-8 |ref| + 2^-8 A + C u S,     A = sum_k P |V|,     S = sum_k P (w + wbar) |V|,
    w[q][k] = 1 + ln2 (c sum_i |q_i||k_i| + |lse2[q]|),  wbar[q] = sum_k P w.

Both terms are attn_ref's forward ones, unchanged: the kernel is that forward (P is rounded to bf16 for the MFMA, hence A;
the exponent argument, the lazy rescale and the final 1 / l are the same fp32 operations, hence S); only which keys a
query sees, and where they are read from, differ.

The constant.  Not picked in advance: ``model_extend`` below is the kernel in fp32 (64-key absolute tiles of the cache, a
wave of 16 queries skips tiles wholly past its last query's limit, online softmax, the running maximum moves only when
some query of the wave exceeds it by more than RESC = 8, P rounded to bf16 before P V); with rnd=False P and the result
stay fp32, and test_attn_extend_ref_cpu.py measures its worst error / (u S) over every shape, lens vector and family of
this module.  C = 4x that measurement rounded up, attn_ref's margin (the GPU sums in another order and v_exp_f32 is a few
ulp).

Measured fp32 part (MEASURED, worst error / (u S) of the model with the roundings off, rounded up): O 3.9 (3.83, on far_masked
behind 384 cached tokens, whose scores are hundreds of log2 units in magnitude; gauss 0.2).
Recorded worst error / bound (roundings on): fp32 model 0.878 (test_attn_extend_ref_cpu.py); kernels on an MI355X
(test_attn_extend_gpu.py): 0.878 (RECORDED_GPU below; model and kernel share the worst element: the bf16 result's own
rounding alone reaches 2^-8 |ref|).

Exact by construction, asserted bitwise: a sequence with lens = 0 has out row 0 = the new v row 0; the cache after the
append differs from the cache before it only in slots lens[b] .. min(lens[b] + Tq, Tmax) - 1, which hold the new k, v.
"""
import torch

from attn_ref import BF, F32, F64, FAMILIES, HD, LN2, LOG2E, RESC, TINY, U, Elem, bits_equal, check_bf16, f32, gen_flash, split_heads  # noqa: F401

TILE = 64                       # ops.kernels.EXTEND_TILE (the GPU test asserts that they agree)
MEASURED = {"O": 3.9}
C = {k: 4.0 * v for k, v in MEASURED.items()}
# worst error / bound of the kernels on an MI355X (test_attn_extend_gpu.py prints it)
RECORDED_GPU = {"O": 0.878}

# (B, H, Tmax, Tq): one tile of queries; two tiles, three heads; one head pair, a cache that is no multiple of 128; three
# sequences
SHAPES = [(1, 1, 2 * TILE, TILE), (2, 3, 384, 128), (1, 2, 320, TILE), (3, 2, 448, TILE)]
MUTATIONS = ["no_offset", "miss_self", "stale_slot", "skip_cache", "append_at_zero"]
GARBAGE = 2.0 ** 60


def lens_vectors(B, Tmax, Tq):
    """every uniform lens of {0, 1, 63, 64, 65, Tmax - Tq}, one ragged mix, and one vector with lens + Tq > Tmax (its
    rows at positions >= Tmax are unchecked; at Tmax = 2 Tq = 128 that also holds for the last row of lens = 65)"""
    vals = sorted({0, 1, 63, 64, 65, Tmax - Tq})
    out = [[v] * B for v in vals]
    out.append([vals[(2 * i + 1) % len(vals)] for i in range(B)] if B > 1 else [vals[len(vals) // 2]])
    out.append([Tmax - Tq + 7 + 16 * i for i in range(B)])
    return out


def cases():
    return [(s, lv) for s in SHAPES for lv in lens_vectors(s[0], s[2], s[3])]


def clamp_lens(lens, Tmax):
    return lens.long().clamp(0, Tmax)


def positions(lens, Tq, Tmax):
    """[B][Tq]: position lens[b] + j of query j (lens clamped)"""
    return clamp_lens(lens, Tmax)[:, None] + torch.arange(Tq, device=lens.device)[None, :]


def gen_extend(family, B, H, Tmax, Tq, lens, nan=False):
    """Seeded inputs of one call, bf16 on the CPU: rows lens[b] .. lens[b] + Tq - 1 of attn_ref.gen_flash(family, B, Tmax,
    H) are the new tokens (so the call is causal rows p of that forward; a position >= Tmax takes row Tmax - 1), rows <
    lens[b] fill the cache, and every slot >= lens[b] holds large finite garbage (2^60-scaled Gaussian).  ``nan``: slots
    >= lens[b] + Tq hold NaN bit patterns instead.  -> qkv [B*Tq][3*H*64], kcache, vcache [B][H][Tmax][64], lens int32"""
    full = gen_flash(family, B, Tmax, H)[0]
    lens_t = torch.tensor(lens, dtype=torch.int32)
    pos = positions(lens_t, Tq, Tmax)
    qkv = full.view(B, Tmax, -1)[torch.arange(B)[:, None], pos.clamp(max=Tmax - 1)].reshape(B * Tq, -1).contiguous()
    _, k, v = split_heads(full, B, Tmax, H)
    g = torch.Generator().manual_seed(177 + FAMILIES.index(family) + 3 * B + Tmax + 5 * H + Tq)
    junk = (torch.randn(2, B, H, Tmax, HD, generator=g, dtype=F64) * GARBAGE).to(BF)
    slot = torch.arange(Tmax)[None, :]
    stale = (slot >= pos[:, :1])[:, None, :, None]
    kc, vc = torch.where(stale, junk[0], k), torch.where(stale, junk[1], v)
    if nan:
        past = (slot >= pos[:, :1] + Tq)[:, None, :, None]
        pat = torch.tensor([0x7fc0, 0xffc1 - 65536, 0x7f81, -1], dtype=torch.int16).view(BF)     # quiet, signalling, -NaN
        nans = pat[torch.arange(Tmax * HD) % 4].view(Tmax, HD)
        kc, vc = torch.where(past, nans, kc), torch.where(past, nans, vc)
    return qkv, kc.contiguous(), vc.contiguous(), lens_t


def new_rows(qkv, B, H):
    """q, k, v of the new tokens, views [B][H][Tq][64]"""
    x = qkv.view(B, -1, 3, H, HD).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def ref_cache_after(qkv, kcache, vcache, lens, at_zero=False):
    """the cache a correct append leaves: slot lens[b] + j < Tmax of every (b, h) holds the new k / v row j, nothing else
    changes (``at_zero``: the planted error that stores row j at slot j)"""
    B, H, Tmax, _ = kcache.shape
    _, kn, vn = new_rows(qkv, B, H)
    Tq = kn.shape[2]
    p0 = torch.zeros(B, dtype=torch.long, device=kcache.device) if at_zero else clamp_lens(lens, Tmax).to(kcache.device)
    j = torch.arange(Tmax, device=kcache.device)[None, :] - p0[:, None]              # [B][Tmax]: the new row of a slot
    new = ((j >= 0) & (j < Tq))[:, None, :, None]
    jj = j.clamp(0, Tq - 1)[:, None, :, None].expand(B, H, Tmax, HD)
    return torch.where(new, kn.gather(2, jj), kcache), torch.where(new, vn.gather(2, jj), vcache)


def _visible(lim, Tmax):
    return torch.arange(Tmax, device=lim.device)[None, None, :] <= lim[:, :, None]    # [B][Tq][Tmax]


def ref_extend(qkv, kcache, vcache, lens, scale):
    """-> (Elem over out [B*Tq][H*64], checked bool [B*Tq]: the rows whose position is < Tmax)"""
    B, H, Tmax, _ = kcache.shape
    ka, va = ref_cache_after(qkv, kcache, vcache, lens)
    q = new_rows(qkv, B, H)[0].double()
    Tq = q.shape[2]
    pos = positions(lens.to(kcache.device), Tq, Tmax)
    vis = _visible(pos.clamp(max=Tmax - 1), Tmax)[:, None]                             # [B][1][Tq][Tmax]
    real = vis.any(2).squeeze(1)[:, None, :, None]                                     # slots some query sees: real data
    k = torch.where(real, ka, torch.zeros_like(ka)).double()
    v = torch.where(real, va, torch.zeros_like(va)).double()
    c = f32(scale) * LOG2E
    s2 = (c * (q @ k.transpose(-1, -2))).masked_fill(~vis, float("-inf"))             # [B][H][Tq][Tmax]
    aqk = c * (q.abs() @ k.abs().transpose(-1, -2))
    m = s2.max(-1, keepdim=True).values
    lse2 = m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))
    P = torch.exp2(s2 - lse2)
    w = 1.0 + LN2 * (aqk + lse2.abs())
    wbar = (P * w).sum(-1, keepdim=True)
    mg = lambda t: t.permute(0, 2, 1, 3).reshape(B * Tq, H * HD)                       # noqa: E731
    return Elem(mg(P @ v), mg(P @ v.abs()), mg((P * (w + wbar)) @ v.abs())), (pos < Tmax).reshape(-1)


def check_extend(out, ref, qkv, lens, Tmax, what="O"):
    """a kernel's (or model's) out against ref_extend's result: the bound on every checked row, and row 0 of a sequence
    with lens = 0 bitwise the new v row 0.  -> worst error / bound"""
    e, checked = ref
    worst = check_bf16(out[checked], Elem(e.ref[checked], e.A[checked], e.S[checked]), C["O"], what)
    B = lens.numel()
    Tq = out.shape[0] // B
    H = out.shape[1] // HD
    v0 = new_rows(qkv, B, H)[2][:, :, 0].reshape(B, H * HD)
    for b in torch.nonzero(clamp_lens(lens, Tmax) == 0).flatten().tolist():
        assert torch.equal(out[b * Tq], v0[b]), f"lens = 0: out row 0 of sequence {b} must be its v row 0 bitwise"
    return worst


def fp32_part(got, ref):
    """worst |got - ref| / (u S) over the checked rows of a model run without bf16 roundings (what MEASURED records)"""
    e, checked = ref
    r = ((got[checked].double() - e.ref[checked]).abs() - TINY).clamp_min(0.0) / (U * e.S[checked] + 1e-300)
    return r.max().item()


def _rb(t, rnd):
    return t.to(BF).float() if rnd else t


def model_extend(qkv, kcache, vcache, lens, scale, mut=None, rnd=True):
    """kv_cache_append_kernel + attn_extend_kernel in fp32 -> out ([B*Tq][H*64] bf16, or fp32 with rnd=False), kcache,
    vcache after the append.  Planted errors (``mut``): no_offset (query j sees keys <= j), miss_self (keys <= lens + j -
    1), stale_slot (keys <= lens + j + 1), skip_cache (only the new keys lens .. lens + j), append_at_zero (k, v of row j
    stored at slot j)."""
    B, H, Tmax, _ = kcache.shape
    dev = kcache.device
    ka, va = ref_cache_after(qkv, kcache, vcache, lens, at_zero=mut == "append_at_zero")
    q = new_rows(qkv, B, H)[0].float()
    Tq = q.shape[2]
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    pos = positions(lens.to(dev), Tq, Tmax)                                            # [B][Tq]
    lim = pos
    if mut == "no_offset":
        lim = torch.arange(Tq, device=dev)[None, :].expand(B, Tq)
    elif mut == "miss_self":
        lim = pos - 1
    elif mut == "stale_slot":
        lim = pos + 1
    lim = lim.clamp(max=Tmax - 1)
    lo = pos[:, :1] if mut == "skip_cache" else torch.zeros(B, 1, dtype=torch.long, device=dev)
    wlast = lim.view(B, Tq // 16, 16)[:, :, -1:].expand(B, Tq // 16, 16).reshape(B, Tq)     # the wave's last query
    blast = lim[:, -1]                                                                 # rows past it: zeroed V
    m = torch.full((B, H, Tq), float("-inf"), dtype=F32, device=dev)
    l = torch.zeros(B, H, Tq, dtype=F32, device=dev)
    o = torch.zeros(B, H, Tq, HD, dtype=F32, device=dev)
    for k0 in range(0, Tmax, 64):
        live = (k0 <= wlast)[:, None, :].expand(B, H, Tq)
        if not live.any():
            break
        keys = k0 + torch.arange(64, device=dev)
        rows = keys.clamp(max=Tmax - 1)
        kt = ka[:, :, rows].float()
        vt = torch.where((keys[None, :] > blast[:, None])[:, None, :, None], torch.zeros((), dtype=BF, device=dev),
                         va[:, :, rows]).float()
        s = q @ kt.transpose(-1, -2)                                                   # [B][H][Tq][64]
        masked = ((keys[None, None, :] > lim[:, :, None]) | (keys[None, None, :] < lo[:, :, None]))[:, None]
        s = torch.where(masked, torch.full((), float("-inf"), dtype=F32, device=dev), s)
        mt = s.max(-1).values * c
        gt = (mt > m + RESC) & live
        moved = gt.view(B, H, Tq // 16, 16).any(-1, keepdim=True).expand(B, H, Tq // 16, 16).reshape(B, H, Tq) & live
        mn = torch.where(moved, torch.maximum(m, mt), m)
        alpha = torch.where(moved, torch.exp2(m - mn), torch.ones_like(m))
        p = torch.exp2((s.double() * c - mn.double().unsqueeze(-1)).float())
        pv = _rb(p, rnd) @ vt
        l = torch.where(live, l * alpha + p.sum(-1), l)
        o = torch.where(live[..., None], o * alpha.unsqueeze(-1) + pv, o)
        m = torch.where(live, mn, m)
    O = (o * (1.0 / l).unsqueeze(-1)).permute(0, 2, 1, 3).reshape(B * Tq, H * HD)
    return (O.to(BF) if rnd else O), ka, va
