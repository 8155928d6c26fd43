"""A float64 reference of one decode-attention call (csrc/kernels/attention_decode.hip), the elementwise bound the kernel
is held to, an fp32 model of the kernel (a stand-in for a correct kernel, and the carrier of planted errors) and the seeded
inputs shared by test_attn_decode_gpu.py and the CPU self-check test_attn_decode_ref_cpu.py.  The house pattern of
attn_ref.py / attn_doc_ref.py; everything here runs on CPU and GPU tensors alike.

``ref_decode`` computes, in float64, from exactly what the kernel is handed: the packed qkv row of the new token (bf16),
the cache as it stands before the call (bf16; slot p = lens[b] and everything after it may hold anything), lens and the
fp32 scale.  p is clamped into [0, Tmax - 1] as in the kernel.  The keys of (b, h) are cache slots 0..p-1 and the new key.

Bound.  Notation of attn_ref: u = 2^-24, c = scale * log2(e), scores in log2 units t = c*s, P = exp2(t - lse2), and

    |got - ref| <= 2^-8 |ref| + 2^-8 A + C u S.

A = 0: the decode kernel keeps P in fp32 (it does NOT round P to bf16 before the V product; attention.hip's forward does),
so the only bf16 rounding is that of the stored result, 2^-8 |ref|.

S, to first order.  Key k lies in chunk i with maximum m_i; M = max_i m_i.  The kernel forms
    t_k = fl(c fl(q.k))              a 64-term fp32 accumulation, the fp32 constant c and one product:
                                     u (c sum_j |q_j||k_j| + 2 |t_k|)
    p_k = exp2(fl(t_k - m_i))        u |t_k - m_i| from the subtraction, about one ulp from v_exp_f32
    w_i = exp2(fl(m_i - M))          the combine: u |m_i - M| and another ulp of v_exp_f32
and the weight of key k in the result is p_k w_i / L.  m_i and M are only reference points (they cancel exactly), so what
counts is the rounding of the two subtractions, and since t_k <= m_i <= M their magnitudes add up to exactly M - t_k.  exp2
turns an argument error e into the relative error ln2 e.  So P carries the relative error u w,

    w[k] = 2 + ln2 (c sum_j |q_j||k_j| + |lse2| + (M - t_k)),

which is attn_ref's w = 1 + ln2 (aqk + |lse2|) (|lse2| stands for the magnitude of the scaled scores near the maximum, as
there) extended by the combine: the second exponential's ulp and the (M - t_k) of the two subtractions.  P (M - t_k) is at
most x 2^-x <= 0.54, so the extension is a bounded constant per key and costs a far-away chunk nothing.  The normaliser
L = sum_i w_i l_i carries the P-weighted mean wbar = sum_k P w; the final division O / L and the products w_i o_i add
roundings of their own, one more u on every term.  With w >= 2 also covering the fp32 accumulation of P V:

    S = sum_k P (w + wbar + 1) |V|.

With one chunk (direct-write path) w_i = 1 exactly and the same S holds with room to spare.

The constant.  Not picked in advance: ``model_decode`` below is the kernel in fp32 (chunked partials with the kernel's
chunk sizes, neutral partials past p, then the combine); with rnd=False the result stays fp32, and test_attn_decode_ref_cpu.py
measures its worst error / (u S) over every shape, lens vector and family of this module.  C = 4x that measurement rounded
up, attn_ref's margin (the GPU sums in another order and v_exp_f32 is a few ulp).

Measured fp32 part (MEASURED, worst error / (u S) of the model with the rounding off, rounded up): O 1.7 (worst
on far_masked, whose scores are 280 log2 units in magnitude; gauss 0.14).
Recorded worst error / bound (rounding on): fp32 model 0.987 (test_attn_decode_ref_cpu.py); kernels on an MI355X
(test_attn_decode_gpu.py): 0.987 (RECORDED_GPU below; model and kernel share the worst element).  The bf16 result reaches ~1 because its own rounding alone reaches
2^-8 |ref|.

Exact by construction, asserted bitwise by the GPU test: lens = 0 gives out = v_new; slots > p and other sequences' caches
change no output bit; the cache after the call differs from the cache before it in slot p only, which holds the new k, v.
"""
import torch

from attn_ref import BF, F32, F64, FAMILIES, HD, LN2, LOG2E, TINY, U, Elem, bits_equal, check_bf16, f32, gen_flash, split_heads  # noqa: F401

MEASURED = {"O": 1.7}
C = {k: 4.0 * v for k, v in MEASURED.items()}
# worst error / bound of the kernels on an MI355X (test_attn_decode_gpu.py prints it)
RECORDED_GPU = {"O": 0.987}

# (B, H, Tmax, chunk): single chunk (direct write); several chunks; a partial last chunk; three sequences; 256-key chunks
SHAPES = [(1, 1, 128, 128), (2, 3, 384, 128), (1, 2, 200, 64), (3, 2, 320, 64), (2, 1, 1024, 256)]
MUTATIONS = ["no_new_key", "drop_partial", "no_rescale", "stale_slot"]
GARBAGE = 2.0 ** 60


def lens_vectors(B, Tmax, chunk):
    """every uniform lens of {0, 1, chunk - 1, chunk, chunk + 1, Tmax - 1} that fits the cache, plus one ragged mix"""
    vals = sorted({v for v in (0, 1, chunk - 1, chunk, chunk + 1, Tmax - 1) if 0 <= v <= Tmax - 1})
    out = [[v] * B for v in vals]
    out.append([vals[(2 * i + 1) % len(vals)] for i in range(B)] if B > 1 else [vals[len(vals) // 2]])
    return out


def cases():
    return [(s, lv) for s in SHAPES for lv in lens_vectors(s[0], s[2], s[3])]


def clamp_lens(lens, Tmax):
    return lens.long().clamp(0, Tmax - 1)


def gen_decode(family, B, H, Tmax, lens):
    """Seeded inputs of one call, bf16 on the CPU: row p = lens[b] of attn_ref.gen_flash(family, B, Tmax, H) is the new
    token (so the call is causal row p of that forward), rows < p fill the cache, and every slot >= p holds large finite
    garbage (2^60-scaled Gaussian).  -> qkv [B][3*H*64], kcache, vcache [B][H][Tmax][64], lens int32 [B]"""
    full = gen_flash(family, B, Tmax, H)[0]
    lens_t = torch.tensor(lens, dtype=torch.int32)
    p = clamp_lens(lens_t, Tmax)
    qkv = full.view(B, Tmax, -1)[torch.arange(B), p].contiguous()
    _, k, v = split_heads(full, B, Tmax, H)
    g = torch.Generator().manual_seed(77 + FAMILIES.index(family) + 3 * B + Tmax + 5 * H)
    junk = (torch.randn(2, B, H, Tmax, HD, generator=g, dtype=F64) * GARBAGE).to(BF)
    stale = (torch.arange(Tmax)[None, :] >= p[:, None])[:, None, :, None]
    return (qkv, torch.where(stale, junk[0], k).contiguous(), torch.where(stale, junk[1], v).contiguous(), lens_t)


def new_rows(qkv, B, H):
    """q, k, v of the new token, views [B][H][64]"""
    x = qkv.view(B, 3, H, HD)
    return x[:, 0], x[:, 1], x[:, 2]


def ref_cache_after(qkv, kcache, vcache, lens):
    """the cache a correct call leaves: slot p of every (b, h) holds the new k / v row, nothing else changes"""
    B, H, Tmax, _ = kcache.shape
    _, kn, vn = new_rows(qkv, B, H)
    at = (torch.arange(Tmax, device=kcache.device)[None, :] == clamp_lens(lens, Tmax)[:, None])[:, None, :, None]
    return torch.where(at, kn.unsqueeze(2), kcache), torch.where(at, vn.unsqueeze(2), vcache)


def ref_decode(qkv, kcache, vcache, lens, scale):
    """-> Elem over out [B][H*64]: the float64 result, A = 0 (P stays fp32 in the kernel) and S of the module docstring"""
    B, H, Tmax, _ = kcache.shape
    ka, va = ref_cache_after(qkv, kcache, vcache, lens)
    vis = (torch.arange(Tmax, device=kcache.device)[None, :] <= clamp_lens(lens, Tmax)[:, None])[:, None, :]     # [B][1][Tmax]
    k = torch.where(vis.unsqueeze(-1), ka, torch.zeros_like(ka)).double()
    v = torch.where(vis.unsqueeze(-1), va, torch.zeros_like(va)).double()
    q = new_rows(qkv, B, H)[0].double()
    c = f32(scale) * LOG2E
    s2 = (c * (k @ q.unsqueeze(-1)).squeeze(-1)).masked_fill(~vis, float("-inf"))         # [B][H][Tmax]
    aqk = c * (k.abs() @ q.abs().unsqueeze(-1)).squeeze(-1)
    M = s2.max(-1, keepdim=True).values
    lse2 = M + torch.log2(torch.exp2(s2 - M).sum(-1, keepdim=True))
    P = torch.exp2(s2 - lse2)
    w = 2.0 + LN2 * (aqk + lse2.abs() + (M - s2).masked_fill(~vis, 0.0))
    wbar = (P * w).sum(-1, keepdim=True)
    O = (P.unsqueeze(-2) @ v).squeeze(-2)
    S = ((P * (w + wbar + 1.0)).unsqueeze(-2) @ v.abs()).squeeze(-2)
    return Elem(O.reshape(B, H * HD), torch.zeros(B, H * HD, dtype=F64, device=O.device), S.reshape(B, H * HD))


def check_decode(out, e, what="O"):
    return check_bf16(out, e, C["O"], what)


def model_decode(qkv, kcache, vcache, lens, scale, chunk, mut=None, rnd=True):
    """attn_decode_kernel + attn_decode_combine_kernel in fp32: per chunk of ``chunk`` keys m_i, l_i = sum P, o_i = P V
    with P = exp2(t - m_i) in fp32 (neutral past p: m = -inf, l = 0, o = 0), then out = sum_i w_i o_i / sum_i w_i l_i with
    w_i = exp2(m_i - M) (one chunk: o / l directly).  rnd=False keeps the result in fp32.  Planted errors (``mut``):
    no_new_key (the new key left out: keys 0..p-1), drop_partial (the partial of the chunk that holds slot p dropped when
    there is an earlier one), no_rescale (w_i = 1), stale_slot (slot p + 1 of the cache read as a key)."""
    B, H, Tmax, _ = kcache.shape
    dev = kcache.device
    ka, va = ref_cache_after(qkv, kcache, vcache, lens)
    k, v = ka.float(), va.float()
    q = new_rows(qkv, B, H)[0].float()
    c = (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()
    t = (k @ q.unsqueeze(-1)).squeeze(-1) * c                                              # [B][H][Tmax] fp32
    p = clamp_lens(lens, Tmax).to(dev)
    keys = torch.arange(Tmax, device=dev)
    last = p - 1 if mut == "no_new_key" else (p + 1 if mut == "stale_slot" else p)
    vis = (keys[None, :] <= last[:, None])[:, None, :].expand(B, H, Tmax)
    ms, ls, os_ = [], [], []
    for k0 in range(0, Tmax, chunk):
        sl = slice(k0, min(k0 + chunk, Tmax))
        live = (k0 <= p)[:, None].expand(B, H)                                             # else neutral
        tv = t[:, :, sl].masked_fill(~vis[:, :, sl], float("-inf"))
        m = tv.max(-1).values
        pk = torch.exp2(tv - m.unsqueeze(-1))
        pk = torch.where(vis[:, :, sl], pk, torch.zeros_like(pk))
        o = (pk.unsqueeze(-2) @ torch.where(vis[:, :, sl].unsqueeze(-1), v[:, :, sl], torch.zeros_like(v[:, :, sl]))).squeeze(-2)
        if mut == "drop_partial":
            live = live & ~(((p // chunk) * chunk == k0) & (p >= chunk))[:, None]
        ms.append(torch.where(live, m, torch.full_like(m, float("-inf"))))
        ls.append(torch.where(live, pk.sum(-1), torch.zeros_like(m)))
        os_.append(torch.where(live.unsqueeze(-1), o, torch.zeros_like(o)))
    if len(ms) == 1:
        out = os_[0] / ls[0].unsqueeze(-1)
    else:
        M = torch.stack(ms).max(0).values
        L = torch.zeros_like(M)
        O = torch.zeros_like(os_[0])
        for m, l, o in zip(ms, ls, os_):
            w = torch.exp2(m - M)
            if mut == "no_rescale":
                w = torch.where(l > 0, torch.ones_like(w), torch.zeros_like(w))
            L = L + w * l
            O = O + w.unsqueeze(-1) * o
        out = O / L.unsqueeze(-1)
    out = out.reshape(B, H * HD)
    return out.to(BF) if rnd else out
