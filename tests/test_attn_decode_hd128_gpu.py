"""csrc/kernels/attention_decode_hd128.hip through ops.kernels.attn_decode, attn_decode_multi and kv_cache_fill (the head
dim is the cache's last dimension): the single-query kernel against a float64 reference under attn_decode_ref's bound (its
S and C["O"]), the multi-query kernel against successive single-query calls bit for bit, the cache fill, the guards."""
import math

import pytest
import torch

import attn_decode_ref as R
from pytorch_distributed_nn_amd.ops import kernels as K
from attn_ref import BF, F64, LN2, LOG2E, U, bits_equal, f32

pytestmark = pytest.mark.gpu
HD = 128
SCALE = 1.0 / math.sqrt(HD)
SHAPES = [(1, 1, 128, 128), (2, 3, 384, 128), (1, 2, 200, 64), (2, 1, 512, 256)]      # (B, H, Tmax, chunk)
IDS = ["x".join(map(str, s)) for s in SHAPES]
_FULL = {}


def gen(B, H, Tmax, lens, S=1):
    """Gaussian bf16, seeded per shape and generated once: rows lens[b] .. lens[b]+S-1 of ``full`` [B][Tmax][3*H*128] are
    the new tokens (indices past the end wrap, they are only inputs), rows before them the cache; every slot >= lens[b]
    holds 2^60-scaled garbage.  -> qkv [B*S][3*H*128], kcache, vcache [B][H][Tmax][128], lens int32 [B], on the GPU"""
    if (B, H, Tmax) not in _FULL:
        g = torch.Generator().manual_seed(1000 * B + 10 * H + Tmax)
        _FULL[B, H, Tmax] = (torch.randn(B, Tmax, 3, H, HD, generator=g).to(BF).cuda(),
                             (torch.randn(2, B, H, Tmax, HD, generator=g, dtype=F64) * R.GARBAGE).to(BF).cuda())
    full, junk = _FULL[B, H, Tmax]
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    rows = (ln.long().clamp(0, Tmax - 1)[:, None] + torch.arange(S, device="cuda")[None, :]) % Tmax
    qkv = full[torch.arange(B, device="cuda")[:, None], rows].reshape(B * S, 3 * H * HD).contiguous()
    stale = (torch.arange(Tmax, device="cuda")[None, :] >= ln[:, None])[:, None, :, None]
    kc = torch.where(stale, junk[0], full[:, :, 1].transpose(1, 2)).contiguous()
    vc = torch.where(stale, junk[1], full[:, :, 2].transpose(1, 2)).contiguous()
    return qkv, kc, vc, ln


def reference(qkv, kc, vc, ln, scale):
    """float64, from exactly what the kernel is handed: the keys of (b, h) are cache slots 0..p-1 and the new key, p =
    lens[b] clamped.  -> ref [B][H*128], S of attn_decode_ref's docstring, and the cache a correct call leaves"""
    B, H, Tmax, _ = kc.shape
    p = ln.long().clamp(0, Tmax - 1)
    t = torch.arange(Tmax, device=kc.device)
    new, vis = (t[None, :] == p[:, None])[:, None, :, None], (t[None, :] <= p[:, None])[:, None, :]
    q, kn, vn = qkv.view(B, 3, H, HD).unbind(1)
    ka, va = torch.where(new, kn.unsqueeze(2), kc), torch.where(new, vn.unsqueeze(2), vc)
    k = torch.where(vis.unsqueeze(-1), ka, torch.zeros_like(ka)).double()
    v = torch.where(vis.unsqueeze(-1), va, torch.zeros_like(va)).double()
    c = f32(scale) * LOG2E
    s2 = (c * (k @ q.double().unsqueeze(-1)).squeeze(-1)).masked_fill(~vis, float("-inf"))
    aqk = c * (k.abs() @ q.double().abs().unsqueeze(-1)).squeeze(-1)
    M = s2.max(-1, keepdim=True).values
    lse2 = M + torch.log2(torch.exp2(s2 - M).sum(-1, keepdim=True))
    P = torch.exp2(s2 - lse2)
    w = 2.0 + LN2 * (aqk + lse2.abs() + (M - s2).masked_fill(~vis, 0.0))
    wbar = (P * w).sum(-1, keepdim=True)
    O = (P.unsqueeze(-2) @ v).squeeze(-2).reshape(B, H * HD)
    S = ((P * (w + wbar + 1.0)).unsqueeze(-2) @ v.abs()).squeeze(-2).reshape(B, H * HD)
    return O, S, ka, va


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_single_query_against_float64(shape):
    """|got - ref| <= 2^-8 |ref| + C["O"] u S elementwise, and the exact properties, at every lens vector of
    attn_decode_ref.lens_vectors.  Recorded on an MI355X: worst error / bound 0.942, 0.970, 0.945, 0.943 for the four
    shapes (the bf16 result's own rounding alone reaches 2^-8 |ref|)."""
    B, H, Tmax, chunk = shape
    worst = 0.0
    for lens in R.lens_vectors(B, Tmax, chunk):
        qkv, kc, vc, ln = gen(B, H, Tmax, lens)
        q0, k2, v2 = qkv.clone(), kc.clone(), vc.clone()
        out = K.attn_decode(qkv, k2, v2, ln, chunk=chunk)             # scale defaults to 1 / sqrt(128)
        ref, S, ka, va = reference(qkv, kc, vc, ln, SCALE)
        ratio = ((out.double() - ref).abs() / (2.0 ** -8 * ref.abs() + R.C["O"] * U * S)).max().item()
        worst = max(worst, ratio)
        print(f"{shape} lens={lens}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, f"lens={lens}: error / bound {ratio:.3f}"
        assert bits_equal(k2, ka) and bits_equal(v2, va), f"lens={lens}: the cache is not the old one with slot p replaced"
        assert bits_equal(qkv, q0), "qkv changed"
        k3, v3 = kc.clone(), vc.clone()
        assert bits_equal(K.attn_decode(qkv, k3, v3, ln, chunk=chunk), out) and bits_equal(k3, k2), "not repeatable"
        if max(lens) == 0:
            assert bits_equal(out, qkv.view(B, 3, H * HD)[:, 2].contiguous()), "lens = 0: out is not v_new"
    print(f"{shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("shape", SHAPES[1:3], ids=IDS[1:3])
def test_multi_query_is_the_single_query_calls_in_sequence(shape, S):
    """out and both caches, bit for bit, against S attn_decode calls with lens advanced by one between them; the lens
    values put the new keys at the start, across a chunk boundary, at the end of the cache and one past it (lens + S >
    Tmax: the last query lands on slot Tmax - 1 again, as the clamped single-query call does)"""
    B, H, Tmax, chunk = shape
    vals = [0, chunk - S + 1, Tmax - S, Tmax - S + 1]
    for lens in [[v] * B for v in vals] + [[vals[(2 * i + 1) % 4] for i in range(B)]]:
        qkv, kc, vc, ln = gen(B, H, Tmax, lens, S)
        k2, v2 = kc.clone(), vc.clone()
        out = K.attn_decode_multi(qkv, k2, v2, ln, S, chunk=chunk)
        ks, vs, ls, outs = kc.clone(), vc.clone(), ln.clone(), []
        for j in range(S):
            outs.append(K.attn_decode(qkv.view(B, S, -1)[:, j].contiguous(), ks, vs, ls, chunk=chunk))
            ls += 1
        assert torch.equal(out.view(torch.int16), torch.stack(outs, 1).reshape(B * S, -1).view(torch.int16)), f"out, lens={lens}"
        assert torch.equal(k2.view(torch.int16), ks.view(torch.int16)), f"kcache, lens={lens}"
        assert torch.equal(v2.view(torch.int16), vs.view(torch.int16)), f"vcache, lens={lens}"


@pytest.mark.parametrize("T", [1, 127, 128, 200])
def test_kv_cache_fill(T):
    B, H, Tmax = 2, 3, 200
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B * T, 3 * H * HD, generator=g).to(BF).cuda()
    kc, vc = torch.randn(2, B, H, Tmax, HD, generator=g).to(BF).cuda().unbind(0)
    kc, vc = kc.contiguous(), vc.contiguous()
    q0, k0, v0 = qkv.clone(), kc.clone(), vc.clone()
    K.kv_cache_fill(qkv, kc, vc, B, T)
    x = qkv.view(B, T, 3, H, HD)
    assert bits_equal(kc[:, :, :T], x[:, :, 1].transpose(1, 2)) and bits_equal(vc[:, :, :T], x[:, :, 2].transpose(1, 2))
    assert bits_equal(kc[:, :, T:], k0[:, :, T:]) and bits_equal(vc[:, :, T:], v0[:, :, T:]), "slots >= T touched"
    assert bits_equal(qkv, q0)


def test_guards():
    B, H, Tmax = 2, 2, 128
    qkv, kc, vc, ln = gen(B, H, Tmax, [3, 4])
    u8, sc = kc.view(torch.uint8)[..., :HD].contiguous(), torch.ones(B, H, Tmax, device="cuda")
    tq = torch.zeros(B * 64, 3 * H * HD, dtype=BF, device="cuda")
    for bad in (lambda: K.attn_decode(qkv[:, :3 * H * 64].contiguous(), kc, vc, ln),              # a head-dim-64 qkv
                lambda: K.attn_decode(qkv, kc[..., :96].contiguous(), vc[..., :96].contiguous(), ln),
                lambda: K.attn_decode(qkv, kc.transpose(1, 2), vc.transpose(1, 2), ln),           # not contiguous
                lambda: K.kv_cache_fill(qkv[:, :3 * H * 64].contiguous(), kc, vc, B, 1),
                lambda: K.attn_decode_fp8(qkv, u8, u8.clone(), sc, sc.clone(), ln),               # 64 only, all three
                lambda: K.kv_cache_append(tq, kc, vc, ln),
                lambda: K.attn_extend(tq, kc, vc, ln)):
        with pytest.raises(ValueError):
            bad()
    assert K.attn_decode_multi_ws(B, 3, H, Tmax, 64, d=HD) == 3 * K.attn_decode_ws(B, H, Tmax, 64, d=HD) > 0
    from pytorch_distributed_nn_amd.ops._backend import lib, ptr, stream
    part = torch.empty(K.attn_decode_multi_ws(B, 1, H, Tmax, 64, d=HD), device="cuda")
    out = torch.empty(B, H * HD, dtype=BF, device="cuda")
    args = [ptr(qkv), ptr(kc), ptr(vc), ptr(ln), ptr(out), ptr(part)]
    for entry, s in ((lib().pdnn_attn_decode_hd128, ()), (lib().pdnn_attn_decode_multi_hd128, (1,))):
        assert entry(*args, B, *s, H, Tmax, 96, SCALE, stream()) != 0
        assert entry(*args, 0, *s, H, Tmax, 64, SCALE, stream()) != 0
        assert entry(None, *args[1:], B, *s, H, Tmax, 64, SCALE, stream()) != 0
    assert lib().pdnn_kv_cache_fill_hd128(ptr(qkv), ptr(kc), ptr(vc), B, Tmax + 1, H, Tmax, stream()) != 0
    assert lib().pdnn_kv_cache_fill_hd128(ptr(qkv), None, ptr(vc), B, 1, H, Tmax, stream()) != 0
