"""The multi-query decode-attention kernel (csrc/kernels/attention_decode.hip, attn_decode_multi) on the GPU: bit for bit
S successive single-query calls (output and cache), nothing written outside slots lens..lens+S-1, every query within the
single-query bound of the float64 reference of tests/attn_decode_ref.py, repeatable, and safe on a malformed lens."""
import pytest
import torch

import attn_ref as A
import attn_decode_ref as R

pytestmark = pytest.mark.gpu
SCALE = 0.125
S_ALL = (1, 2, 5, 8)
FAMILIES = ("gauss", "growing")
SENT_K, SENT_V = 2.0 ** 60, -(2.0 ** 59)        # slots at or past lens[b]: large, finite, recognisable


def K():
    from pytorch_distributed_nn_amd.ops import kernels
    return kernels


def lens_vectors(B, S, Tmax, chunk):
    """uniform 0, 1, chunk-1, chunk, chunk-S+1 (the S new keys straddle a chunk boundary), Tmax-S, and a ragged mix"""
    vals = [0, 1, chunk - 1, chunk, chunk - S + 1, Tmax - S]
    out = [[v] * B for v in dict.fromkeys(vals)]
    if B > 1:
        out.append([vals[(2 * i + 1) % len(vals)] for i in range(B)])
    return out


_FULL = {}


def _full(family, B, Tmax, H):
    """the seeded problem, generated once and left unchanged"""
    key = (family, B, Tmax, H)
    if key not in _FULL:
        _FULL[key] = A.gen_flash(family, B, Tmax, H)[0]
    return _FULL[key]


def gen(family, B, S, H, Tmax, lens):
    """rows lens[b] .. lens[b]+S-1 of a seeded causal problem are the new tokens, rows before them the cache; every slot
    at or past lens[b] holds the sentinel.  -> qkv [B*S][3*H*64], kcache, vcache, lens (all on the GPU)"""
    full = _full(family, B, Tmax, H)
    p = torch.tensor(lens)
    rows = p[:, None] + torch.arange(S)[None, :]
    qkv = full.view(B, Tmax, -1)[torch.arange(B)[:, None], rows].reshape(B * S, -1).contiguous()
    _, k, v = A.split_heads(full, B, Tmax, H)
    stale = (torch.arange(Tmax)[None, :] >= p[:, None])[:, None, :, None]
    kc = torch.where(stale, torch.full_like(k, SENT_K), k).contiguous()
    vc = torch.where(stale, torch.full_like(v, SENT_V), v).contiguous()
    return qkv.cuda(), kc.cuda(), vc.cuda(), torch.tensor(lens, dtype=torch.int32).cuda()


def sequential(qkv, kc, vc, ln, S, chunk):
    """S single-query calls, lens advanced by one between them -> out [B*S][H*64], cache after"""
    B = kc.shape[0]
    k2, v2, l2 = kc.clone(), vc.clone(), ln.clone()
    rows = qkv.view(B, S, -1)
    outs = []
    for j in range(S):
        outs.append(K().attn_decode(rows[:, j].contiguous(), k2, v2, l2, chunk=chunk))
        l2 += 1
    return torch.stack(outs, 1).reshape(B * S, -1), k2, v2


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("chunk", [64, 128, 256])
def test_multi_against_sequential_and_reference(chunk, H, B):
    Tmax = 2 * chunk + 40
    worst = 0.0
    for S in S_ALL:
        for lens in lens_vectors(B, S, Tmax, chunk):
            for family in FAMILIES:
                qkv, kc, vc, ln = gen(family, B, S, H, Tmax, lens)
                q0, l0 = qkv.clone(), ln.clone()
                k2, v2 = kc.clone(), vc.clone()
                out = K().attn_decode_multi(qkv, k2, v2, ln, S, chunk=chunk)
                what = f"{family} S={S} lens={lens}"
                # (a) bit for bit the S sequential calls, and S = 1 the single-query kernel itself
                so, sk, sv = sequential(qkv, kc, vc, ln, S, chunk)
                assert A.bits_equal(out, so), f"{what}: out differs from {S} sequential attn_decode calls"
                assert A.bits_equal(k2, sk) and A.bits_equal(v2, sv), f"{what}: cache differs from the sequential calls"
                assert A.bits_equal(qkv, q0) and A.bits_equal(ln, l0), f"{what}: inputs changed"
                # (b) only slots lens .. lens+S-1 changed, to the new rows
                pos = torch.arange(Tmax, device="cuda")[None, :] - ln.long()[:, None]
                new = ((pos >= 0) & (pos < S))[:, None, :, None]
                assert A.bits_equal(torch.where(new, kc, k2), kc) and A.bits_equal(torch.where(new, vc, v2), vc), \
                    f"{what}: a slot outside lens..lens+S-1 changed"
                x = qkv.view(B, S, 3, H, A.HD)
                assert A.bits_equal(k2[new.expand_as(k2)].view(B, H, S, A.HD), x[:, :, 1].transpose(1, 2).contiguous())
                assert A.bits_equal(v2[new.expand_as(v2)].view(B, H, S, A.HD), x[:, :, 2].transpose(1, 2).contiguous())
                # (c) every query against the float64 reference, on the cache its predecessors left
                kj, vj = kc, vc
                for j in range(S):
                    qj = qkv.view(B, S, -1)[:, j].contiguous()
                    e = R.ref_decode(qj, kj, vj, ln + j, SCALE)
                    try:
                        worst = max(worst, R.check_decode(out.view(B, S, -1)[:, j].contiguous(), e))
                    except AssertionError as err:
                        raise AssertionError(f"{what} query {j}: {err}") from None
                    kj, vj = R.ref_cache_after(qj, kj, vj, ln + j)
                # repeatable
                k3, v3 = kc.clone(), vc.clone()
                out_b = K().attn_decode_multi(qkv, k3, v3, ln, S, chunk=chunk)
                assert A.bits_equal(out, out_b) and A.bits_equal(k2, k3) and A.bits_equal(v2, v3), f"{what}: not repeatable"
    print(f"multi chunk={chunk} H={H} B={B}: worst error / single-query bound {worst:.3f}")


@pytest.mark.parametrize("S", [2, 8])
def test_malformed_lens_stays_inside_the_buffers(S):
    """lens of -3, Tmax and Tmax + 5: wrong numbers are allowed, a write outside the cache, out or part is not"""
    B, H, chunk = 3, 2, 64
    Tmax = 2 * chunk + 40
    G = 4096
    qkv, kc, vc, _ = gen("gauss", B, S, H, Tmax, [1] * B)
    ln = torch.tensor([-3, Tmax, Tmax + 5], dtype=torch.int32, device="cuda")
    n = kc.numel()
    slab = torch.full((2 * n + 3 * G,), 3.0, dtype=A.BF, device="cuda")
    kk = slab[G:G + n].view_as(kc)
    vv = slab[2 * G + n:2 * G + 2 * n].view_as(vc)
    kk.copy_(kc)
    vv.copy_(vc)
    no = B * S * H * 64
    oslab = torch.full((no + 2 * G,), 5.0, dtype=A.BF, device="cuda")
    ws = K().attn_decode_multi_ws(B, S, H, Tmax, chunk)
    pslab = torch.full((ws + 2 * G,), 9.0, dtype=torch.float32, device="cuda")
    K().attn_decode_multi(qkv, kk, vv, ln, S, chunk=chunk, out=oslab[G:G + no].view(B * S, H * 64), part=pslab[G:G + ws])
    torch.cuda.synchronize()
    for g in (slab[:G], slab[G + n:2 * G + n], slab[2 * G + 2 * n:]):
        assert bool((g == 3.0).all()), "wrote outside the cache"
    assert bool((oslab[:G] == 5.0).all() and (oslab[-G:] == 5.0).all())
    assert bool((pslab[:G] == 9.0).all() and (pslab[-G:] == 9.0).all())


def test_wrapper_guards():
    k = K()
    B, S, H, Tmax = 2, 3, 1, 128
    qkv, kc, vc, ln = gen("gauss", B, S, H, Tmax, [4, 9])
    assert k.attn_decode_multi_ws(B, 1, H, Tmax, 64) == k.attn_decode_ws(B, H, Tmax, 64)
    assert k.attn_decode_multi_ws(B, S, H, Tmax, 64) == S * k.attn_decode_ws(B, H, Tmax, 64)
    for bad in (0, 9, 2.0):
        with pytest.raises(ValueError):
            k.attn_decode_multi(qkv, kc, vc, ln, bad)
    with pytest.raises(ValueError):
        k.attn_decode_multi(qkv[:-1], kc, vc, ln, S)
    with pytest.raises(ValueError):
        k.attn_decode_multi(qkv, kc, vc, ln.long(), S)
    with pytest.raises(ValueError):
        k.attn_decode_multi(qkv, kc, vc, ln, S, chunk=32)
    with pytest.raises(ValueError):
        k.attn_decode_multi(qkv, kc, vc, ln, S, part=torch.empty(8, device="cuda"))
