"""The fp8 key/value cache kernels (csrc/kernels/attention_cache_fp8.hip) on the GPU.  Fill / append: codes and scales
bitwise quantize_rows_reference.  Decode: attn_decode_ref's float64 reference and bound, unchanged, on the dequantised
cache and the round-tripped new k / v (the kernel's operands are exactly those values, and a power-of-two scale adds no
rounding).  Multi: bitwise S single-query calls.  Extend: bitwise attn_extend on the dequantised bf16 cache.  Slots no
query may see hold code 0x7F (NaN) and scale NaN throughout.
Recorded on an MI355X: decode worst error / bound 0.984 (the bf16 kernels: attn_decode_ref.RECORDED_GPU, 0.987)."""
import pytest
import torch

import attn_decode_ref as R
import attn_extend_ref as X
import attn_ref as A
from pytorch_distributed_nn_amd.ops.quant import dequantize_rows, quantize_rows_reference

pytestmark = pytest.mark.gpu
SCALE = 0.125


def K():
    from pytorch_distributed_nn_amd.ops import kernels
    return kernels


def quant(t):
    """[..., 64] -> (codes uint8 [..., 64], scales fp32 [...]) by the reference rule, computed on the CPU, on t's device"""
    q, inv = quantize_rows_reference(t.reshape(-1, 64).cpu())
    return q.view(t.shape).to(t.device), inv.view(t.shape[:-1]).to(t.device)


def rt(t):
    q, s = quant(t)
    return dequantize_rows(q.reshape(-1, 64).cpu(), s.reshape(-1).cpu()).view(t.shape).to(t.device)


def fp8_cache(kc, vc, lens):
    """bf16 caches [B][H][Tmax][64] -> [kq, vq, ks, vs] on the GPU: rows < lens[b] quantised, every other slot 0x7F / NaN"""
    stale = (torch.arange(kc.shape[2])[None, :] >= lens.long().cpu()[:, None])[:, None, :].to(kc.device)
    (kq, ks), (vq, vs) = quant(kc), quant(vc)
    codes = [torch.where(stale[..., None], torch.full_like(q, 0x7F), q).cuda() for q in (kq, vq)]
    return codes + [torch.where(stale, torch.full_like(s, float("nan")), s).cuda() for s in (ks, vs)]


def same(got, want, what):
    for g, w, name in zip(got, want, ("k codes", "v codes", "k scales", "v scales")):
        assert A.bits_equal(g, w), f"{what}: {name} differ"


def stored(cache, qkv, B, Tq, H, start):
    """``cache`` [kq, vq, ks, vs] with row b*Tq + j of qkv quantised into slot start[b] + j where that is < Tmax"""
    out = [t.clone() for t in cache]
    x = qkv.view(B, Tq, 3, H, 64)
    for b in range(B):
        n = max(0, min(Tq, out[0].shape[2] - start[b]))
        for i in (0, 1):
            q, s = quant(x[b, :n, 1 + i].transpose(0, 1))
            out[i][b, :, start[b]:start[b] + n], out[2 + i][b, :, start[b]:start[b] + n] = q, s
    return out


@pytest.mark.parametrize("B,H,T,Tmax,lens", [(1, 1, 128, 128, None), (2, 3, 128, 320, None), (1, 1, 64, 128, [100]),
                                             (2, 3, 64, 320, [0, 255]), (2, 3, 64, 320, [300, 7])])
def test_fill_and_append_are_the_reference_bitwise(B, H, T, Tmax, lens):
    """lens None: kv_cache_fill_fp8 of T rows; else kv_cache_append_fp8 of T = 64 rows at ragged lens, one running past Tmax"""
    qkv = torch.randn(B * T, 3 * H * 64, generator=torch.Generator().manual_seed(T + Tmax)).to(A.BF)
    k0, v0 = qkv.view(B * T, 3, H, 64)[:, 1, 0], qkv.view(B * T, 3, H, 64)[:, 2, 0]         # planted rows, head 0
    k0[0] = 0.0
    k0[1:3] *= 2.0 ** -4                                         # |x| < 1: the planted element below is the row's amax,
    v0[1:3] *= 2.0 ** -4                                         # in the first or the last lane of the row's group
    k0[1, 5], k0[2, 63] = 1.75, -1.7578125                       # amax mantissa exactly 0.875, and the next bf16 above it
    v0[1, 63], v0[2, 5] = -1.75, 1.7578125
    assert [t.abs().max().item() for t in (k0[1], k0[2], v0[1], v0[2])] == [1.75, 1.7578125, 1.75, 1.7578125]
    k0[3] *= 1e30
    k0[4] *= 1e-30
    qkv = qkv.cuda()
    before = [torch.full((B, H, Tmax, 64), 0x55, dtype=torch.uint8, device="cuda") for _ in range(2)] + \
             [torch.full((B, H, Tmax), 7.0, device="cuda") for _ in range(2)]
    got = [t.clone() for t in before]
    if lens is None:
        K().kv_cache_fill_fp8(qkv, *got, B, T)
    else:
        K().kv_cache_append_fp8(qkv, *got, torch.tensor(lens, dtype=torch.int32, device="cuda"))
    same(got, stored(before, qkv, B, T, H, lens or [0] * B), f"lens={lens}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_decode_against_reference(shape):
    B, H, Tmax, chunk = shape
    worst = 0.0
    for lens in R.lens_vectors(B, Tmax, chunk):
        for family in R.FAMILIES:
            qkv, kc, vc, ln = (t.cuda() for t in R.gen_decode(family, B, H, Tmax, lens))
            cache = fp8_cache(kc, vc, ln)
            q2 = qkv.clone().view(B, 3, H, 64)
            q2[:, 1:] = rt(q2[:, 1:])
            ref = R.ref_decode(q2.view(B, -1), rt(kc), rt(vc), ln, SCALE)
            q0, l0 = qkv.clone(), ln.clone()
            got = [t.clone() for t in cache]
            out = K().attn_decode_fp8(qkv, *got, ln, chunk=chunk, scale=SCALE)
            try:
                worst = max(worst, R.check_decode(out, ref))
            except AssertionError as err:
                raise AssertionError(f"{family} lens={lens}: {err}") from None
            again = [t.clone() for t in cache]
            assert A.bits_equal(K().attn_decode_fp8(qkv, *again, ln, chunk=chunk, scale=SCALE), out), "not repeatable"
            assert A.bits_equal(qkv, q0) and A.bits_equal(ln, l0), "inputs changed"
            same(got, stored(cache, qkv, B, 1, H, R.clamp_lens(ln, Tmax).tolist()), f"{family} lens={lens}")
    print(f"decode fp8 {shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("amax", [1.75, 1.7578125])
def test_decode_quantises_the_new_token_at_the_exponent_boundary(amax):
    """the new k and v rows' amax has mantissa exactly 0.875, or is the next bf16 above it, in one lane of the key's four"""
    B, H, Tmax, chunk = 1, 2, 128, 64
    qkv, kc, vc, ln = (t.cuda() for t in R.gen_decode("gauss", B, H, Tmax, [70]))
    new = qkv.view(B, 3, H, 64)[:, 1:]
    new *= 2.0 ** -4
    new[:, 0, :, 5], new[:, 1, :, 63] = amax, -amax
    assert bool((new.abs().amax(-1) == amax).all())
    cache = fp8_cache(kc, vc, ln)
    got = [t.clone() for t in cache]
    K().attn_decode_fp8(qkv, *got, ln, chunk=chunk, scale=SCALE)
    same(got, stored(cache, qkv, B, 1, H, [70]), f"amax={amax}")


@pytest.mark.parametrize("Tmax", [384, 320])                     # 320: the last chunk of 128 reaches past Tmax
@pytest.mark.parametrize("S", [2, 5, 8])
def test_multi_is_bitwise_the_single_query_calls(S, Tmax):
    B, H, chunk = 2, 3, 128
    lens = [chunk - 2, Tmax - 3]                                 # across a chunk boundary, and past the cache's end
    full = A.gen_flash("gauss", B, Tmax, H)[0].cuda()
    _, kc, vc = A.split_heads(full, B, Tmax, H)
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    cache = fp8_cache(kc.contiguous(), vc.contiguous(), ln)
    pos = (ln.long()[:, None] + torch.arange(S, device="cuda")[None, :]).clamp(max=Tmax - 1)
    qkv = full.view(B, Tmax, -1)[torch.arange(B, device="cuda")[:, None], pos].contiguous()        # [B][S][3*H*64]
    multi = [t.clone() for t in cache]
    out = K().attn_decode_multi_fp8(qkv.view(B * S, -1), *multi, ln, S, chunk=chunk, scale=SCALE).view(B, S, -1)
    single, snaps, outs = [t.clone() for t in cache], [], []
    for j in range(S):                                           # a row that has reached Tmax overwrites its last slot:
        outs.append(K().attn_decode_fp8(qkv[:, j].contiguous(), *single, ln + j, chunk=chunk, scale=SCALE))
        snaps.append([t.clone() for t in single])                # it is compared up to its last call inside the cache
    for b in range(B):
        n = min(S, Tmax - lens[b])
        assert A.bits_equal(out[b, :n], torch.stack(outs, 1)[b, :n]), f"row {b}: output"
        same([t[b] for t in multi], [t[b] for t in snaps[n - 1]], f"row {b}")


@pytest.mark.parametrize("Tq", [64, 128])
@pytest.mark.parametrize("l0", [0, 1, 63, 64, 65, -1])
def test_extend_is_bitwise_the_bf16_kernel_on_the_dequantised_cache(Tq, l0):
    B, H, Tmax = 2, 2, 320
    lens = [Tmax - Tq if l0 < 0 else l0, 65 if l0 in (0, -1) else 0]         # ragged
    qkv, kc, vc, ln = (t.cuda() for t in X.gen_extend("gauss", B, H, Tmax, Tq, lens))
    cache = fp8_cache(kc, vc, ln)
    K().kv_cache_append_fp8(qkv, *cache, ln)
    out = K().attn_extend_fp8(qkv, *cache, ln, scale=SCALE)
    q2 = qkv.clone().view(B * Tq, 3, H, 64)
    q2[:, 1:] = rt(q2[:, 1:])
    q2 = q2.view(B * Tq, -1)
    kd, vd = rt(kc), rt(vc)
    K().kv_cache_append(q2, kd, vd, ln)
    assert A.bits_equal(out, K().attn_extend(q2, kd, vd, ln, scale=SCALE))
