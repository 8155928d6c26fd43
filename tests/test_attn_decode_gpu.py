"""The decode-attention kernels (csrc/kernels/attention_decode.hip) on the GPU: per element, over every element, against
the float64 reference of tests/attn_decode_ref.py, on every shape x lens vector x family; bitwise repeatability, untouched
inputs, the exact cache update, the exact properties, sequential consistency with the causal flash forward,
kv_cache_fill, the wrapper's guards and graph capture."""
import pytest
import torch

import attn_ref as A
import attn_decode_ref as R

pytestmark = pytest.mark.gpu
SCALE = 0.125
IDS = ["x".join(map(str, s)) for s in R.SHAPES]
WORST = {}


def K():
    from pytorch_distributed_nn_amd.ops import kernels
    return kernels


def _gpu(*ts):
    return tuple(t.cuda() for t in ts)


def _call(qkv, kc, vc, ln, chunk):
    """one call on copies of the cache -> out, cache after"""
    k2, v2 = kc.clone(), vc.clone()
    out = K().attn_decode(qkv, k2, v2, ln, chunk=chunk)
    return out, k2, v2


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_decode_against_reference(shape):
    B, H, Tmax, chunk = shape
    for lens in R.lens_vectors(B, Tmax, chunk):
        for family in R.FAMILIES:
            qkv, kc, vc, ln = _gpu(*R.gen_decode(family, B, H, Tmax, lens))
            q0, l0 = qkv.clone(), ln.clone()
            e = R.ref_decode(qkv, kc, vc, ln, SCALE)
            out, k2, v2 = _call(qkv, kc, vc, ln, chunk)
            try:
                r = R.check_decode(out, e)
            except AssertionError as err:
                raise AssertionError(f"{family} lens={lens}: {err}") from None
            WORST["O"] = max(WORST.get("O", 0.0), r)
            out_b, k3, v3 = _call(qkv, kc, vc, ln, chunk)
            assert A.bits_equal(out, out_b) and A.bits_equal(k2, k3) and A.bits_equal(v2, v3), "not repeatable bitwise"
            assert A.bits_equal(qkv, q0) and A.bits_equal(ln, l0), "inputs changed"
            ka, va = R.ref_cache_after(qkv, kc, vc, ln)
            assert A.bits_equal(k2, ka) and A.bits_equal(v2, va), "cache: only slot lens[b] may change, to the new k / v"
            p = R.clamp_lens(ln, Tmax)
            at = torch.arange(Tmax, device="cuda")[None, :] == p[:, None]
            assert bool((k2 != kc).any(-1).any(1)[at].all()), "slot lens[b] held garbage and must have changed"
    print(f"decode worst error / bound so far: {WORST}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_exact_properties(shape):
    B, H, Tmax, chunk = shape
    # lens = 0: out is the new v, bitwise
    qkv, kc, vc, ln = _gpu(*R.gen_decode("gauss", B, H, Tmax, [0] * B))
    out, _, _ = _call(qkv, kc, vc, ln, chunk)
    assert A.bits_equal(out.view(B, H, A.HD), R.new_rows(qkv, B, H)[2].contiguous())
    # slots > lens[b] and another sequence's cache change no output bit
    lens = R.lens_vectors(B, Tmax, chunk)[-1]
    qkv, kc, vc, ln = _gpu(*R.gen_decode("growing", B, H, Tmax, lens))
    out, _, _ = _call(qkv, kc, vc, ln, chunk)
    past = (torch.arange(Tmax, device="cuda")[None, :] > ln.long()[:, None])[:, None, :, None]
    k2 = torch.where(past, (kc.float() * -0.5 + 3.0).to(A.BF), kc)
    v2 = torch.where(past, torch.full_like(vc, -7.0), vc)
    assert A.bits_equal(_call(qkv, k2, v2, ln, chunk)[0], out), "a slot past lens[b] was read"
    if B > 1:
        k3, v3 = kc.clone(), vc.clone()
        k3[1:], v3[1:] = 1.5, -2.5
        assert A.bits_equal(_call(qkv, k3, v3, ln, chunk)[0][0], out[0]), "sequence 0 read another sequence's cache"


@pytest.mark.parametrize("shape", R.SHAPES[1:4], ids=IDS[1:4])
def test_malformed_lens_stays_inside_the_cache(shape):
    """lens[b] >= Tmax (and < 0) raises nothing and touches nothing outside the cache: guard regions around every buffer"""
    B, H, Tmax, chunk = shape
    G = 4096
    qkv, kc, vc, _ = _gpu(*R.gen_decode("gauss", B, H, Tmax, [1] * B))
    for bad in ([Tmax] * B, [Tmax + 77] * B, [2 ** 31 - 1] * B, [-5] * B):
        ln = torch.tensor(bad, dtype=torch.int32, device="cuda")
        n = kc.numel()
        slab = torch.full((2 * n + 3 * G,), 3.0, dtype=A.BF, device="cuda")
        kk = slab[G:G + n].view_as(kc)
        vv = slab[2 * G + n:2 * G + 2 * n].view_as(vc)
        kk.copy_(kc)
        vv.copy_(vc)
        oslab = torch.full((B * H * 64 + 2 * G,), 5.0, dtype=A.BF, device="cuda")
        ws = K().attn_decode_ws(B, H, Tmax, chunk)
        pslab = torch.full((ws + 2 * G,), 9.0, dtype=torch.float32, device="cuda")
        K().attn_decode(qkv, kk, vv, ln, chunk=chunk, out=oslab[G:G + B * H * 64].view(B, H * 64), part=pslab[G:G + ws])
        torch.cuda.synchronize()
        for g in (slab[:G], slab[G + n:2 * G + n], slab[2 * G + 2 * n:]):
            assert bool((g == 3.0).all()), f"lens={bad[0]}: wrote outside the cache"
        assert bool((oslab[:G] == 5.0).all() and (oslab[-G:] == 5.0).all())
        assert bool((pslab[:G] == 9.0).all() and (pslab[-G:] == 9.0).all())
        # the clamped slot is the only one written
        ka, va = R.ref_cache_after(qkv, kc, vc, ln)
        assert A.bits_equal(kk.contiguous(), ka) and A.bits_equal(vv.contiguous(), va)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("T,chunk", [(128, 64), (384, 128)])
def test_sequential_decode_is_the_causal_forward(family, T, chunk):
    """decode t = 0..T-1 from an empty cache: every step within the attn_ref causal-forward bound of row t, and the
    final cache is the K and V of qkv bitwise"""
    B, H = 2, 2
    full = A.gen_flash(family, B, T, H)[0].cuda()
    rows = full.view(B, T, -1)
    kc = torch.full((B, H, T, A.HD), float("nan"), dtype=A.BF, device="cuda")
    vc = kc.clone()
    ln = torch.zeros(B, dtype=torch.int32, device="cuda")
    outs = torch.empty(B, T, H * A.HD, dtype=A.BF, device="cuda")
    part = torch.empty(K().attn_decode_ws(B, H, T, chunk), dtype=torch.float32, device="cuda")
    for t in range(T):
        outs[:, t].copy_(K().attn_decode(rows[:, t].contiguous(), kc, vc, ln, chunk=chunk, part=part))
        ln += 1
    eO, _ = A.ref_flash_fwd(full, B, T, H, SCALE, True)
    r = A.check_bf16(outs.view(B * T, -1), eO, A.C["O"], "O")
    _, k, v = A.split_heads(full, B, T, H)
    assert A.bits_equal(kc, k.contiguous()) and A.bits_equal(vc, v.contiguous())
    print(f"sequential {family} T={T}: worst error / causal-forward bound {r:.3f}")


@pytest.mark.parametrize("T", [1, 127, 128, 200])
def test_kv_cache_fill(T):
    B, H, Tmax = 2, 3, 200
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B * T, 3 * H * 64, generator=g).to(A.BF).cuda()
    kc = torch.randn(B, H, Tmax, 64, generator=g).to(A.BF).cuda()
    vc = torch.randn(B, H, Tmax, 64, generator=g).to(A.BF).cuda()
    k0, v0, q0 = kc.clone(), vc.clone(), qkv.clone()
    K().kv_cache_fill(qkv, kc, vc, B, T)
    _, k, v = A.split_heads(qkv, B, T, H)
    assert A.bits_equal(kc[:, :, :T], k) and A.bits_equal(vc[:, :, :T], v)
    assert A.bits_equal(kc[:, :, T:], k0[:, :, T:]) and A.bits_equal(vc[:, :, T:], v0[:, :, T:]), "slots >= T touched"
    assert A.bits_equal(qkv, q0)


def test_guards():
    B, H, Tmax = 2, 2, 128
    qkv, kc, vc, ln = _gpu(*R.gen_decode("gauss", B, H, Tmax, [3, 4]))
    k = K()
    k.attn_decode(qkv, kc.clone(), vc.clone(), ln)           # the default chunk is a valid one
    assert k.DECODE_CHUNK in k.DECODE_CHUNKS
    bad = [
        lambda: k.attn_decode(qkv, kc, vc, ln, chunk=96),
        lambda: k.attn_decode(qkv, kc, vc, ln, chunk=32),
        lambda: k.attn_decode(qkv.float(), kc, vc, ln),
        lambda: k.attn_decode(qkv, kc.float(), vc, ln),
        lambda: k.attn_decode(qkv, kc, vc, ln.long()),
        lambda: k.attn_decode(qkv.t().contiguous().t(), kc, vc, ln),
        lambda: k.attn_decode(qkv, kc.transpose(1, 2), vc, ln),
        lambda: k.attn_decode(qkv, kc, vc[:, :, ::2], ln),
        lambda: k.attn_decode(qkv.cpu(), kc, vc, ln),
        lambda: k.attn_decode(qkv, kc.cpu(), vc, ln),
        lambda: k.attn_decode(qkv, kc, vc, ln.cpu()),
        lambda: k.attn_decode(qkv[:1], kc, vc, ln),
        lambda: k.attn_decode(qkv, kc, vc, ln, out=torch.empty(B, H * 64, device="cuda")),
        lambda: k.attn_decode(qkv, kc, vc, ln, part=torch.empty(4, device="cuda")),
        lambda: k.kv_cache_fill(qkv, kc, vc, B, Tmax + 1),
        lambda: k.kv_cache_fill(qkv, kc, vc, B, 2),
        lambda: k.kv_cache_fill(qkv.float(), kc, vc, B, 1),
        lambda: k.kv_cache_fill(qkv.cpu(), kc, vc, B, 1),
        lambda: k.kv_cache_fill(qkv, kc.transpose(1, 2), vc, B, 1),
    ]
    for i, f in enumerate(bad):
        try:
            f()
        except ValueError:
            continue
        pytest.fail(f"guard {i} did not raise")
    # the C entry points validate too
    from pytorch_distributed_nn_amd.ops._backend import lib, ptr, stream
    part = torch.empty(k.attn_decode_ws(B, H, Tmax, 64), device="cuda")
    out = torch.empty(B, H * 64, dtype=A.BF, device="cuda")
    args = [ptr(qkv), ptr(kc), ptr(vc), ptr(ln), ptr(out), ptr(part)]
    assert lib().pdnn_attn_decode(*args, B, H, Tmax, 96, SCALE, stream()) != 0
    assert lib().pdnn_attn_decode(*args, 0, H, Tmax, 64, SCALE, stream()) != 0
    assert lib().pdnn_attn_decode(None, *args[1:], B, H, Tmax, 64, SCALE, stream()) != 0
    assert lib().pdnn_kv_cache_fill(ptr(qkv), ptr(kc), ptr(vc), B, Tmax + 1, H, Tmax, stream()) != 0
    assert lib().pdnn_kv_cache_fill(ptr(qkv), None, ptr(vc), B, 1, H, Tmax, stream()) != 0


def test_captured_step_follows_lens():
    """one captured attn_decode, lens advanced on the device between three replays: each equals the eager call bitwise"""
    B, H, Tmax, chunk = 2, 3, 384, 128
    full = A.gen_flash("gauss", B, Tmax, H)[0].cuda().view(B, Tmax, -1)
    start = torch.tensor([126, 255], dtype=torch.int32, device="cuda")
    _, k, v = A.split_heads(full.view(B * Tmax, -1), B, Tmax, H)

    def fresh():
        return k.contiguous().clone(), v.contiguous().clone(), start.clone()
    # eager
    kc, vc, ln = fresh()
    eager = []
    for s in range(3):
        q = full[torch.arange(B), ln.long()].contiguous()
        eager.append(K().attn_decode(q, kc, vc, ln, chunk=chunk).clone())
        ln += 1
    ke, ve = kc, vc
    # captured: static qkv in, static out and part
    kc, vc, ln = fresh()
    qs = torch.empty(B, 3 * H * 64, dtype=A.BF, device="cuda")
    out = torch.empty(B, H * 64, dtype=A.BF, device="cuda")
    part = torch.empty(K().attn_decode_ws(B, H, Tmax, chunk), dtype=torch.float32, device="cuda")
    qs.copy_(full[torch.arange(B), ln.long()])
    kw, vw = kc.clone(), vc.clone()
    K().attn_decode(qs, kw, vw, ln, chunk=chunk, out=out, part=part)        # warm-up on scratch caches
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K().attn_decode(qs, kc, vc, ln, chunk=chunk, out=out, part=part)
    for s in range(3):
        qs.copy_(full[torch.arange(B), ln.long()])
        graph.replay()
        assert A.bits_equal(out, eager[s]), f"replay {s} differs from the eager call"
        ln += 1
    torch.cuda.synchronize()
    assert A.bits_equal(kc, ke) and A.bits_equal(vc, ve)
