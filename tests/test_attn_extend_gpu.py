"""The append + extend kernels (csrc/kernels/attention_extend.hip) on the GPU: per element, over every checked element,
against the float64 reference of tests/attn_extend_ref.py, on every shape x lens vector x family and over NaN slots;
bitwise repeatability, untouched inputs, the exact cache update, the exact properties, malformed lens between guard
slabs, the guards of the wrappers and of the C entries, and graph capture."""
import pytest
import torch

import attn_ref as A
import attn_extend_ref as R

pytestmark = pytest.mark.gpu
SCALE = 0.125
IDS = ["x".join(map(str, s)) for s in R.SHAPES]
WORST = {}


def K():
    from pytorch_distributed_nn_amd.ops import kernels
    return kernels


def _gpu(*ts):
    return tuple(t.cuda() for t in ts)


def _call(qkv, kc, vc, ln):
    """append + extend on copies of the cache -> out, cache after"""
    k2, v2 = kc.clone(), vc.clone()
    K().kv_cache_append(qkv, k2, v2, ln)
    return K().attn_extend(qkv, k2, v2, ln, scale=SCALE), k2, v2


def _each(shape):
    B, H, Tmax, Tq = shape
    for lens in R.lens_vectors(B, Tmax, Tq):
        for family in R.FAMILIES:
            yield family, lens, False
    yield "gauss", R.lens_vectors(B, Tmax, Tq)[-2], True


def test_tile_is_the_reference_modules():
    assert K().EXTEND_TILE == R.TILE


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_extend_against_reference(shape):
    B, H, Tmax, Tq = shape
    for family, lens, nan in _each(shape):
        qkv, kc, vc, ln = _gpu(*R.gen_extend(family, B, H, Tmax, Tq, lens, nan=nan))
        q0, l0 = qkv.clone(), ln.clone()
        ref = R.ref_extend(qkv, kc, vc, ln, SCALE)
        out, k2, v2 = _call(qkv, kc, vc, ln)
        try:
            r = R.check_extend(out, ref, qkv, ln, Tmax)
        except AssertionError as err:
            raise AssertionError(f"{family} lens={lens} nan={nan}: {err}") from None
        WORST["O"] = max(WORST.get("O", 0.0), r)
        out_b, k3, v3 = _call(qkv, kc, vc, ln)
        assert A.bits_equal(out, out_b) and A.bits_equal(k2, k3) and A.bits_equal(v2, v3), "not repeatable bitwise"
        assert A.bits_equal(qkv, q0) and A.bits_equal(ln, l0), "inputs changed"
        ka, va = R.ref_cache_after(qkv, kc, vc, ln)
        assert A.bits_equal(k2, ka) and A.bits_equal(v2, va), \
            f"{family} lens={lens}: cache: only slots lens[b] .. min(lens[b] + Tq, Tmax) - 1 may change, to the new k / v"
        pos = R.positions(ln, Tq, Tmax)
        slot = torch.arange(Tmax, device="cuda")[None, :]
        new = (slot >= pos[:, :1]) & (slot <= pos[:, -1:])
        assert bool((k2 != kc).any(-1).any(1)[new].all()), "the new slots held garbage and must have changed"
    print(f"extend worst error / bound so far: {WORST}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_exact_properties(shape):
    B, H, Tmax, Tq = shape
    lens = R.lens_vectors(B, Tmax, Tq)[-2]                      # the ragged mix
    qkv, kc, vc, ln = _gpu(*R.gen_extend("growing", B, H, Tmax, Tq, lens))
    out, _, _ = _call(qkv, kc, vc, ln)
    # slots past a sequence's last visible key change no output bit (NaN, Inf and plain values)
    past = (torch.arange(Tmax, device="cuda")[None, :] >= ln.long()[:, None] + Tq)[:, None, :, None]
    for fill_k, fill_v in ((float("nan"), float("inf")), (float("-inf"), float("nan")), (3.0, -7.0)):
        k2 = torch.where(past, torch.full_like(kc, fill_k), kc)
        v2 = torch.where(past, torch.full_like(vc, fill_v), vc)
        assert A.bits_equal(_call(qkv, k2, v2, ln)[0], out), f"a slot past the last visible key was read ({fill_k}, {fill_v})"
    # the slots the append overwrites are never read before it
    own = (torch.arange(Tmax, device="cuda")[None, :] >= ln.long()[:, None])[:, None, :, None]
    k2 = torch.where(own, torch.full_like(kc, float("nan")), kc)
    assert A.bits_equal(_call(qkv, k2, vc, ln)[0], out)
    if B > 1:
        k3, v3 = kc.clone(), vc.clone()
        k3[1:], v3[1:] = 1.5, -2.5
        assert A.bits_equal(_call(qkv, k3, v3, ln)[0][:Tq], out[:Tq]), "sequence 0 read another sequence's cache"


@pytest.mark.parametrize("shape", R.SHAPES[1:], ids=IDS[1:])
def test_malformed_lens_stays_inside_the_buffers(shape):
    """lens[b] < 0, = Tmax, = 2^30 raises nothing and touches nothing outside the cache, out and qkv: guard slabs"""
    B, H, Tmax, Tq = shape
    G = 4096
    qkv, kc, vc, _ = _gpu(*R.gen_extend("gauss", B, H, Tmax, Tq, [1] * B))
    n, no, nq = kc.numel(), B * Tq * H * 64, qkv.numel()
    for bad in ([-5] * B, [Tmax] * B, [2 ** 30] * B, [Tmax - 3] + [2 ** 31 - 1] * (B - 1)):
        ln = torch.tensor(bad, dtype=torch.int32, device="cuda")
        slab = torch.full((2 * n + 3 * G,), 3.0, dtype=A.BF, device="cuda")
        kk = slab[G:G + n].view_as(kc)
        vv = slab[2 * G + n:2 * G + 2 * n].view_as(vc)
        kk.copy_(kc)
        vv.copy_(vc)
        oslab = torch.full((no + 2 * G,), 5.0, dtype=A.BF, device="cuda")
        qslab = torch.full((nq + 2 * G,), 7.0, dtype=A.BF, device="cuda")
        qq = qslab[G:G + nq].view_as(qkv)
        qq.copy_(qkv)
        K().kv_cache_append(qq, kk, vv, ln)
        K().attn_extend(qq, kk, vv, ln, out=oslab[G:G + no].view(B * Tq, H * 64), scale=SCALE)
        torch.cuda.synchronize()
        for g in (slab[:G], slab[G + n:2 * G + n], slab[2 * G + 2 * n:]):
            assert bool((g == 3.0).all()), f"lens={bad}: wrote outside the cache"
        assert bool((oslab[:G] == 5.0).all() and (oslab[-G:] == 5.0).all()), f"lens={bad}: wrote outside out"
        assert bool((qslab[:G] == 7.0).all() and (qslab[-G:] == 7.0).all()) and A.bits_equal(qq.contiguous(), qkv)
        # the clamped slots are the only ones written
        ka, va = R.ref_cache_after(qkv, kc, vc, ln)
        assert A.bits_equal(kk.contiguous(), ka) and A.bits_equal(vv.contiguous(), va)


def test_guards():
    B, H, Tmax, Tq = 2, 2, 256, R.TILE
    qkv, kc, vc, ln = _gpu(*R.gen_extend("gauss", B, H, Tmax, Tq, [3, 4]))
    k = K()
    bad = [
        lambda f: f(qkv.float(), kc, vc, ln),
        lambda f: f(qkv, kc.float(), vc, ln),
        lambda f: f(qkv, kc, vc, ln.long()),
        lambda f: f(qkv.t().contiguous().t(), kc, vc, ln),
        lambda f: f(qkv, kc.transpose(1, 2), vc, ln),
        lambda f: f(qkv, kc, vc[:, :, ::2], ln),
        lambda f: f(qkv.cpu(), kc, vc, ln),
        lambda f: f(qkv, kc.cpu(), vc, ln),
        lambda f: f(qkv, kc, vc, ln.cpu()),
        lambda f: f(qkv[:-1], kc, vc, ln),
        lambda f: f(qkv[:B * Tq // 2], kc, vc, ln),                # Tq = half a tile
        lambda f: f(qkv, kc, vc, ln[:1]),
    ]
    for name in ("kv_cache_append", "attn_extend"):
        for i, case in enumerate(bad):
            try:
                case(getattr(k, name))
            except ValueError:
                continue
            pytest.fail(f"{name}: guard {i} did not raise")
    with pytest.raises(ValueError):
        k.attn_extend(qkv, kc, vc, ln, out=torch.empty(B * Tq, H * 64, device="cuda"))
    # the C entry points validate too
    from pytorch_distributed_nn_amd.ops._backend import lib, ptr, stream
    out = torch.empty(B * Tq, H * 64, dtype=A.BF, device="cuda")
    k0, v0 = kc.clone(), vc.clone()
    ap = [ptr(qkv), ptr(kc), ptr(vc), ptr(ln)]
    ex = ap + [ptr(out)]
    assert lib().pdnn_attn_extend_tile() == k.EXTEND_TILE
    for dims in ((0, Tq, H, Tmax), (B, 0, H, Tmax), (B, Tq, 0, Tmax), (B, Tq, H, 0), (B, Tq - 1, H, Tmax),
                 (B, Tq + R.TILE // 2, H, Tmax)):
        assert lib().pdnn_kv_cache_append(*ap, *dims, stream()) != 0, dims
        assert lib().pdnn_attn_extend(*ex, *dims, SCALE, stream()) != 0, dims
    for i in range(4):
        assert lib().pdnn_kv_cache_append(*ap[:i], None, *ap[i + 1:], B, Tq, H, Tmax, stream()) != 0
    for i in range(5):
        assert lib().pdnn_attn_extend(*ex[:i], None, *ex[i + 1:], B, Tq, H, Tmax, SCALE, stream()) != 0
    torch.cuda.synchronize()
    assert A.bits_equal(kc, k0) and A.bits_equal(vc, v0), "a refused call launched"


def test_captured_append_extend_follows_lens():
    """one captured append + extend, lens advanced on the device between three replays: each equals the eager calls
    bitwise, outputs and cache"""
    B, H, Tmax, Tq = 2, 3, 448, R.TILE
    full = A.gen_flash("gauss", B, Tmax, H)[0].cuda().view(B, Tmax, -1)
    start = torch.tensor([1, 190], dtype=torch.int32, device="cuda")
    _, k, v = A.split_heads(full.view(B * Tmax, -1), B, Tmax, H)
    j = torch.arange(Tq, device="cuda")[None, :]

    def fresh():
        return k.contiguous().clone(), v.contiguous().clone(), start.clone()

    def rows(ln):
        return full[torch.arange(B, device="cuda")[:, None], ln.long()[:, None] + j].reshape(B * Tq, -1).contiguous()
    kc, vc, ln = fresh()
    eager = []
    for s in range(3):
        q = rows(ln)
        K().kv_cache_append(q, kc, vc, ln)
        eager.append(K().attn_extend(q, kc, vc, ln, scale=SCALE).clone())
        ln += Tq
    ke, ve = kc, vc
    kc, vc, ln = fresh()
    qs = rows(ln)
    out = torch.empty(B * Tq, H * 64, dtype=A.BF, device="cuda")
    kw, vw = kc.clone(), vc.clone()
    K().kv_cache_append(qs, kw, vw, ln)                          # warm-up on scratch caches
    K().attn_extend(qs, kw, vw, ln, out=out, scale=SCALE)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K().kv_cache_append(qs, kc, vc, ln)
        K().attn_extend(qs, kc, vc, ln, out=out, scale=SCALE)
    for s in range(3):
        qs.copy_(rows(ln))
        graph.replay()
        assert A.bits_equal(out, eager[s]), f"replay {s} differs from the eager calls"
        ln += Tq
    torch.cuda.synchronize()
    assert A.bits_equal(kc, ke) and A.bits_equal(vc, ve)
