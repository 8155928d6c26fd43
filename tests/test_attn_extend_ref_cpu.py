"""CPU self-check of tests/attn_extend_ref.py: the fp32 model of the append + extend kernels against the float64 reference
on every shape x lens vector x family (and the NaN variant); its fp32 part (roundings off) against
attn_extend_ref.MEASURED, printed; lens = 0 through ref_extend against attn_ref.ref_flash_fwd; every planted error caught."""
import functools

import pytest
import torch

import attn_ref as A
import attn_extend_ref as R

SCALE = 0.125
WORST, FP32 = {}, {}
IDS = ["x".join(map(str, s)) for s in R.SHAPES]


@functools.lru_cache(maxsize=None)
def _case(family, shape, lens, nan=False):
    B, H, Tmax, Tq = shape
    qkv, kc, vc, ln = R.gen_extend(family, B, H, Tmax, Tq, list(lens), nan=nan)
    return qkv, kc, vc, ln, R.ref_extend(qkv, kc, vc, ln, SCALE)


def _each(shape):
    B, H, Tmax, Tq = shape
    for lens in R.lens_vectors(B, Tmax, Tq):
        for family in R.FAMILIES:
            yield family, tuple(lens), False
    yield "gauss", tuple(R.lens_vectors(B, Tmax, Tq)[-2]), True           # the ragged mix over NaN slots


def _check(shape, family, lens, nan, mut=None):
    qkv, kc, vc, ln, ref = _case(family, shape, lens, nan)
    out, ka, va = R.model_extend(qkv, kc, vc, ln, SCALE, mut=mut)
    want = R.ref_cache_after(qkv, kc, vc, ln)
    assert A.bits_equal(ka, want[0]) and A.bits_equal(va, want[1]), "the cache after the append"
    return R.check_extend(out, ref, qkv, ln, shape[2])


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_model_passes_the_bound(shape):
    for family, lens, nan in _each(shape):
        try:
            r = _check(shape, family, lens, nan)
        except AssertionError as err:
            raise AssertionError(f"{family} lens={lens} nan={nan}: {err}") from None
        WORST["O"] = max(WORST.get("O", 0.0), r)
    print(f"worst error / bound so far: {WORST}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_fp32_part_is_within_measured(shape):
    """the model with the roundings off: error / (u S) <= MEASURED = C / 4 (the margin left to the GPU's other order)"""
    for family, lens, nan in _each(shape):
        qkv, kc, vc, ln, ref = _case(family, shape, lens, nan)
        r = R.fp32_part(R.model_extend(qkv, kc, vc, ln, SCALE, rnd=False)[0], ref)
        FP32["O"] = max(FP32.get("O", 0.0), r)
        assert r <= R.MEASURED["O"], (family, lens, r)
    assert R.C["O"] == 4.0 * R.MEASURED["O"]
    print(f"fp32 part, worst error / (u S) so far: {FP32}")


def test_inputs_are_what_they_say():
    assert R.TILE in (64, 128) and all(s[3] % R.TILE == 0 for s in R.SHAPES)
    qkv, kc, vc, ln = R.gen_extend("gauss", 2, 3, 384, 128, [5, 129])
    full = A.gen_flash("gauss", 2, 384, 3)[0]
    q, k, v = A.split_heads(full, 2, 384, 3)
    assert torch.equal(qkv[128 + 7], full.view(2, 384, -1)[1, 129 + 7]) and ln.dtype == torch.int32
    assert torch.equal(kc[0, :, :5], k[0, :, :5]) and torch.equal(vc[1, :, :129], v[1, :, :129])
    assert bool((kc[0, :, 5:].float().abs() > 2.0 ** 40).all() and torch.isfinite(kc.float()).all())
    ka, va = R.ref_cache_after(qkv, kc, vc, ln)
    assert torch.equal(ka[1, :, 129:257], k[1, :, 129:257]) and torch.equal(va[0, :, 5:133], v[0, :, 5:133])
    assert torch.equal(ka[:, :, 257:], kc[:, :, 257:]) and torch.equal(ka[0, :, :5], kc[0, :, :5])
    assert torch.equal(va[0, :, 133:], vc[0, :, 133:])
    # the NaN variant: NaN exactly in slots >= lens + Tq, of more than one bit pattern
    _, kn, vn, _ = R.gen_extend("gauss", 2, 3, 384, 128, [5, 129], nan=True)
    assert bool(torch.isnan(kn[0, :, 133:].float()).all() and torch.isfinite(kn[0, :, :133].float()).all())
    assert bool(torch.isnan(vn[1, :, 257:].float()).all()) and kn[0, 0, 133].view(torch.int16).unique().numel() == 4
    # a malformed lens is clamped, like the kernels'
    assert torch.equal(R.clamp_lens(torch.tensor([-3, 500], dtype=torch.int32), 384), torch.tensor([0, 384]))
    for B, H, Tmax, Tq in R.SHAPES:
        lv = R.lens_vectors(B, Tmax, Tq)
        assert all(len(v) == B and min(v) >= 0 for v in lv)
        assert all([u] * B in lv for u in (0, 1, 63, 64, 65, Tmax - Tq)) and min(lv[-1]) + Tq > Tmax
        # the overflow vector leaves some rows unchecked and checks the others
        ck = (R.positions(torch.tensor(lv[-1]), Tq, Tmax) < Tmax)
        assert bool(ck.any(1).all()) and not bool(ck.all(1).any())


@pytest.mark.parametrize("family", R.FAMILIES)
def test_lens_zero_is_the_causal_forward(family):
    """Tq new tokens behind an empty cache are the first Tq rows of the causal flash forward"""
    Tq, H, Tmax = 128, 2, 192
    qkv, kc, vc, ln = R.gen_extend(family, 1, H, Tmax, Tq, [0])
    e, checked = R.ref_extend(qkv, kc, vc, ln, SCALE)
    eO, _ = A.ref_flash_fwd(qkv, 1, Tq, H, SCALE, True)
    assert bool(checked.all())
    assert torch.allclose(e.ref, eO.ref, rtol=1e-12, atol=1e-300) and torch.allclose(e.S, eO.S, rtol=1e-12, atol=1e-300)
    assert torch.allclose(e.A, eO.A, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_planted_errors_break_the_bound(mut):
    caught = []
    for shape in R.SHAPES:
        for family, lens, nan in _each(shape):
            try:
                _check(shape, family, lens, nan, mut=mut)
            except AssertionError:
                caught.append((shape, family, lens))
    assert caught, f"{mut}: no case noticed the planted error"
    print(f"{mut}: caught on {len(caught)} cases")
