"""CPU self-check of tests/attn_decode_ref.py: the fp32 model of the decode-attention kernels against the float64
reference on every shape x lens vector x family; its fp32 part (rounding off) against attn_decode_ref.MEASURED; a causal row
sequence through ref_decode against attn_ref.ref_flash_fwd; every planted error caught."""
import functools

import pytest
import torch

import attn_ref as A
import attn_decode_ref as R

SCALE = 0.125
WORST, FP32 = {}, {}
IDS = ["x".join(map(str, s)) for s in R.SHAPES]


@functools.lru_cache(maxsize=None)
def _case(family, shape, lens):
    B, H, Tmax, chunk = shape
    qkv, kc, vc, ln = R.gen_decode(family, B, H, Tmax, list(lens))
    return qkv, kc, vc, ln, R.ref_decode(qkv, kc, vc, ln, SCALE)


def _each(shape):
    B, H, Tmax, chunk = shape
    for lens in R.lens_vectors(B, Tmax, chunk):
        for family in R.FAMILIES:
            yield family, tuple(lens)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_model_passes_the_bound(shape):
    for family, lens in _each(shape):
        qkv, kc, vc, ln, e = _case(family, shape, lens)
        try:
            r = R.check_decode(R.model_decode(qkv, kc, vc, ln, SCALE, shape[3]), e)
        except AssertionError as err:
            raise AssertionError(f"{family} lens={lens}: {err}") from None
        WORST["O"] = max(WORST.get("O", 0.0), r)
    print(f"worst error / bound so far: {WORST}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_fp32_part_is_within_measured(shape):
    """the model with the rounding off: error / (u S) <= MEASURED = C / 4 (the margin left to the GPU's other order)"""
    for family, lens in _each(shape):
        qkv, kc, vc, ln, e = _case(family, shape, lens)
        r = A.fp32_part(R.model_decode(qkv, kc, vc, ln, SCALE, shape[3], rnd=False), e)
        FP32["O"] = max(FP32.get("O", 0.0), r)
        assert r <= R.MEASURED["O"], (family, lens, r)
    assert R.C["O"] == 4.0 * R.MEASURED["O"]
    print(f"fp32 part, worst error / (u S) so far: {FP32}")


def test_inputs_are_what_they_say():
    qkv, kc, vc, ln = R.gen_decode("gauss", 2, 3, 384, [5, 129])
    full = A.gen_flash("gauss", 2, 384, 3)[0]
    q, k, v = A.split_heads(full, 2, 384, 3)
    assert torch.equal(qkv[1], full.view(2, 384, -1)[1, 129]) and ln.dtype == torch.int32
    assert torch.equal(kc[0, :, :5], k[0, :, :5]) and torch.equal(vc[1, :, :129], v[1, :, :129])
    assert bool((kc[0, :, 5:].float().abs() > 2.0 ** 40).all() and torch.isfinite(kc.float()).all())
    ka, va = R.ref_cache_after(qkv, kc, vc, ln)
    assert torch.equal(ka[1, :, 129], k[1, :, 129]) and torch.equal(va[0, :, 5], v[0, :, 5])
    assert torch.equal(ka[:, :, 130:], kc[:, :, 130:]) and torch.equal(ka[0, :, :5], kc[0, :, :5])
    # a malformed lens is clamped, like the kernel's
    assert torch.equal(R.clamp_lens(torch.tensor([-3, 500], dtype=torch.int32), 384), torch.tensor([0, 383]))
    for B, H, Tmax, chunk in R.SHAPES:
        lv = R.lens_vectors(B, Tmax, chunk)
        assert all(len(v) == B and 0 <= min(v) and max(v) <= Tmax - 1 for v in lv)
        assert [0] * B in lv and [Tmax - 1] * B in lv


@pytest.mark.parametrize("family", R.FAMILIES)
def test_row_sequence_is_the_causal_forward(family):
    """query t against keys 0..t for every t at once (sequence t of a batch of T, lens = t, one shared cache) is row t of
    the causal flash forward"""
    T, H = 192, 2
    full = A.gen_flash(family, 1, T, H)[0]
    _, k, v = A.split_heads(full, 1, T, H)
    lens = torch.arange(T, dtype=torch.int32)
    e = R.ref_decode(full, k.expand(T, H, T, A.HD).contiguous(), v.expand(T, H, T, A.HD).contiguous(), lens, SCALE)
    eO, _ = A.ref_flash_fwd(full, 1, T, H, SCALE, True)
    assert torch.allclose(e.ref, eO.ref, rtol=1e-12, atol=1e-300)
    assert bool((e.S >= eO.S).all())            # the decode S extends the forward's


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_planted_errors_break_the_bound(mut):
    caught = []
    for shape in R.SHAPES:
        for family, lens in _each(shape):
            qkv, kc, vc, ln, e = _case(family, shape, lens)
            try:
                R.check_decode(R.model_decode(qkv, kc, vc, ln, SCALE, shape[3], mut=mut), e)
            except AssertionError:
                caught.append((shape, family, lens))
    assert caught, f"{mut}: no shape noticed the planted error"
    print(f"{mut}: caught on {len(caught)} cases")
