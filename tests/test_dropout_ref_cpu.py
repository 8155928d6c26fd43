"""CPU self-check of tests/dropout_ref.py: the generator's statistics and purity, the torch generator of the CPU model
path against it, the constants MEASURED / C from the fp32 models, and every planted error caught by the bounds."""
import math

import pytest
import torch

import attn_ref as A
import dropout_ref as R

SC = 0.125


def _sigma(p, n):
    pe = R.p_eff(p)
    return math.sqrt(pe * (1 - pe) / n)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction(p):
    a = R.keep_attn(R.STATE, R.SITE, p, 2, 2, 256)
    r = R.keep_rows(R.STATE, 6, p, 130, 768)
    for m in (a, r, a[0, 0], a[:, :, :, 0::4], a[:, :, :, 3::4]):       # whole masks, one head, one byte of every word
        n = m.numel()
        assert abs(m.double().mean().item() - (1 - R.p_eff(p))) <= 5 * _sigma(p, n), (p, n)
    assert R.p_eff(0.1) == 26 / 256 and R.p_eff(0.5) == 0.5 and R.p_eff(0.996) == 255 / 256 and R.p_eff(0.0) == 0.0


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_masks_that_differ_in_one_coordinate_are_independent(p):
    B, H, T = 2, 2, 256
    base = R.keep_attn(R.STATE, R.SITE, p, B, H, T)
    others = {"seed": R.keep_attn((R.STATE[0] + 1, R.STATE[1]), R.SITE, p, B, H, T),
              "step": R.keep_attn((R.STATE[0], R.STATE[1] + 1), R.SITE, p, B, H, T),
              "site": R.keep_attn(R.STATE, R.SITE + 1, p, B, H, T),
              "head": base.roll(1, 1), "batch": base.roll(1, 0)}
    pe = R.p_eff(p)
    want = pe * pe + (1 - pe) * (1 - pe)
    n = base.numel()
    sig = math.sqrt(want * (1 - want) / n)
    for name, m in others.items():
        agree = (m == base).double().mean().item()
        assert abs(agree - want) <= 5 * sig, (name, agree, want)
    rows = R.keep_rows(R.STATE, 6, p, 130, 768)
    for m in (R.keep_rows((R.STATE[0], R.STATE[1] + 1), 6, p, 130, 768), R.keep_rows(R.STATE, 5, p, 130, 768)):
        agree = (m == rows).double().mean().item()
        assert abs(agree - want) <= 5 * math.sqrt(want * (1 - want) / rows.numel())


def test_mask_is_a_pure_function_of_its_key():
    a = R.keep_attn(R.STATE, R.SITE, 0.1, 3, 2, 128)
    assert torch.equal(a, R.keep_attn(R.STATE, R.SITE, 0.1, 3, 2, 128))
    assert torch.equal(a[:1], R.keep_attn(R.STATE, R.SITE, 0.1, 1, 2, 128))            # stream b * H + h, not the batch size
    # a larger p drops a superset (one threshold on the same bytes)
    assert bool((R.keep_attn(R.STATE, R.SITE, 0.5, 3, 2, 128) <= a).all())
    assert bool(R.keep_rows(R.STATE, 6, 0.0, 3, 72).all())


def test_torch_generator_equals_the_numpy_one():
    from pytorch_distributed_nn_amd.ops import transformer as TX
    for p in R.MASK_PS:
        assert TX.dropout_threshold(p) == R.threshold(p) and TX.dropout_scale(p) == R.scale_of(p)
        for site, state in ((0, R.STATE), (R.SITE_EMBD, (2 ** 63 - 1, 2 ** 40)), (4 * 11 + 2, (0, 0))):
            assert torch.equal(TX.dropout_keep_reference(state, site, p, rows=(3, 72)), R.keep_rows(state, site, p, 3, 72))
            assert torch.equal(TX.dropout_keep_reference(torch.tensor(state), site, p, attn=(3, 2, 128)),
                               R.keep_attn(state, site, p, 3, 2, 128))
    assert TX.SITE_EMBD == R.SITE_EMBD
    for bad in (1.0, -0.01, float("nan")):
        with pytest.raises(ValueError):
            TX.dropout_threshold(bad)


@pytest.fixture(scope="module")
def measured():
    """one pass over every case: the fp32 parts of the models without bf16 roundings, and the checks with them"""
    worst = {m: {k: 0.0 for k in R.MEASURED[m]} for m in R.MEASURED}
    ratios = {}
    for fam, (B, T, H), p, lay in R.cases():
        mode = "doc" if lay else "plain"
        qkv, dO = A.gen_flash(fam, B, T, H)
        doc = R.doc_of(lay, B, T)
        keep = R.keep_attn(R.STATE, R.SITE, p, B, H, T)
        ref = R.ref_drop_fwd(qkv, keep, p, B, T, H, SC, doc)
        O, l2 = R.model_drop_fwd(qkv, keep, p, B, T, H, SC, doc, rnd=False)
        mag = (ref[1].bound - A.U * ref[1].ref.abs()) / (R.C[mode]["lse2"] * A.U)
        r = {"O": A.fp32_part(O, ref[0]),
             "lse2": (((l2.double() - ref[1].ref).abs() - A.U * ref[1].ref.abs()).clamp_min(0) / (A.U * mag)).max().item()}
        Og, lg = ref[0].ref.to(A.BF).contiguous(), ref[1].ref.float().contiguous()
        rb = R.ref_drop_bwd(qkv, Og, dO, lg, keep, p, B, T, H, SC, doc)
        d = A.dqkv_parts(R.model_drop_bwd(qkv, Og, dO, lg, keep, p, B, T, H, SC, doc, rnd=False), B, T, H)
        r.update({n: A.fp32_part(d[n], rb[n]) for n in ("dQ", "dK", "dV")})
        for k, v in r.items():
            worst[mode][k] = max(worst[mode][k], v)
        # the models with their bf16 roundings pass the checks the kernels are held to
        O, l2 = R.model_drop_fwd(qkv, keep, p, B, T, H, SC, doc)
        got = R.check_drop_fwd(O, l2, ref, doc)
        got.update(R.check_drop_bwd(R.model_drop_bwd(qkv, Og, dO, lg, keep, p, B, T, H, SC, doc), rb, B, T, H, doc))
        for k, v in got.items():
            ratios[k] = max(ratios.get(k, 0.0), v)
    return worst, ratios


def test_constants_are_four_times_the_measured_fp32_error(measured):
    worst, ratios = measured
    print("fp32 parts:", worst, "\nworst error / bound with bf16 roundings:", ratios)
    for mode in R.MEASURED:
        for k, v in R.MEASURED[mode].items():
            assert worst[mode][k] <= v, (mode, k, worst[mode][k])
            assert v <= 1.25 * worst[mode][k] + 0.1, (mode, k, "MEASURED is not the measurement", worst[mode][k])
            assert R.C[mode][k] == 4.0 * v
    assert all(v <= 1.0 for v in ratios.values())


def _caught(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mut", R.FWD_MUTS)
def test_planted_forward_errors_exceed_the_bound(mut):
    hit = []
    for (B, T, H), lay in [((3, 128, 2), None), ((1, 256, 3), "off_edges")]:
        qkv, _ = A.gen_flash("gauss", B, T, H)
        doc = R.doc_of(lay, B, T)
        keep = R.keep_attn(R.STATE, R.SITE, 0.1, B, H, T)
        ref = R.ref_drop_fwd(qkv, keep, 0.1, B, T, H, SC, doc)
        R.check_drop_fwd(*R.model_drop_fwd(qkv, keep, 0.1, B, T, H, SC, doc), ref, doc)               # unplanted: passes
        O, l2 = R.model_drop_fwd(qkv, keep, 0.1, B, T, H, SC, doc, mut=mut)
        hit.append(_caught(lambda: R.check_drop_fwd(O, l2, ref, doc)))
    assert any(hit), mut


@pytest.mark.parametrize("mut", R.BWD_MUTS)
def test_planted_backward_errors_exceed_the_bound(mut):
    hit = []
    for (B, T, H), lay in [((3, 128, 2), None), ((1, 256, 3), "off_edges")]:
        qkv, dO = A.gen_flash("gauss", B, T, H)
        doc = R.doc_of(lay, B, T)
        keep = R.keep_attn(R.STATE, R.SITE, 0.1, B, H, T)
        Og, lg = R.drop_forward_given(qkv, keep, 0.1, B, T, H, SC, doc)
        ref = R.ref_drop_bwd(qkv, Og, dO, lg, keep, 0.1, B, T, H, SC, doc)
        R.check_drop_bwd(R.model_drop_bwd(qkv, Og, dO, lg, keep, 0.1, B, T, H, SC, doc), ref, B, T, H, doc)
        k2, O2 = keep, Og
        if mut == "next_step":
            k2 = R.keep_attn((R.STATE[0], R.STATE[1] + 1), R.SITE, 0.1, B, H, T)
        if mut == "delta_undropped":      # delta = rowsum(dO o O) from the O of the forward without dropout
            O2 = R.drop_forward_given(qkv, torch.ones_like(keep), 0.0, B, T, H, SC, doc)[0]
        dqkv = R.model_drop_bwd(qkv, O2, dO, lg, k2, 0.1, B, T, H, SC, doc, mut=mut)
        hit.append(_caught(lambda: R.check_drop_bwd(dqkv, ref, B, T, H, doc)))
    assert any(hit), mut


def test_rows_reference():
    x = torch.tensor([[1.0, -2.0, 3.0, 0.5, 1.0, 1.0, 1.0, 1.0]]).to(A.BF)
    keep = R.keep_rows(R.STATE, 6, 0.5, 1, 8)
    ref, bound = R.ref_rows(x, x, keep, 0.5)
    assert torch.equal(ref, x.double() + keep.double() * x.double() * 2.0) and bool((bound > 0).all())
