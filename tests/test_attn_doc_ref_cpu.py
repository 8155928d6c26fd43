"""CPU self-check of tests/attn_doc_ref.py: the fp32 models of the packed-document flash kernels against the float64
reference on every layout x shape x family; their fp32 parts (bf16 roundings off) against attn_doc_ref.MEASURED; every
planted error caught; the semantics of the document bounds on the CPU mirror of the bounds kernel."""
import functools

import pytest
import torch

import attn_ref as A
import attn_doc_ref as R

SCALE = 0.125
CASES = [(lay, shape) for lay in R.LAYOUTS for shape in R.SHAPES]
WORST, FP32 = {}, {}


@functools.lru_cache(maxsize=None)
def _case(family, layout, shape):
    B, T, H = shape
    qkv, dO = R.gen_doc(family, B, T, H, SCALE)
    ds, de = R.layout_bounds(layout, B, T)
    fwd = R.ref_doc_fwd(qkv, ds, de, B, T, H, SCALE)
    Og, lg = fwd[0].ref.to(A.BF).contiguous(), fwd[1].ref.float().contiguous()
    bwd = R.ref_doc_bwd(qkv, Og, dO, lg, ds, de, B, T, H, SCALE)
    return qkv, dO, ds, de, fwd, Og, lg, bwd


def _run(family, layout, shape, mut=None, nf=2):
    """both models with roundings against the reference -> ratios; raises AssertionError on a miss"""
    B, T, H = shape
    qkv, dO, ds, de, fwd, Og, lg, bwd = _case(family, layout, shape)
    O, lse2 = R.model_doc_fwd(qkv, ds, de, B, T, H, SCALE, mut=mut)
    r = R.check_doc_fwd(qkv, O, lse2, ds, de, B, T, H, SCALE, ref=fwd)
    dqkv = R.model_doc_bwd(qkv, Og, dO, lg, ds, de, B, T, H, SCALE, mut=mut, nf=nf)
    r.update(R.check_doc_bwd(qkv, Og, dO, lg, dqkv, ds, de, B, T, H, SCALE, ref=bwd))
    return r


def test_layouts_are_what_they_say():
    assert R.layout_starts("one", 256) == [0]
    assert R.layout_starts("unit", 128) == list(range(128))
    assert R.layout_starts("tile_edges", 256) == [0, 64, 128, 192]
    assert R.layout_starts("off_edges", 128) == [0, 63, 65, 127]           # 129 is past T: dropped
    assert R.layout_starts("skip_lead", 128) == [0]
    assert R.layout_starts("last_token", 384) == [0, 383]
    ds, de = R.layout_bounds("late_in_wave", 3, 128)
    assert ds[0, 99] == 60 and ds[0, 100] == 100 and de[0, 59] == 60 and de[0, 127] == 128
    assert not torch.equal(ds[0], ds[1]) and not torch.equal(ds[1], ds[2])  # sequences of a batch differ
    for lay in R.LAYOUTS:
        ds, de = R.layout_bounds(lay, 2, 384)
        t = torch.arange(384)[None, :]
        assert ds.dtype == torch.int32 and bool((ds <= t).all() and (t < de).all())
        assert bool((ds[:, 1:] >= ds[:, :-1]).all() and (de[:, 1:] >= de[:, :-1]).all())


@pytest.mark.parametrize("layout,shape", CASES, ids=[f"{lay}-{'x'.join(map(str, s))}" for lay, s in CASES])
def test_models_pass_the_bounds(layout, shape):
    for family in R.FAMILIES:
        for nf in (1, 2):
            try:
                r = _run(family, layout, shape, nf=nf)
            except AssertionError as e:
                raise AssertionError(f"{family}, NF={nf}: {e}") from None
            for n, v in r.items():
                WORST[n] = max(WORST.get(n, 0.0), v)
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("layout,shape", CASES, ids=[f"{lay}-{'x'.join(map(str, s))}" for lay, s in CASES])
def test_fp32_parts_within_measured(layout, shape):
    """bf16 roundings off: worst error / (u S) of the DOC models stays within attn_doc_ref.MEASURED (its own record,
    above attn_ref's on far_masked_before; attn_ref's constants are not touched)"""
    B, T, H = shape
    for family in R.FAMILIES:
        qkv, dO, ds, de, fwd, Og, lg, bwd = _case(family, layout, shape)
        O, lse2 = R.model_doc_fwd(qkv, ds, de, B, T, H, SCALE, rnd=False)
        got = {"O": A.fp32_part(O, fwd[0]),
               "lse2": (((lse2.double() - fwd[1].ref).abs() - A.U * fwd[1].ref.abs()).clamp_min(0.0)
                        / ((fwd[1].bound - A.U * fwd[1].ref.abs()) / R.C["lse2"])).max().item()}
        for nf in (1, 2):
            parts = A.dqkv_parts(R.model_doc_bwd(qkv, Og, dO, lg, ds, de, B, T, H, SCALE, rnd=False, nf=nf), B, T, H)
            for n in ("dQ", "dK", "dV"):
                got[n] = max(got.get(n, 0.0), A.fp32_part(parts[n], bwd[n]))
        for n, v in got.items():
            FP32[n] = max(FP32.get(n, 0.0), v)
            assert v <= R.MEASURED[n], (family, n, v, R.MEASURED[n])
    print("worst fp32 error / (u S) so far: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(FP32.items())))


# where each planted error is looked for first (any layout x shape may catch it; these do)
_WHERE = {"start_off_by_one": [("off_edges", (1, 256, 3))], "end_off_by_one": [("off_edges", (1, 256, 3))],
          "block_start_for_all_waves": [("late_in_wave", (1, 128, 1))], "lead_tile_skipped": [("off_edges", (1, 256, 3))],
          "edge_unmasked": [("many_in_wave", (1, 256, 3))], "no_inf_guard": [("late_in_wave", (1, 128, 1))],
          "bounds_of_batch0": [("one", (3, 128, 2))]}


@pytest.mark.parametrize("mut", R.MUTS)
def test_planted_errors_are_caught(mut):
    assert set(_WHERE) == set(R.MUTS)
    caught = []
    for layout, shape in _WHERE[mut] + CASES:
        for family in ("gauss", "far_masked_before"):
            try:
                _run(family, layout, shape, mut=mut)
            except AssertionError as e:
                caught.append((layout, shape, family, str(e)[:80]))
        if caught:
            break
    assert caught, f"{mut}: no case caught it"
    print(mut, "caught by", caught[0])


def test_no_inf_guard_is_the_nan_of_the_issue():
    """late_in_wave: query 100's first key tile is fully masked; from m = -inf that tile gives NaN, from the floor not"""
    B, T, H = 1, 128, 1
    qkv, dO, ds, de, *_ = _case("gauss", "late_in_wave", (B, T, H))
    O, lse2 = R.model_doc_fwd(qkv, ds, de, B, T, H, SCALE, mut="no_inf_guard")
    assert torch.isnan(O.float()[100]).all() and torch.isnan(lse2[0, 0, 100])
    O, lse2 = R.model_doc_fwd(qkv, ds, de, B, T, H, SCALE)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse2).all()


def test_far_masked_before_overflows_before_the_mask():
    """the family does what it is for: P of a key before the document start is inf in fp32 until the mask zeroes it"""
    B, T, H = 1, 256, 3
    qkv, dO, ds, de, fwd, Og, lg, bwd = _case("far_masked_before", "tile_edges", (B, T, H))
    q, k, v = (t.float() for t in A.split_heads(qkv, B, T, H))
    c = A.f32(SCALE) * A.LOG2E
    p = torch.exp2(((q @ k.transpose(-1, -2)).double() * c - lg.double().unsqueeze(-1)).float())
    assert torch.isinf(p[0, 0, 200, 0]) and torch.isfinite(p[0, 0, 200, 192:201]).all()


def test_doc_bounds_semantics():
    E = 7
    T = 12
    rows = {"none": [1] * T, "at0": [E] + [1] * (T - 1), "at_end": [1] * (T - 1) + [E], "adjacent": [1] * 5 + [E, E] + [1] * 5}
    idx = torch.tensor(list(rows.values()), dtype=torch.int64)
    ds, de = R.bounds_from_tokens(idx, E)
    n = list(rows).index
    assert ds[n("none")].tolist() == [0] * T and de[n("none")].tolist() == [T] * T
    assert ds[n("at0")].tolist() == [0] + [1] * (T - 1) and de[n("at0")].tolist() == [1] + [T] * (T - 1)
    assert ds[n("at_end")].tolist() == [0] * T and de[n("at_end")].tolist() == [T] * T   # the EOT belongs to the document it ends
    assert ds[n("adjacent")].tolist() == [0] * 6 + [6] + [7] * 5                          # the second EOT is a document of one
    assert de[n("adjacent")].tolist() == [6] * 6 + [7] + [T] * 5
    # the same through the layouts: an EOT at start - 1 of every document reproduces the layout's bounds
    for lay in R.LAYOUTS:
        st = R.layout_starts(lay, 128)
        tok = torch.ones(1, 128, dtype=torch.int64)
        tok[0, [s - 1 for s in st if s > 0]] = E
        want = R.bounds_of_starts(st, 128)
        got = R.bounds_from_tokens(tok, E)
        assert torch.equal(got[0][0], want[0]) and torch.equal(got[1][0], want[1]), lay
