"""CPU self-check of tests/gemm_skinny_ref.py: the fp32 model of the skinny-M GEMM's own summation order stays inside
every bound on every case test_gemm_skinny_gpu.py runs (the integer family exactly), its fp32 part is below the constant
gemm_ref measured for the other engines (so that constant is used unchanged, capped by K + 3), the mirrored partition of
K has the properties the kernel relies on, and each planted error leaves the bounds on at least one case of the GPU list.
If the model left a bound, the bound (not the kernel) would be wrong; if a planted error passed, the cases would be too
weak."""
import functools

import pytest
import torch

import gemm_ref as A
import gemm_skinny_ref as S

WORST = {}
FP32 = {}
CASES = S.cases()
BY_ID = {cid: (args, opt) for cid, args, opt in CASES}
ALL_SHAPES = S.SHAPES + S.BIG


def _note(name, ratio, table=WORST, label="worst error / bound so far"):
    table[name] = max(table.get(name, 0.0), ratio)
    print(f"{label}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(table.items())))
    return ratio


@functools.lru_cache(maxsize=None)
def _case(cid):
    c = S.build(*BY_ID[cid])
    return c, S.reference(c)


def test_partition_covers_k_once_and_depends_on_n_k_only():
    for M, N, K in ALL_SHAPES + [(1, 2304, 768), (1, 768, 768), (1, 3072, 768), (1, 768, 3072), (1, 50304, 768)]:
        nw, sl = S.partition(N, K)
        r = S.slices(N, K)
        assert nw in S.WAVES and sl % S.UNIT == 0 and len(r) == nw
        assert r[0][0] == 0 and max(k1 for _, k1 in r) == K and all(r[i][1] == r[i + 1][0] for i in range(nw - 1))
        assert all(k0 % S.UNIT == 0 or k0 == K for k0, _ in r)           # a slice starts on a unit: only its end is ragged
        covered = sorted(int(i) for k0, k1 in r for u in range(k0, k1, S.UNIT) for h in (0, 1)
                         for i in S._mfma_idx(u, h) if i < k1)
        assert covered == list(range(K))
    assert [S.partition(N, K) for N, K in ((2304, 768), (768, 768), (3072, 768), (768, 3072), (50304, 768))] == \
        [(12, 64), (12, 64), (6, 128), (12, 256), (4, 192)]


def test_case_list_covers_what_it_claims():
    assert len(BY_ID) == len(CASES) == 2 * len(S.VARIANTS) * len(ALL_SHAPES)
    shapes = set(ALL_SHAPES)
    assert {m for m, _, _ in shapes} >= {1, 2, 15, 16, 17, 31, 32, 33, 63, 64}
    assert {n for _, n, _ in shapes} >= {8, 16, 24, 40, 136} and {k for _, _, k in shapes} >= set(S.KS)
    assert set(S.KS) >= {8, 32, 72, 136, 520}
    for b in (S.UNIT, 128, 256, 384, 768):                               # a piece either side of unit, step and slice edges
        assert {b - 8, b, b + 8} <= set(S.KS), b
    assert {S.partition(N, K)[0] for _, N, K in shapes} == set(S.WAVES)
    assert any(len([1 for k0, k1 in S.slices(N, K) if k1 == k0]) for _, N, K in shapes)        # an empty wave
    assert any(N % 16 == 8 and -(-N // 16) * 4 >= S.MIN_WAVES for _, N, _ in shapes)
    fams = {(args[1], name.split("-")[0]) for name, args, _ in CASES}
    assert {f for f, _ in fams} == set(A.FAMILIES)
    for M, N, K in shapes:
        assert 1 <= M <= S.MAX_M and K % 8 == 0 and N % 8 == 0 and 16 * K < 2 ** 24


def test_constant_is_gemm_refs_and_below_the_ceiling():
    for K in sorted({k for _, _, k in ALL_SHAPES}):
        assert A.acc_const("acc", K) < K + 4
        assert A.acc_const("acc", K) == A.C["acc"] or K < A.C["acc"]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_meets_every_bound(shape):
    for cid, args, _ in S.cases([shape]):
        c, ref = _case(cid)
        try:
            for n, r in S.check(c, S.model_skinny(c), ref).items():
                _note(n, r)
        except AssertionError as e:
            raise AssertionError(f"{cid}: {e}") from None
        if c.act == 0:
            part = A.fp32_part(S.model_skinny(c, rnd=False)["y"], ref["y"])
            _note("acc", part, FP32, "fp32 part, worst error / (u S) so far")
            # the constant of the bound stays gemm_ref's: this kernel's order is no worse than the ones measured there
            assert part <= A.MEASURED["acc"], (cid, part)


@pytest.mark.parametrize("mut", S.MUTATIONS)
def test_every_planted_error_is_rejected(mut):
    caught = []
    for cid, args, opt in CASES:
        M, N, K = args[2:5]
        if (M, N, K) in S.BIG and mut not in ("wave_slice_skipped", "wave_slice_twice"):
            continue                                                      # the small shapes decide; the big ones are slow
        c, ref = _case(cid)
        try:
            S.check(c, S.model_skinny(c, mut), ref)
        except AssertionError:
            caught.append(cid)
    print(f"{mut}: rejected on {len(caught)} of {len(CASES)} cases, e.g. {caught[:3]}")
    assert caught, f"planted error {mut} passes every case of the GPU list"


def test_integer_family_is_exact_in_the_model():
    n = 0
    for cid, args, _ in CASES:
        if args[1] == "integer" and args[2:5] not in S.BIG:
            c, ref = _case(cid)
            y = S.model_skinny(c)["y"]
            assert A.bits_equal(y + 0.0, ref["y"].ref.to(torch.bfloat16) + 0.0), cid
            n += 1
    assert n >= 20
