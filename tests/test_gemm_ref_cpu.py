"""CPU self-check of tests/gemm_ref.py: the float64 references agree with torch's float64 matmul / GELU and its
autograd, the input families have the properties their names claim, an fp32 model of every entry point stays inside every
bound on every case the GPU tests run (its fp32 part is what gemm_ref.MEASURED records, the bounds' constants being 4x
that and below the analytic ceiling; the integer family is exact), and each planted error leaves the bounds on at least
one case the GPU suite runs.  If a model left a bound, the bound (not a kernel) would be wrong; if a planted error
passed, the inputs or bounds would be too weak.  The last test documents the gap this closes: the whole-tensor
``rel() < 1e-2`` of test_kernels_gpu.py passes two of the planted errors at the output scale of its largest shape."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_ref as A

WORST = {}
FP32 = {}
CASES = A.all_cases()
BY_ID = {cid: (args, opt) for group in CASES.values() for cid, args, opt in group}


def _note(name, ratio, table=WORST, label="worst error / bound so far"):
    table[name] = max(table.get(name, 0.0), ratio)
    print(f"{label}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(table.items())))
    return ratio


def _fp32(name, ratio):
    _note(name, ratio, FP32, "fp32 part, worst error / (u S) so far")


@functools.lru_cache(maxsize=None)
def _case(cid):
    c = A.build(*BY_ID[cid])
    return c, A.reference(c)


def test_constants_are_four_times_the_measurement_and_below_the_ceiling():
    assert all(A.C[k] == 4.0 * A.MEASURED[k] for k in A.MEASURED) and set(A.C) == set(A.MEASURED)
    min_k = min(args[4] for args, _ in BY_ID.values())
    assert min_k == A.MIN_K
    # K exact products, K - 1 additions, alpha, bias, the slab sum: any order errs by at most (K + 4) u S
    for K in sorted({args[4] for args, _ in BY_ID.values()}):
        assert A.acc_const("acc", K) < K + 4 and A.acc_const("rowsum", K) < K + 4
        assert A.acc_const("acc", K) == A.C["acc"] or K < A.C["acc"]


def test_case_lists_cover_what_they_claim():
    ids = [cid for group in CASES.values() for cid, _, _ in group]
    assert len(ids) == len(set(ids))
    shapes = {args[2:5] for args, _ in BY_ID.values() if args[0] in ("nt", "nn", "nt_ex")}
    for s in A.MUT_SHAPES + A.MUT_F32_SHAPES + A.NT_SHAPES + A.F32_SHAPES + A.pp_bn_all() + A.EPI_SHAPES:
        assert s in shapes, s
    for cid, (args, opt) in BY_ID.items():
        M, N, K = args[2:5]
        assert K % 8 == 0 and 16 * K < 2 ** 24
        if args[0] in ("wgrad", "splitk"):
            assert K % 32 == 0 and N % 8 == 0, cid
    sp = {(args[4], opt["splits"]) for args, opt in BY_ID.values() if args[0] == "wgrad"}
    assert sp >= {(K, s) for K in A.WGRAD_K for s in A.WGRAD_SPLITS}
    assert any(s > K // 32 for K, s in sp) and any(K // 32 % s for K, s in sp if s <= K // 32)
    # every engine's operand conditions are met by some shape, so forcing it runs it
    assert any(K % 64 == 0 and M >= 8 and N >= 8 for M, N, K in shapes)
    assert any(K % 32 == 0 and K % 64 and M >= 16 and N >= 16 for M, N, K in shapes)


# ---------------------------------------------------------------------------------------------- references
def test_reference_matches_torch_float64():
    c = A.make("nt_ex", "gauss", 72, 40, 96, 1, act=2, bias=True, res=True, alpha=True)
    a, b = c.a.double().requires_grad_(True), c.b.double()
    pre = A.f32(c.alpha) * (a @ b) + c.bias.double()
    y = F.gelu(pre, approximate="tanh") + c.res.double()
    ref = A.reference(c)
    assert torch.allclose(ref["aux"].ref, pre.detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(ref["y"].ref, y.detach(), rtol=1e-7, atol=1e-7)          # the kernel's fp32 constants
    x = torch.linspace(-9, 9, 1999, dtype=torch.float64).requires_grad_(True)
    F.gelu(x, approximate="tanh").sum().backward()
    assert torch.allclose(A.gelu_grad64(x.detach())[0], x.grad, rtol=1e-6, atol=1e-7)
    c = A.make("wgrad", "gauss", 24, 16, 64, 2, alpha=0.5, old=True, rowsum=True)
    ref = A.reference(c)
    assert torch.allclose(ref["y"].ref, c.old.double() + 0.5 * c.a.double() @ c.b.double(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(ref["rowsum"].ref, c.rowsum_old.double() + 0.5 * c.a.double().sum(1), rtol=1e-13, atol=1e-13)


def test_split_ranges_cover_every_slice_once():
    for K in A.WGRAD_K:
        for s in A.WGRAD_SPLITS:
            r = A.split_ranges(K, s)
            assert len(r) == min(s, K // 32) and r[0][0] == 0 and r[-1][1] == K
            assert all(r[i][1] == r[i + 1][0] for i in range(len(r) - 1))
            lens = [(k1 - k0) // 32 for k0, k1 in r]
            assert max(lens) - min(lens) <= 1 and lens == sorted(lens, reverse=True)


@pytest.mark.parametrize("family", A.FAMILIES)
def test_families_are_what_they_claim(family):
    for M, N, K in [(129, 72, 96), (16, 16, 32), (264, 136, 544)]:
        c = A.make("nt", family, M, N, K, 3, bias=True, res=True, alpha=True)
        a, b = c.a.double(), c.b.double()
        ref, mag = a @ b, a.abs() @ b.abs()
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        if family == "positive":
            assert (a > 0).all() and (b > 0).all() and torch.allclose(ref, mag)
        elif family == "cancelling":
            assert (ref.abs() / mag).median().item() < 0.05          # gauss: ~ 1 / sqrt(K) ~ 0.1 .. 0.2
        elif family == "integer":
            assert A._distinct(a) and A._distinct(b) and a.abs().max() <= 4 and (a == a.round()).all()
            assert c.alpha in A.INT_ALPHA and (c.bias == c.bias.round()).all() and (c.res.double() == c.res.double().round()).all()
            y = A.reference(c)["y"].ref
            assert torch.equal(y.float().double(), y)                  # exact in fp32: any order gives these bits
        elif family == "poisoned":
            assert c.poison


def test_causal_operands_are_triangular_with_nan_outside():
    for mode in (2, 3):
        c = A.make("batched", "gauss", 520, 8, 520, 0, causal=mode, amode=mode - 2, bmode=1)
        a = c.a.double()
        q, k = torch.arange(520)[:, None], torch.arange(520)[None, :]
        inside = (k <= q) if mode == 2 else (k >= q)
        assert torch.isfinite(a[inside]).all() and (a[inside] != 0).any()
        nan = torch.isnan(a)
        assert nan.any() and not (nan & inside).any()
        assert (a[~inside & ~nan] == 0).all()
        # no 128- or 256-row tile's reduction range reaches a NaN
        for bm in (128, 256):
            for m0 in range(0, 520, bm):
                rows = slice(m0, min(m0 + bm, 520))
                cols = slice(0, min(520, m0 + bm)) if mode == 2 else slice(m0, 520)
                assert not nan[rows, cols].any()


# ------------------------------------------------------------------------------------- models inside the bounds
def _inside(cid):
    c, ref = _case(cid)
    for sl in ((32, 64) if c.ep not in ("wgrad", "splitk") else (32,)):
        for n, r in A.check(c, A.model(c, sl=sl), ref).items():
            _note(n, r)
    if c.family == "integer":
        return
    for sl in ((32, 64) if c.ep not in ("wgrad", "splitk") else (32,)):
        _fp32_parts(c, ref, A.model(c, rnd=False, sl=sl))


def _fp32_parts(c, ref, raw):
    if c.act == 2:
        if "aux" in raw:
            _fp32("acc", A.fp32_part(raw["aux"], ref["aux"]))
    elif c.du is None:
        y = raw["y"]
        if c.causal == 1:
            y = torch.where(A.causal1_mask(c, y.device), y, ref["y"].ref.float())
        _fp32("acc", A.fp32_part(y, ref["y"]))
    if "rowsum" in raw:
        _fp32("rowsum", A.fp32_part(raw["rowsum"], ref["rowsum"]))


def _gelu_fp32_part():
    """s(x) and gelu'(x) in fp32 over every bf16 value of |x| <= 16 against float64: what C_gelu / C_dgelu are 4x of"""
    x = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    x = x[torch.isfinite(x) & (x.abs() <= 16.0)]
    xd = x.double()
    ok = xd != 0
    _fp32("gelu", ((A.model_gelu(x).double() - A.gelu64(xd)).abs()[ok] / (A.U * xd.abs()[ok])).max().item())
    gp, G = A.gelu_grad64(xd)
    _fp32("dgelu", (((A.model_gelu_grad(x).double() - gp).abs() - A.TINY).clamp_min(0.0) / (A.U * G + 1e-300)).max().item())


@functools.lru_cache(maxsize=None)
def _sweep():
    """every case of every group once -> {group: [failures]}; fills WORST and FP32"""
    fails = {g: [] for g in CASES}
    for g in CASES:
        for cid, _, _ in CASES[g]:
            try:
                _inside(cid)
            except AssertionError as e:
                fails[g].append(f"{cid}: {e}")
    _gelu_fp32_part()
    return fails


@pytest.mark.parametrize("group", list(CASES))
def test_models_inside_bounds(group):
    fails = _sweep()[group]
    assert not fails, fails[:5]


def test_measured_constants_match():
    """MEASURED is the measurement itself (both ways, to 2%): a better model or a padded table would both show.  The
    models round every slice sum and exp2 once from float64, so the figures do not depend on the host."""
    _sweep()
    assert set(FP32) == set(A.MEASURED)
    for k, v in A.MEASURED.items():
        assert abs(FP32[k] - v) <= 0.02 * v, (k, FP32[k], v)


# --------------------------------------------------------------------------------------------- planted errors
def _mut_ids(eps):
    shapes = set(A.MUT_SHAPES + A.MUT_F32_SHAPES)
    out = []
    for cid, (args, opt) in BY_ID.items():
        if args[0] not in eps:
            continue
        if args[0] in ("nt", "nn", "nt_ex") and args[2:5] not in shapes:
            continue
        out.append(cid)
    return out


PLAIN = ("nt", "nn", "nt_ex")
WHERE = {"drop_last_slice": PLAIN + ("splitk", "wgrad"), "k64_tail": PLAIN, "acc_not_cleared": PLAIN,
         "alpha_ignored": ("nt", "nn", "wgrad", "tn", "batched"), "alpha_after_bias": ("nt",), "bias_shift4": ("nt", "nt_ex"),
         "bias_skipped_n4": ("nt",), "relu_skipped_f32": ("nt",), "res_before_act": ("nt_ex",), "col_swap": PLAIN + ("batched",),
         "row_low": PLAIN, "overwrite": ("tn", "wgrad"), "split_twice": ("wgrad", "splitk"), "split_skipped": ("wgrad", "splitk"),
         "rowsum_no_alpha": ("wgrad",), "rowsum_per_coltile": ("wgrad",), "causal2_short": ("batched",),
         "causal3_late": ("batched",), "bf16_trunc": PLAIN + ("splitk",)}


def test_every_planted_error_is_listed():
    assert set(WHERE) == set(A.MUTATIONS) and len(A.MUTATIONS) == 19


@pytest.mark.parametrize("mut", A.MUTATIONS)
def test_planted_error_is_rejected(mut):
    hit = []
    for cid in _mut_ids(WHERE[mut]):
        c, ref = _case(cid)
        try:
            A.check(c, A.model(c, mut=mut), ref)
        except AssertionError:
            hit.append(cid)
    print(f"{mut}: rejected on {len(hit)} cases, among them {hit[:6]}")
    assert hit, mut
    fams = {BY_ID[h][0][1] for h in hit}
    assert "integer" in fams, (mut, "the exact family must reject it")
    if mut in ("drop_last_slice", "split_skipped"):
        assert "positive" in fams
    if mut == "bias_skipped_n4":
        assert all(BY_ID[h][0][3] % 4 for h in hit)


# -------------------------------------------------------------------------------------------------- the gap
def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


@pytest.mark.parametrize("mut", ["bias_shift4", "bf16_trunc"])
def test_whole_tensor_rel_passes_what_the_elementwise_bound_rejects(mut):
    """test_kernels_gpu.py's check at (4096, 768, 3072): unit Gaussian operands and bias, rel() < 1e-2.  The same K and
    family, so the same output scale (max |y| ~ 250), at fewer rows and with a ragged last column tile."""
    M, N, K = 256, 776, 3072
    n = torch.arange(768, N)
    for idx in range(8):
        c = A.make("nt", "gauss", M, N, K, idx, bias=True)
        c.bias = c.bias / 2.0                                        # unit Gaussian, as in that test
        # rel() hides an error below 1e-2 max |y| ~ 2.5, less the bf16 rounding (~ 0.5).  Take the first seed whose
        # shifted bias entries differ by less than 2: the difference of two unit Gaussians has sigma 1.4, so most do.
        if (c.bias[(n + 4).clamp_max(N - 1)] - c.bias[n]).abs().max() < 2.0:
            break
    wrong = A.model(c, mut=mut)["y"]
    ref32 = c.a.float() @ c.b.float() + c.bias
    assert 200.0 < ref32.abs().max().item() < 320.0
    assert _rel(wrong, ref32) < 1e-2, "the existing check would have caught it"
    with pytest.raises(AssertionError):
        A.check(c, {"y": wrong})
    A.check(c, A.model(c))
