"""CPU self-check of tests/conv_ref.py: the float64 reference agrees with torch's float64 conv2d and its autograd (on
the CPU), the input families have the properties their names claim, the case lists reach the configurations they are
there for (the launch arithmetic of the kernels mirrored in conv_ref and asserted against recorded expectations), no
element of any fused-BN-backward case lies in the mask's ambiguity band, an fp32 model of the kernels stays inside every
bound on every case the GPU tests run (its fp32 part is what conv_ref.MEASURED records; the integer family is exact),
and each planted error leaves the bounds.  If a model left a bound, the bound (not a kernel) would be wrong; if a planted
error passed, the inputs or bounds would be too weak."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as A
import gemm_ref as G

WORST = {}
BY_ID = A.by_id()
GROUPS = A.all_cases()


def _note(name, ratio, table=WORST, label="worst error / bound so far"):
    table[name] = max(table.get(name, 0.0), ratio)
    print(f"{label}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(table.items())))
    return ratio


@functools.lru_cache(maxsize=None)
def _case(cid):
    return A.make(*BY_ID[cid])


@functools.lru_cache(maxsize=None)
def _run(cid):
    """the clean model on one case -> (worst error / bound per kind, fp32 part of the accumulation, of the slab)"""
    c = _case(cid)
    out = A.model(c)
    r = A.check(c, out)
    raw = A.model(c, rnd=False)
    acc = 0.0
    if c.epi != "bnb":
        acc = A.fp32_part(raw["y"], A.reference(c, dt_own=out.get("dt", out.get("a1")))["y"])
    slab = A.slab_fp32_part(c, out["y"], out["slab"]) if "slab" in out else 0.0
    return r, acc, slab


def test_constants():
    assert A.MEASURED["acc"] > G.MEASURED["acc"] and A.C_ACC == 4.0 * A.MEASURED["acc"]     # above gemm_ref's: its own
    assert A.K_SLAB == 4.0 * A.MEASURED["slab"] and A.C_ACC_LONG == 4.0 * A.MEASURED["acc_long"]
    for args in BY_ID.values():
        terms = (1 if args[0] == "p1" else 9) * args[2]
        assert A.acc_const(terms) < terms + 4
        assert A.acc_const(terms) == (A.C_ACC_LONG if terms > A.LONG_TERMS else A.C_ACC)
        assert 9 * args[2] * 10 * 4 < 2 ** 24


def test_case_lists_reach_what_they_claim():
    ids = [cid for group in GROUPS.values() for cid, _ in group]
    assert len(ids) == len(set(ids))
    # ---- halo 3x3: the geometry the predicates give (recorded expectations)
    assert (A.W_MAX64, A.W_MAX128, A.W_MAXRES) == (85, 38, 85)
    assert A.c3_smem(64, 73) == 80 * 1024 and A.c3_smem(64, 74) > 80 * 1024      # 73: widest with seven halo rows
    assert A.c3_smem(64, 85) == 80 * 1024 - 128 and A.c3_smem(64, 86) > 80 * 1024
    assert A.c3_smem(128, 38) <= 80 * 1024 < A.c3_smem(128, 39)
    assert not A.halo_supported(280, 56, 64, 128) and A.halo_supported(280, 56, 64, 64)  # Co = 128 at W = 56: no halo shape
    assert A.halo_nb(192, 11, 128) == 64 and A.halo_nb(128, 38, 0) == 128 and A.halo_nb(128, 38, 64) == 64
    halo = [a for _, a in GROUPS["halo"]]
    for _, (Nimg, H, W), Ci, Co, _, _ in halo:
        assert A.halo_supported(Nimg * H * W, W, Ci, Co), (Nimg, H, W, Ci, Co)
    shapes = {(a[1], a[2], a[3]) for a in halo}
    P = lambda s: s[0][0] * s[0][1] * s[0][2]                                         # noqa: E731
    assert {P(s) for s in shapes} >= {1, 255, 256, 257, 513}
    assert any(s[0][2] == 1 and P(s) > 256 for s in shapes) and any(s[0][1] == 1 and s[0][2] == 73 for s in shapes)
    assert any(s[0][0] > 1 and s[0][1] * s[0][2] < 256 and P(s) > 256 and 256 % s[0][2] for s in shapes)   # both straddles
    assert any(P(s) > 256 and P(s) % 256 for s in shapes)                             # partial last tile
    assert any(s[0][2] == A.W_MAX64 and s[1:] == (64, 64) for s in shapes)
    assert any(s[0][2] == A.W_MAX128 and s[2] % 128 == 0 for s in shapes)
    assert {(64, 192), (128, 64), (256, 128)} <= {s[1:] for s in shapes}
    for s in shapes:                                                                   # every shape x every variant
        assert {a[4] for a in halo if (a[1], a[2], a[3]) == s} == {v[0] for v in A.V_HALO}
    fams = {(a[4], a[5]) for a in halo}
    assert fams == {(v[0], f) for v in A.V_HALO for f in A.FAMILIES}                   # every family meets every variant
    # the weight-resident kernel (nb = 1) takes the 64 -> 64 shapes without prologues, at its widest W too
    assert any(A.resident_ok(a[2], a[3], a[1][2], A.VARIANT[a[4]][3], A.VARIANT[a[4]][4]) and a[1][2] == A.W_MAXRES
               for a in halo)
    # ---- A-stationary 1x1: weight steps
    assert A.areg_plan(600, 256, 192) == (32, 2, 3) and A.areg_plan(600, 64, 192) == (64, 1, 3)
    assert A.areg_plan(600, 128, 320) == (64, 1, 5) and A.areg_plan(600, 64, 128) == (64, 2, 1)
    assert A.areg_plan(*A.AREG_BIG) == (64, 1, 2) and -(-A.AREG_BIG[0] // 256) >= 512     # production branch g = 1
    areg = [a for _, a in GROUPS["areg"]]
    for K in (64, 128, 256):
        for v in A.V_AREG:
            st = {A.areg_plan(a[1][2], K, a[3])[2] > 1 for a in areg if a[2] == K and a[4] == v[0]}
            assert st == {True, False}, (K, v[0], st)                                  # steps == 1 and steps > 1
        assert {a[1][2] for a in areg if a[2] == K} >= set(A.AREG_P)
    # ---- stride 2
    assert A.W_MAXS2 == 108 and A.s2_supported(4, 108, 128, 128) and not A.s2_supported(4, 110, 128, 128)
    s2 = [a for _, a in GROUPS["s2"]]
    for _, (Nimg, H, W), Ci, Co, vn, _ in s2:
        assert A.s2_supported(H, W, *((Co, Ci) if A.VARIANT[vn][1] else (Ci, Co)))
    half = {a[1][0] * a[1][1] * a[1][2] // 4 for a in s2}
    assert half >= {1, 9, 255, 256, 510, 297} and {a[1] for a in s2} >= {(1, 2, 2), (1, 4, A.W_MAXS2)}
    assert {(a[1], a[4]) for a in s2} == {(sh, v[0]) for sh, _, _ in A.S2 for v in A.V_S2}
    assert {(a[4], a[5]) for a in s2} == {(v[0], f) for v in A.V_S2 for f in A.FAMILIES}
    # ---- long reduction
    wide = [a for _, a in GROUPS["wide"]]
    assert {a[2] for a in wide} == {512, 576, 8192} and {a[3] for a in wide} == {64, 192, 1024}
    for K in (512, 576):
        assert {a[4] for a in wide if a[2] == K} == {v[0] for v in A.V_WIDE}
    assert all(A.VARIANT[a[4]][3] for a in wide if a[2] == 8192)                        # K = 8192 with pre=


def test_reference_matches_torch_float64_conv_and_autograd():
    for dgrad in (False, True):
        c = A.make("c3", (2, 5, 6), 64, 64, "dg_plain" if dgrad else "fwd_plain", "gauss")
        c.wk = c.wk[:16] if not dgrad else c.wk[:, :, :16]            # smaller: fwd 64 -> 16, dgrad 16 -> 64
        if dgrad:
            c.x, c.Ci = c.x[:, :16].contiguous(), 16
            W = A.layer_weight(c).double()                           # [K = 16][9][C = 64]
            xin = torch.zeros(2, 64, 5, 6, dtype=torch.float64, requires_grad=True)
            y = F.conv2d(xin, W.view(16, 3, 3, 64).permute(0, 3, 1, 2), padding=1)
            y.backward(c.x.double().view(2, 5, 6, 16).permute(0, 3, 1, 2))
            want = xin.grad.permute(0, 2, 3, 1).reshape(60, 64)
        else:
            c.Co = 16
            want = F.conv2d(c.x.double().view(2, 5, 6, 64).permute(0, 3, 1, 2),
                            c.wk.double().view(16, 3, 3, 64).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(60, 16)
        ref = A.reference(c)["y"]
        assert torch.allclose(ref.ref, want, rtol=1e-12, atol=1e-12)
        assert (ref.S >= ref.ref.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("family", A.FAMILIES)
def test_families_are_what_they_claim(family):
    c = A.make("c3", (3, 9, 11), 64, 192, "dg_pre1_bnb", family)
    x, w = c.x.double(), c.wk.double()
    assert torch.isfinite(x).all() and torch.isfinite(w).all()
    e = A.reference(A.make("c3", (3, 9, 11), 64, 192, "fwd_plain", family))["y"]
    if family == "positive":
        assert (x > 0).all() and (w > 0).all()
    elif family == "cancelling":
        assert (e.ref.abs() / e.S).median().item() < 0.05
    elif family == "integer":
        assert x.abs().max() <= 4 and (x == x.round()).all() and (w == w.round()).all()
        assert A._distinct_rows(x) and A._distinct_rows(w.permute(1, 0, 2).reshape(9, -1))
        dt = A.ref_operand(c)[0]
        assert (dt == dt.round()).all() and dt.abs().max() <= 10 and torch.equal(e.ref.float().double(), e.ref)
    elif family == "poisoned":
        assert c.poison


def test_no_element_in_the_mask_band_and_zeros_are_planted():
    n = 0
    for cid, args in BY_ID.items():
        if A.VARIANT[args[4]][2] != "bnb":
            continue
        c = _case(cid)
        m, band, zero = A.mask_parts(c)
        assert not band.any(), cid
        assert zero.any() or c.P < 8, cid
        n += int(zero.sum())
    assert n > 1000


@pytest.mark.parametrize("cid", [cid for g in ("halo", "areg", "wide", "s2", "gen") for cid, _ in GROUPS[g]])
def test_model_is_inside_every_bound(cid):
    r, acc, slab = _run(cid)
    for k, v in r.items():
        _note(k, v)
    if _case(cid).family == "integer":
        assert all(v == 0.0 for k, v in r.items() if not k.startswith("slab"))


def test_measured_constants():
    terms = lambda cid: (1 if BY_ID[cid][0] == "p1" else 9) * BY_ID[cid][2]           # noqa: E731
    acc = max((_run(cid)[1], cid) for cid in BY_ID if terms(cid) <= A.LONG_TERMS)
    long = max((_run(cid)[1], cid) for cid in BY_ID if terms(cid) > A.LONG_TERMS)
    slab = max((_run(cid)[2], cid) for cid in BY_ID)
    print(f"fp32 part, worst error / (u S): acc {acc[0]:.3f} ({acc[1]}), acc_long {long[0]:.3f} ({long[1]}), "
          f"slab {slab[0]:.3f} ({slab[1]})")
    assert abs(acc[0] / A.MEASURED["acc"] - 1.0) <= 0.02, acc
    assert abs(long[0] / A.MEASURED["acc_long"] - 1.0) <= 0.02, long
    assert abs(slab[0] / A.MEASURED["slab"] - 1.0) <= 0.02, slab


def _changed(a, b):
    return any(not (torch.equal(a[k], b[k]) if a[k].dtype == torch.float64 else G.bits_equal(a[k], b[k])) for k in a)


# cases a planted error changes but the bound forgives (recorded; all are pro / pre-without-dt_out cases outside the
# positive and integer families, where y carries the operand's unseen rounding): a rise is a weakening
FORGIVEN = dict({m: 0 for m in A.MUTATIONS}, bf16_trunc=98)


@pytest.mark.parametrize("mut", A.MUTATIONS)
def test_planted_errors_are_caught(mut):
    """on every case of the GPU lists (up to 600 pixels) whose model output the planted error changes: caught.  Where y
    carries the Lipschitz term of an unseen operand rounding (pro, pre without dt_out), the slack is 2^-8 of the
    magnitude, so only errors of full size are asked for there: the positive and integer families (a truncating
    conversion errs by a rounding's size: there it is the integer family's to catch)."""
    hit, forgiven = {}, 0
    for cid, args in BY_ID.items():
        if args[1][0] * args[1][1] * args[1][2] > 600:
            continue
        if mut in ("left_wrap", "tap_drop_border") and args[0] != "c3":
            continue
        if mut == "bit_order" and A.VARIANT[args[4]][2] != "resmask":
            continue
        if mut == "mask_ge" and A.VARIANT[args[4]][2] != "bnb":
            continue
        if mut == "stats_lastrow_twice" and A.VARIANT[args[4]][2] not in ("stats", "bnb"):
            continue
        if mut == "wstep_next" and (args[0] != "p1" or args[2] > 256):
            continue
        c = _case(cid)
        clean, bad = A.model(c), A.model(c, mut=mut)
        if not _changed(clean, bad):
            continue
        slack = (c.pro == 1 or c.pre == 2) and (c.family not in ("positive", "integer")
                                           or (mut == "bf16_trunc" and c.family != "integer"))
        try:
            A.check(c, bad)
            caught = False
        except AssertionError:
            caught = True
        assert caught or slack, (mut, cid)
        forgiven += not caught
        group = "halo" if args[0] == "c3" else args[0] if args[0] in ("s2", "gen") else "areg" if args[2] <= 256 else "wide"
        hit[group] = hit.get(group, 0) + caught
    print(f"{mut}: caught per kernel group {hit}, forgiven (operand-rounding slack) {forgiven}")
    want = {"tap_drop_border": {"halo"}, "no_flip": {"halo", "s2"}, "left_wrap": {"halo"}, "wstep_next": {"areg"},
            "bit_order": {"halo", "areg", "wide"}}.get(mut, {"halo", "areg", "wide", "s2"})
    assert all(hit.get(g, 0) >= 3 for g in want), (mut, hit)
    assert forgiven <= FORGIVEN[mut], (mut, forgiven)


# ------------------------------------------------------------------------------------------------ weight gradients
WG = dict(A.wgrad_cases())


@functools.lru_cache(maxsize=None)
def _wg(cid):
    c = A.wg_make(*WG[cid])
    return c, A.wg_reference(c)


def test_wgrad_cases_reach_every_route_and_plan_boundary():
    routes = {A.wg_route(*a[:5]) for a in WG.values()}
    assert routes == {"direct", "direct_s2", "pp", "gemm"}
    direct = [a for a in WG.values() if A.wg_route(*a[:5]) == "direct"]
    assert {a[0][2] for a in direct} == {7, 14, 28, 56} and {a[4] for a in direct} == {0, 1}
    assert any(a[0][1] % 2 for a in direct) and any(a[2] != a[3] for a in direct)
    assert {a[0][2] // 2 for a in WG.values() if A.wg_route(*a[:5]) == "direct_s2"} == {7, 14, 28}
    assert A.wg_route((30, 1, 14), (3, 1, 1), 64, 64, 0) == "gemm" and not any(A.w3_supported(1, W, 64, 64) for W in (7, 14, 28, 56))
    P = lambda a: a[0][0] * a[0][1] * a[0][2]                                         # noqa: E731
    assert {126, 252, 266} <= {P(a) for a in direct}                                   # either side of one tile
    assert A.w3_plan(2016, 256, 256) == (8, 8) and A.w3_plan(2072, 256, 256) == (9, 8) and A.w3_plan(4144, 256, 128) == (17, 16)
    assert {2016, 2072, 4144} <= {P(a) for a in direct}
    assert A.wg_route((1, 1, 256), (1, 1, 0), 64, 128, 0) == "pp" and A.wg_route((1, 1, 250), (1, 1, 0), 64, 128, 0) == "gemm"
    assert A.wg_route((1, 1, 256), (1, 1, 0), 128, 64, 1) == "gemm"
    for fam in A.FAMILIES:
        assert any(a[5] == fam for a in WG.values())
    assert all(any(a[5] == "integer" for a in WG.values() if A.wg_route(*a[:5]) == r) for r in routes)


def test_wgrad_reference_matches_torch_autograd():
    for geo, img in (((3, 1, 1), (2, 5, 6)), ((3, 2, 1), (1, 7, 9)), ((1, 2, 0), (2, 6, 6))):
        c = A.wg_make(img, geo, 72, 64, 0, "gauss")
        R, st, pad = geo
        w = torch.zeros(64, 72, R, R, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(c.x.double().view(*img, 72).permute(0, 3, 1, 2), w, stride=st, padding=pad)
        y.backward(c.dy.double().view(img[0], y.shape[2], y.shape[3], 64).permute(0, 3, 1, 2))
        want = w.grad.permute(0, 2, 3, 1).reshape(64, R * R, 72) + c.old.double()
        assert torch.allclose(A.wg_reference(c).ref, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cid", list(WG))
def test_wgrad_model_is_inside_the_bound(cid):
    c, e = _wg(cid)
    got = A.wg_model(c)
    _note("dW", A.wg_check(c, got, e))


def test_wgrad_measured_constant():
    worst = max((A.fp32_part(A.wg_model(_wg(cid)[0]), _wg(cid)[1]), cid) for cid in WG)
    print(f"fp32 part, worst error / (u S): wgrad {worst[0]:.3f} ({worst[1]})")
    assert abs(worst[0] / A.MEASURED["wgrad"] - 1.0) <= 0.02, worst
    for cid in WG:
        c, e = _wg(cid)
        assert e.c <= c.Po + A.w3_plan(c.Po, c.Ci, c.Co)[1] + 3


@pytest.mark.parametrize("mut", A.WG_MUTATIONS)
def test_wgrad_planted_errors_are_caught(mut):
    hit = 0
    for cid in WG:
        c, e = _wg(cid)
        bad = A.wg_model(c, mut)
        if G.bits_equal(bad, A.wg_model(c)):
            continue
        with pytest.raises(AssertionError):
            A.wg_check(c, bad, e)
        hit += 1
    assert hit >= 5, (mut, hit)
