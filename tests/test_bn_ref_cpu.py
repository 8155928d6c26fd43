"""CPU self-check of tests/bn_ref.py: the float64 reference agrees with torch's batch norm and its autograd, an fp32
model of every kernel (same formulas in fp32, result rounded to bf16; sums in the kernels' order) stays inside every
bound on every input the GPU tests use, the summation model's measured error is what bn_ref.K_MEASURED records, and
each planted error leaves the bounds on at least one case.  If a model left a bound, the bound (not a kernel) would be
wrong; if a planted error passed, the inputs or the bounds would be too weak."""
import functools

import pytest
import torch
import torch.nn.functional as F

import bn_ref as B

WORST = {}
IDS = [f"{L}x{C}" for L, C in B.SHAPES]
MUTANT_SHAPES = [(1, 8), (2, 8), (3137, 24), (147, 2048)]


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    return ratio


@functools.lru_cache(maxsize=None)
def _case(L, C):
    return B.given_coeffs(B.gen_case(L, C))


def _masks(c):
    """(mode, mask source, mask) per mask mode, from the model's own y"""
    y, bits = B.model_apply(c.x, c.scale, c.shift, relu=True)
    return [(0, None, None), (1, y, B.ref_mask(1, c.x, msrc=y)),
            (2, None, B.ref_mask(2, c.x, mscale=c.mscale, mshift=c.mshift)), (3, bits, B.ref_mask(3, c.x, msrc=bits))]


def test_launch_geometry():
    """The iteration counts the GPU tests' docstrings state, recomputed from the grid functions."""
    it = lambda L, C, grid: B.row_iters(L, C, grid(L, C))
    assert B.rpi(2048) == 1 and B.stream_grid(147, 2048) == 147 and it(147, 2048, B.stream_grid) == (1, 1)
    assert B.stream_grid(1100, 2048) == 512 and it(1100, 2048, B.stream_grid) == (2, 3)
    assert B.reduce_grid(1100, 2048) == 35 and it(1100, 2048, B.reduce_grid) == (31, 32)   # odd count: BN_UR tail
    assert B.reduce_grid(2500, 2048) == 79 > B.STAT_BINS
    assert B.rpi(200) == 10 and B.idle_threads(200) == 6 and it(10243, 200, B.stream_grid) == (2, 3)
    assert B.reduce_grid(10243, 200) == 33 and it(10243, 200, B.reduce_grid) == (31, 32)
    assert B.rpi(24) == 85 and B.idle_threads(24) == 1 and B.stream_grid(3137, 24) == 37
    assert it(32845, 64, B.stream_grid) == (2, 3)
    assert B.rpi(8) == 256 and B.idle_threads(8) == 0 and it(131372, 8, B.stream_grid) == (1, 2)
    assert B.stream_grid(4096, 256) == 512 and it(4096, 256, B.stream_grid) == (1, 1)
    assert B.reduce_grid(4096, 256) == 16 and it(4096, 256, B.reduce_grid) == (32, 32)


def test_ref64_matches_torch_float64():
    c = _case(3137, 24)
    L, C = c.L, c.C
    xd = c.x.double().requires_grad_(True)
    gd, bd = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    rm, rv = c.rm.double().clone(), c.rv.double().clone()
    eps, mom = B.f32(B.EPS), B.f32(0.1)
    y = F.relu(F.batch_norm(xd, rm, rv, gd, bd, True, mom, eps))
    ref = B.ref_forward(c.x, c.gamma, c.beta, c.rm, c.rv, 0.1)
    assert torch.allclose(ref["run_mean"][0], rm, rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref["run_var"][0], rv, rtol=1e-12, atol=1e-14)
    y64, _ = B.ref_apply(c.x, ref["scale"][0], ref["shift"][0], relu=True)
    assert torch.allclose(y64, y.detach(), rtol=1e-11, atol=1e-11)
    y.backward(c.gy.double())
    mean, var = B.stats64(c.x)
    inv = 1.0 / torch.sqrt(var + eps)
    mask = y.detach() > 0
    red = B.ref_bwd_reduce(c.gy, c.x, mean, inv, mask)
    assert torch.allclose(red["dgamma"][0], gd.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(red["dbeta"][0], bd.grad, rtol=1e-10, atol=1e-10)
    dx, _ = B.ref_bwd_apply(c.gy, c.x, mean, inv, c.gamma, red["dgamma"][0], red["dbeta"][0], mask)
    assert torch.allclose(dx, xd.grad, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_generators_make_every_term_matter(L, C):
    """dbeta/L and xhat*dgamma/L are order-one parts of dx; gamma has its zero, negative and large entries; the
    constant channel has var = 0 exactly; x*mscale + mshift is exact in fp32 and has exact zeros."""
    c = _case(L, C)
    mean, var = B.stats64(c.x)
    assert var[B.CONST].item() == 0.0
    assert c.gamma[0] == 0 and c.gamma[1] < 0 and c.gamma[2] == 24
    v64 = c.x.double() * c.mscale.double() + c.mshift.double()
    assert torch.equal((c.x.float() * c.mscale + c.mshift).double(), v64)
    if L >= 147:
        assert 0.02 < (v64 == 0).double().mean().item() < 0.1
        assert (mean.abs() / var.sqrt().clamp_min(1e-3))[-1].item() > 6.0      # the last channel: ~8 sigma
        for mode, _, mask in _masks(c):
            red = B.ref_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mask)
            rms = B.ref_gm(c.gy, mask).double().pow(2).mean().sqrt().item()
            live = var > 0
            # in at least a quarter of the channels (mode 2 masks a far-from-zero channel entirely or not at all)
            assert (red["dbeta"][0] / L).abs()[live].quantile(0.75).item() > 0.2 * rms, mode
            assert (red["dgamma"][0] / L).abs()[live].quantile(0.75).item() > 0.2 * rms, mode


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_summation_model_error_is_what_the_module_records(L, C):
    """error / (u sum|terms|) of blocked_sum32 in three orders, for the four sums; K_SUM is 4x the recorded maximum."""
    c = _case(L, C)
    xd = c.x.double()
    mask = B.ref_mask(2, c.x, mscale=c.mscale, mshift=c.mshift)
    gm = B.ref_gm(c.gy, mask)
    tq = gm.float() * (c.x.float() - c.mean) * c.invstd
    tq64 = gm.double() * (xd - c.mean.double()) * c.invstd.double()
    for name, t32, t64 in (("stats", c.x.float(), xd), ("stats", c.x.float() ** 2, xd * xd),
                           ("backward", gm.float(), gm.double()), ("backward", tq, tq64)):
        for order in range(3):
            err = (B.blocked_sum32(t32, C, order) - t64.sum(0)).abs()
            k = (err / (B.U * t64.abs().sum(0)).clamp_min(1e-300)).max().item()
            _note("k " + name, k)
            assert k <= B.K_MEASURED[name], (name, order, k)
    assert all(B.K_SUM[n] == 4.0 * B.K_MEASURED[n] for n in B.K_MEASURED)


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_model_forward_inside_bounds(L, C):
    c = _case(L, C)
    for mom, order in ((0.1, 0), (1.0, 1), (0.1, 2)):
        ref = B.ref_forward(c.x, c.gamma, c.beta, c.rm, c.rv, mom)
        got = B.model_forward(c.x, c.gamma, c.beta, c.rm, c.rv, mom, order=order)
        for k in ref:
            _note("forward", B.check_vec(got[k], ref[k], k))
    ref = B.ref_forward(c.x, None, None, None, None, 0.1)
    got = B.model_forward(c.x, None, None, None, None, 0.1)
    assert set(ref) == set(got) == {"mean", "invstd", "scale", "shift"}
    for k in ref:
        _note("forward", B.check_vec(got[k], ref[k], k))
    for g, b in ((c.gamma, c.beta), (None, None)):
        ref = B.ref_eval_coeff(B.EPS, g, b, c.rm, c.rv)
        sc, sh = B.model_eval_coeff(B.EPS, g, b, c.rm, c.rv)
        _note("eval", max(B.check_vec(sc, ref["scale"], "scale"), B.check_vec(sh, ref["shift"], "shift")))


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_model_apply_inside_bounds(L, C):
    c = _case(L, C)
    for res, rsc, rsh in ((None, None, None), (c.res, None, None), (c.res, c.rscale, c.rshift)):
        for relu in (True, False):
            ref, S = B.ref_apply(c.x, c.scale, c.shift, res, rsc, rsh, relu)
            y, bits = B.model_apply(c.x, c.scale, c.shift, res, rsc, rsh, relu)
            _note("y", B.check_elem(y, ref, S, B.C_Y, "y"))
            if relu:
                B.check_bits(bits, y)


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_model_backward_inside_bounds(L, C):
    c = _case(L, C)
    for mode, _, mask in _masks(c):
        red = B.ref_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mask)
        red2 = B.ref_bwd_reduce(c.gy, c.x2, c.mean2, c.invstd2, mask)
        for order in range(3):
            dg, db = B.model_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mask, order)
            dg2, db2 = B.model_bwd_reduce(c.gy, c.x2, c.mean2, c.invstd2, mask, order)
            _note("dgamma/dbeta", max(B.check_vec(dg, red["dgamma"], "dgamma"), B.check_vec(db, red["dbeta"], "dbeta"),
                                      B.check_vec(dg2, red2["dgamma"], "dgamma2"),
                                      B.check_vec(db2, red2["dbeta"], "dbeta2")))
        ref, S = B.ref_bwd_apply(c.gy, c.x, c.mean, c.invstd, c.gamma, dg, db, mask)
        _note("dx", B.check_elem(B.model_bwd_apply(c.gy, c.x, c.mean, c.invstd, c.gamma, dg, db, mask), ref, S,
                                 B.C_DX, "dx"))
        ref, S = B.ref_bwd_apply(c.gy, c.x2, c.mean2, c.invstd2, c.gamma2, dg2, db2, mask)
        _note("dx", B.check_elem(B.model_bwd_apply(c.gy, c.x2, c.mean2, c.invstd2, c.gamma2, dg2, db2, mask), ref, S,
                                 B.C_DX, "dx2"))
        ref, S = B.ref_bwd_apply(c.gy, c.x, c.mean, c.invstd, None, dg, db, mask)          # gamma = None
        _note("dx", B.check_elem(B.model_bwd_apply(c.gy, c.x, c.mean, c.invstd, None, dg, db, mask), ref, S, B.C_DX,
                                 "dx, no gamma"))


# --------------------------------------------------------------------------------------------- planted errors
def _rejected(fn):
    """fn(case) runs the checks on a mutated model; -> the shapes on which a bound was left"""
    hit = []
    for L, C in MUTANT_SHAPES:
        try:
            fn(_case(L, C))
        except AssertionError:
            hit.append((L, C))
    print("rejected on", hit)
    return hit


def _bwd_apply_mutant(mut):
    def run(c):
        for mode, _, mask in _masks(c):
            red = B.ref_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mask)
            dg, db = red["dgamma"][0].float(), red["dbeta"][0].float()
            ref, S = B.ref_bwd_apply(c.gy, c.x, c.mean, c.invstd, c.gamma, dg, db, mask)
            B.check_elem(B.model_bwd_apply(c.gy, c.x, c.mean, c.invstd, c.gamma, dg, db, mask, mut=mut), ref, S,
                         B.C_DX, "dx")
    return run


@pytest.mark.parametrize("mut", [None, "no_dbeta", "no_dgamma", "invL", "last_row_unwritten", "last_row_stale"])
def test_planted_error_in_bwd_apply(mut):
    hit = _rejected(_bwd_apply_mutant(mut))
    assert (hit == []) if mut is None else hit, mut


@pytest.mark.parametrize("mut", ["biased", "no_eps"])
def test_planted_error_in_finalize(mut):
    def run(c):
        ref = B.ref_forward(c.x, c.gamma, c.beta, c.rm, c.rv, 0.1)
        got = B.model_forward(c.x, c.gamma, c.beta, c.rm, c.rv, 0.1, biased=mut == "biased", no_eps=mut == "no_eps")
        for k in ref:
            B.check_vec(got[k], ref[k], k)
    assert _rejected(run), mut


def test_planted_error_second_bn_swapped():
    """mean2 / invstd2 taken from the first BN in the X2 variants: in the reduce and in the apply"""
    def reduce(c):
        mask = _masks(c)[3][2]
        red2 = B.ref_bwd_reduce(c.gy, c.x2, c.mean2, c.invstd2, mask)
        dg2, db2 = B.model_bwd_reduce(c.gy, c.x2, c.mean, c.invstd, mask)
        B.check_vec(dg2, red2["dgamma"], "dgamma2")

    def apply(c):
        mask = _masks(c)[3][2]
        red2 = B.ref_bwd_reduce(c.gy, c.x2, c.mean2, c.invstd2, mask)
        dg2, db2 = red2["dgamma"][0].float(), red2["dbeta"][0].float()
        ref, S = B.ref_bwd_apply(c.gy, c.x2, c.mean2, c.invstd2, c.gamma2, dg2, db2, mask)
        B.check_elem(B.model_bwd_apply(c.gy, c.x2, c.mean, c.invstd, c.gamma2, dg2, db2, mask), ref, S, B.C_DX, "dx2")
    assert _rejected(reduce) and _rejected(apply)


def test_planted_error_mask_greater_equal():
    def run(c):
        y = B.model_apply(c.x, c.scale, c.shift, relu=True)[0]
        for mode, kw in ((1, dict(msrc=y)), (2, dict(mscale=c.mscale, mshift=c.mshift))):
            mask, bad = B.ref_mask(mode, c.x, **kw), B.ref_mask(mode, c.x, strict=False, **kw)
            red = B.ref_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mask)
            dg, db = B.model_bwd_reduce(c.gy, c.x, c.mean, c.invstd, bad)
            B.check_vec(db, red["dbeta"], f"dbeta, mode {mode}")
    hit = _rejected(run)
    assert (3137, 24) in hit and (147, 2048) in hit

    def gm(c):                                     # mode 2 alone, through the bitwise gm check
        bad = B.ref_mask(2, c.x, mscale=c.mscale, mshift=c.mshift, strict=False)
        B.check_gm(B.ref_gm(c.gy, bad), c.gy, B.ref_mask(2, c.x, mscale=c.mscale, mshift=c.mshift))
    assert _rejected(gm)


@pytest.mark.parametrize("mut", ["no_rshift", "last_row_unwritten", "last_row_stale"])
def test_planted_error_in_apply(mut):
    def run(c):
        ref, S = B.ref_apply(c.x, c.scale, c.shift, c.res, c.rscale, c.rshift, True)
        y, bits = B.model_apply(c.x, c.scale, c.shift, c.res, c.rscale, c.rshift, True, mut=mut)
        B.check_elem(y, ref, S, B.C_Y, "y")
    assert _rejected(run), mut
