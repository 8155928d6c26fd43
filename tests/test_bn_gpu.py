"""The BatchNorm kernels (csrc/kernels/batchnorm.hip) against a float64 reference, elementwise, at the shapes where they
take another path, and the entry points' guards.

test_kernels_gpu.py::test_bn_train_fwd_bwd runs one shape (L = 4096, C = 256: one row per thread-row, no loop) and
compares in max-norm, which hides the dbeta/L and xhat*dgamma/L terms of dx.  Here every output element is held to the
bounds tests/bn_ref.py states and derives (tests/test_bn_ref_cpu.py shows that a correct fp32 model stays inside them
and that planted errors do not), each kernel from exactly the operands it is given.

Shapes (L, C), with RPI = 256 / (C/8) rows per block iteration, the apply grid min(512, ceil(L*C/8 / 256)) and the reduce
grid min(512, ceil(L / (32 RPI))); the counts are asserted in test_bn_ref_cpu.py::test_launch_geometry:
  (1, 8), (2, 8)   L = 1 (the L > 1 guard of the unbiased variance, invL = 1) and L = 2
  (147, 2048)      RPI = 1, 147 blocks of one row: fewer rows than the 512-block cap
  (1100, 2048)     apply: 512 blocks, step 512, 2-3 rows per thread-row and the clamped last prefetch; reduce: 35
                   blocks, 31-32 rows per thread-row, so the unroll-by-2 tail runs
  (2500, 2048)     reduce grid of 79 blocks: blocks 64-78 fold into bins 0-14
  (10243, 200)     RPI = 10, 6 idle threads, 2-3 rows per thread-row, last finalize column of 8 channels
  (3137, 24)       C/8 = 3, RPI = 85, 1 idle thread, a single partial finalize column
  (32845, 64)      2-3 rows per thread-row
  (131372, 8)      C/8 = 1, RPI = 256, 1-2 rows per thread-row
  (4096, 256)      the baseline shape of test_bn_train_fwd_bwd

A separate module on purpose: the autouse GEMM-engine fixture of test_kernels_gpu.py would run every case five times
for nothing."""
import functools

import pytest
import torch

import bn_ref as B

pytestmark = pytest.mark.gpu

BF, F32 = B.BF, B.F32
IDS = [f"{L}x{C}" for L, C in B.SHAPES]
SENTINEL = -1234.0                  # exactly representable in bf16, far from every output value
PAD = 3                             # sentinel rows before and after an embedded buffer
WORST = {}


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import _backend, kernels
    assert _backend.available(), "HIP kernel library must load on a GPU box"
    return kernels


@functools.lru_cache(maxsize=None)
def _case(L, C):
    """Inputs of one shape on the device with the fp32 coefficients the kernels are handed: built once, shared, never
    written (every test compares them with clones)."""
    return B.given_coeffs(B.case_to(B.gen_case(L, C), "cuda"))


def _snapshot(c):
    return {k: v.clone() for k, v in vars(c).items() if torch.is_tensor(v)}


def _unchanged(c, snap):
    for k, v in snap.items():
        assert torch.equal(getattr(c, k), v), f"input {k} was written"


@functools.lru_cache(maxsize=None)
def _relu_out(L, C):
    """(y, bits) of bn_apply(relu, want_mask) on the case: the mask sources of modes 1 and 3; checked in
    test_bn_apply"""
    from pytorch_distributed_nn_amd.ops import kernels
    c = _case(L, C)
    return kernels.bn_apply(c.x, c.scale, c.shift, relu=True, want_mask=True)


def _mask_args(c, mode):
    """-> (kwargs of the wrappers, reference mask) for a mask mode"""
    if mode == 0:
        return {}, None
    if mode == 2:
        return dict(mscale=c.mscale, mshift=c.mshift), B.ref_mask(2, c.x, mscale=c.mscale, mshift=c.mshift)
    y, bits = _relu_out(c.L, c.C)
    src = y if mode == 1 else bits
    return dict(msrc=src), B.ref_mask(mode, c.x, msrc=src)


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_bn_forward_chain(K, L, C):
    """bn_stats -> bn_finalize with running statistics at momentum 0.1 and 1.0, and without them (and without gamma /
    beta): mean, invstd, scale, shift, run_mean, run_var per channel; the slab comes back zeroed."""
    c = _case(L, C)
    snap = _snapshot(c)
    for mom, affine, running in ((0.1, True, True), (1.0, True, True), (0.1, False, False), (0.1, True, False)):
        gamma, beta = (c.gamma, c.beta) if affine else (None, None)
        rm, rv = (c.rm.clone(), c.rv.clone()) if running else (None, None)
        slab, rows = K.bn_stats(c.x)
        assert rows == K.STAT_BINS and slab.shape == (2 * K.STAT_BINS, C)
        mean, inv, sc, sh = K.bn_finalize(slab, rows, L, B.EPS, mom, gamma, beta, rm, rv)
        ref = B.ref_forward(c.x, gamma, beta, c.rm if running else None, c.rv if running else None, mom)
        got = {"mean": mean, "invstd": inv, "scale": sc, "shift": sh}
        if running:
            got.update(run_mean=rm, run_var=rv)
        assert set(got) == set(ref)
        for k in ref:
            _note("forward " + k, B.check_vec(got[k], ref[k], f"{k} (momentum {mom})"))
        assert not slab.any(), "the finalize must leave the bins zeroed"
    _unchanged(c, snap)


@pytest.mark.parametrize("L,C", [(1, 8), (10243, 200), (147, 2048)], ids=["8", "200", "2048"])
def test_bn_eval_coeff(K, L, C):
    c = _case(L, C)
    snap = _snapshot(c)
    for gamma, beta in ((c.gamma, c.beta), (None, None)):
        sc, sh = K.bn_eval_coeff(B.EPS, gamma, beta, c.rm, c.rv)
        ref = B.ref_eval_coeff(B.EPS, gamma, beta, c.rm, c.rv)
        _note("eval", max(B.check_vec(sc, ref["scale"], "scale"), B.check_vec(sh, ref["shift"], "shift")))
    _unchanged(c, snap)


def _res_variants(c):
    return (("plain", None, None, None), ("identity", c.res, None, None), ("scaled", c.res, c.rscale, c.rshift))


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_bn_apply(K, L, C):
    """Every branch of the launcher: no residual / identity residual / residual*rscale + rshift, each with and without
    ReLU, the three mask variants (bits = (y > 0) of the kernel's own y, y bitwise the unmasked variant's), and a
    separate ``out=`` buffer.  y is checked from the fp32 scale / shift the kernel is given."""
    c = _case(L, C)
    snap = _snapshot(c)
    for name, res, rsc, rsh in _res_variants(c):
        for relu in (True, False):
            ref, S = B.ref_apply(c.x, c.scale, c.shift, res, rsc, rsh, relu)
            y = K.bn_apply(c.x, c.scale, c.shift, res=res, rscale=rsc, rshift=rsh, relu=relu)
            _note("y", B.check_elem(y, ref, S, B.C_Y, f"y ({name}, relu={relu})"))
            out = torch.full((L, C), SENTINEL, device="cuda", dtype=BF)
            r = K.bn_apply(c.x, c.scale, c.shift, res=res, rscale=rsc, rshift=rsh, relu=relu, out=out)
            assert r.data_ptr() == out.data_ptr() and torch.equal(out, y)
            if relu:
                ym, bits = K.bn_apply(c.x, c.scale, c.shift, res=res, rscale=rsc, rshift=rsh, relu=True,
                                      want_mask=True)
                assert torch.equal(ym, y), name
                B.check_bits(bits, ym)
                y0, none = K.bn_apply(c.x, c.scale, c.shift, res=res, rscale=rsc, rshift=rsh, relu=True,
                                      want_mask=False)
                assert none is None and torch.equal(y0, y)
    y, bits = _relu_out(L, C)                                           # what the backward tests use as mask sources
    assert torch.equal(y, K.bn_apply(c.x, c.scale, c.shift, relu=True))
    B.check_bits(bits, y)
    _unchanged(c, snap)


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_bn_apply_embedded_buffers(K, L, C):
    """Output, residual and mask buffers each a row range inside a larger sentinel-filled allocation: the rows and
    bytes before and after must survive (a clamped prefetch of row L-1 that turned into a store, or a store past row
    L-1, would not), and the result is bitwise that of the plain call."""
    c = _case(L, C)
    snap = _snapshot(c)
    big_y = torch.full((L + 2 * PAD, C), SENTINEL, device="cuda", dtype=BF)
    big_r = torch.full((L + 2 * PAD, C), SENTINEL, device="cuda", dtype=BF)
    big_m = torch.full((L + 2 * PAD, C // 8), 0xA5, device="cuda", dtype=torch.uint8)
    y, res, bits = big_y[PAD:PAD + L], big_r[PAD:PAD + L], big_m[PAD:PAD + L]
    res.copy_(c.res)
    assert y.is_contiguous() and res.is_contiguous() and bits.is_contiguous()
    for name, r, rsc, rsh in (("plain", None, None, None), ("identity", res, None, None),
                              ("scaled", res, c.rscale, c.rshift)):
        want, wbits = K.bn_apply(c.x, c.scale, c.shift, res=None if r is None else c.res, rscale=rsc, rshift=rsh,
                                 relu=True, want_mask=True)
        y.fill_(SENTINEL)
        bits.fill_(0xA5)
        K.call("pdnn_bn_apply", K.ptr(c.x), L, C, K.ptr(c.scale), K.ptr(c.shift), K.ptr(r), K.ptr(rsc), K.ptr(rsh), 1,
               K.ptr(y), K.ptr(bits), K.stream())
        assert torch.equal(y, want) and torch.equal(bits, wbits), name
        for big, v in ((big_y, SENTINEL), (big_r, SENTINEL), (big_m, 0xA5)):
            assert bool((big[:PAD] == v).all()) and bool((big[PAD + L:] == v).all()), name
        assert torch.equal(res, c.res)
    _unchanged(c, snap)


def _check_reduce(K, c, slab, rows, x, mean, invstd, mask, what):
    dg, db = K.bn_bwd_finalize(slab, rows)
    red = B.ref_bwd_reduce(c.gy, x, mean, invstd, mask)
    _note("dgamma", B.check_vec(dg, red["dgamma"], "dgamma " + what))
    _note("dbeta", B.check_vec(db, red["dbeta"], "dbeta " + what))
    assert not slab.any(), "the finalize must leave the bins zeroed"


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_bn_bwd_reduce(K, L, C):
    """bn_bwd_reduce + bn_bwd_finalize: sum gm and sum gm*xhat per channel for mask mode 0, mode 1 on bn_apply's y,
    mode 2 on the exact-coefficient mask (x*mscale + mshift, with entries exactly zero: masked), mode 3 on bn_apply's
    bits; and with a second BN (x2) for modes 0, 1, 3, where both slabs are checked."""
    c = _case(L, C)
    snap = _snapshot(c)
    y0, bits0 = (t.clone() for t in _relu_out(L, C))
    for mode in (0, 1, 2, 3):
        kw, mask = _mask_args(c, mode)
        slab, slab2, rows = K.bn_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mode=mode, **kw)
        assert slab2 is None
        _check_reduce(K, c, slab, rows, c.x, c.mean, c.invstd, mask, f"(mode {mode})")
        if mode != 2:
            slab, slab2, rows = K.bn_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mode=mode, x2=c.x2, mean2=c.mean2,
                                                invstd2=c.invstd2, **kw)
            _check_reduce(K, c, slab, rows, c.x, c.mean, c.invstd, mask, f"(mode {mode}, with x2)")
            _check_reduce(K, c, slab2, rows, c.x2, c.mean2, c.invstd2, mask, f"of the second BN (mode {mode})")
    _unchanged(c, snap)
    assert torch.equal(_relu_out(L, C)[0], y0) and torch.equal(_relu_out(L, C)[1], bits0), "a mask source was written"


# (mode, second BN, want_gm, want_dx): every branch of pdnn_bn_bwd_apply's dispatch
ALL_BRANCHES = [(0, False, False, True), (1, False, False, True), (2, False, False, True), (3, False, False, True),
                (0, True, False, True), (1, True, False, True), (3, True, False, True),
                (1, True, True, True), (3, True, True, True),
                (1, False, True, True), (2, False, True, True), (3, False, True, True),
                (1, False, True, False), (3, False, True, False)]
# the ones the ResNet blocks take: the block output's BN (+ the shortcut's BN), and gm for an unmasked residual
RESNET_BRANCHES = [(3, False, False, True), (3, True, False, True), (3, False, True, True)]


def _run_bwd_apply(K, c, branches):
    snap = _snapshot(c)
    y, bits = _relu_out(c.L, c.C)
    y0, bits0 = y.clone(), bits.clone()
    given = {}
    for mode, second, want_gm, want_dx in branches:
        kw, mask = _mask_args(c, mode)
        if mode not in given:                 # dgamma / dbeta as passed in: the float64 sums rounded to fp32
            r1 = B.ref_bwd_reduce(c.gy, c.x, c.mean, c.invstd, mask)
            r2 = B.ref_bwd_reduce(c.gy, c.x2, c.mean2, c.invstd2, mask)
            given[mode] = tuple(r[k][0].float() for r in (r1, r2) for k in ("dgamma", "dbeta"))
        dg, db, dg2, db2 = given[mode]
        if second:
            kw = dict(kw, x2=c.x2, mean2=c.mean2, invstd2=c.invstd2, gamma2=c.gamma2, dgamma2=dg2, dbeta2=db2)
        what = f"(mode {mode}, x2={second}, want_gm={want_gm}, want_dx={want_dx})"
        dx, dx2, gm = K.bn_bwd_apply(c.gy, c.x, c.mean, c.invstd, c.gamma, dg, db, mode=mode, want_dx=want_dx,
                                     want_gm=want_gm, **kw)
        assert (dx is not None) == want_dx and (dx2 is not None) == second and (gm is not None) == want_gm, what
        if want_dx:
            ref, S = B.ref_bwd_apply(c.gy, c.x, c.mean, c.invstd, c.gamma, dg, db, mask)
            _note("dx", B.check_elem(dx, ref, S, B.C_DX, "dx " + what))
        if second:
            ref, S = B.ref_bwd_apply(c.gy, c.x2, c.mean2, c.invstd2, c.gamma2, dg2, db2, mask)
            _note("dx2", B.check_elem(dx2, ref, S, B.C_DX, "dx2 " + what))
        if want_gm:
            B.check_gm(gm, c.gy, mask)
    _unchanged(c, snap)
    assert torch.equal(y, y0) and torch.equal(bits, bits0), "a mask source was written"
    return given


@pytest.mark.parametrize("L,C", B.ALL_BRANCH_SHAPES, ids=[f"{L}x{C}" for L, C in B.ALL_BRANCH_SHAPES])
def test_bn_bwd_apply_all_branches(K, L, C):
    """Every kernel of the launcher's table: modes 0-3; a second BN with modes 0, 1, 3 (and with gm for 1, 3); gm with
    modes 1, 2, 3; gm without dx with modes 1 and 3.  dx, dx2 elementwise from the dgamma / dbeta passed in, gm
    bitwise, inputs compared with clones.  Also gamma = None (the kernel's k = invstd)."""
    c = _case(L, C)
    given = _run_bwd_apply(K, c, ALL_BRANCHES)
    dg, db = given[0][:2]
    dx, _, _ = K.bn_bwd_apply(c.gy, c.x, c.mean, c.invstd, None, dg, db, mode=0)
    ref, S = B.ref_bwd_apply(c.gy, c.x, c.mean, c.invstd, None, dg, db, None)
    _note("dx", B.check_elem(dx, ref, S, B.C_DX, "dx (gamma None)"))


@pytest.mark.parametrize("L,C", B.SHAPES, ids=IDS)
def test_bn_bwd_apply_resnet_branches(K, L, C):
    """The branches the ResNet blocks take, at every shape: mode 3 alone, with the shortcut's BN, and with gm."""
    _run_bwd_apply(K, _case(L, C), RESNET_BRANCHES)


# ------------------------------------------------------------------------------------------------ guards
def _bad_vectors(v):
    """wrong dtype, wrong length (short, long), not contiguous"""
    C = v.numel()
    return {"fp64": v.double(), "bf16": v.to(BF), "short": v[:C - 8], "long": torch.cat([v, v[:8]]),
            "strided": torch.stack([v, v], 1)[:, 0]}


def _bad_acts(t):
    """wrong dtype, a row short, a column slice of a wider tensor, transposed storage, 1-D"""
    L, C = t.shape
    wide = torch.cat([t, t], 1)
    return {"fp32": t.float(), "fp16": t.half(), "short": t[:L - 1], "slice": wide[:, :C],
            "transposed": t.t().contiguous().t(), "flat": t.reshape(-1)}


def test_bn_entry_points_reject_bad_arguments(K, monkeypatch):
    """Every wrapper raises ValueError before anything is launched.  For the duration of the checks ``kernels.call``
    is a stub that fails the test if anything reaches it, so no bad combination can launch whatever the state of the
    guards; afterwards one well-formed call of each wrapper still goes through."""
    L, C = 6, 64
    g = torch.Generator(device="cuda").manual_seed(3)
    act = lambda l=L, ch=C: torch.randn(l, ch, device="cuda", generator=g).to(BF)
    vec = lambda ch=C: torch.rand(ch, device="cuda", generator=g) + 0.5
    x, gy, res, x2, y = act(), act(), act(), act(), act()
    mean, inv, gamma, dg, db, sc, sh = (vec() for _ in range(7))
    bits = torch.zeros(L, C // 8, device="cuda", dtype=torch.uint8)
    second = dict(x2=x2, mean2=mean, invstd2=inv, gamma2=gamma, dgamma2=dg, dbeta2=db)

    def launched(name, *a):
        pytest.fail(f"{name} reached the launcher")

    def slab(ch=C, rows=2 * K.STAT_BINS):
        return torch.zeros(rows, ch, device="cuda")

    monkeypatch.setattr(K, "call", launched)
    no = pytest.raises(ValueError)
    # channel counts no kernel handles: C > 2048 (RPI = 0) and C % 8 != 0, in every wrapper
    for ch in (2056, 4096, 12, 4):
        xb, gb, v = act(2, ch), act(2, ch), vec(ch)
        with no:
            K.bn_stats(xb)
        with no:
            K.bn_apply(xb, v, v)
        with no:
            K.bn_bwd_reduce(gb, xb, v, v)
        with no:
            K.bn_bwd_apply(gb, xb, v, v, v, v, v)
        with no:
            K.bn_finalize(slab(ch), K.STAT_BINS, 2, 1e-5, 0.1, v, v, None, None)
        with no:
            K.bn_bwd_finalize(slab(ch), K.STAT_BINS)
    # variants without a kernel, and outputs that would come back uninitialised
    with no:
        K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=2, mscale=sc, mshift=sh, **second)
    with no:
        K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=0, want_gm=True)
    with no:
        K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=3, msrc=bits, want_dx=False, want_gm=True, **second)
    with no:
        K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=0, want_dx=False)
    with no:
        K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=0, want_dx=False, want_gm=True)
    with no:
        K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=2, mscale=sc, mshift=sh, want_dx=False, want_gm=True)
    with no:
        K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=1, msrc=y, want_dx=False)
    for mode in (4, -1):
        with no:
            K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=mode, msrc=y)
        with no:
            K.bn_bwd_reduce(gy, x, mean, inv, mode=mode, msrc=y)
    # operands a mode or a variant needs and would read through null
    for mode in (1, 3):
        with no:
            K.bn_bwd_reduce(gy, x, mean, inv, mode=mode)
        with no:
            K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=mode)
    for kw in (dict(mscale=sc), dict(mshift=sh), {}):
        with no:
            K.bn_bwd_reduce(gy, x, mean, inv, mode=2, **kw)
        with no:
            K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=2, **kw)
    for missing in ("mean2", "invstd2", "dgamma2", "dbeta2"):
        with no:
            K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, **{k: v for k, v in second.items() if k != missing})
    for missing in ("mean2", "invstd2"):
        with no:
            K.bn_bwd_reduce(gy, x, mean, inv, x2=x2, **{k: second[k] for k in ("mean2", "invstd2") if k != missing})
    with no:
        K.bn_apply(x, sc, sh, rscale=sc, rshift=sh)                     # coefficients of a residual that is not there
    with no:
        K.bn_apply(x, sc, sh, res=res, rscale=sc)
    with no:
        K.bn_apply(x, sc, sh, res=res, rshift=sh)
    with no:
        K.bn_apply(x, sc, sh, relu=False, want_mask=True)
    with no:
        K.bn_finalize(slab(), K.STAT_BINS, L, 1e-5, 0.1, gamma, gamma, mean, None)
    with no:
        K.bn_finalize(slab(), K.STAT_BINS, 0, 1e-5, 0.1, gamma, gamma, None, None)
    with no:
        K.bn_finalize(slab(rows=64), 32, L, 1e-5, 0.1, gamma, gamma, None, None)
    with no:
        K.bn_finalize(slab().double(), K.STAT_BINS, L, 1e-5, 0.1, gamma, gamma, None, None)
    with no:
        K.bn_bwd_finalize(slab(rows=64), 32)
    with no:
        K.bn_bwd_finalize(slab(), K.STAT_BINS, dgamma=dg)
    with no:
        K.bn_bwd_finalize(slab(), K.STAT_BINS, acc=(dg, None))
    with no:
        K.bn_stats(x[:0])
    # the mode-3 mask must be bn_apply's [L][C/8] uint8 bits
    for what, m in {"y": y, "[L][C] bytes": torch.zeros(L, C, device="cuda", dtype=torch.uint8),
                    "int8": bits.to(torch.int8), "short": bits[:L - 1], "narrow": bits[:, :C // 8 - 1],
                    "flat": bits.reshape(-1)}.items():
        with no:
            K.bn_bwd_reduce(gy, x, mean, inv, mode=3, msrc=m)
        with no:
            K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=3, msrc=m)
    with no:
        K.bn_bwd_reduce(gy, x, mean, inv, mode=1, msrc=bits)
    # dtypes, shapes, contiguity of the activations
    for what, b in _bad_acts(x).items():
        if what != "short":                             # as x itself, a shorter tensor is just a smaller L
            with no:
                K.bn_stats(b)
            with no:
                K.bn_apply(b, sc, sh)
        with no:
            K.bn_apply(x, sc, sh, res=b)
        with no:
            K.bn_apply(x, sc, sh, out=b)
        with no:
            K.bn_bwd_reduce(b, x, mean, inv)
        with no:
            K.bn_bwd_reduce(gy, b, mean, inv)
        with no:
            K.bn_bwd_reduce(gy, x, mean, inv, mode=1, msrc=b)
        with no:
            K.bn_bwd_reduce(gy, x, mean, inv, x2=b, mean2=mean, invstd2=inv)
        with no:
            K.bn_bwd_apply(b, x, mean, inv, gamma, dg, db)
        with no:
            K.bn_bwd_apply(gy, b, mean, inv, gamma, dg, db)
        with no:
            K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=1, msrc=b)
        with no:
            K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, **dict(second, x2=b))
    # dtypes and lengths of the per-channel vectors, position by position
    for what, b in _bad_vectors(mean).items():
        for i in range(2):
            a = [sc, sh]
            a[i] = b
            with no:
                K.bn_apply(x, *a)
            with no:
                K.bn_apply(x, sc, sh, res=res, rscale=a[0], rshift=a[1])
            with no:
                K.bn_bwd_reduce(gy, x, *a)
            with no:
                K.bn_bwd_reduce(gy, x, mean, inv, mode=2, mscale=a[0], mshift=a[1])
            with no:
                K.bn_bwd_reduce(gy, x, mean, inv, x2=x2, mean2=a[0], invstd2=a[1])
            with no:
                K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, mode=2, mscale=a[0], mshift=a[1])
            with no:
                K.bn_finalize(slab(), K.STAT_BINS, L, 1e-5, 0.1, *a, None, None)
            with no:
                K.bn_finalize(slab(), K.STAT_BINS, L, 1e-5, 0.1, gamma, gamma, *a)
            with no:
                K.bn_bwd_finalize(slab(), K.STAT_BINS, *a)
            with no:
                K.bn_bwd_finalize(slab(), K.STAT_BINS, acc=tuple(a))
            with no:
                K.bn_eval_coeff(1e-5, *([b, sh] if i == 0 else [sc, b]), mean, inv)
        if what != "long":                              # a longer running mean alone just defines a larger C
            with no:
                K.bn_eval_coeff(1e-5, gamma, gamma, b, inv)
        with no:
            K.bn_eval_coeff(1e-5, gamma, gamma, mean, b)
        for i in range(5):
            a = [mean, inv, gamma, dg, db]
            a[i] = b
            with no:
                K.bn_bwd_apply(gy, x, *a)
        for k in ("mean2", "invstd2", "gamma2", "dgamma2", "dbeta2"):
            with no:
                K.bn_bwd_apply(gy, x, mean, inv, gamma, dg, db, **dict(second, **{k: b}))
    monkeypatch.undo()
    # one well-formed call of each wrapper still goes through
    s, rows = K.bn_stats(x)
    m_, i_, sc_, sh_ = K.bn_finalize(s, rows, L, 1e-5, 0.1, gamma, gamma, mean.clone(), inv.clone())
    K.bn_eval_coeff(1e-5, gamma, None, mean, inv)
    yy, bb = K.bn_apply(x, sc_, sh_, res=res, rscale=sc, rshift=sh, relu=True, want_mask=True)
    s, s2, rows = K.bn_bwd_reduce(gy, x, m_, i_, mode=3, msrc=bb, x2=x2, mean2=m_, invstd2=i_)
    dg_, db_ = K.bn_bwd_finalize(s, rows)
    dg2_, db2_ = K.bn_bwd_finalize(s2, rows, acc=(dg.clone(), db.clone()))
    dx, dx2, gm = K.bn_bwd_apply(gy, x, m_, i_, gamma, dg_, db_, mode=3, msrc=bb, x2=x2, mean2=m_, invstd2=i_,
                                 gamma2=None, dgamma2=dg2_, dbeta2=db2_, want_gm=True)
    assert torch.isfinite(dx.float()).all() and torch.isfinite(dx2.float()).all() and torch.isfinite(gm.float()).all()


def test_bn_c_entry_points_refuse_before_launching(K):
    """The C entry points themselves return hipErrorInvalidValue (HipError here) for C % 8 != 0, C > 2048, L < 1, a
    null required pointer and a variant the dispatch table has no kernel for; each check sits before the grid is
    computed and before any launch.  pdnn_bn_reduce_rows answers 0 for such C where it used to divide by zero."""
    from pytorch_distributed_nn_amd.ops._backend import HipError, lib
    L, C = 6, 64
    x = torch.zeros(L, C, device="cuda", dtype=BF)
    o = torch.zeros(L, C, device="cuda", dtype=BF)
    v = torch.ones(C, device="cuda")
    slab = torch.zeros(2 * K.STAT_BINS, C, device="cuda")
    bits = torch.zeros(L, C // 8, device="cuda", dtype=torch.uint8)
    p, st = K.ptr, K.stream()
    for ch in (2056, 12, 0):
        assert lib().pdnn_bn_reduce_rows(L, ch) == 0
    assert lib().pdnn_bn_reduce_rows(L, C) == 1
    no = pytest.raises(HipError)
    for l, ch in ((L, 2056), (L, 12), (L, 0), (0, C), (-1, C)):
        with no:
            K.call("pdnn_bn_stats", p(x), l, ch, p(slab), st)
        with no:
            K.call("pdnn_bn_apply", p(x), l, ch, p(v), p(v), None, None, None, 1, p(o), None, st)
        with no:
            K.call("pdnn_bn_bwd_reduce", p(x), p(x), l, ch, p(v), p(v), 0, None, None, None, p(slab), None, None, None,
                   None, st)
        with no:
            K.call("pdnn_bn_bwd_apply", p(x), p(x), l, ch, p(v), p(v), p(v), p(v), p(v), 0, None, None, None, p(o),
                   None, None, None, None, None, None, None, None, st)
    for ch in (2056, 12, 0):
        with no:
            K.call("pdnn_bn_finalize", p(slab), K.STAT_BINS, ch, float(L), 1e-5, 0.1, None, None, None, None, p(v),
                   p(v), p(v), p(v), st)
        with no:
            K.call("pdnn_bn_bwd_finalize", p(slab), K.STAT_BINS, ch, p(v), p(v), 0, None, None, st)
    with no:
        K.call("pdnn_bn_finalize", p(slab), K.STAT_BINS, C, 0.0, 1e-5, 0.1, None, None, None, None, p(v), p(v), p(v),
               p(v), st)
    with no:
        K.call("pdnn_bn_finalize", p(slab), K.STAT_BINS, C, float(L), 1e-5, 0.1, None, None, p(v), None, p(v), p(v),
               p(v), p(v), st)
    with no:
        K.call("pdnn_bn_bwd_finalize", p(slab), K.STAT_BINS, C, None, p(v), 0, None, None, st)
    with no:                                                        # mask bits without ReLU
        K.call("pdnn_bn_apply", p(x), L, C, p(v), p(v), None, None, None, 0, p(o), p(bits), st)
    with no:                                                        # rscale without a residual
        K.call("pdnn_bn_apply", p(x), L, C, p(v), p(v), None, p(v), p(v), 1, p(o), None, st)
    with no:                                                        # no output
        K.call("pdnn_bn_apply", p(x), L, C, p(v), p(v), None, None, None, 1, None, None, st)
    for mode, msrc, msc, msh in ((1, None, None, None), (3, None, None, None), (2, None, p(v), None),
                                 (2, None, None, p(v)), (4, p(x), p(v), p(v))):
        with no:
            K.call("pdnn_bn_bwd_reduce", p(x), p(x), L, C, p(v), p(v), mode, msrc, msc, msh, p(slab), None, None,
                   None, None, st)
        with no:
            K.call("pdnn_bn_bwd_apply", p(x), p(x), L, C, p(v), p(v), p(v), p(v), p(v), mode, msrc, msc, msh, p(o),
                   None, None, None, None, None, None, None, None, st)
    with no:                                                        # x2 without its slab
        K.call("pdnn_bn_bwd_reduce", p(x), p(x), L, C, p(v), p(v), 0, None, None, None, p(slab), p(x), p(v), p(v),
               None, st)

    def bwd_apply(mode, dx, x2, dx2, gm, dg2=p(v)):
        K.call("pdnn_bn_bwd_apply", p(x), p(x), L, C, p(v), p(v), p(v), p(v), p(v), mode, p(bits if mode == 3 else x),
               p(v), p(v), dx, x2, p(v), p(v), p(v), dg2, p(v), dx2, gm, st)
    o2, o3 = torch.zeros_like(o), torch.zeros_like(o)
    for args in ((2, p(o), p(x), p(o2), None),          # second BN with mode 2
                 (0, p(o), None, None, p(o3)),          # gm with mode 0
                 (0, None, None, None, None),           # no dx: modes 0, 2, a second BN, no gm
                 (2, None, None, None, p(o3)),
                 (3, None, p(x), p(o2), p(o3)),
                 (1, None, None, None, None),
                 (1, p(o), p(x), None, None),           # x2 without dx2
                 (1, p(o), None, p(o2), None)):         # dx2 without x2
        with no:
            bwd_apply(*args)
    with no:
        bwd_apply(1, p(o), p(x), p(o2), None, dg2=None)
    assert not o.any() and not o2.any() and not o3.any() and not slab.any(), "a refused call wrote an output"
