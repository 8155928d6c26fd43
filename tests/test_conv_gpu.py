"""The direct stride-1 convolution kernels (csrc/kernels/conv3x3.hip, conv1x1_wide.hip, the epilogues and operand
prologues of conv_direct.h) and the stride-2 halo kernels (conv_s2.hip) against the float64 reference of tests/conv_ref.py, element by element, over every element,
with the bounds derived there; the integer family bit for bit.

Every case is called on the kernel's own entry (conv3x3 under set_conv3x3_mode(1, nb) for nb in auto / 1 / 64 / 128 with
pdnn_conv3x3_force(1), conv1x1_panel); a data gradient's weight is made from the layer's weight by conv3x3_flip /
transpose_bf16 and must equal the case's kernel-layout weight bit for bit.  test_public_routes_give_the_same_bits sends
cases through conv_fwd / conv_dgrad (set_panel_mode(1), tuning wide1x1_dgrad = 1) and asks for the direct call's bits.
Where a forced nb does not apply (nb = 1 off the 64 -> 64 shapes or with a prologue, nb = 128 at Co % 128 != 0) the
kernel falls back and the case is still checked.

Every case also asserts: outputs (y / gm, dt_out, pro_out, dW) are views into sentinel-filled buffers with guard rows,
bitwise intact after the call -- except y where the entry allocates it itself and takes no out= (conv3x3s2, conv_fwd,
conv_dgrad with the fused BN backward): there only dt_out / pro_out are guarded; the inputs (x and pre's t between NaN rows in the poisoned family, 777 elsewhere) are bitwise unchanged;
the call run twice gives the same bits for y and dt_out (the slab is summed by atomics: both runs meet its bound); the
slab comes from stat_bins and is read as the existing tests read it.  The worst error / bound per output kind is printed.

Which case runs which kernel template (conv_ref.all_cases(); every shape of a list runs every variant named):
  conv3x3_kernel<NB, EPI, PRE, 0, FP>   NB = 128: the Co = 128 shapes of HALO under nb = 0 / 128; NB = 64: every shape
        under nb = 64, the Co = 64 / 192 shapes under any nb.  EPI plain / stats / res (res, resmask) / bnb with
        PRE = false: fwd_plain, dg_plain / fwd_stats / dg_res, dg_resmask / dg_bnb; PRE = true: dg_pre1_plain /
        dg_pre2_stats / dg_pre2_resmask, dg_pre1_res / dg_pre1_bnb; FP: fwd_pro_plain, fwd_pro_stats
  conv3x3_w64_kernel<EPI>               the 64 -> 64 shapes of HALO under nb = 1: fwd_plain / fwd_stats / dg_res,
        dg_resmask / dg_bnb (W = 85, its widest, among them)
  conv1x1_areg_kernel<KC, NB, EPI, PRE, FP>   (1, 64) K = 64, (2, 64) K = 128, (4, 32) K = 256, AREG_KN x AREG_P: each
        of the 12 variants of V_AREG at steps == 1 (N = 64 / 128) and steps > 1 (N = 192 / 320; K = 256, N = 192 is
        g = 2 with 3 steps), and AREG_BIG (513 pixel tiles: g = 1, 2 steps)
  conv3x3s2_kernel<DG, EPI, PRE, FP>    S2 x V_S2 (test_s2_halo): DG = false: fwd_plain / fwd_stats, FP: fwd_pro_plain,
        fwd_pro_stats and with pro_out fwd_pro2_plain, fwd_pro2_stats; DG = true, plain / bnb: dg_plain / dg_bnb,
        PRE: dg_pre1_plain, dg_pre2_plain / dg_pre1_bnb, dg_pre2_bnb
  conv3x3s2_dgrad_pair_kernel<EPI>      dg_plain / dg_bnb of S2 again under tuning s2_halo | 128
  conv3x3_wgrad_kernel<FP> + reduce<PG> WGRAD direct stride-1 shapes (test_wgrad), pro0 / pro1; PG = 1 and PG = 2 (G = 16)
  conv3x3s2_wgrad_kernel<FP>            the stride-2 shapes of WGRAD at Wo = 7 / 14 / 28 under s2_halo | 8
  pp_wgrad (ping-pong 1x1)              wg 1x1x256 64 -> 128; its fallback pdnn_conv_wgrad at 1x1x250 and with pro=
  pdnn_conv_fwd / pdnn_conv_dgrad / pdnn_conv_wgrad (implicit GEMM)   GEN x V_GEN (test_implicit_gemm_fallback, every
        direct route off: set_conv3x3_mode(0), set_panel_mode(0), s2_halo = 0, wide1x1_dgrad = 0) and the C = 72 /
        odd-size / H = 1 shapes of WGRAD
  conv1x1_wide_kernel<EPI, PRE>         WIDE_KN x WIDE_P: the 9 variants of V_WIDE; K = 8192 with PRE (WIDE_LONG);
        conv_dgrad's route at K = 512 -> N = 1024 (WIDE_DGRAD)
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import bn_ref as B
import conv_ref as A
from gemm_ref import bits_equal

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
WORST = {}
CASES = A.all_cases()
BY_ID = A.by_id()


def _note(r):
    for k, v in r.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import kernels, _backend
    assert _backend.available(), "HIP kernel library must load on a GPU box"
    return kernels


@pytest.fixture()
def halo_forced(K):
    oldf = K.lib().pdnn_conv3x3_force(1)
    old = K.set_conv3x3_mode(1, 0)
    yield
    K.set_conv3x3_mode(*old)
    K.lib().pdnn_conv3x3_force(oldf)


# ------------------------------------------------------------------------------------------------ buffers
def _sentinel(t):
    t.view(torch.int16).fill_(0x7FC1)
    return t


def _guard(c):
    return 2 * c.img[2] + 8 if c.T == 9 else 8


def stored(t, g, poison):
    """[P][C] -> (buffer [g + P + g][C] with NaN (poisoned) or 777 rows around, the contiguous view of t inside)"""
    buf = torch.full((t.shape[0] + 2 * g, t.shape[1]), float("nan") if poison else A.PAD_FILL, dtype=t.dtype, device=t.device)
    view = buf[g:g + t.shape[0]]
    view.copy_(t)
    return buf, view


def guarded(P, C, g):
    buf = _sentinel(torch.empty(P + 2 * g, C, dtype=BF, device="cuda"))
    return buf, buf[g:g + P]


def guard_intact(buf, g, what):
    want = _sentinel(torch.empty_like(buf))
    want[g:buf.shape[0] - g].copy_(buf[g:buf.shape[0] - g])
    assert bits_equal(buf, want), f"{what}: written outside the output (guard rows changed)"


@functools.lru_cache(maxsize=8)
def _case(cid):
    """the case on the GPU, its operands in storage, the layer's weight of a data gradient, the reference"""
    c = A.case_to(A.make(*BY_ID[cid]), "cuda")
    g = _guard(c)
    st = SimpleNamespace(bufs=[c.wk], g=g, res=None, rmask=None, bn=None, pt=None)
    xb, st.x = stored(c.x, g, c.poison)
    st.bufs.append(xb)
    if c.res is not None:
        b, st.res = stored(c.res, g, False)
        st.bufs.append(b)
    if c.keep is not None:
        st.rmask = B.pack_bits(c.keep).contiguous()
        st.bufs.append(st.rmask)
    if c.bn is not None:
        b, t = stored(c.bn[0], g, False)
        st.bn = (t,) + tuple(c.bn[1:])
        st.bufs += [b] + list(c.bn[1:])
    if c.pre:
        b, st.pt = stored(c.pre_ops[0], g, c.poison)
        st.bufs += [b] + list(c.pre_ops[1:])
    if c.pro:
        st.bufs += list(c.pro_ops)
    st.wl = A.layer_weight(c) if c.dgrad else None
    if st.wl is not None:
        st.bufs.append(st.wl)
    st.snap = [b.clone() for b in st.bufs]
    ref = A.reference(c)                   # (pre == 1 / pro == 2: its "dt" / "a1"; y is then checked from the kernel's own)
    return c, st, ref


def kernel_weight(K, c, st):
    """the weight the kernel takes: a data gradient's is built from the layer's weight by the project's own kernels"""
    if not c.dgrad or c.kind == "gen":
        return c.wk
    if c.T == 9:
        w = K.conv3x3_flip(st.wl.view(c.Ci, 3, 3, c.Co)).view(c.Co, 9, c.Ci)
    else:
        w = K.transpose_bf16(st.wl.view(c.Ci, c.Co)).view(c.Co, 1, c.Ci)
    assert bits_equal(w, c.wk), "conv3x3_flip / transpose_bf16: not W'[c][tap][k] = W[k][8 - tap][c]"
    return w


def launch(K, c, st, w):
    """one call into fresh guarded outputs -> {"y", "dt"?, "slab"?}; asserts the guards and the inputs"""
    Nimg, H, W = c.img
    ybuf, y = guarded(c.Po, c.Co, st.g)
    dbuf = dt = abuf = a1 = None
    pre = None
    if c.pre:
        if c.pre == 1:
            dbuf, dt = guarded(c.P, c.Ci, st.g)
        pre = (st.pt,) + tuple(c.pre_ops[1:]) + (dt,)
    kw = dict(want_stats=c.epi == "stats", res=st.res, bn=st.bn, res_mask=st.rmask, pre=pre, pro=c.pro_ops)
    if c.kind == "gen":
        # the implicit-GEMM fallback through the public entries with every direct route switched off; conv_fwd and the
        # fused-BN conv_dgrad allocate y themselves (no out=): no guard rows there
        R = c.R
        if not c.dgrad:
            y, slab = K.conv_fwd(st.x.view(Nimg, H, W, c.Ci), w.view(c.Co, R, R, c.Ci), c.st, c.pad, pro=c.pro_ops,
                                 want_stats=c.epi == "stats")
            ybuf = None
        else:
            Ho, Wo = A.out_hw(c.img, R, c.st, c.pad)
            bn = None if st.bn is None else (st.bn[0].view(Nimg, H, W, c.Co),) + st.bn[1:]
            got = K.conv_dgrad(st.x.view(Nimg, Ho, Wo, c.Ci), st.wl.view(c.Ci, R, R, c.Co), (Nimg, H, W, c.Co), c.st, c.pad,
                               res=None if st.res is None else st.res.view(Nimg, H, W, c.Co), bn=bn, res_mask=st.rmask,
                               out=None if bn is not None else y.view(Nimg, H, W, c.Co))
            if bn is not None:
                y, slab = got
                ybuf = None
            else:
                slab = None
        y = y.reshape(c.Po, c.Co)
    elif c.kind == "s2":
        # conv3x3s2 allocates y itself (no out=): the guarded outputs here are dt_out and pro_out
        xin = (Nimg, H // 2, W // 2, c.Ci) if c.dgrad else (Nimg, H, W, c.Ci)
        if c.pro == 2:
            abuf, a1 = guarded(c.P, c.Ci, st.g)
        bn = None if st.bn is None else (st.bn[0].view(Nimg, H, W, c.Co),) + st.bn[1:]
        y, slab = K.conv3x3s2(st.x.view(*xin), w.view(c.Co, 3, 3, c.Ci), dgrad=c.dgrad, want_stats=c.epi == "stats", bn=bn,
                              pre=pre, pro=c.pro_ops, pro_out=None if a1 is None else a1.view(*xin))
        y = y.view(c.Po, c.Co)
        ybuf = None
    elif c.T == 9:
        _, slab = K.conv3x3(st.x.view(Nimg, H, W, c.Ci), w.view(c.Co, 3, 3, c.Ci), out=y.view(Nimg, H, W, c.Co), **kw)
    else:
        _, slab = K.conv1x1_panel(st.x, w.view(c.Co, c.Ci), out=y, **kw)
    torch.cuda.synchronize()
    if ybuf is not None:
        guard_intact(ybuf, st.g, "y")
    outs = {"y": y}
    if a1 is not None:
        guard_intact(abuf, st.g, "pro_out")
        outs["a1"] = a1
    if dt is not None:
        guard_intact(dbuf, st.g, "dt_out")
        outs["dt"] = dt
    if c.epi in ("stats", "bnb"):
        assert slab is not None and slab.shape == (2 * K.STAT_BINS, c.Co)
        outs["slab"] = A.slab_totals(slab, c.Co)
    else:
        assert slab is None
    for b, s in zip(st.bufs, st.snap):
        assert bits_equal(b, s), "a kernel wrote to one of its inputs (or the rows around them)"
    return outs


def run_case(K, cid):
    c, st, ref = _case(cid)
    w = kernel_weight(K, c, st)
    o1 = launch(K, c, st, w)
    r = A.check(c, o1, ref)
    o2 = launch(K, c, st, w)
    assert bits_equal(o1["y"], o2["y"]), "y differs between two runs"
    for k in ("dt", "a1"):
        if k in o1:
            assert bits_equal(o1[k], o2[k]), k + " differs between two runs"
    if "slab" in o2:                                   # atomics: the second run's slab meets the bound too
        ref2 = A.ref_slab(c, o2["y"])
        for i, k in enumerate(("slab_s", "slab_q")):
            A._check_vec64(o2["slab"][i], ref2[k][0], ref2[k][1], k + " (second run)")
    _note(r)
    return r


# ------------------------------------------------------------------------------------------------ tests
def test_predicates_match_their_mirror(K, halo_forced):
    lib = K.lib()
    for W in list(range(1, 131)) + [255, 256, 257]:
        for Ci, Co in ((64, 64), (64, 128), (128, 192), (72, 64), (64, 32)):
            assert lib.pdnn_conv3x3_supported(1, 3, W, Ci, Co) == int(A.halo_supported(3 * W, W, Ci, Co)), (W, Ci, Co)
    for _, (kind, img, Ci, Co, _, _) in CASES["halo"]:
        assert lib.pdnn_conv3x3_supported(*img, Ci, Co) == 1
    for W in range(2, 140, 2):
        assert lib.pdnn_conv3x3s2_supported(1, 4, W, 128, 256) == int(A.s2_supported(4, W, 128, 256)), W
    assert lib.pdnn_conv3x3s2_supported(1, 3, 4, 128, 128) == 0 and lib.pdnn_conv3x3s2_supported(1, 4, 4, 64, 128) == 0
    for _, (kind, img, Ci, Co, vn, _) in CASES["s2"]:
        lc = (Co, Ci) if A.VARIANT[vn][1] else (Ci, Co)
        assert lib.pdnn_conv3x3s2_supported(*img, *lc) == 1
    for _, (kind, img, Ci, Co, _, _) in CASES["areg"]:
        assert lib.pdnn_conv1x1_panel_supported(img[2], Ci, Co) == 1
    for _, (kind, img, Ci, Co, _, _) in CASES["wide"]:
        assert lib.pdnn_conv1x1_wide_supported(img[2], Ci, Co) == 1
    assert lib.pdnn_conv1x1_wide_supported(257, 8256, 64) == 0 and lib.pdnn_conv1x1_wide_supported(257, 520, 64) == 0


@pytest.mark.parametrize("cid", [cid for cid, _ in CASES["halo"]])
def test_halo3x3(K, halo_forced, cid):
    for nb in A.HALO_NB:
        K.set_conv3x3_mode(1, nb)
        run_case(K, cid)


@pytest.mark.parametrize("cid", [cid for cid, _ in CASES["s2"]])
def test_s2_halo(K, cid):
    """forward and data gradient of the stride-2 halo kernels; a data gradient without pre= runs on the per-class kernel
    and on the class-pair kernel (tuning s2_halo bit 128); all four parity classes are in dx and are all compared"""
    from pytorch_distributed_nn_amd import tuning
    v = A.VARIANT[BY_ID[cid][4]]
    old = tuning.get("s2_halo")
    try:
        for pair in ((0, 1) if v[1] and not v[3] else (0,)):
            tuning.set("s2_halo", (old & ~128) | (128 if pair else 0))
            run_case(K, cid)
    finally:
        tuning.set("s2_halo", old)


@pytest.fixture()
def direct_routes_off(K):
    """every direct kernel switched off: conv_fwd / conv_dgrad / conv_wgrad fall back to the implicit-GEMM engine"""
    from pytorch_distributed_nn_amd import tuning
    old3, oldp = K.set_conv3x3_mode(0), K.set_panel_mode(0)
    olds, oldw = tuning.set("s2_halo", 0), tuning.set("wide1x1_dgrad", 0)
    yield
    tuning.set("wide1x1_dgrad", oldw)
    tuning.set("s2_halo", olds)
    K.set_panel_mode(oldp)
    K.set_conv3x3_mode(*old3)


@pytest.mark.parametrize("cid", [cid for cid, _ in CASES["gen"]])
def test_implicit_gemm_fallback(K, direct_routes_off, cid):
    run_case(K, cid)


WG = dict(A.wgrad_cases())


@pytest.mark.parametrize("cid", list(WG))
def test_wgrad(K, cid):
    """conv_wgrad on every route (conv_ref.wg_route, asserted against the library's predicates), accumulated into a
    non-zero fp32 dW inside a guarded buffer; inputs unchanged; two runs give the same bits on the direct routes (block
    partials + an ordered reduce), and both meet the bound on the others (split-K slabs / atomics)"""
    from pytorch_distributed_nn_amd import tuning
    c = A.case_to(A.wg_make(*WG[cid]), "cuda")
    Nimg, H, W = c.img
    Ho, Wo = A.out_hw(c.img, c.R, c.st, c.pad)
    route = A.wg_route(c.img, (c.R, c.st, c.pad), c.Ci, c.Co, c.pro)
    lib = K.lib()
    assert (lib.pdnn_conv3x3_wgrad_supported(Nimg, H, W, c.Ci, c.Co) == 1) == (route == "direct") or (c.R, c.st) != (3, 1)
    if (c.R, c.st) == (3, 2):
        assert (lib.pdnn_conv3x3s2_wgrad_supported(Nimg, H, W, c.Ci, c.Co) == 1) == (route == "direct_s2")
    e = A.wg_reference(c)
    g = 8
    xb, x = stored(c.x, 2 * W + 8, c.poison)
    db, dy = stored(c.dy, 2 * W + 8, c.poison)
    ins = [xb, db] + list(c.pro_ops or ())
    snap = [t.clone() for t in ins]
    old = tuning.set("s2_halo", tuning.get("s2_halo") | 8)
    try:
        outs = []
        for _ in range(2):
            buf = torch.empty(c.Co * c.T + 2 * g, c.Ci, device="cuda")
            buf.view(torch.int32).fill_(0x7FC00001)
            out = buf[g:g + c.Co * c.T].view(c.Co, c.R, c.R, c.Ci)
            out.copy_(c.old.view(c.Co, c.R, c.R, c.Ci))
            K.conv_wgrad(x.view(Nimg, H, W, c.Ci), dy.view(Nimg, Ho, Wo, c.Co), c.R, c.R, c.st, c.pad, pro=c.pro_ops, out=out)
            torch.cuda.synchronize()
            want = torch.empty_like(buf)
            want.view(torch.int32).fill_(0x7FC00001)
            want[g:-g].copy_(buf[g:-g])
            assert bits_equal(buf, want), "dW: written outside the output (guard rows changed)"
            for t, sn in zip(ins, snap):
                assert bits_equal(t, sn), "conv_wgrad wrote to one of its inputs (or the rows around them)"
            outs.append(out.reshape(c.Co, c.T, c.Ci).clone())
            _note({"dW_" + route: A.wg_check(c, outs[-1], e)})
        if route in ("direct", "direct_s2"):
            assert bits_equal(outs[0], outs[1]), "dW differs between two runs"
    finally:
        tuning.set("s2_halo", old)


@pytest.mark.parametrize("cid", [cid for cid, _ in CASES["areg"]])
def test_areg1x1(K, cid):
    run_case(K, cid)


@pytest.mark.parametrize("cid", [cid for cid, _ in CASES["wide"]])
def test_wide1x1(K, cid):
    run_case(K, cid)


ROUTED = [cid for cid, a in ([e for e in CASES["halo"] if e[1][1] in ((1, 27, 19), (3, 9, 11))]
                            + [e for e in CASES["areg"] if e[1][1][2] == 600 and e[1][3] in (192, 320)]
                            + [e for e in CASES["wide"] if e[1][3] == 1024])
          if a[4] != "dg_pre2_stats"]                  # conv_dgrad has no statistics epilogue


@pytest.mark.parametrize("cid", ROUTED)
def test_public_routes_give_the_same_bits(K, halo_forced, cid):
    """conv_fwd / conv_dgrad route these cases to the kernels above: same bits as the direct call, and inside the bounds"""
    c, st, ref = _case(cid)
    Nimg, H, W = c.img
    oldp = K.set_panel_mode(1)
    from pytorch_distributed_nn_amd import tuning
    oldw = tuning.set("wide1x1_dgrad", 1)
    try:
        direct = launch(K, c, st, kernel_weight(K, c, st))
        shp = (Nimg, H, W)
        if not c.dgrad:
            assert c.pre == 0
            y, slab = K.conv_fwd(st.x.view(*shp, c.Ci), c.wk.view(c.Co, 3 if c.T == 9 else 1, 3 if c.T == 9 else 1, c.Ci),
                                 1, 1 if c.T == 9 else 0, pro=c.pro_ops, want_stats=c.epi == "stats")
        else:
            R = 3 if c.T == 9 else 1
            wl = st.wl.view(c.Ci, R, R, c.Co)
            assert K.dgrad_pre_ok((*shp, c.Ci), tuple(wl.shape), 1, R // 2) or not c.pre
            dt = torch.empty(c.P, c.Ci, device="cuda", dtype=BF) if c.pre == 1 else None
            pre = (st.pt,) + tuple(c.pre_ops[1:]) + (dt,) if c.pre else None
            bn = None if st.bn is None else (st.bn[0].view(*shp, c.Co),) + st.bn[1:]
            got = K.conv_dgrad(st.x.view(*shp, c.Ci), wl, (*shp, c.Co), 1, R // 2,
                               res=None if st.res is None else st.res.view(*shp, c.Co), bn=bn, res_mask=st.rmask, pre=pre)
            y, slab = got if bn is not None else (got, None)
            if dt is not None:
                assert bits_equal(dt, direct["dt"])
        torch.cuda.synchronize()
        for b, sn in zip(st.bufs, st.snap):
            assert bits_equal(b, sn), "a routed call wrote to one of its inputs (or the rows around them)"
        assert bits_equal(y.reshape(c.P, c.Co), direct["y"].contiguous())
        if slab is not None:
            outs = {"y": y.reshape(c.P, c.Co), "slab": A.slab_totals(slab, c.Co)}
            for i, (k, (sref, sb)) in enumerate(A.ref_slab(c, outs["y"]).items()):
                A._check_vec64(outs["slab"][i], sref, sb, k)
    finally:
        tuning.set("wide1x1_dgrad", oldw)
        K.set_panel_mode(oldp)
