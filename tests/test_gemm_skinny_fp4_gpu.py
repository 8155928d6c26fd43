"""csrc/kernels/gemm_skinny_fp4.hip on the GPU.  Quantiser: bit for bit ops/quant.py, |dq - w| <= max(2^-2 |w|, 2^-2 2^e).
GEMM: every element against gemm_ref's float64 reference on the exact dq, bounds unchanged from the fp8 test; K over the
load (32), unit (256), step (512) and plan edges, one and two row groups per wave with equal bits."""
import pytest
import torch

import gemm_ref as A
from gemm_skinny_ref import VARIANTS
from test_gemm_skinny_gpu import K, _sentinel, guard_intact, guarded   # noqa: F401  (K: the kernels fixture)
from pytorch_distributed_nn_amd.ops._backend import lib, stream
from pytorch_distributed_nn_amd.ops.quant import dequantize_blocks as _dq, quantize_blocks_reference

pytestmark = pytest.mark.gpu
BF, U8 = torch.bfloat16, torch.uint8
MS, NS = [1, 16, 17, 33, 64], [8, 24, 136]
KS = [32, 96, 224, 256, 288, 480, 512, 544, 736, 768, 800, 1056, 2208, 4640]
SHAPES = [(MS[i % 5], NS[i % 3], k) for i, k in enumerate(KS)]
SHAPES += [(3, 2304, 768), (2, 4104, 224), (5, 8, 10272)]       # 10272: a slice of three steps, the weight ring wraps


@pytest.mark.parametrize("N,Kd", [(8, 32), (24, 160), (136, 768), (8, 4640)])
def test_quantiser_is_the_definition(K, N, Kd):
    g = torch.Generator().manual_seed(N + Kd)
    w = torch.randn(N, Kd, generator=g) * torch.logspace(-3, 2, N)[:, None]
    w[0] = 0.0                                   # zero blocks
    w[2] = w[3] = torch.randn(Kd, generator=g).clamp(-0.7, 0.7)
    w[2, 5], w[3, 5] = 0.75, -0.75390625         # amax = 6 * 2^-3, and the next bf16 above it: e = -3 | -2
    w[4, :8] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, -2.5, 3.5, -5.0])     # amax 6, e = 0: every tie
    w[4, 8:32] = 0.0
    w = w.to(BF)
    q, sc = K.quant_blocks_mxfp4(w.cuda())
    q_ref, sc_ref = quantize_blocks_reference(w)
    assert sc_ref[0, 0] == 127 and sc_ref[2, 0] == 124 and sc_ref[3, 0] == 125 and q_ref[4, :4].tolist() == [0x07, 0x22, 0xC4, 0xE6]
    assert torch.equal(sc.cpu(), sc_ref) and torch.equal(q.cpu(), q_ref)
    wd, s = w.double(), torch.ldexp(torch.ones(N, Kd // 32, dtype=torch.float64), sc_ref.int() - 127).repeat_interleave(32, 1)
    assert ((_dq(q, sc).cpu().double() - wd).abs() <= torch.maximum(0.25 * wd.abs(), 0.25 * s)).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_against_fp64(K, shape):
    M, N, Kd = shape
    assert lib().pdnn_gemm_skinny_fp4_plan(N, Kd) in (2, 3, 4, 6, 8)
    si, worst, nb = SHAPES.index(shape), 0.0, Kd // 32
    for vi, (name, opt) in enumerate(VARIANTS):
        fam, pad = ("gauss", "poisoned")[(si + vi) % 2], 8 * ((si + vi) // 2 % 2)
        c = A.case_to(A.make("skinny", fam, M, N, Kd, si + vi, pad=pad, **opt), "cuda")
        q, sc = K.quant_blocks_mxfp4(c.b.t().contiguous())
        qbuf = torch.full((N + 4, Kd // 2), 0x77, dtype=U8, device="cuda")      # guard codes 6.0 around q
        qbuf[2:2 + N] = q
        sflat = torch.full((N * nb + 64,), 0xFF, dtype=U8, device="cuda")       # guard scales NaN around sc; an odd base
        scv = sflat[32 + vi % 2:32 + vi % 2 + N * nb].view(N, nb)               # for every other variant
        scv.copy_(sc)
        c.b = _dq(q, sc).t()                     # the kernel's weight, exactly: the reference is a bf16 GEMM on it
        ref = A.reference(c)
        xbuf = torch.full((M + 2, Kd + pad), float("nan"), dtype=BF, device="cuda")
        xbuf[:M, :Kd] = c.a
        rbuf, res = guarded(M, N, pad, c.res) if c.res is not None else (None, None)
        bufs = [t for t in (xbuf, qbuf, sflat, rbuf, c.bias) if t is not None]
        snap = [b.clone() for b in bufs]
        ys = []
        for groups in (0, 1, 2) if M <= 32 else (0, 1):
            obuf, y = guarded(M, N, pad)
            K.gemm_skinny_fp4(xbuf[:M, :Kd], qbuf[2:2 + N], scv, bias=c.bias, act=c.act, res=res, out=y, groups=groups)
            guard_intact(obuf, M, N, name)
            ys.append(y)
        torch.cuda.synchronize()
        assert torch.isfinite(ys[0].float()).all(), f"{name}: read the NaN outside an operand"
        worst = max(worst, *A.check(c, {"y": ys[0]}, ref).values())
        for y in ys[1:]:
            assert A.bits_equal(ys[0], y), f"{name}: not repeatable, or the bits depend on the row groups per wave"
        for b, s in zip(bufs, snap):
            assert A.bits_equal(b, s), f"{name}: the kernel wrote to one of its inputs"
    print(f"{shape}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("M", [1, 17, 64])
def test_batch_invariance(K, M):
    for (N, Kd), act in (((136, 544), 2), ((24, 2208), 0)):
        c = A.case_to(A.make("skinny", "gauss", M, N, Kd, M, bias=True, act=act, res=True), "cuda")
        q, sc = K.quant_blocks_mxfp4(c.b.t().contiguous())
        y = K.gemm_skinny_fp4(c.a, q, sc, bias=c.bias, act=c.act, res=c.res)
        for b in sorted({0, M // 2, M - 1}):
            one = K.gemm_skinny_fp4(c.a[b:b + 1], q, sc, bias=c.bias, act=c.act, res=c.res[b:b + 1])
            assert A.bits_equal(y[b:b + 1], one), f"M = {M}, N = {N}, K = {Kd}: row {b} differs from its 1-row call"
            x2 = (torch.randn(M, Kd, device="cuda") * 3).to(BF)
            r2 = torch.randn(M, N, device="cuda").to(BF)
            x2[b], r2[b] = c.a[b], c.res[b]
            y2 = K.gemm_skinny_fp4(x2, q, sc, bias=c.bias, act=c.act, res=r2)
            assert A.bits_equal(y2[b], y[b]), f"M = {M}, N = {N}, K = {Kd}: row {b} changed with the other rows"


def test_guards_raise_before_any_launch(K):
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)                       # noqa: E731
    L, p = lib(), (lambda t: t.data_ptr())
    ok = dict(x=z(4, 64), q=z(24, 32, dt=U8), sc=z(24, 2, dt=U8), act=0, out=_sentinel(torch.empty(4, 24, device="cuda", dtype=BF)))
    for kw in (dict(x=z(0, 64), out=None), dict(x=z(65, 64), out=None), dict(x=z(4, 80), q=z(24, 40, dt=U8)), dict(act=1),
               dict(q=z(20, 32, dt=U8), sc=z(20, 2, dt=U8), out=None), dict(x=z(4, 64).float()), dict(q=z(24, 48, dt=U8)),
               dict(q=z(24, 64, dt=U8)[:, ::2]), dict(res=z(4, 32)), dict(bias=z(24)), dict(sc=z(24, 3, dt=U8)),
               dict(sc=z(24, 2, dt=torch.int8)), dict(groups=3), dict(x=z(40, 64), out=None, groups=2)):
        a = {**ok, **kw}
        with pytest.raises(ValueError):
            K.gemm_skinny_fp4(a.pop("x"), a.pop("q"), a.pop("sc"), **a)
    for M, N, Kd, act, ldx, px in ((0, 24, 64, 0, 64, 1), (65, 24, 64, 0, 64, 1), (4, 20, 64, 0, 64, 1), (4, 24, 80, 0, 80, 1),
                                   (4, 24, 64, 1, 64, 1), (4, 24, 64, 0, 56, 1), (4, 24, 64, 0, 64, 0)):
        assert L.pdnn_gemm_skinny_fp4(p(ok["x"]) * px or None, ldx, p(ok["q"]), p(ok["sc"]), p(ok["out"]), 24, M, N, Kd, None,
                                      act, None, stream()) != 0
    assert L.pdnn_gemm_skinny_fp4_rg(p(ok["x"]), 64, p(ok["q"]), p(ok["sc"]), p(ok["out"]), 24, 40, 24, 64, None, 0, None, 2,
                                     stream()) != 0
    for N, Kd in ((24, 80), (20, 64), (24, 16), (0, 64)):          # the shapes the wrappers refuse, and only those
        with pytest.raises(ValueError):
            K.quant_blocks_mxfp4(z(N, Kd))
        assert L.pdnn_gemm_skinny_fp4_plan(N, Kd) == 0
        assert L.pdnn_quant_blocks_mxfp4(p(ok["x"]), N, Kd, p(ok["q"]), p(ok["sc"]), stream()) != 0
    assert L.pdnn_gemm_skinny_fp4_plan(8, 32) > 0
    torch.cuda.synchronize()
    assert (ok["out"].view(torch.int16) == 0x7FC1).all(), "a rejected call launched"
