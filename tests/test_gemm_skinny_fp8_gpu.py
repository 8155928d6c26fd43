"""csrc/kernels/gemm_skinny_fp8.hip on the GPU.  Quantiser: bit for bit ops/quant.py, |dq - w| <= max(2^-4 |w|, 2^-10 inv)
(half an ulp of three mantissa bits; half the subnormal spacing).  GEMM: every element against gemm_ref's float64
reference on the exact dq, bounds unchanged; K over the load, unit, step and plan edges.  MI355X: worst error / bound 0.988."""
import pytest
import torch

import gemm_ref as A
from gemm_skinny_ref import VARIANTS
from test_gemm_skinny_gpu import K, _sentinel, guard_intact, guarded   # noqa: F401  (K: the kernels fixture)
from pytorch_distributed_nn_amd.ops._backend import lib, stream
from pytorch_distributed_nn_amd.ops.quant import dequantize_rows as _dq, quantize_rows_reference

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MS, NS = [1, 16, 17, 33, 64], [8, 24, 136]
KS = [16, 112, 128, 144, 368, 384, 400, 496, 512, 528, 640, 656, 768, 784, 896, 912, 1040, 2192, 4624]
SHAPES = [(MS[i % 5], NS[i % 3], k) for i, k in enumerate(KS)]
SHAPES += [(64, 24, 2192), (1, 136, 4624), (3, 2304, 768), (2, 4104, 208)]


@pytest.mark.parametrize("N,Kd", [(8, 16), (24, 144), (136, 768), (8, 4624)])      # 4624: past the kept chunks
def test_quantiser_is_the_definition(K, N, Kd):
    g = torch.Generator().manual_seed(N + Kd)
    w = torch.randn(N, Kd, generator=g) * torch.logspace(-3, 2, N)[:, None]
    w[0] = 0.0                                   # an all-zero row
    w[1] = torch.randn(Kd, generator=g).sign() * 300.0
    w[1, 2], w[1, 3] = 300.0 * 2.0 ** -16, -300.0 * 2.0 ** -20         # an e4m3 subnormal, and zero
    w[2] = w[3] = torch.randn(Kd, generator=g).clamp(-4, 4)
    w[2, 5], w[3, 5] = 56.0, -56.25              # amax = 448 * 2^-3, and the next bf16 above it: e = -3 | -2
    w = w.to(BF)
    q, inv = K.quant_rows_e4m3(w.cuda())
    q_ref, inv_ref = quantize_rows_reference(w)
    assert inv_ref[2].item() == 0.125 and inv_ref[3].item() == 0.25 and inv_ref[0].item() == 1.0
    assert A.bits_equal(inv.cpu(), inv_ref)
    assert torch.equal(q.cpu().view(torch.float8_e4m3fn).float(), q_ref.view(torch.float8_e4m3fn).float())
    dq, wd = _dq(q, inv).cpu().double(), w.double()
    assert dq[1, 3] == 0 and 0 < dq[1, 2] < 2.0 ** -6 * inv_ref[1].item()
    assert ((dq - wd).abs() <= torch.maximum(2.0 ** -4 * wd.abs(), 2.0 ** -10 * inv_ref.double()[:, None])).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_against_fp64(K, shape):
    M, N, Kd = shape
    assert lib().pdnn_gemm_skinny_fp8_plan(N, Kd) in (2, 3, 4, 6, 8)
    si, worst = SHAPES.index(shape), 0.0
    for vi, (name, opt) in enumerate(VARIANTS):
        fam, pad = ("gauss", "poisoned")[(si + vi) % 2], 8 * ((si + vi) // 2 % 2)
        c = A.case_to(A.make("skinny", fam, M, N, Kd, si + vi, pad=pad, **opt), "cuda")
        qbuf = torch.full((N + 4, Kd), 0x7F, dtype=torch.uint8, device="cuda")
        q, inv = K.quant_rows_e4m3(c.b.t().contiguous())
        qbuf[2:2 + N] = q
        c.b = _dq(q, inv).t()                    # the kernel's weight, exactly: the reference is a bf16 GEMM on it
        ref = A.reference(c)
        xbuf = torch.full((M + 2, Kd + pad), float("nan"), dtype=BF, device="cuda")
        xbuf[:M, :Kd] = c.a
        rbuf, res = guarded(M, N, pad, c.res) if c.res is not None else (None, None)
        bufs = [t for t in (xbuf, qbuf, inv, rbuf, c.bias) if t is not None]
        snap = [b.clone() for b in bufs]
        ys = []
        for _ in range(2):
            obuf, y = guarded(M, N, pad)
            K.gemm_skinny_fp8(xbuf[:M, :Kd], qbuf[2:2 + N], inv, bias=c.bias, act=c.act, res=res, out=y)
            guard_intact(obuf, M, N, name)
            ys.append(y)
        torch.cuda.synchronize()
        assert torch.isfinite(ys[0].float()).all(), f"{name}: read the NaN outside an operand"
        worst = max(worst, *A.check(c, {"y": ys[0]}, ref).values())
        assert A.bits_equal(ys[0], ys[1]), f"{name}: not repeatable: a race"
        for b, s in zip(bufs, snap):
            assert A.bits_equal(b, s), f"{name}: the kernel wrote to one of its inputs"
    print(f"{shape}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("M", [1, 17, 64])
def test_batch_invariance(K, M):
    for (N, Kd), act in (((136, 528), 2), ((24, 2192), 0)):
        c = A.case_to(A.make("skinny", "gauss", M, N, Kd, M, bias=True, act=act, res=True), "cuda")
        q, inv = K.quant_rows_e4m3(c.b.t().contiguous())
        y = K.gemm_skinny_fp8(c.a, q, inv, bias=c.bias, act=c.act, res=c.res)
        for b in sorted({0, M // 2, M - 1}):
            one = K.gemm_skinny_fp8(c.a[b:b + 1], q, inv, bias=c.bias, act=c.act, res=c.res[b:b + 1])
            assert A.bits_equal(y[b:b + 1], one), f"M = {M}, N = {N}, K = {Kd}: row {b} differs from its 1-row call"
            x2 = (torch.randn(M, Kd, device="cuda") * 3).to(BF)
            r2 = torch.randn(M, N, device="cuda").to(BF)
            x2[b], r2[b] = c.a[b], c.res[b]
            y2 = K.gemm_skinny_fp8(x2, q, inv, bias=c.bias, act=c.act, res=r2)
            assert A.bits_equal(y2[b], y[b]), f"M = {M}, N = {N}, K = {Kd}: row {b} changed with the other rows"


def test_guards_raise_before_any_launch(K):
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)                       # noqa: E731
    U8, L, p = torch.uint8, lib(), (lambda t: t.data_ptr())
    ok = dict(x=z(4, 64), q=z(24, 64, dt=U8), inv=torch.ones(24, device="cuda"), act=0,
              out=_sentinel(torch.empty(4, 24, device="cuda", dtype=BF)))
    for kw in (dict(x=z(0, 64), out=None), dict(x=z(65, 64), out=None), dict(x=z(4, 72), q=z(24, 72, dt=U8)), dict(act=1),
               dict(q=z(20, 64, dt=U8), inv=ok["inv"][:20], out=None), dict(x=z(4, 64).float()), dict(q=z(24, 80, dt=U8)),
               dict(q=z(24, 128, dt=U8)[:, ::2]), dict(res=z(4, 32)), dict(bias=z(24)), dict(inv=ok["inv"][:16])):
        a = {**ok, **kw}
        with pytest.raises(ValueError):
            K.gemm_skinny_fp8(a.pop("x"), a.pop("q"), a.pop("inv"), **a)
    for M, N, Kd, act, ldx, px in ((0, 24, 64, 0, 64, 1), (65, 24, 64, 0, 64, 1), (4, 20, 64, 0, 64, 1), (4, 24, 72, 0, 72, 1),
                                   (4, 24, 64, 1, 64, 1), (4, 24, 64, 0, 56, 1), (4, 24, 64, 0, 64, 0)):
        assert L.pdnn_gemm_skinny_fp8(p(ok["x"]) * px or None, ldx, p(ok["q"]), p(ok["inv"]), p(ok["out"]), 24, M, N, Kd, None,
                                      act, None, stream()) != 0
    for N, Kd in ((24, 72), (20, 64), (24, 8), (0, 64)):           # the shapes the wrappers refuse, and only those
        with pytest.raises(ValueError):
            K.quant_rows_e4m3(z(N, Kd))
        assert L.pdnn_gemm_skinny_fp8_plan(N, Kd) == 0
        assert L.pdnn_quant_rows_e4m3(p(ok["x"]), N, Kd, p(ok["q"]), p(ok["inv"]), stream()) != 0
    assert L.pdnn_gemm_skinny_fp8_plan(8, 16) > 0
    torch.cuda.synchronize()
    assert (ok["out"].view(torch.int16) == 0x7FC1).all(), "a rejected call launched"
