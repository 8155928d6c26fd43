"""csrc/kernels/gemm_wq.hip on the GPU, both formats: every element against gemm_ref's float64 reference on the exact dq
(bounds unchanged: gemm_ref.acc_const), at the edges of both tiles, of a load, of the k-step and of the double buffer;
a row's bits against the other tile, another M and other rows; the refusals.  MI355X: worst error / bound 0.996 (fp4, 129 x 72 x 64),
reached through the bf16 rounding of the result itself, as in gemm_ref."""
import pytest
import torch

import gemm_ref as A
from gemm_skinny_ref import VARIANTS
from test_gemm_skinny_gpu import K, _sentinel, guard_intact, guarded   # noqa: F401  (K: the kernels fixture)
from pytorch_distributed_nn_amd.ops._backend import lib, stream
from pytorch_distributed_nn_amd.ops.quant import dequantize_blocks, dequantize_rows

pytestmark = pytest.mark.gpu
BF, U8 = torch.bfloat16, torch.uint8
# fmt -> (quantiser, GEMM, dequantiser, K's granularity, reduction elements per byte of q)
FMT = {"fp8": ("quant_rows_e4m3", "gemm_wq_fp8", dequantize_rows, 16, 1),
       "fp4": ("quant_blocks_mxfp4", "gemm_wq_fp4", dequantize_blocks, 32, 2)}
MS = [1, 63, 64, 65, 127, 128, 129, 257]                    # the row edges of both tiles
NS = [8, 56, 64, 72, 120, 128, 136, 200]                    # one ragged tile, around both widths, a ragged second tile
KS = {"fp8": [16, 48, 64, 80, 144, 208], "fp4": [32, 64, 96, 160, 224]}     # a load, the k-step, the double-buffer wrap
BIG = {"fp8": (264, 392, 208), "fp4": (264, 392, 224)}      # several blocks both ways
SHAPES = [(f, (MS[i % 8], NS[(3 * i + 1) % 8], KS[f][i % len(KS[f])])) for f in FMT for i in range(10)]
SHAPES += [(f, s) for f in FMT for s in (BIG[f], (128, 2304, 768), (64, 768, 3072))]


def _family(i, opt, Kd):
    if Kd > 1536:               # the constant behind acc_const was measured up to K = 1536
        return ("gauss", "poisoned", "integer" if not opt.get("act") else "gauss")[i % 3]
    fam = A.FAMILIES[i % 5]
    return "gauss" if fam == "integer" and opt.get("act") else fam


@pytest.mark.parametrize("fmt,shape", SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_gemm_against_fp64(K, fmt, shape):
    (M, N, Kd), (quant, gemm, dq, _, per) = shape, FMT[fmt]
    si, worst = SHAPES.index((fmt, shape)), 0.0
    for vi, (name, opt) in enumerate(VARIANTS):
        fam = _family(si + vi, opt, Kd)
        pad = 8 if fam == "poisoned" else 8 * ((si + vi) // 2 % 2)
        c = A.case_to(A.make("wq", fam, M, N, Kd, si + vi, pad=pad, **opt), "cuda")
        q, scl = getattr(K, quant)(c.b.t().contiguous())
        qbuf = torch.full((N + 4, Kd // per), 0x7F, dtype=U8, device="cuda")     # q inside a buffer of other codes
        qbuf[2:2 + N] = q
        c.b = dq(q, scl).t()                     # the kernel's weight, exactly: the reference is a bf16 GEMM on it
        ref = A.reference(c)
        xbuf = torch.full((M + 2, Kd + 8), float("nan"), dtype=BF, device="cuda")       # NaN pad columns and rows past M
        xbuf[:M, :Kd] = c.a
        rbuf, res = guarded(M, N, pad, c.res) if c.res is not None else (None, None)
        bufs = [t for t in (xbuf, qbuf, scl, rbuf, c.bias) if t is not None]
        snap = [b.clone() for b in bufs]
        ys = []
        for _ in range(2):
            obuf, y = guarded(M, N, pad)
            getattr(K, gemm)(xbuf[:M, :Kd], qbuf[2:2 + N], scl, bias=c.bias, act=c.act, res=res, out=y)
            guard_intact(obuf, M, N, name)
            ys.append(y)
        torch.cuda.synchronize()
        assert torch.isfinite(ys[0].float()).all(), f"{name}: read the NaN outside an operand"
        worst = max(worst, *A.check(c, {"y": ys[0]}, ref).values())
        assert A.bits_equal(ys[0], ys[1]), f"{name}: not repeatable: a race"
        for b, s in zip(bufs, snap):
            assert A.bits_equal(b, s), f"{name}: the kernel wrote to one of its inputs"
    print(f"{fmt} {shape}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("fmt", list(FMT))
def test_row_bits_do_not_depend_on_m_or_tile(K, fmt):
    quant, gemm, _, gran, _ = FMT[fmt]
    M, N, Kd = 257, 136, 208 if fmt == "fp8" else 224
    c = A.case_to(A.make("wq", "gauss", M, N, Kd, 1, bias=True, act=2, res=True), "cuda")
    q, scl = getattr(K, quant)(c.b.t().contiguous())
    run = lambda x, res, **kw: getattr(K, gemm)(x, q, scl, bias=c.bias, act=2, res=res, **kw)      # noqa: E731
    other = 192 - lib().pdnn_gemm_wq_plan(M, N)                  # the tile the rule does not choose for this call
    assert other in (64, 128) and lib().pdnn_gemm_wq_plan(8192, 2304) == 128 and lib().pdnn_gemm_wq_plan(128, 768) == 64
    y = run(c.a, c.res)
    assert A.bits_equal(run(c.a, c.res, tile=other), y), "the bits depend on the tile"
    for b in (0, M // 2, M - 1):
        lo = min(b, M - 64)                                      # a 64-row call that holds row b, on the other tile
        y64 = run(c.a[lo:lo + 64], c.res[lo:lo + 64], tile=other)
        assert A.bits_equal(y64[b - lo], y[b]), f"row {b} differs in a 64-row call on the {other}-row tile"
        x2, r2 = (torch.randn(M, Kd, device="cuda") * 3).to(BF), torch.randn(M, N, device="cuda").to(BF)
        x2[b], r2[b] = c.a[b], c.res[b]
        assert A.bits_equal(run(x2, r2)[b], y[b]), f"row {b} changed with the other rows"


def test_guards_raise_before_any_launch(K):
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)                       # noqa: E731
    L, p = lib(), (lambda t: t.data_ptr())
    out = _sentinel(torch.empty(4, 24, device="cuda", dtype=BF))
    for gemm, entry, Kd, per, scl in (("gemm_wq_fp8", "pdnn_gemm_wq_fp8", 64, 1, torch.ones(24, device="cuda")),
                                      ("gemm_wq_fp4", "pdnn_gemm_wq_fp4", 64, 2, z(24, 2, dt=U8))):
        ok = dict(x=z(4, Kd), q=z(24, Kd // per, dt=U8), scl=scl, act=0, out=out)
        for kw in (dict(x=z(0, Kd), out=None), dict(x=z(4, Kd + 8), q=z(24, (Kd + 8) // per, dt=U8)), dict(act=1),
                   dict(q=z(20, Kd // per, dt=U8), scl=scl[:20], out=None), dict(x=z(4, Kd).float()), dict(tile=32),
                   dict(q=z(24, Kd // per + 16, dt=U8)), dict(q=z(24, 2 * Kd // per, dt=U8)[:, ::2]), dict(res=z(4, 32)),
                   dict(bias=z(24)), dict(scl=scl[:16]), dict(x=z(4, 2 * Kd)[:, ::2])):
            a = {**ok, **kw}
            with pytest.raises(ValueError):
                getattr(K, gemm)(a.pop("x"), a.pop("q"), a.pop("scl"), **a)
        for M, N, Kk, act, ldx, ldc, px in ((0, 24, Kd, 0, Kd, 24, 1), (4, 20, Kd, 0, Kd, 24, 1), (4, 24, Kd + 8, 0, Kd + 8, 24, 1),
                                            (4, 24, Kd, 1, Kd, 24, 1), (4, 24, Kd, 0, Kd - 8, 24, 1), (4, 24, Kd, 0, Kd, 16, 1),
                                            (4, 24, Kd, 0, Kd, 24, 0)):
            assert getattr(L, entry)(p(ok["x"]) * px or None, ldx, p(ok["q"]), p(scl), p(out), ldc, M, N, Kk, None, act, None,
                                     stream()) != 0
        assert getattr(L, entry + "_tile")(p(ok["x"]), Kd, p(ok["q"]), p(scl), p(out), 24, 4, 24, Kd, None, 0, None, 96, stream()) != 0
    assert L.pdnn_gemm_wq_plan(0, 24) == 0 and L.pdnn_gemm_wq_plan(4, 20) == 0 and L.pdnn_gemm_wq_plan(4, 24) == 64
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == 0x7FC1).all(), "a rejected call launched"
