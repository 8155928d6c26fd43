"""csrc/kernels/gemm_skinny_pro.hip on the GPU: the LayerNorm prologue's image against the float64 LayerNorm of
attn_ref (the bound of the LayerNorm forward's own test), and the GEMM behind the image bit for bit against gemm_skinny /
gemm_skinny_fp8."""
import pytest
import torch

import attn_ref as A
from test_gemm_skinny_gpu import K, _sentinel, guard_intact, guarded   # noqa: F401  (K: the kernels fixture)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# M: one row | no divisor of any NW | the full tile.  D: 64 = 8 chunks, lanes 8..63 idle | 520 = chunk 65, a second chunk
# for lane 0 only | the model width | the limit.  N: a ragged single group | full + ragged.  Rotated, not crossed.
MS, DS, NS = [1, 5, 16], [64, 520, 768, 2048], [8, 40]
SHAPES = [(MS[i % 3], D, NS[i % 2]) for i, D in enumerate(DS)] + [(16, 2048, 8), (5, 64, 40)]
SITES = [("qkv", dict(bias=True, act=0)), ("fc", dict(bias=True, act=2)), ("plain", dict(bias=False, act=0))]


def _weights(K, N, D, seed):
    """-> {"bf16": w, "fp8": (q, inv)} (fp8 only where D % 16 == 0), bias fp32 [N]"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, D, generator=g) * 0.5).to(BF).cuda()
    ws = {"bf16": w}
    if D % 16 == 0:
        ws["fp8"] = K.quant_rows_e4m3(w)
    return ws, torch.randn(N, generator=g).cuda()


def _unfused(K, x, w, **kw):
    return K.gemm_skinny_fp8(x, *w, **kw) if isinstance(w, tuple) else K.gemm_skinny(x, w, **kw)


@pytest.mark.parametrize("M,D,N", SHAPES)
def test_ln_image_against_fp64_and_gemm_bits(K, M, D, N):
    c = A.case_to(A.gen_ln(M, D), "cuda")          # rows cycle through Gaussian, mean 100 sigma, constant, ...
    ref = A.ref_layernorm_fwd(c.x, c.gamma, c.beta)[0]
    ws, bias = _weights(K, N, D, 7 * M + D + N)
    xbuf = torch.full((M + 2, D + 8), float("nan"), dtype=BF, device="cuda")      # a padded row stride
    xbuf[:M, :D] = c.x
    for fmt, w in ws.items():
        for site, opt in SITES:
            for pad in (0, 8):
                image = _sentinel(torch.empty(M, D, dtype=BF, device="cuda"))
                obuf, y = guarded(M, N, pad)
                b = bias if opt["bias"] else None
                K.gemm_skinny_ln(xbuf[:M, :D], c.gamma, c.beta, A.EPS, w, bias=b, act=opt["act"], out=y, image=image)
                guard_intact(obuf, M, N, site)
                worst = A.check_bound(image, ref, f"image {fmt} {site}")
                assert torch.equal(y, _unfused(K, image, w, bias=b, act=opt["act"])), (fmt, site, pad)
    print(f"{(M, D, N)}: image worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("r", [0, 7, 15])
def test_row_invariance(K, r):
    c = A.case_to(A.gen_ln(16, 768), "cuda")
    ws, bias = _weights(K, 40, 768, 3)
    for w in ws.values():
        y = K.gemm_skinny_ln(c.x, c.gamma, c.beta, A.EPS, w, bias=bias, act=2)
        assert torch.equal(y[r:r + 1], K.gemm_skinny_ln(c.x[r:r + 1], c.gamma, c.beta, A.EPS, w, bias=bias, act=2))


def test_guards(K):
    from pytorch_distributed_nn_amd.ops._backend import lib, ptr, stream
    dev = dict(device="cuda")
    x = torch.zeros(17, 2056 + 8, dtype=BF, **dev)
    gam, w = torch.ones(2056, **dev), torch.zeros(8, 2056, dtype=BF, **dev)
    out = _sentinel(torch.empty(17, 8, dtype=BF, **dev))

    def ln(M, D, xs=None, **kw):
        xs = x[:M, :D] if xs is None else xs
        return K.gemm_skinny_ln(xs, gam[:D], gam[:D], 1e-5, w[:, :D].contiguous(), out=out[:M], **kw)
    bad = [lambda: ln(17, 768), lambda: ln(2, 2056), lambda: ln(2, 12),
           lambda: ln(2, 768, x.view(-1)[1:1 + 2 * 768].view(2, 768)),                       # a misaligned x
           lambda: ln(2, 768, image=torch.empty(2 * 768 + 8, dtype=BF, **dev)[1:1 + 2 * 768].view(2, 768))]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    # the C entries refuse the same before any launch
    L = lib()
    args = lambda M, D: (ptr(x), x.stride(0), ptr(gam), ptr(gam), 1e-5, ptr(w), ptr(out), 8, M, 8, D, None, 0, None, stream())   # noqa: E731
    assert L.pdnn_gemm_skinny_ln(*args(17, 768)) != 0 and L.pdnn_gemm_skinny_ln(*args(2, 2056)) != 0
    assert L.pdnn_gemm_skinny_ln(*args(2, 12)) != 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), _sentinel(torch.empty_like(out)).view(torch.int16)), "a refused call wrote out"
