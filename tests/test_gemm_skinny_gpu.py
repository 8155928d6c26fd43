"""The skinny-M weight-streaming GEMM (csrc/kernels/gemm_skinny.hip, ops.kernels.gemm_skinny) and the decode embedding
gather (ops.kernels.embedding_decode) on the GPU.

Reference check: every case of tests/gemm_skinny_ref.py, every element, against the float64 reference with gemm_ref's
bounds; the integer family bit for bit.  x is a view into a larger buffer whose pad columns and rows from M on hold NaN
(poisoned family; 777 elsewhere), w a view with such rows before row 0 and after row N - 1; out is a view into a buffer
of sentinels with guard rows before and after and pad columns, all bitwise untouched after the call, and the 16-row tile's
rows >= M with them; the inputs are bitwise unchanged; two calls give the same bits.  Batch invariance: row b of an M-row
call is bitwise the 1-row call on that row, whatever the other rows hold.  Guards raise before anything is launched.  One
captured call replays bitwise.  The worst error / bound is printed.

Recorded on an MI355X: y_bf16 0.995, gelu_y_noaux 0.931 (the bf16 rounding of the result itself; the integer family exact).
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import gemm_ref as A
import gemm_skinny_ref as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
WORST = {}
GUARD = 18                                       # guard rows before and after an output: more than a 16-row tile
ALL_SHAPES = S.SHAPES + S.BIG


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import kernels, _backend
    assert _backend.available(), "HIP kernel library must load on a GPU box"
    return kernels


def _sentinel(t):
    t.view(torch.int16).fill_(0x7FC1)            # a NaN bit pattern no kernel produces
    return t


def guarded(M, N, pad, fill=None):
    buf = _sentinel(torch.empty(M + 2 * GUARD, N + pad, dtype=BF, device="cuda"))
    view = buf[GUARD:GUARD + M, :N]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def tail_rows_written(buf, M, N):
    """rows >= M (guard rows after the view) that no longer hold the sentinel"""
    want = _sentinel(torch.empty_like(buf[GUARD + M:]))
    return int((buf[GUARD + M:].view(torch.int16) != want.view(torch.int16)).any(1).sum().item())


def guard_intact(buf, M, N, what):
    want = _sentinel(torch.empty_like(buf))
    want[GUARD:GUARD + M, :N] = buf[GUARD:GUARD + M, :N]
    assert A.bits_equal(buf, want), f"{what}: written outside the output (guard rows / pad columns changed)"


def stored_x(c):
    """x [M][K] inside a buffer [M + 2][K + pad]: pad columns and the rows from M on hold NaN (poisoned) or 777"""
    buf = torch.full((c.M + 2, c.K + c.pad), float("nan") if c.poison else A.PAD_FILL, dtype=BF, device="cuda")
    buf[:c.M, :c.K] = c.a
    return buf, buf[:c.M, :c.K]


def stored_w(c):
    """w [N][K] contiguous, with two such rows before row 0 and after row N - 1"""
    buf = torch.full((c.N + 4, c.K), float("nan") if c.poison else A.PAD_FILL, dtype=BF, device="cuda")
    buf[2:2 + c.N] = c.b.t()
    return buf, buf[2:2 + c.N]


@functools.lru_cache(maxsize=None)
def _case(cid, args, opt_items):
    c = A.case_to(S.build(args, dict(opt_items)), "cuda")
    ref = S.reference(c)
    xb, x = stored_x(c)
    wb, w = stored_w(c)
    st = SimpleNamespace(x=x, w=w, res=None, bufs=[xb, wb])
    if c.res is not None:
        rb, st.res = guarded(c.M, c.N, c.pad, c.res)
        st.bufs.append(rb)
    if c.bias is not None:
        st.bufs.append(c.bias)
    st.snap = [b.clone() for b in st.bufs]
    return c, ref, st


def launch(K, c, st):
    obuf, y = guarded(c.M, c.N, c.pad)
    K.gemm_skinny(st.x, st.w, bias=c.bias, act=c.act, res=st.res, out=y)
    tail = tail_rows_written(obuf, c.M, c.N)
    if tail == 0:
        guard_intact(obuf, c.M, c.N, "y")
    return {"y": y, "tail_rows": tail}


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_skinny_reference(K, shape):
    from pytorch_distributed_nn_amd.ops._backend import lib
    assert lib().pdnn_gemm_skinny_plan(shape[1], shape[2]) == S.partition(shape[1], shape[2])[0]
    for cid, args, opt in S.cases([shape]):
        c, ref, st = _case(cid, args, tuple(sorted(opt.items())))
        try:
            o1 = launch(K, c, st)
            o2 = launch(K, c, st)
            torch.cuda.synchronize()
            for n, r in S.check(c, o1, ref).items():
                _note(n, r)
            assert torch.isfinite(o1["y"].float()).all(), "read the NaN outside an operand"
            assert A.bits_equal(o1["y"], o2["y"]), "not repeatable: a race"
            for b, s in zip(st.bufs, st.snap):
                assert A.bits_equal(b, s), "the kernel wrote to one of its inputs (or their padding)"
        except AssertionError as e:
            raise AssertionError(f"{cid}: {e}") from None


@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_batch_invariance(K, M):
    for (N, Kd), opt in (((136, 520), dict(bias=True, act=2, res=True)), ((2304, 768), dict(bias=True)),
                         ((40, 72), dict())):
        c = A.case_to(A.make("skinny", "gauss", M, N, Kd, M, **opt), "cuda")
        w = c.b.t().contiguous()
        y = K.gemm_skinny(c.a, w, bias=c.bias, act=c.act, res=c.res)
        for b in sorted({0, M // 2, M - 1}):
            one = K.gemm_skinny(c.a[b:b + 1], w, bias=c.bias, act=c.act, res=None if c.res is None else c.res[b:b + 1])
            assert A.bits_equal(y[b:b + 1], one), f"M = {M}, N = {N}, K = {Kd}: row {b} differs from its 1-row call"
            x2 = (torch.randn(M, Kd, device="cuda") * 3).to(BF)
            x2[b] = c.a[b]
            r2 = None
            if c.res is not None:
                r2 = torch.randn(M, N, device="cuda").to(BF)
                r2[b] = c.res[b]
            y2 = K.gemm_skinny(x2, w, bias=c.bias, act=c.act, res=r2)
            assert A.bits_equal(y2[b], y[b]), f"M = {M}, N = {N}, K = {Kd}: row {b} changed with the other rows"


def test_guards_raise_before_any_launch(K):
    from pytorch_distributed_nn_amd.ops._backend import lib, stream
    x = torch.zeros(4, 64, device="cuda", dtype=BF)
    w = torch.zeros(24, 64, device="cuda", dtype=BF)
    out = _sentinel(torch.empty(4, 24, device="cuda", dtype=BF))
    bad = [dict(x=torch.zeros(0, 64, device="cuda", dtype=BF)), dict(x=torch.zeros(65, 64, device="cuda", dtype=BF)),
           dict(x=torch.zeros(4, 60, device="cuda", dtype=BF), w=torch.zeros(24, 60, device="cuda", dtype=BF)),
           dict(w=torch.zeros(20, 64, device="cuda", dtype=BF)), dict(x=x.float()),
           dict(w=torch.zeros(24, 128, device="cuda", dtype=BF)[:, ::2]), dict(act=1),
           dict(res=torch.zeros(4, 32, device="cuda", dtype=BF)), dict(res=torch.zeros(5, 24, device="cuda", dtype=BF)),
           dict(bias=torch.zeros(24, device="cuda", dtype=BF)), dict(w=torch.zeros(24, 72, device="cuda", dtype=BF))]
    for kw in bad:
        a = dict(x=x, w=w, out=out)
        a.update(kw)
        if a["x"].shape[0] != 4 or a["w"].shape[0] != 24:
            a.pop("out")
        with pytest.raises(ValueError):
            K.gemm_skinny(a.pop("x"), a.pop("w"), **a)
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == 0x7FC1).all(), "a rejected call launched"
    p = lambda t: t.data_ptr()                                                       # noqa: E731
    for M, N, Kd, act in ((0, 24, 64, 0), (65, 24, 64, 0), (4, 20, 64, 0), (4, 24, 60, 0), (4, 24, 64, 1), (4, 0, 64, 0)):
        assert lib().pdnn_gemm_skinny(p(x), 64, p(w), p(out), 24, M, N, Kd, None, act, None, stream()) != 0
    assert lib().pdnn_gemm_skinny(None, 64, p(w), p(out), 24, 4, 24, 64, None, 0, None, stream()) != 0
    assert lib().pdnn_gemm_skinny(p(x), 56, p(w), p(out), 24, 4, 24, 64, None, 0, None, stream()) != 0    # ldx < K
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == 0x7FC1).all(), "a rejected entry-point call launched"
    assert K.SKINNY_MAX_M in (1, 2, 4, 8, 16, 32, 64)


def test_graph_capture_replays_on_new_contents(K):
    c = A.case_to(A.make("skinny", "gauss", 5, 136, 520, 0, bias=True, act=2, res=True), "cuda")
    w = c.b.t().contiguous()
    x, out = c.a.clone(), torch.empty(5, 136, device="cuda", dtype=BF)
    K.gemm_skinny(x, w, bias=c.bias, act=c.act, res=c.res, out=out)                  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                        # one stream
        K.gemm_skinny(x, w, bias=c.bias, act=c.act, res=c.res, out=out)
    x.copy_((torch.randn(5, 520, device="cuda") * 2).to(BF))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert A.bits_equal(out, K.gemm_skinny(x, w, bias=c.bias, act=c.act, res=c.res))


@pytest.mark.parametrize("B,D", [(1, 8), (3, 128), (16, 768)])
def test_embedding_decode_is_the_torch_expression(K, B, D):
    V, P = 97, 12
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + D)
    wte = torch.randn(V, D, device="cuda", generator=g).to(BF)
    wpe = torch.randn(P, D, device="cuda", generator=g).to(BF)
    last = P - 1
    tok = torch.randint(0, V, (B,), device="cuda", generator=g)
    lens = torch.randint(0, P, (B,), device="cuda", generator=g).int()
    tok[0], lens[0] = 0, last + 5                                     # above last
    if B > 1:
        tok[1], lens[1] = V - 1, 0
        tok[2], lens[2] = 3, -4                                       # negative: clamped to 0
    snap = (tok.clone(), lens.clone(), wte.clone(), wpe.clone())
    x = K.embedding_decode(tok, lens, wte, wpe)
    pos = lens.long().clamp(0, last)
    want = (wte.index_select(0, tok).float() + wpe.index_select(0, pos).float()).to(BF)
    assert A.bits_equal(x, want)
    out = torch.empty(B, D, device="cuda", dtype=BF)
    assert K.embedding_decode(tok, lens, wte, wpe, out=out) is out and A.bits_equal(out, want)
    # malformed tokens: the address is clamped before the load (embedding_decode_kernel), so some finite row, no fault
    for badtok in (-1, V):
        bad = tok.clone()
        bad[-1] = badtok
        xb = K.embedding_decode(bad, lens, wte, wpe)
        torch.cuda.synchronize()
        assert torch.isfinite(xb.float()).all()
        assert A.bits_equal(xb[-1], (wte[min(max(badtok, 0), V - 1)].float() + wpe[pos[-1]].float()).to(BF))
    for a, b in zip((tok, lens, wte, wpe), snap):
        assert A.bits_equal(a, b)
    for kw in (dict(tok=tok.int()), dict(lens=lens.long()), dict(wpe=wpe[:, :D - 8] if D > 8 else wpe.float()),
               dict(lens=lens[:0])):
        a = dict(tok=tok, lens=lens, wte=wte, wpe=wpe)
        a.update(kw)
        with pytest.raises(ValueError):
            K.embedding_decode(a["tok"], a["lens"], a["wte"], a["wpe"])
