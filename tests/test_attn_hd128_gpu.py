"""The head-dim-128 flash kernels (csrc/kernels/attention_hd128.hip) through K.flash_attn_fwd / _bwd against the float64
chain reference of tests/attn_ref.py (ref_chain, written with the head dim as an argument), element by element, with the
chain's own constants: the chain rounds P and dS to bf16 as these kernels' MFMA operands do, and the bounds are sums of
term magnitudes, so they follow the reduction length.  Shapes: one tile; two query tiles with an odd head count; an odd
count of 128-tiles with a batch stride.

Measured error / bound on an MI355X (y, dV, dQ, dK): 1x128x1 causal 0.688 0.719 0.335 0.495, full 0.600 0.640 0.323
0.408; 1x256x3 causal 0.716 0.807 0.359 0.410, full 0.650 0.719 0.280 0.296; 2x384x2 causal 0.747 0.844 0.462 0.444, full
0.766 0.700 0.318 0.317; lse2 <= 0.027.  The constants are the chain's, none was fitted: the dQ kernel forms
delta = sum_k P dP as the chain does (the kernel file's header says why; with delta = rowsum(dO . O) from the bf16 O,
dQ measured 1.07 - 2.93 here, and the d = 64 kernels' dQ 1.906 under the same bound at (1, 256, 3, 64))."""
import functools
import math

import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu
D = 128
SC = 1.0 / math.sqrt(D)
CONST = {n: A.C["ch_" + n] for n in ("y", "dV", "dQ", "dK")}          # the chain's own constants, unchanged
SHAPES = [(1, 128, 1), (1, 256, 3), (2, 384, 2)]
CASES = [(s, c) for s in SHAPES for c in (True, False)]
IDS = [f"{'x'.join(map(str, s))}-{'causal' if c else 'full'}" for s, c in CASES]


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import kernels, _backend
    assert _backend.available()
    return kernels


@functools.lru_cache(maxsize=None)
def _case(shape, causal):
    B, T, H = shape
    qkv, dO = (t.cuda() for t in A.gen_chain(B, T, H, D))
    return qkv, dO, A.ref_chain(qkv, dO, B, T, H, D, causal)


def _ref_lse2(qkv, B, T, H, causal):
    """attn_ref.ref_flash_fwd's lse2 and its bound, at this head dim"""
    q, k, _ = (t.double() for t in A.split_heads(qkv, B, T, H, D))
    c = A.f32(SC) * A.LOG2E
    s2, aqk = c * (q @ k.transpose(-1, -2)), c * (q.abs() @ k.abs().transpose(-1, -2))
    if causal:
        s2 = s2.masked_fill(A.above_diag(T, qkv.device), float("-inf"))
    m = s2.max(-1, keepdim=True).values
    lse2 = m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))
    mag = (torch.exp2(s2 - lse2) * aqk).sum(-1) + lse2.squeeze(-1).abs() + A.RESC + math.log2(T)
    return A.Vec(lse2.squeeze(-1), A.C["lse2"] * A.U * mag + A.U * lse2.squeeze(-1).abs())


@pytest.mark.parametrize("shape,causal", CASES, ids=IDS)
def test_forward_backward_float64(K, shape, causal):
    B, T, H = shape
    qkv, dO, ref = _case(shape, causal)
    out, lse2 = K.flash_attn_fwd(qkv, B, T, H, SC, causal)
    dqkv = K.flash_attn_bwd(qkv, out, dO, lse2, B, T, H, SC, causal)
    got = dict(A.dqkv_parts(dqkv, B, T, H, D), y=A.heads(out, B, T, H, D))
    A.check_f32(lse2, _ref_lse2(qkv, B, T, H, causal), "lse2")
    failed = []
    for n in ("y", "dV", "dK", "dQ"):              # every output is checked; the failures are reported together
        try:
            print(n, "worst error / bound", A.check_bf16(got[n], ref[n], CONST[n], n))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masked_keys_contribute_nothing(K, shape):
    """NaN in the K and V rows of the last 128 tokens of one (b, h): every query before them is finite and unchanged"""
    B, T, H = shape
    qkv, dO, _ = _case(shape, True)
    out, lse2 = K.flash_attn_fwd(qkv, B, T, H, SC, True)
    dqkv = K.flash_attn_bwd(qkv, out, dO, lse2, B, T, H, SC, True)
    b, h = B - 1, H - 1
    bad = qkv.clone()
    k, v = A.split_heads(bad, B, T, H, D)[1:]
    k[b, h, T - 128:] = float("nan")
    v[b, h, T - 128:] = float("nan")
    assert bad.isnan().sum().item() == 2 * 128 * D
    out2, lse2b = K.flash_attn_fwd(bad, B, T, H, SC, True)
    dqkv2 = K.flash_attn_bwd(bad, out2, dO, lse2b, B, T, H, SC, True)
    keep = torch.ones(B, H, T, dtype=torch.bool, device="cuda")
    keep[b, h, T - 128:] = False
    for name, x, y in (("out", A.heads(out, B, T, H, D), A.heads(out2, B, T, H, D)), ("lse2", lse2, lse2b),
                       ("dQ", A.dqkv_parts(dqkv, B, T, H, D)["dQ"], A.dqkv_parts(dqkv2, B, T, H, D)["dQ"])):
        assert torch.isfinite(y[keep].float()).all(), name
        assert A.bits_equal(x[keep], y[keep]), name


def test_repeatable_and_inputs_untouched(K):
    B, T, H = shape = (1, 256, 3)
    qkv, dO, _ = _case(shape, True)
    snap = qkv.clone(), dO.clone()
    runs = []
    for _ in range(2):
        out, lse2 = K.flash_attn_fwd(qkv, B, T, H, SC, True)
        runs.append((out, lse2, K.flash_attn_bwd(qkv, out, dO, lse2, B, T, H, SC, True)))
    for x, y in zip(*runs):
        assert A.bits_equal(x, y), "not repeatable: a race"
    assert torch.equal(qkv, snap[0]) and torch.equal(dO, snap[1]), "a kernel wrote to one of its inputs"


def test_guards(K, monkeypatch):
    B, T, H = 1, 128, 2
    bf = lambda *s: torch.zeros(*s, device="cuda", dtype=A.BF)                  # noqa: E731
    qkv, out, lse2 = bf(T, 3 * H * D), bf(T, H * D), torch.zeros(B, H, T, device="cuda")
    ib = torch.zeros(B, T, device="cuda", dtype=torch.int32)
    state = torch.zeros(2, device="cuda", dtype=torch.int64)
    delta, dqkv = torch.zeros_like(lse2), torch.zeros_like(qkv)
    monkeypatch.setattr(K, "call", lambda *a: pytest.fail(f"{a[0]} was called"))
    for q, t, kw in ((bf(T, 3 * H * 96), T, {}), (bf(64, 3 * H * D), 64, {}), (qkv, T, {"doc": (ib, ib)}),
                     (qkv, T, {"drop": (0.1, state, 0)})):
        with pytest.raises(ValueError):
            K.flash_attn_fwd(q, B, t, H, SC, **kw)
        with pytest.raises(ValueError):
            K.flash_attn_bwd(q, out, out, lse2, B, t, H, SC, **kw)
    p, L, st = K.ptr, K.lib(), K.stream()
    for t, h, l2 in ((64, H, lse2), (T, 0, lse2), (T, H, None)):
        assert L.pdnn_flash_attn_hd128_fwd(p(qkv), p(out), p(l2), B, t, h, SC, 1, st) != 0
        assert L.pdnn_flash_attn_hd128_bwd(p(qkv), p(out), p(out), p(l2), p(delta), p(dqkv), B, t, h, SC, 1, st) != 0
