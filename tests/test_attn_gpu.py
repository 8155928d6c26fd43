"""The flash-attention kernels (csrc/kernels/attention.hip), the unfused softmax kernels and attention chain, and the
LayerNorm kernels (csrc/kernels/transformer.hip) against the float64 reference of tests/attn_ref.py, element by
element, over every element, with the bounds derived there.

Part A: flash forward / backward at attn_ref.FLASH_SHAPES (one block; non-power-of-two H and B through the 1-D block
  index; an odd count of 128-tiles; long key loops), causal and not, on every input family, the backward under all eight
  (attn_bwd_wide, attn_delta_in_dq) variants on attn_ref.CROSS_SHAPES and under the defaults elsewhere.  The backward is
  handed the float64 forward rounded to bf16 / fp32.  Every call runs twice and must repeat bitwise (no atomics).
Part B: attn_softmax_fwd / bwd alone at T in {4, 12, 252, 256, 260, 1028} (the 256-key stride and its tail), rows not
  a multiple of 4, NaN above the diagonal of S and dP, dS aliasing P and not; then attention_fwd / attention_bwd end
  to end at shapes the dispatcher sends there (d != 64 or T % 128 != 0).
Part C: LayerNorm at the template boundaries (D) and the rows-per-wave loop boundaries (R) of attn_ref.ln_cases().
The worst error / bound per output is printed."""
import functools
from types import SimpleNamespace

import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCALE = 0.125
WORST = {}
VARIANTS = [(w, d) for w in (0, 1, 2, 3) for d in (0, 1)]
BWD_CASES = ([(s, w, d) for s in A.CROSS_SHAPES for w, d in VARIANTS]
             + [(s, 3, 1) for s in A.FLASH_SHAPES if s not in A.CROSS_SHAPES])


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    return ratio


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import kernels, _backend
    assert _backend.available()
    return kernels


@functools.lru_cache(maxsize=None)
def _flash(family, shape, causal):
    """inputs on the GPU, the float64 forward (reference and as handed to the backward) and backward references"""
    B, T, H = shape
    qkv, dO = (t.cuda() for t in A.gen_flash(family, B, T, H, SCALE))
    fwd = A.ref_flash_fwd(qkv, B, T, H, SCALE, causal)
    Og, lg = fwd[0].ref.to(BF).contiguous(), fwd[1].ref.float().contiguous()
    bwd = A.ref_flash_bwd(qkv, Og, dO, lg, B, T, H, SCALE, causal)
    return SimpleNamespace(qkv=qkv, dO=dO, fwd=fwd, Og=Og, lg=lg, bwd=bwd, snap=(qkv.clone(), dO.clone(), Og.clone(), lg.clone()))


def _inputs_unchanged(c):
    for t, s in zip((c.qkv, c.dO, c.Og, c.lg), c.snap):
        assert torch.equal(t, s), "a kernel wrote to one of its inputs"


# ------------------------------------------------------------------------------------------------ part A
@pytest.mark.parametrize("shape", A.FLASH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flash_forward(K, shape):
    B, T, H = shape
    for family in A.FAMILIES:
        for causal in (True, False):
            c = _flash(family, shape, causal)
            O, lse2 = K.flash_attn_fwd(c.qkv, B, T, H, SCALE, causal)
            O2, lse2b = K.flash_attn_fwd(c.qkv, B, T, H, SCALE, causal)
            assert A.bits_equal(O, O2) and A.bits_equal(lse2, lse2b), (family, causal, "not repeatable: a race")
            try:
                r = A.check_flash_fwd(c.qkv, O, lse2, B, T, H, SCALE, causal, ref=c.fwd)
            except AssertionError as e:
                raise AssertionError(f"{family}, causal={causal}: {e}") from None
            for n, v in r.items():
                _note(n, v)
            _inputs_unchanged(c)


@pytest.mark.parametrize("shape,wide,delta_in_dq", BWD_CASES,
                         ids=[f"{'x'.join(map(str, s))}-wide{w}-delta{d}" for s, w, d in BWD_CASES])
def test_flash_backward(K, shape, wide, delta_in_dq):
    B, T, H = shape
    old_w, old_d = K.tune_set("attn_bwd_wide", wide), K.tune_set("attn_delta_in_dq", delta_in_dq)
    try:
        for family in A.FAMILIES:
            for causal in (True, False):
                c = _flash(family, shape, causal)
                dqkv = K.flash_attn_bwd(c.qkv, c.Og, c.dO, c.lg, B, T, H, SCALE, causal)
                again = K.flash_attn_bwd(c.qkv, c.Og, c.dO, c.lg, B, T, H, SCALE, causal)
                assert A.bits_equal(dqkv, again), (family, causal, "not repeatable: a race")
                assert torch.isfinite(dqkv.float()).all(), (family, causal)
                try:
                    r = A.check_flash_bwd(c.qkv, c.Og, c.dO, c.lg, dqkv, B, T, H, SCALE, causal, ref=c.bwd)
                except AssertionError as e:
                    raise AssertionError(f"{family}, causal={causal}: {e}") from None
                for n, v in r.items():
                    _note(n, v)
                _inputs_unchanged(c)
    finally:
        K.tune_set("attn_bwd_wide", old_w)
        K.tune_set("attn_delta_in_dq", old_d)


# ------------------------------------------------------------------------------------------------ part B
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("T", A.SOFTMAX_T)
def test_softmax_kernels_alone(K, T, causal):
    S, dP = (t.cuda() for t in A.gen_softmax(T, causal))
    rows = S.shape[0]
    assert rows % 4 == 3
    mask = A._row_mask(rows, T, causal, S.device)
    S0, dP0 = S.clone(), dP.clone()
    P = torch.full((rows, T), 7.0, device="cuda", dtype=BF)
    lse = torch.full((rows,), float("nan"), device="cuda")
    K.attn_softmax_fwd(S, P, lse, rows, T, SCALE, causal)
    eP, vl = A.ref_softmax_fwd(S, SCALE, causal)
    _note("sm_P", A.check_bf16(P, eP, A.C["sm_P"], "P"))
    _note("sm_lse", A.check_f32(lse, vl, "lse"))
    if causal:
        assert (P[mask] == 0).all(), "P above the diagonal must be exactly 0"
    e = A.ref_softmax_bwd(P, dP, SCALE, causal)
    dS = torch.full((rows, T), 7.0, device="cuda", dtype=BF)
    P0 = P.clone()
    K.attn_softmax_bwd(P, dP, dS, rows, T, SCALE, causal)
    assert torch.equal(P, P0)
    _note("sm_dS", A.check_bf16(dS, e, A.C["sm_dS"], "dS"))
    if causal:
        assert (dS[mask] == 0).all(), "dS above the diagonal must be exactly 0"
    alias = P.clone()
    K.attn_softmax_bwd(alias, dP, alias, rows, T, SCALE, causal)              # dS written over P, as attention_bwd does
    assert A.bits_equal(alias, dS), "dS over P differs from dS into its own buffer"
    assert A.bits_equal(S.view(torch.int32), S0.view(torch.int32)) and A.bits_equal(dP.view(torch.int32), dP0.view(torch.int32))


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", A.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unfused_chain(K, shape, causal):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    B, T, H, d = shape
    assert not TX.use_flash(T, H * d, H)
    qkv, dO = (t.cuda() for t in A.gen_chain(B, T, H, d))
    ref = A.ref_chain(qkv, dO, B, T, H, d, causal)
    y, P, S = TX.attention_fwd(qkv, B, T, H, causal)
    _note("ch_y", A.check_bf16(A.heads(y, B, T, H, d), ref["y"], A.C["ch_y"], "y"))
    dqkv = TX.attention_bwd(dO, qkv, P, B, T, H, causal, dS_buf=S)
    got = A.dqkv_parts(dqkv, B, T, H, d)
    for n in ("dV", "dQ", "dK"):
        _note("ch_" + n, A.check_bf16(got[n], ref[n], A.C["ch_" + n], n))


# ------------------------------------------------------------------------------------------------ part C
@pytest.mark.parametrize("R,D", A.ln_cases())
def test_layernorm(K, R, D):
    c = A.case_to(A.gen_ln(R, D), "cuda")
    (yr, yb), mean, rstd = A.ref_layernorm_fwd(c.x, c.gamma, c.beta)
    y, mu, rs = K.layernorm_fwd(c.x, c.gamma, c.beta, A.EPS)
    _note("ln_y", A.check_bound(y, (yr, yb), "y"))
    _note("ln_mean", A.check_f32(mu, mean, "mean"))
    _note("ln_rstd", A.check_f32(rs, rstd, "rstd"))
    m_, r_ = mean.ref.float(), rstd.ref.float()              # the backward is handed the float64 statistics
    for dres, acc in ((None, False), (c.dres, False), (c.dres, True)):
        old = (c.old_dg, c.old_db) if acc else None
        ref = A.ref_layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, dres, old)
        if acc:
            dg, db = c.old_dg.clone(), c.old_db.clone()
            dx, none_g, none_b = K.layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, dres=dres, acc=(dg, db))
            assert none_g is None and none_b is None
        else:
            dx, dg, db = K.layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, dres=dres)
        dx2 = K.layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, dres=dres)[0]
        assert A.bits_equal(dx, dx2), "dx is row-local: it must repeat bitwise"
        _note("ln_dx", A.check_bf16(dx, ref["dx"], A.C["ln_dx"], "dx"))
        _note("ln_dgamma", A.check_f32(dg, ref["dgamma"], "dgamma"))
        _note("ln_dbeta", A.check_f32(db, ref["dbeta"], "dbeta"))


# ------------------------------------------------------------------------------------------------ guards
def test_wrappers_reject_bad_arguments(K, monkeypatch):
    """ValueError before anything is launched: ``kernels.call`` is a stub that fails the test if reached."""
    B, T, H = 1, 128, 1
    qkv = torch.zeros(B * T, 3 * H * 64, device="cuda", dtype=BF)
    out = torch.zeros(B * T, H * 64, device="cuda", dtype=BF)
    lse2 = torch.zeros(B, H, T, device="cuda")
    x = torch.zeros(4, 64, device="cuda", dtype=BF)
    g = torch.ones(64, device="cuda")
    v = torch.ones(4, device="cuda")

    def launched(name, *a):
        pytest.fail(f"{name} reached the launcher")

    monkeypatch.setattr(K, "call", launched)
    no = pytest.raises(ValueError)
    for b, t, h in ((0, T, H), (B, 0, H), (B, T, 0), (-1, T, H), (B, 64, H)):
        with no:
            K.flash_attn_fwd(qkv, b, t, h, SCALE)
        with no:
            K.flash_attn_bwd(qkv, out, out, lse2, b, t, h, SCALE)
    bad_lse = {"fp64": lse2.double(), "bf16": lse2.to(BF), "strided": torch.zeros(B, H, 2 * T, device="cuda")[:, :, ::2],
               "shape": lse2.reshape(B, T, H) if H > 1 else lse2[:, :, :T - 1]}
    for name, t in bad_lse.items():
        with no:
            K.flash_attn_bwd(qkv, out, out, t, B, T, H, SCALE)
    bad_out = {"fp32": out.float(), "strided": torch.zeros(B * T, 2 * H * 64, device="cuda", dtype=BF)[:, :H * 64],
               "short": out[:-1]}
    for name, t in bad_out.items():
        with no:
            K.flash_attn_bwd(qkv, t, out, lse2, B, T, H, SCALE)
    with no:
        K.flash_attn_bwd(qkv, out, out.float(), lse2, B, T, H, SCALE)
    for xb in (torch.zeros(0, 64, device="cuda", dtype=BF), torch.zeros(4, 4, device="cuda", dtype=BF),
               torch.zeros(4, 0, device="cuda", dtype=BF), torch.zeros(4, 2056, device="cuda", dtype=BF)):
        gb = torch.ones(xb.shape[1], device="cuda")
        vb = torch.ones(xb.shape[0], device="cuda")
        with no:
            K.layernorm_fwd(xb, gb, gb, A.EPS)
        with no:
            K.layernorm_bwd(xb, xb, gb, vb, vb)
    with no:
        K.layernorm_fwd(x, g.double(), g, A.EPS)
    with no:
        K.layernorm_bwd(x, x, g, v.double(), v)
    with no:
        K.layernorm_bwd(x, x, g, v, torch.ones(8, device="cuda")[::2])
    monkeypatch.undo()
    K.layernorm_fwd(x, g, g, A.EPS)                            # a well-formed call still goes through
    K.flash_attn_bwd(qkv, out, out, lse2, B, T, H, SCALE)
    torch.cuda.synchronize()


def test_c_entry_points_refuse_before_launching(K):
    from pytorch_distributed_nn_amd.ops._backend import HipError
    B, T, H = 1, 128, 1
    qkv = torch.zeros(B * T, 3 * H * 64, device="cuda", dtype=BF)
    out = torch.zeros(B * T, H * 64, device="cuda", dtype=BF)
    lse2 = torch.zeros(B, H, T, device="cuda")
    x = torch.zeros(4, 64, device="cuda", dtype=BF)
    g = torch.ones(64, device="cuda")
    v = torch.ones(4, device="cuda")
    slab = K.stat_bins(64, x.device)
    p, st = K.ptr, K.stream()
    plain = (None, None, 0.0, None, 0)                             # doc_start, doc_end, p, state, site
    no = pytest.raises(HipError)
    for b, t, h in ((0, T, H), (B, 0, H), (B, T, 0), (-1, T, H), (B, -128, H), (B, 64, H)):
        with no:
            K.call("pdnn_flash_attn_fwd", p(qkv), p(out), p(lse2), b, t, h, SCALE, 1, *plain, st)
        with no:
            K.call("pdnn_flash_attn_bwd", p(qkv), p(out), p(out), p(lse2), p(lse2), p(qkv), b, t, h, SCALE, 1, *plain, st)
    with no:
        K.call("pdnn_flash_attn_fwd", p(qkv), p(out), None, B, T, H, SCALE, 1, *plain, st)
    with no:
        K.call("pdnn_flash_attn_bwd", p(qkv), None, p(out), p(lse2), p(lse2), p(qkv), B, T, H, SCALE, 1, *plain, st)
    for rows, D in ((0, 64), (-1, 64), (4, 0), (4, 4), (4, 2056)):
        with no:
            K.call("pdnn_layernorm_fwd", p(x), p(g), p(g), p(x), p(v), p(v), rows, D, A.EPS, st)
        with no:
            K.call("pdnn_layernorm_bwd", p(x), p(x), p(g), p(v), p(v), None, p(x), p(slab), rows, D, 1, st)
    torch.cuda.synchronize()
