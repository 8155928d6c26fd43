"""CPU self-check of tests/attn_ref.py: the float64 references agree with torch's float64 attention / layer norm and
their autograd, the input families have the properties their names claim, an fp32 model of every kernel stays inside
every bound on every input the GPU tests use (and its fp32 part is what attn_ref.MEASURED records, the bounds'
constants being 4x that), and each planted error leaves the bounds on at least one case the GPU suite runs.  If a model
left a bound, the bound (not a kernel) would be wrong; if a planted error passed, the inputs or bounds would be too weak."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import attn_ref as A

WORST = {}
FP32 = {}
SCALE = 0.125
MUT_SHAPES = [(1, 128, 1), (1, 256, 3)]


def _note(name, ratio, table=WORST, label="worst error / bound so far"):
    table[name] = max(table.get(name, 0.0), ratio)
    print(f"{label}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(table.items())))
    return ratio


def _fp32(name, ratio):
    _note(name, ratio, FP32, "fp32 part, worst error / (u S) so far")
    assert ratio <= A.MEASURED[name], (name, ratio, A.MEASURED[name])


@functools.lru_cache(maxsize=None)
def _flash(family, shape):
    return A.gen_flash(family, *shape, scale=SCALE)


def test_constants_are_four_times_the_measurement():
    assert all(A.C[k] == 4.0 * A.MEASURED[k] for k in A.MEASURED) and set(A.C) == set(A.MEASURED)


# ---------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("causal", [True, False])
def test_flash_ref_matches_torch_float64(causal):
    B, T, H = 1, 256, 3
    qkv, dO = _flash("gauss", (B, T, H))
    q, k, v = (t.double().detach().clone().requires_grad_(True) for t in A.split_heads(qkv, B, T, H))
    y = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=A.f32(SCALE))
    y.backward(A.heads(dO, B, T, H).double())
    eO, vl = A.ref_flash_fwd(qkv, B, T, H, SCALE, causal)
    assert torch.allclose(eO.ref, A.merge(y.detach()), rtol=1e-11, atol=1e-12)
    s = A.f32(SCALE) * (q @ k.transpose(-1, -2)).detach()
    if causal:
        s = s.masked_fill(A.above_diag(T, s.device), float("-inf"))
    assert torch.allclose(vl.ref, torch.logsumexp(s, -1) * A.LOG2E, rtol=1e-12, atol=1e-12)
    # the backward reference from the exact (unrounded) forward is autograd's gradient
    ref = A.ref_flash_bwd(qkv, eO.ref, dO, vl.ref, B, T, H, SCALE, causal)
    for n, t in (("dQ", q), ("dK", k), ("dV", v)):
        assert torch.allclose(ref[n].ref, t.grad, rtol=1e-9, atol=1e-10), n


def test_layernorm_ref_matches_torch_float64():
    c = A.gen_ln(17, 520)
    x = c.x.double().requires_grad_(True)
    g, b = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    y = F.layer_norm(x, (c.D,), g, b, A.f32(A.EPS))
    (y * c.dy.double()).sum().backward()
    (yr, _), mean, rstd = A.ref_layernorm_fwd(c.x, c.gamma, c.beta)
    assert torch.allclose(yr, y.detach(), rtol=1e-10, atol=1e-10)
    out = A.ref_layernorm_bwd(c.dy, c.x, c.gamma, mean.ref, rstd.ref, c.dres)       # float64 statistics
    assert torch.allclose(out["dx"].ref, x.grad + c.dres.double(), rtol=1e-8, atol=1e-8)
    assert torch.allclose(out["dgamma"].ref, g.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(out["dbeta"].ref, b.grad, rtol=1e-9, atol=1e-9)


def test_chain_ref_matches_torch_float64():
    B, T, H, d = 2, 72, 3, 32
    qkv, dO = A.gen_chain(B, T, H, d)
    q, k, v = (t.double().detach().clone().requires_grad_(True) for t in A.split_heads(qkv, B, T, H, d))
    y = F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=A.f32(1.0 / math.sqrt(d)))
    y.backward(A.heads(dO, B, T, H, d).double())
    ref = A.ref_chain(qkv, dO, B, T, H, d, True)
    assert torch.allclose(ref["y"].ref, y.detach(), rtol=1e-11, atol=1e-12)
    for n, t in (("dQ", q), ("dK", k), ("dV", v)):
        assert torch.allclose(ref[n].ref, t.grad, rtol=1e-9, atol=1e-10), n


@pytest.mark.parametrize("shape", A.FLASH_SHAPES, ids=str)
def test_families_are_what_they_claim(shape):
    B, T, H = shape
    c = A.f32(SCALE) * A.LOG2E
    idx = torch.arange(T)
    for fam in A.FAMILIES:
        qkv, dO = _flash(fam, shape)
        q, k, v = (t.double() for t in A.split_heads(qkv, B, T, H))
        s = c * (q @ k.transpose(-1, -2))
        if fam in ("next_key", "self_key"):
            tgt = (idx + 1) % T if fam == "next_key" else idx
            peak = s[..., idx, tgt]
            rest = s.clone()
            rest[..., idx, tgt] = float("-inf")
            assert (peak - rest.max(-1).values).min().item() >= 12.0, fam
        elif fam == "growing":
            tile = s.view(B, H, T, T // 64, 64).max(-1).values          # [.., query, tile]
            d1 = tile[..., 1] - tile[..., 0]
            assert 7.0 < d1.min().item() and d1.max().item() < 8.0      # just under RESC: the maximum stays
            if T >= 256:
                d2, d3 = tile[..., 2] - tile[..., 0], tile[..., 3] - tile[..., 2]
                assert 15.5 < d2.min().item() and (tile[..., 2] - tile[..., 1]).max().item() < 9.0
                assert d3.min().item() > 12.0
        elif fam == "shrinking":
            lse2 = torch.logsumexp(s * A.LN2, -1) * A.LOG2E
            late = (s[..., 64:] - lse2.unsqueeze(-1)).max().item()
            assert late < -150.0                                         # exp2 underflows to exactly 0 in fp32
            assert torch.exp2(torch.tensor(late, dtype=torch.float32)).item() == 0.0
        elif fam == "far_masked":
            sm = s.masked_fill(A.above_diag(T, s.device), float("-inf"))
            lse2 = torch.logsumexp(sm * A.LN2, -1) * A.LOG2E
            over = (s - lse2.unsqueeze(-1)).masked_fill(~A.above_diag(T, s.device), float("-inf")).max(-1).values
            assert (over > 130.0).float().mean().item() > 0.4            # rows with a masked key that overflows exp2
            assert torch.isinf(torch.exp2(over.max().float()))
        elif fam == "flat":
            assert (q[:, :, 3] == 0).all() and (A.heads(dO, B, T, H)[:, :, 1] == 0).all()


# ------------------------------------------------------------------------------------- models inside the bounds
@pytest.mark.parametrize("shape", A.FLASH_SHAPES, ids=str)
@pytest.mark.parametrize("family", A.FAMILIES)
def test_flash_model_inside_bounds(family, shape):
    B, T, H = shape
    qkv, dO = _flash(family, shape)
    for causal in (True, False):
        O, lse2 = A.model_flash_fwd(qkv, B, T, H, SCALE, causal)
        for n, r in A.check_flash_fwd(qkv, O, lse2, B, T, H, SCALE, causal).items():
            _note(n, r)
        eO, vl = A.ref_flash_fwd(qkv, B, T, H, SCALE, causal)
        O32, l32 = A.model_flash_fwd(qkv, B, T, H, SCALE, causal, rnd=False)
        _fp32("O", A.fp32_part(O32, eO))
        _fp32("lse2", ((l32.double() - vl.ref).abs().sub(A.U * vl.ref.abs()).clamp_min(0)
                       / ((vl.bound - A.U * vl.ref.abs()) / A.C["lse2"])).max().item())
        Og, lg = A.forward_given(qkv, B, T, H, SCALE, causal)
        dqkv = A.model_flash_bwd(qkv, Og, dO, lg, B, T, H, SCALE, causal)
        assert torch.isfinite(dqkv.float()).all()
        for n, r in A.check_flash_bwd(qkv, Og, dO, lg, dqkv, B, T, H, SCALE, causal).items():
            _note(n, r)
        ref = A.ref_flash_bwd(qkv, Og, dO, lg, B, T, H, SCALE, causal)
        got = A.dqkv_parts(A.model_flash_bwd(qkv, Og, dO, lg, B, T, H, SCALE, causal, rnd=False), B, T, H)
        for n in ("dQ", "dK", "dV"):
            _fp32(n, A.fp32_part(got[n], ref[n]))


@pytest.mark.parametrize("T", A.SOFTMAX_T)
def test_softmax_model_inside_bounds(T):
    for causal in (True, False):
        S, dP = A.gen_softmax(T, causal)
        eP, vl = A.ref_softmax_fwd(S, SCALE, causal)
        P, lse = A.model_softmax_fwd(S, SCALE, causal)
        _note("sm_P", A.check_bf16(P, eP, A.C["sm_P"], "P"))
        _note("sm_lse", A.check_f32(lse, vl, "lse"))
        P32, l32 = A.model_softmax_fwd(S, SCALE, causal, rnd=False)
        _fp32("sm_P", A.fp32_part(P32, eP))
        _fp32("sm_lse", ((l32.double() - vl.ref).abs().sub(A.U * vl.ref.abs()).clamp_min(0)
                         / ((vl.bound - A.U * vl.ref.abs()) / A.C["sm_lse"])).max().item())
        e = A.ref_softmax_bwd(P, dP, SCALE, causal)
        dS = A.model_softmax_bwd(P, dP, SCALE, causal)
        _note("sm_dS", A.check_bf16(dS, e, A.C["sm_dS"], "dS"))
        _fp32("sm_dS", A.fp32_part(A.model_softmax_bwd(P, dP, SCALE, causal, rnd=False), e))
        if causal:
            assert (dS[A._row_mask(S.shape[0], T, True, S.device)] == 0).all()


@pytest.mark.parametrize("shape", A.CHAIN_SHAPES, ids=str)
def test_chain_model_inside_bounds(shape):
    B, T, H, d = shape
    qkv, dO = A.gen_chain(B, T, H, d)
    for causal in (True, False):
        ref = A.ref_chain(qkv, dO, B, T, H, d, causal)
        got, g32 = A.model_chain(qkv, dO, B, T, H, d, causal), A.model_chain(qkv, dO, B, T, H, d, causal, rnd=False)
        for n in ref:
            key = "ch_" + n
            _note(key, A.check_bf16(got[n], ref[n], A.C[key], n))
            _fp32(key, A.fp32_part(g32[n], ref[n]))


@pytest.mark.parametrize("R,D", A.ln_cases())
def test_layernorm_model_inside_bounds(R, D):
    c = A.gen_ln(R, D)
    (yr, yb), mean, rstd = A.ref_layernorm_fwd(c.x, c.gamma, c.beta)
    y, mu, rs, var = A.model_layernorm_fwd(c.x, c.gamma, c.beta)
    _note("ln_y", A.check_bound(y, (yr, yb), "y"))
    _note("ln_mean", A.check_f32(mu, mean, "mean"))
    _note("ln_rstd", A.check_f32(rs, rstd, "rstd"))
    xd = c.x.double()
    _fp32("ln_mean", ((mu.double() - mean.ref).abs().sub(A.U * mean.ref.abs()).clamp_min(0)
                      / (A.U * xd.abs().mean(1) + 1e-300)).max().item())
    var64 = ((xd - mu.double().unsqueeze(1)) ** 2).mean(1)          # float64 around the model's own mean
    _fp32("ln_var", ((var.double() - var64).abs() / (A.U * var64 + 1e-300)).max().item())
    # y's fp32 part: against float64 arithmetic on the model's own statistics
    y32 = A.model_layernorm_fwd(c.x, c.gamma, c.beta, rnd=False)[0]
    t = (xd - mu.double().unsqueeze(1)) * rs.double().unsqueeze(1) * c.gamma.double()
    _fp32("ln_y", ((y32.double() - (t + c.beta.double())).abs() / (A.U * (t.abs() + c.beta.double().abs()) + 1e-300)).max().item())
    m_, r_ = mean.ref.float(), rstd.ref.float()
    for dres, old in ((None, None), (c.dres, None), (c.dres, (c.old_dg, c.old_db))):
        ref = A.ref_layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, dres, old)
        for order in (0, 1):
            dx, dg, db = A.model_layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, dres, old, order=order)
            _note("ln_dx", A.check_bf16(dx, ref["dx"], A.C["ln_dx"], "dx"))
            _note("ln_dgamma", A.check_f32(dg, ref["dgamma"], "dgamma"))
            _note("ln_dbeta", A.check_f32(db, ref["dbeta"], "dbeta"))
        _fp32("ln_dx", A.fp32_part(A.model_layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, dres, old, rnd=False)[0], ref["dx"]))
    xh = (xd - m_.double().unsqueeze(1)) * r_.double().unsqueeze(1)
    for t32, t64 in ((c.dy.float(), c.dy.double()), (c.dy.float() * ((c.x.float() - m_.unsqueeze(1)) * r_.unsqueeze(1)), c.dy.double() * xh)):
        for order in (0, 1):
            _fp32("ln_sum", ((A.ln_sum32(t32, order) - t64.sum(0)).abs() / (A.U * t64.abs().sum(0) + 1e-300)).max().item())


# --------------------------------------------------------------------------------------------- planted errors
def _rejected(fn, cases):
    hit = []
    for case in cases:
        try:
            fn(*case)
        except AssertionError:
            hit.append(case)
    print("rejected on", hit)
    return hit


FLASH_MUT_CASES = [(f, s, c) for f in A.FAMILIES for s in MUT_SHAPES for c in (True, False)]


@pytest.mark.parametrize("mut", [None, "mask_ge", "mask_shift", "frag_unmasked", "no_alpha_o", "no_alpha_l", "lse_base_e",
                                 "stale_tile"])
def test_planted_error_in_flash_forward(mut):
    def run(family, shape, causal):
        qkv, _ = _flash(family, shape)
        O, lse2 = A.model_flash_fwd(qkv, *shape, SCALE, causal, mut=mut)
        A.check_flash_fwd(qkv, O, lse2, *shape, SCALE, causal)
    hit = _rejected(run, FLASH_MUT_CASES)
    assert (hit == []) if mut is None else hit, mut
    if mut in ("mask_shift", "no_alpha_o", "no_alpha_l"):
        fam = {"mask_shift": "next_key", "no_alpha_o": "growing", "no_alpha_l": "growing"}[mut]
        assert any(h[0] == fam for h in hit), (mut, "the family built for it must reject it")
    if mut == "mask_ge":
        assert any(h[0] == "self_key" for h in hit)


@pytest.mark.parametrize("mut", [None, "mask_ge", "mask_shift", "frag_unmasked", "delta_neighbour", "dk_no_scale"])
def test_planted_error_in_flash_backward(mut):
    def run(family, shape, causal):
        qkv, dO = _flash(family, shape)
        Og, lg = A.forward_given(qkv, *shape, SCALE, causal)
        dqkv = A.model_flash_bwd(qkv, Og, dO, lg, *shape, SCALE, causal, mut=mut)
        A.check_flash_bwd(qkv, Og, dO, lg, dqkv, *shape, SCALE, causal)
    hit = _rejected(run, FLASH_MUT_CASES)
    assert (hit == []) if mut is None else hit, mut


@pytest.mark.parametrize("mut", ["lim_off_by_one", "tail_skipped"])
def test_planted_error_in_softmax(mut):
    def run(T, causal):
        S, _ = A.gen_softmax(T, causal)
        eP, vl = A.ref_softmax_fwd(S, SCALE, causal)
        S = torch.nan_to_num(S, nan=8.0)             # the leak must be caught by value, not by the NaN filler
        P, lse = A.model_softmax_fwd(S, SCALE, causal, mut=mut)
        A.check_bf16(P, eP, A.C["sm_P"], "P")
        A.check_f32(lse, vl, "lse")
    hit = _rejected(run, [(T, c) for T in A.SOFTMAX_T for c in (True, False)])
    assert hit, mut
    if mut == "tail_skipped":
        assert {h[0] for h in hit} == {260, 1028}     # every T with keys past a whole stride


@pytest.mark.parametrize("mut", ["unbiased", "no_dres", "s2_sign"])
def test_planted_error_in_layernorm(mut):
    def run(R, D):
        c = A.gen_ln(R, D)
        (yr, yb), mean, rstd = A.ref_layernorm_fwd(c.x, c.gamma, c.beta)
        y, mu, rs, _ = A.model_layernorm_fwd(c.x, c.gamma, c.beta, mut=mut)
        A.check_f32(rs, rstd, "rstd")
        A.check_bound(y, (yr, yb), "y")
        m_, r_ = mean.ref.float(), rstd.ref.float()
        ref = A.ref_layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, c.dres)
        dx, dg, db = A.model_layernorm_bwd(c.dy, c.x, c.gamma, m_, r_, c.dres, mut=mut)
        A.check_bf16(dx, ref["dx"], A.C["ln_dx"], "dx")
    cases = [(R, D) for R, D in A.ln_cases() if R <= 33]
    hit = _rejected(run, cases)
    assert len(hit) == len(cases), (mut, "every shape must reject it")
