"""The two flash-attention entries (csrc/kernels/attention.hip: pdnn_flash_attn_fwd / _bwd, ops.kernels.flash_attn_fwd /
_bwd) choose the kernels from their optional arguments.  Here: every combination they refuse returns an error before
anything is launched, and p == 0 is the call without dropout, bit for bit, with and without document bounds."""
import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu
B, T, H = 1, 128, 1
SC = 0.125
POISON = 777.0                      # exactly representable in bf16


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import kernels, _backend
    assert _backend.available()
    return kernels


@pytest.fixture(scope="module")
def data():
    qkv, dO = (t.cuda() for t in A.gen_flash("gauss", B, T, H, SC))
    t = torch.arange(T, device="cuda", dtype=torch.int32)
    ds = torch.where(t < 60, 0, 60).to(torch.int32).expand(B, T).contiguous()       # documents [0, 60) and [60, 128)
    de = torch.where(t < 60, 60, T).to(torch.int32).expand(B, T).contiguous()
    st = torch.tensor([11, 5], dtype=torch.int64, device="cuda")
    return qkv, dO, ds, de, st


def _c_fwd(K, qkv, causal, ds, de, p, st, site, t=T):
    out = torch.full((B * T, H * 64), POISON, device="cuda", dtype=A.BF)
    lse2 = torch.full((B, H, T), POISON, device="cuda")
    rc = K.lib().pdnn_flash_attn_fwd(K.ptr(qkv), K.ptr(out), K.ptr(lse2), B, t, H, SC, causal, K.ptr(ds), K.ptr(de), p,
                                     K.ptr(st), site, K.stream())
    return rc, out, lse2


def _c_bwd(K, qkv, O, dO, l2, causal, ds, de, p, st, site, t=T):
    dqkv = torch.full_like(qkv, POISON)
    delta = torch.full((B, H, T), POISON, device="cuda")
    rc = K.lib().pdnn_flash_attn_bwd(K.ptr(qkv), K.ptr(O), K.ptr(dO), K.ptr(l2), K.ptr(delta), K.ptr(dqkv), B, t, H, SC,
                                     causal, K.ptr(ds), K.ptr(de), p, K.ptr(st), site, K.stream())
    return rc, dqkv, delta


def _refusals(data):
    """name -> (causal, doc_start, doc_end, p, state, site, T)"""
    _, _, ds, de, st = data
    return {"doc, causal = 0": (0, ds, de, 0.0, None, 0, T),
            "p > 0, causal = 0": (0, None, None, 0.1, st, 0, T),
            "p > 0, null state": (1, None, None, 0.1, None, 0, T),
            "p = 1": (1, None, None, 1.0, st, 0, T),
            "p < 0": (1, None, None, -0.1, st, 0, T),
            "site < 0": (1, None, None, 0.1, st, -1, T),
            "doc_start alone": (1, ds, None, 0.0, None, 0, T),
            "doc_end alone": (1, None, de, 0.0, None, 0, T),
            "doc_start alone, p > 0": (1, ds, None, 0.1, st, 0, T),
            # an argument check only: nothing is launched, so the buffers stay those of T = 128
            "p > 0, T > 65536": (1, None, None, 0.1, st, 0, 65536 + 128)}


def test_c_entries_refuse_without_launching(K, data):
    qkv, dO = data[:2]
    O, l2 = K.flash_attn_fwd(qkv, B, T, H, SC)
    for name, (causal, ds, de, p, st, site, t) in _refusals(data).items():
        rc, out, lse2 = _c_fwd(K, qkv, causal, ds, de, p, st, site, t)
        assert rc != 0, name
        torch.cuda.synchronize()
        assert bool((out == POISON).all()) and bool((lse2 == POISON).all()), name
        rc, dqkv, delta = _c_bwd(K, qkv, O, dO, l2, causal, ds, de, p, st, site, t)
        assert rc != 0, name
        torch.cuda.synchronize()
        assert bool((dqkv == POISON).all()) and bool((delta == POISON).all()), name


@pytest.mark.parametrize("with_doc", [False, True], ids=["plain", "doc"])
def test_p_zero_is_the_call_without_dropout(K, data, with_doc):
    qkv, dO, ds, de, st = data
    doc = (ds, de) if with_doc else None
    cd = doc or (None, None)
    O, l2 = K.flash_attn_fwd(qkv, B, T, H, SC, doc=doc)
    g = K.flash_attn_bwd(qkv, O, dO, l2, B, T, H, SC, doc=doc)
    if with_doc:                    # the bounds reached the kernel
        assert not A.bits_equal(O, K.flash_attn_fwd(qkv, B, T, H, SC)[0])
    # the C entries: a null state is accepted and the site ignored
    rc, Oc, l2c = _c_fwd(K, qkv, 1, *cd, 0.0, None, -1)
    assert rc == 0 and A.bits_equal(Oc, O) and A.bits_equal(l2c, l2)
    rc, gc, _ = _c_bwd(K, qkv, O, dO, l2, 1, *cd, 0.0, None, -1)
    assert rc == 0 and A.bits_equal(gc, g)
    # the wrappers: drop with p = 0 against no drop
    Ow, l2w = K.flash_attn_fwd(qkv, B, T, H, SC, doc=doc, drop=(0.0, st, 0))
    assert A.bits_equal(Ow, O) and A.bits_equal(l2w, l2)
    assert A.bits_equal(K.flash_attn_bwd(qkv, O, dO, l2, B, T, H, SC, doc=doc, drop=(0.0, st, 0)), g)
    torch.cuda.synchronize()


def test_wrappers_refuse_doc_or_drop_without_causal(K, data, monkeypatch):
    qkv, dO, ds, de, st = data
    O, l2 = K.flash_attn_fwd(qkv, B, T, H, SC)
    monkeypatch.setattr(K, "call", lambda name, *a: pytest.fail(f"{name} reached the launcher"))
    for kw in (dict(doc=(ds, de)), dict(drop=(0.1, st, 0)), dict(drop=(0.0, st, 0))):
        with pytest.raises(ValueError):
            K.flash_attn_fwd(qkv, B, T, H, SC, False, **kw)
        with pytest.raises(ValueError):
            K.flash_attn_bwd(qkv, O, dO, l2, B, T, H, SC, False, **kw)
