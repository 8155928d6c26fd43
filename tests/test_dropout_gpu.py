"""The dropout kernels on the GPU against tests/dropout_ref.py: the mask exports bit for bit against the integer
generator, the row kernels per element against float64 with the reference mask, the DROP flash-attention kernels (plain
and packed-document, every backward variant) per element against the float64 reference within the recorded bounds."""
import itertools

import pytest
import torch

import attn_ref as A
import dropout_ref as R

pytestmark = pytest.mark.gpu
SC = 0.125
_CACHE = {}


def _K():
    from pytorch_distributed_nn_amd.ops import kernels as K
    return K


def _state(step=None):
    return torch.tensor([R.STATE[0], R.STATE[1] if step is None else step], dtype=torch.int64, device="cuda")


def _case(fam, shape, p, lay):
    """inputs and float64 references of one case, on the CPU, computed once"""
    key = (fam, shape, p, lay)
    if key not in _CACHE:
        B, T, H = shape
        qkv, dO = A.gen_flash(fam, B, T, H)
        doc = R.doc_of(lay, B, T)
        keep = R.keep_attn(R.STATE, R.SITE, p, B, H, T)
        fwd = R.ref_drop_fwd(qkv, keep, p, B, T, H, SC, doc)
        Og, lg = fwd[0].ref.to(A.BF).contiguous(), fwd[1].ref.float().contiguous()
        _CACHE[key] = (qkv, dO, doc, fwd, Og, lg, R.ref_drop_bwd(qkv, Og, dO, lg, keep, p, B, T, H, SC, doc))
    return _CACHE[key]


def _docs(doc):
    return None if doc is None else tuple(t.cuda() for t in doc)


# ------------------------------------------------------------------------------------------------ mask export
@pytest.mark.parametrize("p", R.MASK_PS)
def test_mask_export_equals_the_reference_generator(p):
    K = _K()
    for site, step in itertools.product((0, 4 * 11 + 2), (0, 7)):
        st = _state(step)
        for Rr, D in R.ROW_SHAPES:
            got = K.dropout_mask_rows(Rr, D, p, st, site).cpu()
            assert torch.equal(got, R.keep_rows((R.STATE[0], step), site, p, Rr, D).to(torch.uint8)), (site, step, Rr, D)
        for B, T, H in R.SHAPES:
            got = K.dropout_mask_attn(B, H, T, p, st, site).cpu()
            assert torch.equal(got, R.keep_attn((R.STATE[0], step), site, p, B, H, T).to(torch.uint8)), (site, step, B, T, H)
    assert K.dropout_p_eff(p) == R.p_eff(p)


def test_torch_generator_of_the_cpu_path_equals_the_reference():
    from pytorch_distributed_nn_amd.ops import transformer as TX
    st = _state()
    got = TX.dropout_keep_reference(st, 9, 0.1, attn=(3, 2, 128), device="cuda").cpu()
    assert torch.equal(got, R.keep_attn(R.STATE, 9, 0.1, 3, 2, 128))


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("Rr,D", R.ROW_SHAPES)
@pytest.mark.parametrize("p", R.MASK_PS)
def test_row_kernels(Rr, D, p):
    K = _K()
    g = torch.Generator().manual_seed(100 * Rr + D)
    x = (torch.randn(Rr, D, generator=g, dtype=torch.float64) * 3).to(A.BF)
    res = (torch.randn(Rr, D, generator=g, dtype=torch.float64) * 3).to(A.BF)
    keep = R.keep_rows(R.STATE, 6, p, Rr, D)
    st = _state()
    xc, rc = x.cuda(), res.cuda()
    for r_cpu, r_gpu in ((res, rc), (None, None)):
        ref, bound = R.ref_rows(x, r_cpu, keep, p)
        y = K.dropout_add_fwd(xc, r_gpu, p, st, 6)
        worst = A.check_bound(y.cpu(), (ref, bound), "dropout_add_fwd")
        assert worst <= 1.0
        assert torch.equal(xc.cpu(), x) and torch.equal(rc.cpu(), res) and st.tolist() == list(R.STATE)    # inputs unchanged
        assert ((y.cpu() == 0) | keep | (r_cpu is not None)).all()
    ref, bound = R.ref_rows(x, None, keep, p)
    A.check_bound(K.dropout_bwd(xc, p, st, 6).cpu(), (ref, bound), "dropout_bwd")
    # aliased output inside a sentinel-guarded buffer: the kernel writes its R x D elements and nothing else
    n = Rr * D
    buf = torch.full((n + 128,), 777.0, dtype=A.BF, device="cuda")
    view = buf[64:64 + n].view(Rr, D)
    view.copy_(xc)
    ref, bound = R.ref_rows(x, res, keep, p)
    out = K.dropout_add_fwd(view, rc, p, st, 6, out=view)
    assert out.data_ptr() == view.data_ptr()
    A.check_bound(view.cpu(), (ref, bound), "dropout_add_fwd aliased")
    assert (buf[:64] == 777.0).all() and (buf[64 + n:] == 777.0).all()


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_attention_dropout_fwd_bwd(shape, fam, p):
    K = _K()
    B, T, H = shape
    st = _state()
    for lay in [None] + R.LAYOUTS:
        qkv, dO, doc, fwd, Og, lg, bwd = _case(fam, shape, p, lay)
        q, dd, drop = qkv.cuda(), _docs(doc), (p, st, R.SITE)
        O, l2 = K.flash_attn_fwd(q, B, T, H, SC, doc=dd, drop=drop)
        r = R.check_drop_fwd(O.cpu(), l2.cpu(), fwd, doc)
        # dropout does not touch the softmax: lse2 is the plain (DOC) kernel's, bit for bit
        l2p = K.flash_attn_fwd(q, B, T, H, SC, doc=dd)[1]
        assert A.bits_equal(l2, l2p), (lay, "lse2")
        O2, _ = K.flash_attn_fwd(q, B, T, H, SC, doc=dd, drop=drop)
        assert A.bits_equal(O, O2), "two calls with one key differ"
        dqkv = K.flash_attn_bwd(q, Og.cuda(), dO.cuda(), lg.cuda(), B, T, H, SC, doc=dd, drop=drop)
        r.update(R.check_drop_bwd(dqkv.cpu(), bwd, B, T, H, doc))
        assert A.bits_equal(dqkv, K.flash_attn_bwd(q, Og.cuda(), dO.cuda(), lg.cuda(), B, T, H, SC, doc=dd, drop=drop))
        print(shape, fam, p, lay, {k: round(v, 3) for k, v in r.items()})
    assert st.tolist() == list(R.STATE)


@pytest.mark.parametrize("wide,delta_in_dq", list(itertools.product(range(4), (0, 1))))
def test_attention_dropout_every_backward_variant(wide, delta_in_dq):
    K = _K()
    st = _state()
    old = (K.tune_set("attn_bwd_wide", wide), K.tune_set("attn_delta_in_dq", delta_in_dq))
    try:
        for shape, lay in itertools.product(R.CROSS_SHAPES, (None, "off_edges")):
            B, T, H = shape
            qkv, dO, doc, fwd, Og, lg, bwd = _case("gauss", shape, 0.1, lay)
            dqkv = K.flash_attn_bwd(qkv.cuda(), Og.cuda(), dO.cuda(), lg.cuda(), B, T, H, SC, doc=_docs(doc),
                                    drop=(0.1, st, R.SITE))
            R.check_drop_bwd(dqkv.cpu(), bwd, B, T, H, doc)
    finally:
        K.tune_set("attn_bwd_wide", old[0])
        K.tune_set("attn_delta_in_dq", old[1])


def test_p_zero_is_the_plain_and_the_doc_kernel():
    K = _K()
    B, T, H = 1, 256, 3
    st = _state()
    qkv, dO = (t.cuda() for t in A.gen_flash("gauss", B, T, H))
    for lay in (None, "off_edges"):
        dd = _docs(R.doc_of(lay, B, T))
        O, l2 = K.flash_attn_fwd(qkv, B, T, H, SC, doc=dd, drop=(0.0, st, R.SITE))
        Op, lp = K.flash_attn_fwd(qkv, B, T, H, SC, doc=dd)
        assert A.bits_equal(O, Op) and A.bits_equal(l2, lp)
        g = K.flash_attn_bwd(qkv, O, dO, l2, B, T, H, SC, doc=dd, drop=(0.0, st, R.SITE))
        gp = K.flash_attn_bwd(qkv, Op, dO, lp, B, T, H, SC, doc=dd)
        assert A.bits_equal(g, gp)


def test_wrapper_guards():
    K = _K()
    B, T, H = 1, 128, 1
    qkv, dO = (t.cuda() for t in A.gen_flash("gauss", B, T, H))
    st = _state()
    O, l2 = K.flash_attn_fwd(qkv, B, T, H, SC, drop=(0.1, st, 0))
    bad = [dict(p=1.0), dict(p=-0.1), dict(p=float("nan")), dict(state=st.int()), dict(state=st.cpu()),
           dict(state=torch.zeros(3, dtype=torch.int64, device="cuda")), dict(site=-1)]
    for kw in bad:
        a = dict(p=0.1, state=st, site=0)
        a.update(kw)
        with pytest.raises(ValueError):
            K.flash_attn_fwd(qkv, B, T, H, SC, drop=(a["p"], a["state"], a["site"]))
        with pytest.raises(ValueError):
            K.flash_attn_bwd(qkv, O, dO, l2, B, T, H, SC, drop=(a["p"], a["state"], a["site"]))
        x = torch.zeros(2, 8, dtype=A.BF, device="cuda")
        with pytest.raises(ValueError):
            K.dropout_add_fwd(x, None, a["p"], a["state"], a["site"])
    with pytest.raises(ValueError):
        K.flash_attn_fwd(qkv[:96].contiguous(), 1, 96, 1, SC, drop=(0.1, st, 0))       # T % 128 != 0
    with pytest.raises(ValueError):
        K.flash_attn_fwd(qkv, B, T, H, SC, doc=(torch.zeros(B, T, dtype=torch.int32, device="cuda"), None), drop=(0.1, st, 0))
    with pytest.raises(ValueError):
        K.dropout_add_fwd(torch.zeros(2, 12, dtype=A.BF, device="cuda"), None, 0.1, st, 0)     # D % 8 != 0
    with pytest.raises(ValueError):
        K.dropout_p_eff(1.0)
    # the C entry points refuse a bad p themselves (error return, no launch)
    from pytorch_distributed_nn_amd.ops._backend import lib, ptr, stream
    assert lib().pdnn_flash_attn_fwd(ptr(qkv), ptr(O), ptr(l2), B, T, H, SC, 1, None, None, 1.0, ptr(st), 0, stream()) != 0
    assert lib().pdnn_dropout_add_fwd(ptr(O), None, ptr(O), B * T, 64, -0.5, ptr(st), 0, stream()) != 0
    torch.cuda.synchronize()
