"""The packed-document flash kernels (csrc/kernels/attention.hip, DOC variants; ops.kernels.flash_attn_fwd / _bwd with ``doc``,
doc_bounds) against the float64 reference of tests/attn_doc_ref.py, element by element, over every element, with
the bounds derived there: every layout x shape x family, the backward under all eight (attn_bwd_wide, attn_delta_in_dq)
variants on attn_doc_ref.CROSS_SHAPES and under the defaults elsewhere, handed the float64 forward rounded to bf16 /
fp32.  Every call runs twice and must repeat bitwise; inputs must be unchanged; outputs finite everywhere.  Then the
exact properties: a single document is the plain causal kernel bit for bit, documents are isolated from each other bit
for bit, a document of one token returns its V.  Then the bounds kernel, the guards and graph capture."""
import functools
from types import SimpleNamespace

import pytest
import torch

import attn_ref as A
import attn_doc_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCALE = 0.125
WORST = {}
VARIANTS = [(w, d) for w in (0, 1, 2, 3) for d in (0, 1)]
BWD_CASES = ([(s, w, d) for s in R.CROSS_SHAPES for w, d in VARIANTS]
             + [(s, 3, 1) for s in R.SHAPES if s not in R.CROSS_SHAPES])
_ids = lambda s: "x".join(map(str, s))                                  # noqa: E731


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    return ratio


def _print_worst():
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import kernels, _backend
    assert _backend.available()
    return kernels


class _variant:
    def __init__(self, K, wide, delta_in_dq):
        self.K, self.new = K, (wide, delta_in_dq)

    def __enter__(self):
        self.old = (self.K.tune_set("attn_bwd_wide", self.new[0]), self.K.tune_set("attn_delta_in_dq", self.new[1]))

    def __exit__(self, *exc):
        self.K.tune_set("attn_bwd_wide", self.old[0])
        self.K.tune_set("attn_delta_in_dq", self.old[1])


@functools.lru_cache(maxsize=None)
def _case(family, layout, shape):
    """inputs and bounds on the GPU, the float64 forward (reference, and as handed to the backward), the backward"""
    B, T, H = shape
    qkv, dO = (t.cuda() for t in R.gen_doc(family, B, T, H, SCALE))
    ds, de = (t.cuda() for t in R.layout_bounds(layout, B, T))
    fwd = R.ref_doc_fwd(qkv, ds, de, B, T, H, SCALE)
    Og, lg = fwd[0].ref.to(BF).contiguous(), fwd[1].ref.float().contiguous()
    bwd = R.ref_doc_bwd(qkv, Og, dO, lg, ds, de, B, T, H, SCALE)
    c = SimpleNamespace(qkv=qkv, dO=dO, ds=ds, de=de, fwd=fwd, Og=Og, lg=lg, bwd=bwd)
    c.snap = tuple(t.clone() for t in (qkv, dO, Og, lg, ds, de))
    return c


def _inputs_unchanged(c):
    for t, s in zip((c.qkv, c.dO, c.Og, c.lg, c.ds, c.de), c.snap):
        assert torch.equal(t, s), "a kernel wrote to one of its inputs"


# ------------------------------------------------------------------------------------------- per-element checks
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_doc_forward(K, shape):
    B, T, H = shape
    for layout in R.LAYOUTS:
        for family in R.FAMILIES:
            c = _case(family, layout, shape)
            O, lse2 = K.flash_attn_fwd(c.qkv, B, T, H, SCALE, doc=(c.ds, c.de))
            O2, lse2b = K.flash_attn_fwd(c.qkv, B, T, H, SCALE, doc=(c.ds, c.de))
            assert A.bits_equal(O, O2) and A.bits_equal(lse2, lse2b), (layout, family, "not repeatable: a race")
            try:
                r = R.check_doc_fwd(c.qkv, O, lse2, c.ds, c.de, B, T, H, SCALE, ref=c.fwd)
            except AssertionError as e:
                raise AssertionError(f"{layout}, {family}: {e}") from None
            for n, v in r.items():
                _note(n, v)
            _inputs_unchanged(c)
    _print_worst()


@pytest.mark.parametrize("shape,wide,delta_in_dq", BWD_CASES, ids=[f"{_ids(s)}-wide{w}-delta{d}" for s, w, d in BWD_CASES])
def test_doc_backward(K, shape, wide, delta_in_dq):
    B, T, H = shape
    with _variant(K, wide, delta_in_dq):
        for layout in R.LAYOUTS:
            for family in R.FAMILIES:
                c = _case(family, layout, shape)
                dqkv = K.flash_attn_bwd(c.qkv, c.Og, c.dO, c.lg, B, T, H, SCALE, doc=(c.ds, c.de))
                again = K.flash_attn_bwd(c.qkv, c.Og, c.dO, c.lg, B, T, H, SCALE, doc=(c.ds, c.de))
                assert A.bits_equal(dqkv, again), (layout, family, "not repeatable: a race")
                try:
                    r = R.check_doc_bwd(c.qkv, c.Og, c.dO, c.lg, dqkv, c.ds, c.de, B, T, H, SCALE, ref=c.bwd)
                except AssertionError as e:
                    raise AssertionError(f"{layout}, {family}: {e}") from None
                for n, v in r.items():
                    _note(n, v)
                _inputs_unchanged(c)
    _print_worst()


# ------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("shape", [(1, 256, 3), (2, 384, 1), (1, 640, 2)], ids=_ids)
def test_single_document_is_the_plain_causal_kernel_bitwise(K, shape):
    """same tiles, same order, same arithmetic: O, lse2 and dqkv under every backward variant"""
    B, T, H = shape
    ds, de = (t.cuda() for t in (torch.zeros(B, T, dtype=torch.int32), torch.full((B, T), T, dtype=torch.int32)))
    for family in R.FAMILIES:
        qkv, dO = (t.cuda() for t in R.gen_doc(family, B, T, H, SCALE))
        O, lse2 = K.flash_attn_fwd(qkv, B, T, H, SCALE, True)
        Od, lse2d = K.flash_attn_fwd(qkv, B, T, H, SCALE, doc=(ds, de))
        assert A.bits_equal(O, Od) and A.bits_equal(lse2, lse2d), family
        for wide, delta_in_dq in VARIANTS:
            with _variant(K, wide, delta_in_dq):
                want = K.flash_attn_bwd(qkv, O, dO, lse2, B, T, H, SCALE, True)
                got = K.flash_attn_bwd(qkv, O, dO, lse2, B, T, H, SCALE, doc=(ds, de))
            assert A.bits_equal(want, got), (family, wide, delta_in_dq)


@pytest.mark.parametrize("layout", ["off_edges", "late_in_wave", "many_in_wave", "tile_edges"])
def test_documents_are_isolated_bitwise(K, layout):
    """other documents' q, k, v replaced (2^60-scaled ones among them): the kept document's O and lse2 rows do not
    change by a bit; with dO zero outside one document, dQ, dK and dV outside it are exactly 0"""
    B, T, H = 2, 384, 1
    ds, de = (t.cuda() for t in R.layout_bounds(layout, B, T))
    qkv, dO = (t.cuda() for t in R.gen_doc("gauss", B, T, H, SCALE))
    other, _ = (t.cuda() for t in R.gen_doc("next_key", B, T, H, SCALE))
    other = other.clone()
    other[::3] *= 2.0 ** 60
    O, lse2 = K.flash_attn_fwd(qkv, B, T, H, SCALE, doc=(ds, de))
    tok = torch.arange(T, device="cuda")
    for b in range(B):
        starts = R.layout_starts(R.LAYOUTS[(R.LAYOUTS.index(layout) + b) % len(R.LAYOUTS)], T)
        for s in starts[:6]:
            e = int(de[b, s])
            keep = torch.zeros(B, T, dtype=torch.bool, device="cuda")
            keep[b] = (tok >= s) & (tok < e)
            kf = keep.reshape(B * T)
            mixed = torch.where(kf[:, None], qkv, other)
            Om, lm = K.flash_attn_fwd(mixed, B, T, H, SCALE, doc=(ds, de))
            assert A.bits_equal(Om[kf], O[kf]), (layout, b, s, "O of the kept document changed")
            assert A.bits_equal(lm[b, :, s:e], lse2[b, :, s:e]), (layout, b, s, "lse2 of the kept document changed")
            dOz = torch.where(kf[:, None], dO, torch.zeros_like(dO))
            for wide, delta_in_dq in ((3, 1), (0, 0)):
                with _variant(K, wide, delta_in_dq):
                    dqkv = K.flash_attn_bwd(qkv, O, dOz, lse2, B, T, H, SCALE, doc=(ds, de))
                assert bool((dqkv[~kf] == 0).all()), (layout, b, s, wide, "gradient leaked out of the document")
                assert torch.isfinite(dqkv.float()).all()


def test_unit_layout(K):
    """every token its own document: lse2[q] = c q.k_q within the lse2 bound, O = V within the O bound"""
    B, T, H = 3, 128, 2
    t = torch.arange(T, dtype=torch.int32).expand(B, T).contiguous().cuda()
    qkv, _ = (x.cuda() for x in R.gen_doc("gauss", B, T, H, SCALE))
    O, lse2 = K.flash_attn_fwd(qkv, B, T, H, SCALE, doc=(t, t + 1))
    q, k, v = (x.double() for x in A.split_heads(qkv, B, T, H))
    c = A.f32(SCALE) * A.LOG2E
    want = c * (q * k).sum(-1)
    mag = c * (q.abs() * k.abs()).sum(-1) + want.abs() + A.RESC + 7.0                      # log2 T = 7
    _note("unit_lse2", A.check_f32(lse2, A.Vec(want, R.C["lse2"] * A.U * mag + A.U * want.abs()), "lse2"))
    w = 1.0 + A.LN2 * (c * (q.abs() * k.abs()).sum(-1, keepdim=True) + want.abs().unsqueeze(-1))
    e = A.Elem(A.merge(v), A.merge(v.abs()), A.merge(2.0 * w * v.abs()))
    _note("unit_O", A.check_bf16(O, e, R.C["O"], "O"))
    assert A.bits_equal(A.heads(O, B, T, H), A.split_heads(qkv, B, T, H)[2]), "p = l = 1 exactly: O must be V bitwise"
    _print_worst()


# ------------------------------------------------------------------------------------------- bounds kernel
@pytest.mark.parametrize("T", [128, 1024])
def test_doc_bounds_against_cpu_mirror(K, T):
    E = 50256
    g = torch.Generator().manual_seed(77 + T)
    rows = {"none": torch.randint(0, 1000, (T,), generator=g)}
    rows["at0"] = rows["none"].clone()
    rows["at0"][0] = E
    rows["at_end"] = rows["none"].clone()
    rows["at_end"][T - 1] = E
    rows["adjacent"] = rows["none"].clone()
    rows["adjacent"][[37, 38]] = E
    rows["many"] = torch.where(torch.rand(T, generator=g) < 0.1, torch.tensor(E), rows["none"])
    rows["all"] = torch.full((T,), E)
    names = list(rows)
    for i in range(0, len(names), 3):                              # B = 3, one block per sequence
        idx = torch.stack([rows[n] for n in names[i:i + 3]]).to(torch.int64).contiguous()
        want = R.bounds_from_tokens(idx, E)
        snap = idx.clone()
        got = K.doc_bounds(idx.cuda(), E)
        assert got[0].dtype == torch.int32 and got[0].shape == (3, T)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), names[i:i + 3]
        assert torch.equal(idx, snap)
    for lay in R.LAYOUTS:                                          # the layouts of this suite, through tokens
        st = R.layout_starts(lay, T)
        tok = torch.ones(1, T, dtype=torch.int64)
        tok[0, [s - 1 for s in st if s > 0]] = E
        ds, de = K.doc_bounds(tok.cuda(), E)
        want = R.bounds_of_starts(st, T)
        assert torch.equal(ds[0].cpu(), want[0]) and torch.equal(de[0].cpu(), want[1]), lay


# ------------------------------------------------------------------------------------------------ guards
def test_wrappers_reject_bad_arguments(K, monkeypatch):
    """ValueError before anything is launched: ``kernels.call`` is a stub that fails the test if reached."""
    B, T, H = 1, 128, 1
    qkv = torch.zeros(B * T, 3 * H * 64, device="cuda", dtype=BF)
    out = torch.zeros(B * T, H * 64, device="cuda", dtype=BF)
    lse2 = torch.zeros(B, H, T, device="cuda")
    ds = torch.zeros(B, T, device="cuda", dtype=torch.int32)
    de = torch.full((B, T), T, device="cuda", dtype=torch.int32)
    idx = torch.zeros(B, T, device="cuda", dtype=torch.int64)

    def launched(name, *a):
        pytest.fail(f"{name} reached the launcher")

    monkeypatch.setattr(K, "call", launched)
    no = pytest.raises(ValueError)
    for b, t, h in ((0, T, H), (B, 0, H), (B, T, 0), (-1, T, H), (B, 64, H)):
        with no:
            K.flash_attn_fwd(qkv, b, t, h, SCALE, doc=(ds, de))
        with no:
            K.flash_attn_bwd(qkv, out, out, lse2, b, t, h, SCALE, doc=(ds, de))
    bad = {"none": None, "int64": ds.long(), "strided": torch.zeros(B, 2 * T, device="cuda", dtype=torch.int32)[:, ::2],
           "shape": ds.reshape(T, B)[:T - 1], "flat": ds.reshape(-1), "cpu": ds.cpu()}
    for name, t in bad.items():
        for args in ((t, de), (ds, t)):
            with no:
                K.flash_attn_fwd(qkv, B, T, H, SCALE, doc=args)
            with no:
                K.flash_attn_bwd(qkv, out, out, lse2, B, T, H, SCALE, doc=args)
    with no:
        K.flash_attn_fwd(qkv.float(), B, T, H, SCALE, doc=(ds, de))
    with no:
        K.flash_attn_bwd(qkv, out.float(), out, lse2, B, T, H, SCALE, doc=(ds, de))
    with no:
        K.flash_attn_bwd(qkv, out, out, lse2.double(), B, T, H, SCALE, doc=(ds, de))
    with no:
        K.flash_attn_bwd(qkv, out, out.float(), lse2, B, T, H, SCALE, doc=(ds, de))
    for t in (idx.int(), idx.reshape(-1), idx.cpu(), torch.zeros(B, 2 * T, device="cuda", dtype=torch.int64)[:, ::2],
              torch.zeros(0, T, device="cuda", dtype=torch.int64)):
        with no:
            K.doc_bounds(t, 5)
    with no:
        K.doc_bounds(idx, 5.0)
    monkeypatch.undo()
    K.doc_bounds(idx, 5)                                           # well-formed calls still go through
    K.flash_attn_bwd(qkv, out, out, lse2, B, T, H, SCALE, doc=(ds, de))
    torch.cuda.synchronize()


def test_c_entry_points_refuse_before_launching(K):
    from pytorch_distributed_nn_amd.ops._backend import HipError
    B, T, H = 1, 128, 1
    qkv = torch.zeros(B * T, 3 * H * 64, device="cuda", dtype=BF)
    out = torch.zeros(B * T, H * 64, device="cuda", dtype=BF)
    lse2 = torch.zeros(B, H, T, device="cuda")
    ds = torch.zeros(B, T, device="cuda", dtype=torch.int32)
    de = torch.full((B, T), T, device="cuda", dtype=torch.int32)
    idx = torch.zeros(B, T, device="cuda", dtype=torch.int64)
    p, st = K.ptr, K.stream()
    nodrop = (0.0, None, 0)                                        # p, state, site
    no = pytest.raises(HipError)
    for b, t, h in ((0, T, H), (B, 0, H), (B, T, 0), (-1, T, H), (B, -128, H), (B, 64, H)):
        with no:
            K.call("pdnn_flash_attn_fwd", p(qkv), p(out), p(lse2), b, t, h, SCALE, 1, p(ds), p(de), *nodrop, st)
        with no:
            K.call("pdnn_flash_attn_bwd", p(qkv), p(out), p(out), p(lse2), p(lse2), p(qkv), b, t, h, SCALE, 1, p(ds),
                   p(de), *nodrop, st)
    for a, b in ((None, p(de)), (p(ds), None)):
        with no:
            K.call("pdnn_flash_attn_fwd", p(qkv), p(out), p(lse2), B, T, H, SCALE, 1, a, b, *nodrop, st)
        with no:
            K.call("pdnn_flash_attn_bwd", p(qkv), p(out), p(out), p(lse2), p(lse2), p(qkv), B, T, H, SCALE, 1, a, b,
                   *nodrop, st)
    with no:
        K.call("pdnn_flash_attn_fwd", p(qkv), p(out), None, B, T, H, SCALE, 1, p(ds), p(de), *nodrop, st)
    with no:
        K.call("pdnn_flash_attn_bwd", p(qkv), None, p(out), p(lse2), p(lse2), p(qkv), B, T, H, SCALE, 1, p(ds), p(de),
               *nodrop, st)
    for b, t in ((0, T), (B, 0), (-1, T), (B, -1)):
        with no:
            K.call("pdnn_doc_bounds", p(idx), 5, p(ds), p(de), b, t, st)
    for args in ((None, 5, p(ds), p(de)), (p(idx), 5, None, p(de)), (p(idx), 5, p(ds), None)):
        with no:
            K.call("pdnn_doc_bounds", *args, B, T, st)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ capture
def test_bounds_forward_backward_in_one_graph(K):
    """doc_bounds + DOC forward + backward captured once; the static idx buffer changes between the replays and each
    replay equals the eager result bitwise (no host read-back anywhere on the path)"""
    B, T, H = 1, 256, 3
    E = 9
    qkv, dO = (t.cuda() for t in R.gen_doc("gauss", B, T, H, SCALE))
    toks = []
    for lay in ("off_edges", "late_in_wave"):
        tok = torch.ones(B, T, dtype=torch.int64)
        tok[0, [s - 1 for s in R.layout_starts(lay, T) if s > 0]] = E
        toks.append(tok.cuda())

    def run(idx):
        ds, de = K.doc_bounds(idx, E)
        O, lse2 = K.flash_attn_fwd(qkv, B, T, H, SCALE, doc=(ds, de))
        return O, lse2, K.flash_attn_bwd(qkv, O, dO, lse2, B, T, H, SCALE, doc=(ds, de))

    eager = [tuple(t.clone() for t in run(tok)) for tok in toks]
    assert not A.bits_equal(eager[0][0], eager[1][0])
    static = toks[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static)
    for tok, want in ((toks[1], eager[1]), (toks[0], eager[0])):
        static.copy_(tok)
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip(outs, want):
            assert A.bits_equal(got, w)
