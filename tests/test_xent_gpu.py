"""The cross-entropy kernels (csrc/kernels/softmax_xent.hip) against a float64 reference, elementwise.

test_kernels_gpu.py::test_xent compares in max-norm relative to the reference's largest entry (the one-hot's ~1), so
at a 50304-way vocabulary nearly every softmax entry passes whatever its value.  Here every gradient entry is held to
twice the bf16 rounding of its own reference value and every row's lse / loss to 1e-4 (tests/xent_ref.py states and
derives the bounds; tests/test_xent_ref_cpu.py shows that a correct fp32 model stays inside them), at the sizes,
label positions, layouts and values where the kernels take another path.

A separate module on purpose: the autouse GEMM-engine fixture of test_kernels_gpu.py would run every case five
times for nothing."""
import functools

import pytest
import torch

import xent_ref as X

pytestmark = pytest.mark.gpu

BF, F32 = X.BF, X.F32
SENTINEL = 123.0                    # exactly representable in bf16; no gradient entry can equal it (|d| <= 1)


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import _backend, kernels
    assert _backend.available(), "HIP kernel library must load on a GPU box"
    return kernels


@functools.lru_cache(maxsize=None)
def _case(gen, *args):
    """Inputs of one generator on the device with their float64 reference(s): built once, shared, never written."""
    x, y = getattr(X, gen)(*args)
    return x.cuda(), y.cuda()


@functools.lru_cache(maxsize=None)
def _ref(gen, args, ign=-100):
    x, y = _case(gen, *args)
    return X.ref64(x, y, ign)


def _gs(v):
    return torch.tensor([v], device="cuda", dtype=F32)


def _check_fwd(out, ref, what):
    loss, lse, acc = out[:3]
    r = {"lse": X.check_rows(lse, ref.lse), "loss": X.check_rows(loss, ref.loss), "sum": X.check_sum(acc[0], ref)}
    assert acc[1].item() == ref.count, (what, acc[1].item(), ref.count)
    bad = ~ref.valid
    if bool(bad.any()):
        assert loss[bad].abs().max().item() == 0.0, what
    print(what, {k: round(v, 4) for k, v in r.items()})


def _run_all(K, lg, y, ref, ign=-100, fused=None):
    """xent_fwd, xent_bwd without count (scale g / denom) and with it (g / max(count, 1)), and xent_fwd_grad on a
    copy where the layout allows (``fused`` None: decided by xent_fwd_grad_ok), each against ``ref``."""
    before = lg.clone()
    loss, lse, acc = K.xent_fwd(lg, y, ign)
    _check_fwd((loss, lse, acc), ref, "xent_fwd")
    d = K.xent_bwd(lg, y, lse, _gs(2.0), 4.0, ign)
    assert d.dtype == lg.dtype and d.shape == lg.shape
    print("xent_bwd", round(X.check_grad(d, ref, y, 0.5), 4))
    dm = K.xent_bwd(lg, y, lse, _gs(2.0), 1.0, ign, count=acc[1:2])
    print("xent_bwd count", round(X.check_grad(dm, ref, y, 2.0 / max(ref.count, 1)), 4))
    assert torch.isfinite(dm.float()).all()
    assert torch.equal(lg, before), "xent_fwd / xent_bwd must not write the logits"
    ok = K.xent_fwd_grad_ok(lg)
    assert fused is None or ok == fused
    if ok:
        lg2 = lg.clone()
        out = K.xent_fwd_grad(lg2, y, ign)
        assert out[3].data_ptr() == lg2.data_ptr()
        _check_fwd(out, ref, "xent_fwd_grad")
        print("xent_fwd_grad", round(X.check_grad(out[3], ref, y, 1.0), 4))
        assert out[2][1].item() == acc[1].item()                    # both entry points count the same rows
    return loss, lse, acc


@pytest.mark.parametrize("V,dtype", X.SWEEP, ids=[f"{v}-{'bf16' if d == BF else 'fp32'}" for v, d in X.SWEEP])
def test_xent_sizes(K, V, dtype):
    """R = 37 contiguous rows.  bf16: V = 8 (one active lane, three empty waves); 2048 / 2056 (256 / 257 chunks: no
    second load, one second load); 4096 / 4104 (512 / 513 chunks: third iteration of the two-load loop); 50304 (GPT-2:
    the last register chunk of xent_fwd_grad is partial); 51200 (its limit, all 25 register chunks full); 51208 (past
    the limit: the C entry point refuses, the two-pass kernels still run); 50257 and 10 (scalar path).  fp32 logits at
    V = 10 and 1000."""
    lg, y = _case("gen_sweep", V, dtype)
    fused = dtype == BF and V % 8 == 0 and V <= 51200
    _run_all(K, lg, y, _ref("gen_sweep", (V, dtype)), fused=fused)
    if V == 51208:
        R = lg.shape[0]
        out, loss, lse = torch.empty_like(lg), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
        with pytest.raises(ValueError):
            K.xent_fwd_grad(lg.clone(), y)
        from pytorch_distributed_nn_amd.ops._backend import HipError
        with pytest.raises(HipError):
            K.call("pdnn_xent_fwd_grad", K.ptr(lg), lg.stride(0), R, V, K.ptr(y), -100, K.ptr(loss), K.ptr(lse), None,
                   None, K.ptr(out), out.stride(0), K.stream())


@pytest.mark.parametrize("V", X.PLACEMENT_V)
def test_xent_label_placement(K, V):
    """One row per label: the first and the last element, a chunk owned by each of waves 0-3 at register chunk 0, the
    last register chunk, the second load of the two-load loop.  Loss and gradient are checked per row and per entry, so
    a label whose one-hot or target logit is taken from the wrong place fails its own row."""
    lg, y = _case("gen_placement", V)
    _run_all(K, lg, y, _ref("gen_placement", (V,)), fused=True)


@pytest.mark.parametrize("ign", [-100, 7])
def test_xent_ignored_and_out_of_range_labels(K, ign):
    """ignore_index (the default and a valid class id), labels >= V (also far past int32) and negative labels other
    than ignore_index: loss 0, gradient row exactly 0, not counted."""
    lg, y = _case("gen_ignored")
    ref = _ref("gen_ignored", (), ign)
    assert 0 < ref.count < lg.shape[0] - 5
    _run_all(K, lg, y, ref, ign=ign, fused=True)


def test_xent_all_rows_ignored(K):
    """count == 0: the mean scale is g / max(count, 1), everything is zero and finite."""
    lg, y = _case("gen_all_ignored")
    ref = _ref("gen_all_ignored", ())
    assert ref.count == 0
    loss, lse, acc = _run_all(K, lg, y, ref, fused=True)
    assert acc[0].item() == 0.0 and acc[1].item() == 0.0 and loss.abs().max().item() == 0.0
    d = K.xent_bwd(lg, y, lse, _gs(1.0), 1.0, count=acc[1:2])
    assert torch.isfinite(d.float()).all() and d.abs().max().item() == 0.0


@pytest.mark.parametrize("fused", [0, 1])
def test_lm_head_loss_all_targets_ignored(fused):
    """gpt2_tiny with every target -100, with the two-pass and the fused training forward: the loss is 0 and every
    parameter gradient is finite and zero."""
    from pytorch_distributed_nn_amd import tuning
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    old = tuning.set("xent_fused", fused)
    try:
        torch.manual_seed(5)
        m = build_gpt2("gpt2_tiny").cuda()
        g = torch.Generator(device="cuda").manual_seed(9)
        idx = torch.randint(0, m.config.vocab_size, (2, 128), device="cuda", generator=g)
        tgt = torch.full((2, 128), -100, device="cuda", dtype=torch.int64)
        loss = m(idx, tgt)
        loss.backward()
        assert loss.item() == 0.0
        for n, p in m.named_parameters():
            assert p.grad is not None, n
            assert torch.isfinite(p.grad).all(), n
            assert p.grad.abs().max().item() == 0.0, n
    finally:
        tuning.set("xent_fused", old)


@pytest.mark.parametrize("V,ld,off", [(1000, 1024, 8), (2048, 2056, 0)])
def test_xent_column_slice(K, V, ld, off):
    """Logits as a column slice of a wider buffer (ld > V): the vector paths with a row stride that is not the row
    length.  The padding columns of every buffer the kernels write hold a sentinel that must survive."""
    x, y = _case("gen_strided", V)
    ref = _ref("gen_strided", (V,))
    R = x.shape[0]

    def wide():
        return torch.full((R, ld), SENTINEL, device="cuda", dtype=BF)

    def padding_intact(w):
        return bool((w[:, :off] == SENTINEL).all()) and bool((w[:, off + V:] == SENTINEL).all())

    w = wide()
    lg = w[:, off:off + V]
    lg.copy_(x)
    assert lg.stride(0) == ld and lg.data_ptr() % 16 == 0
    loss, lse, acc = _run_all(K, lg, y, ref, fused=True)            # xent_fwd_grad there runs on a contiguous clone
    assert padding_intact(w)
    # xent_bwd into a strided output (the wrapper's own output is contiguous)
    wd = wide()
    d = wd[:, off:off + V]
    K.call("pdnn_xent_bwd", K.ptr(lg), lg.stride(0), R, V, K.ptr(y), -100, K.ptr(lse), K.ptr(_gs(1.0)), 1.0, None,
           K.ptr(d), d.stride(0), 1, K.stream())
    X.check_grad(d, ref, y, 1.0)
    assert padding_intact(wd) and torch.equal(lg, x)
    # xent_fwd_grad in place over the slice
    out = K.xent_fwd_grad(lg, y)
    assert out[3].data_ptr() == lg.data_ptr()
    _check_fwd(out, ref, "xent_fwd_grad in place, strided")
    X.check_grad(lg, ref, y, 1.0)
    assert padding_intact(w)


def test_xent_fwd_grad_separate_output(K):
    """xent_fwd_grad with ``out`` a separate buffer whose row stride differs from the input's, both ways round: the
    input is left unchanged and the output's padding untouched."""
    V = 2048
    x, y = _case("gen_strided", V)
    ref = _ref("gen_strided", (V,))
    R = x.shape[0]
    wo = torch.full((R, V + 24), SENTINEL, device="cuda", dtype=BF)
    out = wo[:, 8:8 + V]
    src = x.clone()
    res = K.xent_fwd_grad(src, y, out=out)                          # contiguous in, strided out
    assert res[3].data_ptr() == out.data_ptr() and torch.equal(src, x)
    _check_fwd(res, ref, "xent_fwd_grad contiguous -> strided")
    X.check_grad(out, ref, y, 1.0)
    assert bool((wo[:, :8] == SENTINEL).all()) and bool((wo[:, 8 + V:] == SENTINEL).all())
    wi = torch.full((R, V + 8), SENTINEL, device="cuda", dtype=BF)
    src = wi[:, :V]
    src.copy_(x)
    out = torch.full((R, V), SENTINEL, device="cuda", dtype=BF)
    res = K.xent_fwd_grad(src, y, out=out)                          # strided in, contiguous out
    assert torch.equal(src, x) and bool((wi[:, V:] == SENTINEL).all())
    _check_fwd(res, ref, "xent_fwd_grad strided -> contiguous")
    X.check_grad(out, ref, y, 1.0)


def test_xent_misaligned_view(K):
    """A view that starts one element (2 bytes) into its buffer: not 16-byte aligned, so the two-pass kernels take the
    scalar path and xent_fwd_grad refuses it."""
    V = 2048
    x, y = _case("gen_strided", V)
    ref = _ref("gen_strided", (V,))
    R = x.shape[0]
    buf = torch.full((R * V + 16,), SENTINEL, device="cuda", dtype=BF)
    lg = buf[1:1 + R * V].view(R, V)
    lg.copy_(x)
    assert lg.data_ptr() % 16 == 2 and not K.xent_fwd_grad_ok(lg)
    with pytest.raises(ValueError):
        K.xent_fwd_grad(lg, y)
    loss, lse, acc = _run_all(K, lg, y, ref, fused=False)
    # a misaligned output as well
    dbuf = torch.full((R * V + 16,), SENTINEL, device="cuda", dtype=BF)
    d = dbuf[1:1 + R * V].view(R, V)
    K.call("pdnn_xent_bwd", K.ptr(x), x.stride(0), R, V, K.ptr(y), -100, K.ptr(lse), K.ptr(_gs(1.0)), 1.0, None,
           K.ptr(d), d.stride(0), 1, K.stream())
    X.check_grad(d, ref, y, 1.0)
    for b in (buf, dbuf):
        assert b[0].item() == SENTINEL and bool((b[1 + R * V:] == SENTINEL).all())


def test_xent_value_edges(K):
    """V = 4096, all within |x| <= 64: rows of equal logits (0, +-64, 1.25); one logit 60 above the rest with the
    label on it (the label-entry gradient is near 0) and off it; the label on the smallest logit (a large loss);
    all-negative rows around -60."""
    lg, y = _case("gen_edges")
    assert lg.abs().max().item() <= X.XMAX
    _run_all(K, lg, y, _ref("gen_edges", ()), fused=True)


@pytest.mark.parametrize("R,V,lo", [(4096, 2048, 512), (256, 50304, 0)])
def test_xent_fwd_grad_in_place_equals_out_of_place(K, R, V, lo):
    """xent_fwd_grad in place over the logits (the default GPT-2 training path) against the same call with ``out`` a
    separate buffer: loss, lse, acc and the gradient must be bitwise equal -- the arithmetic is identical and has no
    atomics.

    The kernel used to read the target logit back from global memory for the loss after the last barrier, while the
    other waves were already storing the gradient over the same row; the target logit now comes from the registers of
    the lane that holds it.  At R = 4096, V = 2048 every label lies in [512, 2048): chunks owned by waves 1-3, which
    store first -- the placement where that window was widest.  No test can force the interleaving: the fix rests on
    reading the code (nothing reads the row from global memory after the first store).  This is the test that had a
    chance of seeing the race, run once, and it pins the property the fix guarantees."""
    x, y = _case("gen_inplace", R, V, lo)
    assert int(y.min()) >= lo
    sep = torch.empty_like(x)
    src = x.clone()
    l0, s0, a0, d0 = K.xent_fwd_grad(src, y, out=sep)
    assert torch.equal(src, x)
    inp = x.clone()
    l1, s1, a1, d1 = K.xent_fwd_grad(inp, y)
    assert d1.data_ptr() == inp.data_ptr()
    assert torch.equal(s1, s0), "lse"
    assert torch.equal(l1, l0), f"loss differs on {int((l1 != l0).sum())} rows"
    assert torch.equal(a1, a0), "acc"
    assert torch.equal(d1, d0), "gradient"
    ref = X.ref64(x, y)
    _check_fwd((l1, s1, a1), ref, "in place")
    X.check_grad(d1, ref, y, 1.0)


def test_xent_wrappers_reject_bad_row_operands(K):
    """Labels that are not int64, not contiguous or not R long, and an lse of the wrong dtype or length, raise instead
    of being read past their end."""
    lg, y = _case("gen_strided", 2048)
    R = lg.shape[0]
    _, lse, acc = K.xent_fwd(lg, y)
    gs = _gs(1.0)
    y2 = torch.stack([y, y], 1)                                      # [:, 0] is R long, int64, not contiguous
    bad_labels = {"int32": y.int(), "short": y[:R - 1], "long": torch.cat([y, y]), "strided": y2[:, 0],
                  "2-d": y.view(1, R)}
    for what, yy in bad_labels.items():
        with pytest.raises(ValueError):
            K.xent_fwd(lg, yy)
        with pytest.raises(ValueError):
            K.xent_bwd(lg, yy, lse, gs, 1.0)
        with pytest.raises(ValueError):
            K.xent_fwd_grad(lg.clone(), yy)
    l2 = torch.stack([lse, lse], 1)
    for what, ll in {"fp64": lse.double(), "bf16": lse.to(BF), "short": lse[:R - 1], "long": torch.cat([lse, lse]),
                     "strided": l2[:, 0]}.items():
        with pytest.raises(ValueError):
            K.xent_bwd(lg, y, ll, gs, 1.0)
    with pytest.raises(ValueError):
        K.xent_bwd(lg, y, lse, gs, 1.0, count=acc[1:2].double())
    K.xent_bwd(lg, y, lse, gs, 1.0, count=acc[1:2])                  # the well-formed call still goes through
