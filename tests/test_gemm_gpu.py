"""The GEMM engines (csrc/kernels/gemm_mfma.hip, gemm_glds.h, gemm_pp.hip) against the float64 reference of
tests/gemm_ref.py, element by element, over every element, with the bounds derived there; the integer family bit for bit.

Engines.  The five-way ``engine`` fixture of test_kernels_gpu.py (automatic, the register-staged 128-row kernel with
staged and direct stores, glds forced, ping-pong forced) runs every plain-GEMM, gemm_tn_acc and gemm_batched case.  A
forced engine runs only where its operand conditions hold, else the dispatcher falls back and the case is still checked:
    register kernel: any K % 8 == 0
    glds:            K % 64 == 0, M >= 8, N >= 8, N % 8 == 0, 16-byte aligned leading dimensions
    ping-pong:       K % 32 == 0, M >= 16, N >= 16, N % 8 == 0, one batch, not causal
gemm_ref.NT_SHAPES has shapes for each (test_gemm_ref_cpu.py asserts it).  The ping-pong engine is also crossed over
its tile widths (pp_bn 96 / 128 / 192 / 256 / 257 / 288) x pp_sk64 at N either side of each width, and over
pp_epi_slack x pp_epi_pair on two shapes; pp_wgrad and gemm_nt_splitk over K x splits (the 16-split wide reduce, the
clamp at splits > K / 32, uneven splits), bn, alpha, rowsum, a non-zero out.  With the persistent grid shrunk to 8 blocks
(test_pp_several_items_per_block) the plain, split-K and row-sum cases run again with several ragged work items per block.

Every case also asserts: outputs (and aux, the row sums, the split-K workspace) are views into larger buffers filled with
a sentinel bit pattern, ldc > N on half the cases, and everything outside the view is bitwise unchanged after the call;
the inputs (stored with pad columns and tail rows: NaN in the poisoned family, 777 elsewhere) are bitwise unchanged;
the call run twice gives the same bits, except the atomic paths (gemm_tn_acc, rowsum), whose two runs both meet the bound.
The worst error / bound per output is printed."""
import functools
from types import SimpleNamespace

import pytest
import torch

import gemm_ref as A

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
WORST = {}
GUARD = 2                                        # guard rows before and after an output
CASES = A.all_cases()
BY_ID = {cid: (args, opt) for group in CASES.values() for cid, args, opt in group}


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    return ratio


@pytest.fixture(scope="module")
def K():
    from pytorch_distributed_nn_amd.ops import kernels, _backend
    assert _backend.available(), "HIP kernel library must load on a GPU box"
    return kernels


@pytest.fixture(params=[(1, 1, 1), (0, 1, 0), (0, 0, 0), (2, 1, 0), (1, 1, 2)],
                ids=["auto", "reg128", "reg128-direct-store", "glds", "pp"])
def engine(request, K):
    """automatic engine choice, the register-staged 128-tile kernel only (LDS-staged and direct epilogue stores), the
    glds 256-row engine forced wherever it applies, the ping-pong engine forced wherever it applies"""
    glds, staged, pp = request.param
    old = K.set_glds_mode(glds)
    old_s = K.set_staged_store(staged)
    old_p = K.set_pp_mode(pp)
    yield request.param
    K.set_glds_mode(old)
    K.set_staged_store(old_s)
    K.set_pp_mode(old_p)


# ------------------------------------------------------------------------------------------------ buffers
def _sentinel(t):
    """a NaN bit pattern no kernel produces"""
    if t.dtype == BF:
        t.view(torch.int16).fill_(0x7FC1)
    else:
        t.view(torch.int32).fill_(0x7FC00001)
    return t


def stored(t, pad, poison):
    """logical [.., R, C] -> (buffer [.., R + 2, C + pad], view of t inside it): pad columns and two tail rows hold NaN
    (poisoned family) or 777"""
    R, Cc = t.shape[-2:]
    buf = torch.full((*t.shape[:-2], R + 2, Cc + pad), float("nan") if poison else A.PAD_FILL, dtype=t.dtype, device=t.device)
    view = buf[..., :R, :Cc]
    view.copy_(t)
    return buf, view


def guarded(batch, M, N, pad, dtype, fill=None):
    """-> (buffer [*batch, GUARD + M + GUARD, N + pad] of sentinels, its [.., M, N] view holding ``fill``)"""
    buf = _sentinel(torch.empty(*batch, M + 2 * GUARD, N + pad, dtype=dtype, device="cuda"))
    view = buf[..., GUARD:GUARD + M, :N]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guard_intact(buf, view_of, what):
    """everything of ``buf`` outside its view still holds the sentinel, bit for bit"""
    want = _sentinel(torch.empty_like(buf))
    view_of(want).copy_(view_of(buf))
    assert A.bits_equal(buf, want), f"{what}: written outside the output (guard rows / columns changed)"


def _mn(N):
    return lambda t: t[..., GUARD:-GUARD, :N]


@functools.lru_cache(maxsize=None)
def _case(cid):
    """the case on the GPU, its operands in storage layout, the reference"""
    args, opt = BY_ID[cid]
    c = A.case_to(A.build(args, opt), "cuda")
    ref = A.reference(c)
    tr = lambda t: t.transpose(-1, -2).contiguous()                    # noqa: E731
    ep, pad, po = c.ep, c.pad, c.poison
    if ep == "batched":
        sa = stored(tr(c.a) if c.amode else c.a, pad, po)
        sb = stored(c.b if c.bmode else tr(c.b), pad, po)
    elif ep in ("tn", "wgrad"):
        sa, sb = stored(tr(c.a), 2 * pad, po), stored(c.b, 2 * pad, po)     # (fp32 cases pad by 4: operands by 8)
    elif ep == "nn":
        sa, sb = stored(c.a, pad, po), stored(c.b, pad, po)
    elif ep == "nt_ex":                                                   # w must be contiguous
        sa, sb = stored(c.a, pad, po), stored(c.b if c.w_kn else tr(c.b), 0, po)
    else:
        sa, sb = stored(c.a, pad, po), stored(tr(c.b), pad, po)
    st = SimpleNamespace(a=sa[1], b=sb[1], bufs=[sa[0], sb[0]])
    for name, t in (("res", c.res), ("du", c.du)):                        # laid out like the output
        if t is not None:
            buf, view = guarded(c.batch, c.M, c.N, pad, BF, t)
            setattr(st, name, view)
            st.bufs.append(buf)
        else:
            setattr(st, name, None)
    st.bufs += [t for t in (c.bias, c.old, c.rowsum_old) if t is not None]     # passed, or copied into the outputs
    st.snap = [b.clone() for b in st.bufs]
    return c, ref, st


def _inputs_unchanged(st):
    for b, s in zip(st.bufs, st.snap):
        assert A.bits_equal(b, s), "a kernel wrote to one of its inputs (or their padding)"


def launch(K, c, st):
    """one call into fresh guarded outputs -> {"y", "aux"?, "rowsum"?}; asserts every guard"""
    dt = F32 if c.out_f32 else BF
    outs = {}
    obuf, y = guarded(c.batch, c.M, c.N, c.pad, dt, c.old)
    if c.ep == "nt":
        K.gemm_nt(st.a, st.b, bias=c.bias, relu=c.act == 1, out_f32=c.out_f32, alpha=c.alpha, out=y)
    elif c.ep == "nn":
        K.gemm_nn(st.a, st.b, out_f32=c.out_f32, alpha=c.alpha, out=y)
    elif c.ep == "nt_ex":
        abuf, aux = guarded(c.batch, c.M, c.N, c.pad, BF) if c.aux else (None, None)
        K.gemm_nt_ex(st.a, st.b, bias=c.bias, act=c.act, aux=aux, res=st.res, dgelu=st.du, w_kn=c.w_kn, out=y)
        if c.aux:
            guard_intact(abuf, _mn(c.N), "aux")
            outs["aux"] = aux
    elif c.ep == "tn":
        K.gemm_tn_acc(st.a, st.b, y, alpha=c.alpha)
    elif c.ep == "wgrad":
        need = c.splits * (c.M * c.N + 64)
        ws = _sentinel(torch.empty(need + 256, dtype=F32, device="cuda"))
        rbuf = rs = None
        if c.rowsum_old is not None:
            rbuf = _sentinel(torch.empty(c.M + 8, dtype=F32, device="cuda"))
            rs = rbuf[4:4 + c.M]
            rs.copy_(c.rowsum_old)
            outs["rowsum"] = rs
        K.pp_wgrad(st.a, st.b, y, alpha=c.alpha, splits=c.splits, ws=ws[:need], rowsum=rs, bn=c.bn)
        _workspace_intact(ws, c)
        if rbuf is not None:
            guard_intact(rbuf, lambda t: t[4:-4], "rowsum")
    elif c.ep == "splitk":
        need = c.splits * (c.M * c.N + 64)
        ws = _sentinel(torch.empty(need + 256, dtype=F32, device="cuda"))
        y = K.gemm_nt_splitk(st.a, st.b, splits=c.splits, ws=ws[:need])      # (allocates its own output)
        _workspace_intact(ws, c)
    elif c.ep == "batched":
        a4, b4, y4 = st.a, st.b, y
        K.gemm_batched(a4, a4.stride(-2), a4.stride()[:2], c.amode, b4, b4.stride(-2), b4.stride()[:2], c.bmode,
                       y4, y4.stride(-2), y4.stride()[:2], c.M, c.N, c.K, c.batch, alpha=c.alpha, res=st.res, causal=c.causal)
    else:
        raise AssertionError(c.ep)
    guard_intact(obuf, _mn(c.N), "y")
    outs["y"] = y
    return outs


def _workspace_intact(ws, c):
    """split-K slabs: only the M * N floats of each slab the (clamped) split count uses may change"""
    eff = len(A.split_ranges(c.K, c.splits))
    sz = c.M * c.N + 64
    want = _sentinel(torch.empty_like(ws))
    if eff > 1 or c.ep == "splitk":
        for z in range(eff):
            want[z * sz:z * sz + c.M * c.N] = ws[z * sz:z * sz + c.M * c.N]
    assert A.bits_equal(ws, want), "split-K workspace written outside its slabs"


def run(K, cid, atomic=False):
    c, ref, st = _case(cid)
    if c.ep == "batched" and c.batch == (1, 1):
        assert st.a.dim() == 4
    try:
        o1 = launch(K, c, st)
        o2 = launch(K, c, st)
        torch.cuda.synchronize()
        for outs in (o1, o2) if atomic else (o1,):
            for n, r in A.check(c, outs, ref).items():
                _note(n, r)
        for n in o1:
            if not (atomic and n in ("y", "rowsum") and (c.ep == "tn" or n == "rowsum")):
                assert A.bits_equal(o1[n], o2[n]), f"{n}: not repeatable: a race"
        _inputs_unchanged(st)
    except AssertionError as e:
        raise AssertionError(f"{cid}: {e}") from None


def _ids_of(group, shapes=None):
    return [cid for cid, args, _ in CASES[group] if shapes is None or args[2:5] in shapes]


# ------------------------------------------------------------------------------------------------ plain GEMMs
@pytest.mark.parametrize("shape", A.NT_SHAPES + A.F32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_nt_nn_ex(K, engine, shape):
    """gemm_nt / gemm_nn / gemm_nt_ex, every option set of gemm_ref.nt_variants on every family"""
    for cid in _ids_of("nt", {shape}):
        run(K, cid)


@pytest.mark.parametrize("sk64", [0, 1])
@pytest.mark.parametrize("bn", A.PP_BN)
def test_pp_tile_widths(K, bn, sk64):
    """the ping-pong engine forced, every tile configuration, N = bn - 8 / bn / bn + 8, one and two row tiles; K = 128
    takes the 64-deep-slice forms with pp_sk64 = 1, K = 96 their 32-deep fallback"""
    old = K.set_pp_mode(2)
    old_bn, old_sk = K.tune_set("pp_bn", bn), K.tune_set("pp_sk64", sk64)
    try:
        for cid in _ids_of("nt", set(A.pp_bn_shapes(bn))):
            run(K, cid)
    finally:
        K.tune_set("pp_bn", old_bn)
        K.tune_set("pp_sk64", old_sk)
        K.set_pp_mode(old)


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("slack", [0, 1])
@pytest.mark.parametrize("shape", A.EPI_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pp_epilogue_forms(K, shape, slack, pair):
    """buffer stores with the deferred drain (out-of-range offsets must be dropped: the guards) x paired epilogues"""
    old = K.set_pp_mode(2)
    old_sl, old_pr = K.tune_set("pp_epi_slack", slack), K.tune_set("pp_epi_pair", pair)
    try:
        for cid in _ids_of("nt", {shape}):
            run(K, cid)
    finally:
        K.tune_set("pp_epi_slack", old_sl)
        K.tune_set("pp_epi_pair", old_pr)
        K.set_pp_mode(old)


# --------------------------------------------------------------------------------- several work items per block
# The ping-pong grid is persistent: one block per CU, and only with more work items than CUs does a block take a second
# one.  No shape small enough for this file has more than 256.  So the grid is shrunk to 8 blocks with the project's own
# switch for leaving CUs to the collectives (comm world 2, comm_cus = CUs - 8): 27 plain items, up to 68 split-K items.
MULTI_SHAPES = [(520, 776, 96), (264, 1032, 64)]          # 3 x 9 tiles at bn = 96; K % 64 == 0 for the 64-deep forms


@pytest.fixture
def eight_blocks(K):
    cus = K.grid_cus()
    old_w, old_c = K.set_comm_world(2), K.tune_set("comm_cus", cus - 8)
    try:
        assert K.grid_cus() == 8
        yield 8
    finally:
        K.tune_set("comm_cus", old_c)
        K.set_comm_world(old_w)


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("slack", [0, 1, 2])
def test_pp_several_items_per_block(K, eight_blocks, slack, pair):
    """What only a block's second item runs: the accumulators cleared between items, the slice stream running on into
    the next item's slices, the slice count and row-sum switch of item i > 0 of an uneven split-K, and the stores of one
    item draining under the next one's slices (pp_epi_slack: 1 bf16, 2 also fp32) with and without paired epilogues."""
    old = K.set_pp_mode(2)
    old_sl, old_pr, old_bn = K.tune_set("pp_epi_slack", slack), K.tune_set("pp_epi_pair", pair), K.tune_get("pp_bn")
    try:
        for bn in (96, 256):
            K.tune_set("pp_bn", bn)
            for M, N, _ in MULTI_SHAPES:
                assert -(-M // 256) * -(-N // bn) > eight_blocks
            for cid in _ids_of("nt", set(MULTI_SHAPES)):
                run(K, cid)
        K.tune_set("pp_bn", 0)
        many = [i for i in _ids_of("wgrad") + _ids_of("splitk")
                if -(-BY_ID[i][0][2] // 256) * len(A.split_ranges(BY_ID[i][0][4], BY_ID[i][1]["splits"])) > eight_blocks]
        assert any(BY_ID[i][1].get("rowsum") and BY_ID[i][0][4] // 32 % BY_ID[i][1]["splits"] for i in many)
        for cid in many:
            run(K, cid, atomic=True)
    finally:
        K.tune_set("pp_bn", old_bn)
        K.tune_set("pp_epi_slack", old_sl)
        K.tune_set("pp_epi_pair", old_pr)
        K.set_pp_mode(old)


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("Kd", A.WGRAD_K)
def test_pp_wgrad(K, Kd):
    """out += alpha x^T y and rowsum += alpha x.sum(0) on a non-zero out; the slabs' reduce repeats bitwise, the row
    sums' atomics need not"""
    for cid in [i for i in _ids_of("wgrad") if BY_ID[i][0][4] == Kd]:
        run(K, cid, atomic=True)


@pytest.mark.parametrize("Kd", A.WGRAD_K)
def test_gemm_nt_splitk(K, Kd):
    for cid in [i for i in _ids_of("splitk") if BY_ID[i][0][4] == Kd]:
        run(K, cid)


@pytest.mark.parametrize("shape", A.TN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_tn_acc(K, engine, shape):
    """out += alpha x^T y on a non-zero out (fp32 atomics: both runs meet the bound)"""
    for cid in _ids_of("tn", {shape}):
        run(K, cid, atomic=True)


# ------------------------------------------------------------------------------------------------ batched
def test_gemm_batched_dense(K, engine):
    for cid in [i for i in _ids_of("batched") if i.startswith("bat-")]:
        run(K, cid)


@pytest.mark.parametrize("T", A.CAUSAL_T)
def test_gemm_batched_causal(K, engine, T):
    """the attention chain's causal GEMMs: mode 1 compared at k <= q only; modes 2 / 3 with NaN outside every tile's
    reduction range, results finite and within bound"""
    for cid in [i for i in _ids_of("batched") if f"-T{T}-" in i]:
        run(K, cid)
