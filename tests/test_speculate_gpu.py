"""The bookkeeping kernels of a speculative step (csrc/kernels/speculate.hip) on the GPU against ops/speculate.py: exact
integers and exact u on the hand-written cases of tests/speculate_cases.py and on random states; u against the draws
sample_logits makes on its own; and the property the exactness of speculation rests on: every other kernel of the step
gives a row the same bits alone as inside a 64-row call."""
import pytest
import torch

import speculate_cases as C
from pytorch_distributed_nn_amd.ops.speculate import accept_reference, prepare_reference

pytestmark = pytest.mark.gpu
SEED = 1234
BF = torch.bfloat16


def K():
    from pytorch_distributed_nn_amd.ops import kernels
    return kernels


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def run_prepare(kw, seed=SEED):
    """the kernel on the state ``kw`` (as for prepare_reference) -> tok_in, pos, u"""
    R = kw["out"].shape[0] * kw["S"]
    tok_in = torch.full((R,), -1, dtype=torch.int64, device="cuda")
    pos = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    u = torch.full((R,), -1.0, dtype=torch.float32, device="cuda")
    K().spec_prepare(kw["out"], kw["P"], kw["N"], kw["prompt_len"], kw["ntok"], kw["lens"], seed, kw["S"], tok_in, pos, u,
                     guess=kw.get("guess"), ngram=kw.get("ngram", 3))
    return tok_in, pos, u


def check_prepare(kw, want=None):
    before = kw["out"].clone()
    tok_in, pos, u = run_prepare(kw)
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in kw.items()}
    rt, rp, ru = prepare_reference(seed=SEED, **cpu)
    assert tok_in.cpu().tolist() == rt.tolist() and pos.cpu().tolist() == rp.tolist()
    assert bits(u.cpu(), ru), "u differs from ops.sampling.uniform"
    assert torch.equal(kw["out"], before)
    if want is not None:
        assert tok_in.cpu().tolist() == want


@pytest.mark.parametrize("name", sorted(C.PREPARE_NGRAM))
def test_prepare_ngram_cases(name):
    kw, want = C.prepare_ngram_case(name, "cuda")
    check_prepare(kw, want)


def test_prepare_table_case():
    kw, want, pos_want = C.prepare_table_case("cuda")
    check_prepare(kw, want)
    assert run_prepare(kw)[1].cpu().tolist() == pos_want


def run_accept(kw, st):
    done = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    K().spec_accept(st["tok_in"], st["t"], st["out"], kw["P"], kw["N"], st["ntok"], st["lens"], done, st["stats"], kw["S"],
                    finished=st["finished"], eos_token=kw["eos_token"])
    return bool(done.item())


@pytest.mark.parametrize("case", [C.accept_case, C.accept_done_case], ids=["mixed_rows", "done"])
def test_accept_cases(case):
    kw, st, want = case("cuda")
    assert run_accept(kw, st) is want["done"]
    assert st["out"].cpu().tolist() == want["out"]
    assert st["ntok"].cpu().tolist() == want["ntok"] and st["lens"].cpu().tolist() == want["lens"]
    assert st["stats"].cpu().tolist() == want["stats"]
    if want["finished"] is not None:
        assert st["finished"].cpu().tolist() == want["finished"]


def random_state(g, vocab):
    """a state a generation could be in (some rows complete), tokens from a small vocabulary so that n-grams recur"""
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))      # noqa: E731
    B, S, P, N = ri(1, 8), ri(1, 8), ri(1, 40), ri(1, 40)
    pl = torch.randint(1, P + 1, (B,), generator=g, dtype=torch.int32)
    ntok = torch.randint(1, N + 1, (B,), generator=g, dtype=torch.int32)
    if ri(0, 3) == 0:
        ntok[ri(0, B - 1)] = N
    out = torch.randint(0, vocab, (B, P + N), generator=g)
    return dict(out=out, P=P, N=N, prompt_len=pl, ntok=ntok, lens=pl + ntok - 1, S=S)


@pytest.mark.parametrize("seed", range(6))
def test_prepare_and_accept_random(seed):
    g = torch.Generator().manual_seed(seed)
    for it in range(12):
        vocab = (2, 3, 5, 50)[it % 4]
        kw = random_state(g, vocab)
        B, S, P, N = kw["out"].shape[0], kw["S"], kw["P"], kw["N"]
        if it % 3 == 0:
            kw["guess"] = torch.randint(0, vocab, (B, N), generator=g)
        else:
            kw["ngram"] = 1 + it % 5
        gpu = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        check_prepare(gpu)
        tok_in = run_prepare(gpu)[0]
        # drawn tokens: each equals the draft that follows it with probability 3/4, so that runs of every length occur
        t = torch.randint(0, vocab, (B * S,), generator=g)
        same = torch.rand(B * S, generator=g) < 0.75
        nxt = torch.roll(tok_in.cpu(), -1)
        last = torch.arange(B * S) % S == S - 1
        t = torch.where(same & ~last, nxt, t)
        eos = None if it % 2 else int(torch.randint(0, vocab, (1,), generator=g))
        fin = None
        if eos is not None:     # a row is finished iff it has emitted eos
            new = torch.arange(N)[None, :] < kw["ntok"][:, None]
            fin = ((kw["out"][:, P:] == eos) & new).any(1).to(torch.uint8)
        stats = torch.randint(0, 9, (S + 1,), generator=g)
        ref = dict(out=kw["out"].clone(), ntok=kw["ntok"].clone(), lens=kw["lens"].clone(),
                   finished=None if fin is None else fin.clone(), stats=stats.clone())
        done_ref = accept_reference(tok_in.cpu(), t, ref["out"], P, N, ref["ntok"], ref["lens"], ref["finished"], eos,
                                    ref["stats"], S)
        st = dict(tok_in=tok_in, t=t.cuda(), out=gpu["out"], ntok=gpu["ntok"], lens=gpu["lens"],
                  finished=None if fin is None else fin.cuda(), stats=stats.cuda())
        done = run_accept(dict(P=P, N=N, S=S, eos_token=eos), st)
        what = f"seed {seed} it {it}: B={B} S={S} P={P} N={N} eos={eos}"
        assert done is done_ref, what
        for k in ("out", "ntok", "lens", "stats") + (("finished",) if fin is not None else ()):
            assert torch.equal(st[k].cpu(), ref[k]), f"{what}: {k}"


def test_u_is_the_draw_of_sample_logits():
    """tokens drawn with u = spec_prepare's u[b*S + j] equal those sample_logits draws itself at (seed, ntok[b] + j, b)"""
    k = K()
    B, S, V, P, N = 8, 8, 4096, 4, 64
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(B, V, generator=g) * 0.5).to(BF).cuda()
    out = torch.randint(0, V, (B, P + N), generator=g).cuda()
    ntok = torch.tensor([1, 2, 3, 5, 8, 13, 21, 34], dtype=torch.int32, device="cuda")
    pl = torch.full((B,), P, dtype=torch.int32, device="cuda")
    _, _, u = run_prepare(dict(out=out, P=P, N=N, prompt_len=pl, ntok=ntok, lens=pl + ntok - 1, S=S), seed=77)
    with_u = torch.empty(B, dtype=torch.int64, device="cuda")
    own = torch.empty(B, dtype=torch.int64, device="cuda")
    differ = 0
    for j in range(S):
        k.sample_logits(logits, with_u, torch.tensor([0, 0], device="cuda"), u=u.view(B, S)[:, j].contiguous())
        for b in range(B):      # row b of a call is stream b: draw the whole batch at row b's step and keep row b
            k.sample_logits(logits, own, torch.tensor([77, int(ntok[b]) + j], device="cuda"))
            assert int(own[b]) == int(with_u[b]), f"row {b} offset {j}"
        differ += int((with_u != with_u[0]).sum())
    assert differ > 0, "every row drew the same token: the comparison shows nothing"


def test_rows_of_the_step_do_not_depend_on_the_row_count():
    """layernorm_fwd, embedding_decode, gemm_skinny (bias, GELU, residual; GPT-2 small's N, K pairs cut to N <= 256) and
    sample_logits: row r alone has the bits it has inside the 64-row call"""
    k = K()
    M = 64
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    # LayerNorm
    x = rn(M, 768).to(BF).cuda()
    gam, bet = (1 + 0.1 * rn(768)).cuda(), (0.1 * rn(768)).cuda()
    y = k.layernorm_fwd(x, gam, bet, 1e-5)[0]
    for r in range(M):
        assert bits(k.layernorm_fwd(x[r:r + 1].contiguous(), gam, bet, 1e-5)[0][0], y[r]), f"layernorm row {r}"
    # embedding gather
    wte, wpe = rn(512, 768).to(BF).cuda(), rn(128, 768).to(BF).cuda()
    tok = torch.randint(0, 512, (M,), generator=g).cuda()
    pos = torch.randint(0, 140, (M,), generator=g, dtype=torch.int32).cuda()        # some past the table: clamped
    e = k.embedding_decode(tok, pos, wte, wpe)
    for r in range(M):
        assert bits(k.embedding_decode(tok[r:r + 1].contiguous(), pos[r:r + 1].contiguous(), wte, wpe)[0], e[r]), \
            f"embedding row {r}"
    # the five linears of a step: (N, K, bias, act, res)
    for N, Kd, bias, act, res in ((256, 768, True, 0, False), (256, 768, True, 0, True), (256, 768, True, 2, False),
                                  (256, 3072, True, 0, True), (256, 768, False, 0, False)):
        a = rn(M, Kd).to(BF).cuda()
        w = (rn(N, Kd) * Kd ** -0.5).to(BF).cuda()
        bv = rn(N).cuda() if bias else None
        rs = rn(M, N).to(BF).cuda() if res else None
        full = k.gemm_skinny(a, w, bias=bv, act=act, res=rs)
        for r in range(M):
            one = k.gemm_skinny(a[r:r + 1].contiguous(), w, bias=bv, act=act,
                                res=rs[r:r + 1].contiguous() if res else None)
            assert bits(one[0], full[r]), f"gemm_skinny N={N} K={Kd} act={act} res={res} row {r}"
    # the draw, with the uniforms given
    V = 1024
    logits = rn(M, V).to(BF).cuda()
    u = torch.rand(M, generator=g).cuda()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    for kw in (dict(temperature=0.0), dict(temperature=0.8, top_k=20, top_p=0.9), dict(temperature=1.0)):
        full = k.sample_logits(logits, torch.empty(M, dtype=torch.int64, device="cuda"), state, u=u, **kw)
        for r in range(M):
            one = k.sample_logits(logits[r:r + 1], torch.empty(1, dtype=torch.int64, device="cuda"), state,
                                  u=u[r:r + 1].contiguous(), **kw)
            assert int(one[0]) == int(full[r]), f"sample_logits {kw} row {r}"
