"""The sampling kernel (csrc/kernels/sample.hip) against the numpy reference of tests/sample_ref.py: every case in both
logits dtypes, memory hygiene, repeatability and batch invariance, eos, graph replay and the guards."""
import numpy as np
import pytest
import torch

import sample_ref as R

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
U_MAX = 1.0 - 2.0 ** -24


def K():
    from pytorch_distributed_nn_amd.ops import kernels
    return kernels


def _state(seed, step):
    return torch.tensor([seed, step], dtype=torch.int64, device="cuda")


def _run(x, T, k, p, state=None, u=None, **kw):
    """x: CUDA logits [B][V] -> (tok, thr, nkeep) on the CPU"""
    B = x.shape[0]
    tok = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    thr = torch.full((B,), 123.0, device="cuda")
    nkeep = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    K().sample_logits(x, tok, state if state is not None else _state(*R.STATE), temperature=T, top_k=k, top_p=p, u=u,
                      thr=thr, nkeep=nkeep, **kw)
    return tok.cpu(), thr.cpu(), nkeep.cpu()


def _in_poisoned_view(x):
    """a copy of x as a view with ld > V inside a NaN buffer with guard rows -> (view, buffer)"""
    B, V = x.shape
    buf = torch.full((B + 2, V + 13), float("nan"), dtype=x.dtype, device="cuda")
    buf[1:B + 1, 5:5 + V] = x
    return buf[1:B + 1, 5:5 + V], buf


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_every_case(dtype):
    """nkeep / thr equal the reference's (either neighbour on ambiguous rows), the token is accepted under the CDF rule
    with the set taken from the reported threshold; greedy and k = 1 exact.  u: the generator's on even cases, the
    override (0, 1 - 2^-24 and a spread) on odd ones.  Logits live in a NaN-poisoned view and stay bitwise unchanged."""
    worst = 0.0
    for n, (fam, B, V, k, p, T, seed) in enumerate(R.cases()):
        x32 = R.make(fam, B, V, seed)
        if dtype == BF:
            x32 = R.bf16_round(x32)
        view, buf = _in_poisoned_view(torch.from_numpy(x32).to(dtype).cuda())
        before = buf.clone()
        if n % 2:
            us = np.array(([0.0, U_MAX] + list(np.random.default_rng(n).random(B)))[:B], dtype=np.float32)
            us = np.floor(us.astype(np.float64) * 2 ** 24) / 2 ** 24
            tok, thr, nkeep = _run(view, T, k, p, u=torch.tensor(us, dtype=F32, device="cuda"))
        else:
            us = [R.uniform(*R.STATE, b) for b in range(B)]
            tok, thr, nkeep = _run(view, T, k, p)
        assert torch.equal(buf.view(torch.int16 if dtype == BF else torch.int32),
                           before.view(torch.int16 if dtype == BF else torch.int32)), "logits changed"
        for b in range(B):
            d = R.check_row(x32[b], T, k, p, float(us[b]), int(tok[b]), float(thr[b]), int(nkeep[b]))
            worst = max(worst, d)
            if k == 1 and T > 0:                              # equal weights: floor(u n) of the ties, exactly
                l = np.where(np.isnan(x32[b]), -np.inf, x32[b])
                ties = np.nonzero(l == l.max())[0]
                if np.isfinite(l.max()):
                    assert int(tok[b]) == ties[int(float(us[b]) * len(ties))], (fam, V, b)
    print(f"worst distance / EPS over the cases ({dtype}): {worst:.4f}")


def test_outputs_touch_only_their_cells():
    B, V, L = 5, 4099, 9
    x = torch.from_numpy(R.make("gauss1", B, V, 3)).cuda()
    tokb = torch.full((B + 8,), -99, dtype=torch.int64, device="cuda")
    hist = torch.full((B + 2, L), -99, dtype=torch.int64, device="cuda")
    finb = torch.full((B + 16,), 0, dtype=torch.uint8, device="cuda")
    finb[:8] = 77
    finb[8 + B:] = 77
    finb[8 + 1] = 1                                            # row 1 is finished
    tok, h, fin = tokb[4:4 + B], hist[1:1 + B], finb[8:8 + B]
    first = int(R.analyse(x[0].cpu().numpy(), 0.0, None, None)["token"])
    K().sample_logits(x, tok, _state(1, 3), temperature=0.0, history=h, col0=2, finished=fin, eos_token=first)
    want = [int(x[b].argmax()) for b in range(B)]
    want[1] = first
    assert tok.tolist() == want and bool((tokb[:4] == -99).all()) and bool((tokb[4 + B:] == -99).all())
    assert h[:, 5].tolist() == want and int((hist != -99).sum()) == B            # column col0 + step = 5
    assert fin.tolist() == [int(t == first) for t in want] and bool((finb[:8] == 77).all()) and bool((finb[8 + B:] == 77).all())
    # a step past the history's width writes the token, not the history
    K().sample_logits(x, tok, _state(1, 7), temperature=0.0, history=h, col0=2)
    assert int((hist != -99).sum()) == B
    # a sampled call (top-k and top-p: the writer is a lane of the wave that holds the crossing), thr and nkeep in
    # sentinel buffers too
    thrb = torch.full((B + 6,), 55.5, device="cuda")
    nkb = torch.full((B + 6,), -99, dtype=torch.int32, device="cuda")
    tokb.fill_(-99)
    hist.fill_(-99)
    finb[8:8 + B] = 0
    K().sample_logits(x, tok, _state(1, 3), temperature=0.9, top_k=40, top_p=0.9, history=h, col0=2, finished=fin,
                      eos_token=V + 1, thr=thrb[3:3 + B], nkeep=nkb[3:3 + B])
    xs = x.cpu().numpy()
    for b in range(B):
        R.check_row(xs[b], 0.9, 40, 0.9, R.uniform(1, 3, b), int(tok[b]), float(thrb[3 + b]), int(nkb[3 + b]))
    assert bool((tokb[:4] == -99).all()) and bool((tokb[4 + B:] == -99).all())
    assert h[:, 5].tolist() == tok.tolist() and int((hist != -99).sum()) == B
    assert fin.tolist() == [0] * B and bool((finb[:8] == 77).all()) and bool((finb[8 + B:] == 77).all())
    assert bool((thrb[:3] == 55.5).all()) and bool((thrb[3 + B:] == 55.5).all())
    assert bool((nkb[:3] == -99).all()) and bool((nkb[3 + B:] == -99).all())


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_repeatable_and_batch_invariant(dtype):
    B, V = 8, 50257
    x = torch.from_numpy(R.make("gauss1", B, V, 11)).to(dtype).cuda()
    for k, p in [(None, None), (50, 0.9), (None, 0.5)]:
        u = torch.tensor([R.uniform(9, 4, b) for b in range(B)], dtype=F32, device="cuda")
        a = _run(x, 0.8, k, p, state=_state(9, 4))
        b = _run(x, 0.8, k, p, state=_state(9, 4))
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        for r in range(B):                                     # row r alone, its u forced: the same bits
            one = _run(x[r:r + 1], 0.8, k, p, u=u[r:r + 1])
            assert all(torch.equal(s[r:r + 1], t) for s, t in zip(a, one)), (k, p, r)


def test_eos_rows_draw_nothing():
    B, V = 4, 1000
    x = torch.from_numpy(R.make("gauss1", B, V, 2)).cuda()
    fin = torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    tok, thr, nkeep = _run(x, 1.0, 5, None, finished=fin, eos_token=999)
    free = _run(x, 1.0, 5, None)[0]
    assert tok.tolist() == [int(free[0]), 999, int(free[2]), 999] and nkeep.tolist()[1::2] == [0, 0]
    assert fin.tolist() == [0, 1, 0, 1]
    tok, _, _ = _run(x, 1.0, 5, None, finished=fin, eos_token=int(free[0]))
    assert fin.tolist() == [1, 1, int(free[2] == free[0]), 1] and int(tok[1]) == int(free[0])


def test_graph_replay_follows_the_device_step():
    B, V, N = 3, 4099, 6
    x = torch.from_numpy(R.make("gauss1", B, V, 4)).to(BF).cuda()
    state, one = _state(31, 0), torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    tok = torch.zeros(B, dtype=torch.int64, device="cuda")
    hist = torch.full((B, N + 1), -1, dtype=torch.int64, device="cuda")

    def unit():
        K().sample_logits(x, tok, state, temperature=1.0, top_k=100, top_p=0.95, history=hist, col0=1)
        state.add_(one)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        unit()                                                 # warm-up, step 0
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        unit()
    for _ in range(N - 1):                                     # capturing runs nothing: steps 1 .. N - 1
        g.replay()
    torch.cuda.synchronize()
    assert state.tolist() == [31, N] and bool((hist[:, 0] == -1).all())
    for i in range(N):
        want = _run(x, 1.0, 100, 0.95, state=_state(31, i))[0]
        assert hist[:, 1 + i].cpu().tolist() == want.tolist(), i


def test_guards_raise_before_launch():
    x = torch.zeros(2, 64, device="cuda")
    tok, st = torch.zeros(2, dtype=torch.int64, device="cuda"), _state(1, 0)
    S = K().sample_logits
    bad = [lambda: S(x.half(), tok, st), lambda: S(x.t(), tok, st), lambda: S(x.cpu(), tok, st),
           lambda: S(x, tok[:1], st), lambda: S(x, tok.int(), st), lambda: S(x, tok, st.cpu()),
           lambda: S(x, tok, st[:1]), lambda: S(torch.zeros(1, 65537, device="cuda"), tok[:1], st),
           lambda: S(x, tok, st, temperature=-0.1), lambda: S(x, tok, st, temperature=float("nan")),
           lambda: S(x, tok, st, top_k=0), lambda: S(x, tok, st, top_p=0.0),
           lambda: S(x, tok, st, history=torch.zeros(3, 4, dtype=torch.int64, device="cuda")),
           lambda: S(x, tok, st, history=torch.zeros(2, 4, dtype=torch.int64, device="cuda"), col0=4),
           lambda: S(x, tok, st, eos_token=3), lambda: S(x, tok, st, finished=torch.zeros(2, device="cuda")),
           lambda: S(x, tok, st, u=torch.zeros(3, device="cuda")), lambda: S(x, tok, st, nkeep=torch.zeros(2, device="cuda"))]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"guard {i} did not raise")
    assert tok.tolist() == [0, 0]
