"""GPT2.generate on the CPU (gpt2_tiny, plain-PyTorch fp32 cache): the cached path against the uncached loop that re-runs
forward() on the growing row, sampling, eos handling and the errors."""
import pytest
import torch

from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = build_gpt2("gpt2_tiny")
    with torch.no_grad():                # sharper logits than the 0.02 init gives, so that rows differ
        for p in m.parameters():
            p.mul_(4.0)
    return m


def _prompts(B, P, seed=0):
    return torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(seed))


def uncached(model, idx, n, prompt_lens=None):
    """greedy, one full forward per token on the growing row of each sequence -> tokens [B][n], logits [B][n][V]"""
    B, P = idx.shape
    pl = prompt_lens or [P] * B
    toks, lgs = [], []
    with torch.no_grad():
        for b in range(B):
            row = idx[b, :pl[b]].clone()
            t, l = [], []
            for _ in range(n):
                lg = model(row[None])[0, -1].float()
                l.append(lg)
                t.append(lg.argmax())
                row = torch.cat([row, t[-1][None]])
            toks.append(torch.stack(t))
            lgs.append(torch.stack(l))
    return torch.stack(toks), torch.stack(lgs)


CASES = [
    # (B, P, prompt_lens, max_new_tokens)
    (2, 5, None, 12),
    (1, 1, None, 9),
    (2, 127, None, 1),                   # 127 + 1 reaches block_size exactly
    (1, 5, None, 123),                   # 5 + 123 reaches block_size exactly
    (3, 127, [1, 5, 127], 1),            # ragged, the longest reaching block_size
    (3, 9, [1, 5, 9], 20),               # ragged
    (2, 6, [6, 6], 7),                   # prompt_lens given but uniform
]


@pytest.mark.parametrize("B,P,pl,n", CASES, ids=[f"B{c[0]}-P{c[1]}-{'ragged' if c[2] else 'full'}-n{c[3]}" for c in CASES])
def test_cached_generate_is_the_uncached_loop(model, B, P, pl, n):
    idx = _prompts(B, P, seed=P + n)
    out, lg = model.generate(idx, n, temperature=0.0, prompt_lens=pl, return_logits=True)
    assert out.shape == (B, P + n) and out.dtype == torch.int64 and lg.shape == (B, n, 512) and lg.dtype == torch.float32
    assert torch.equal(out[:, :P], idx)
    ref_t, ref_l = uncached(model, idx, n, pl)
    assert torch.equal(out[:, P:], ref_t), "greedy tokens differ from the uncached loop"
    err = (lg - ref_l).abs().max().item()
    bound = 1e-4 * ref_l.abs().max().item()
    print(f"max |logit difference| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    # tensor prompt_lens is the same as the list
    if pl is not None:
        assert torch.equal(model.generate(idx, n, temperature=0.0, prompt_lens=torch.tensor(pl)), out)


def test_top_k_one_is_greedy(model):
    idx = _prompts(2, 7)
    greedy = model.generate(idx, 10, temperature=0.0)
    assert torch.equal(model.generate(idx, 10, temperature=0.7, top_k=1), greedy)


def test_seeded_sampling_stays_in_the_top_k_and_repeats(model):
    idx = _prompts(3, 4, seed=3)
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(123)
        runs.append(model.generate(idx, 16, temperature=1.3, top_k=5, generator=g, return_logits=True))
    (o1, l1), (o2, l2) = runs
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    top = torch.topk(l1, 5, dim=-1).indices                          # [B][n][5]
    assert bool((top == o1[:, 4:, None]).any(-1).all()), "a sampled token outside its step's top-k"
    g = torch.Generator().manual_seed(124)
    assert not torch.equal(model.generate(idx, 16, temperature=1.3, top_k=5, generator=g), o1)
    # without top_k the draw is over the whole vocabulary and still repeats with the seed
    a = model.generate(idx, 8, temperature=2.0, generator=torch.Generator().manual_seed(5))
    b = model.generate(idx, 8, temperature=2.0, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b)


def test_eos_rows_keep_emitting_eos(model):
    idx = _prompts(3, 6, seed=11)
    free = model.generate(idx, 12, temperature=0.0)
    eos = int(free[0, 6 + 3])                                       # what row 0 emits at step 3
    out = model.generate(idx, 12, temperature=0.0, eos_token=eos)
    for b in range(3):
        new, ref = out[b, 6:], free[b, 6:]
        hit = (ref == eos).nonzero()
        if len(hit) == 0:
            assert torch.equal(new, ref)
        else:
            first = int(hit[0])
            assert torch.equal(new[:first + 1], ref[:first + 1]) and bool((new[first:] == eos).all())
    assert bool((out[0, 6 + 3:] == eos).all())


def test_generate_leaves_the_model_alone(model):
    idx = _prompts(2, 8, seed=2)
    tgt = _prompts(2, 8, seed=4)
    model.train()
    before = model(idx, tgt).item()
    model.generate(idx, 5, temperature=0.0)
    assert model.training and torch.is_grad_enabled()
    assert model(idx, tgt).item() == before
    model.eval()


def test_errors(model):
    idx = _prompts(2, 100)
    with pytest.raises(ValueError, match="block size"):
        model.generate(idx, 29)
    model.generate(idx, 28, temperature=0.0)                         # exactly block_size is fine
    with pytest.raises(ValueError, match="block size"):
        model.generate(idx, 100, prompt_lens=[5, 29])
    for bad in ([0, 5], [5, 101], [5]):
        with pytest.raises(ValueError, match="prompt_lens"):
            model.generate(idx, 1, prompt_lens=bad)
    with pytest.raises(ValueError):
        model.generate(idx[0], 1)
    with pytest.raises(ValueError):
        model.generate(idx, -1)
    with pytest.raises(ValueError):
        model.generate(idx, 1, top_k=0)
    assert model.generate(idx, 0).shape == (2, 100)
