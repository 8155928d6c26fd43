"""GPT2.generate(speculate=S) on the CPU (gpt2_tiny, the plain-PyTorch reference path): the tokens are bit for bit those
of generate(sampler="device") with the same seed for every S, draft source and sampling setting; the number of verify
steps for perfect, useless and partly wrong draft tables; the argument errors."""
import math

import pytest
import torch

from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
from pytorch_distributed_nn_amd.ops.speculate import accept_reference

B, P, N, SEED = 3, 9, 24, 11
PL = [4, 9, 6]
DRAWS = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, top_k=20, top_p=0.9)}
_PLAIN = {}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = build_gpt2("gpt2_tiny")
    with torch.no_grad():                # sharper logits than the 0.02 init gives, so that rows differ
        for p in m.parameters():
            p.mul_(4.0)
    return m


def _idx():
    # a prompt that repeats itself, so that the n-gram lookup finds something
    base = torch.randint(0, 512, (B, 3), generator=torch.Generator().manual_seed(5))
    return base.repeat(1, 3)


def plain(model, draw, eos):
    """the plain device-sampler tokens, computed once per setting"""
    key = (draw, eos)
    if key not in _PLAIN:
        _PLAIN[key] = model.generate(_idx(), N, prompt_lens=PL, sampler="device", seed=SEED, eos_token=eos, **DRAWS[draw])
    return _PLAIN[key]


def _eos_of(model, draw):
    """a token that the plain run of row 1 emits in the middle, so that eos handling is exercised"""
    return int(plain(model, draw, None)[1, P + N // 2])


def steps_for(table, truth, S, eos=None):
    """verify steps the loop needs when the drafts come from ``table`` and the draws are ``truth``: accept_reference on
    the true tokens, step by step"""
    out = torch.zeros(B, P + N, dtype=torch.int64)
    out[:, P] = truth[:, 0]
    ntok = torch.ones(B, dtype=torch.int32)
    lens = torch.tensor(PL, dtype=torch.int32)
    fin = (truth[:, 0] == eos).to(torch.uint8) if eos is not None else None
    stats = torch.zeros(S + 1, dtype=torch.int64)
    steps, done = 0, False
    while not done and steps < N - 1:
        tok_in = torch.zeros(B, S, dtype=torch.int64)
        t = torch.zeros(B, S, dtype=torch.int64)
        for b in range(B):
            nt = int(ntok[b])
            tok_in[b, 0] = out[b, P + nt - 1]
            for j in range(S):
                if j:
                    tok_in[b, j] = table[b, min(nt + j - 1, N - 1)]
                t[b, j] = truth[b, min(nt + j, N - 1)]
        done = accept_reference(tok_in.reshape(-1), t.reshape(-1), out, P, N, ntok, lens, fin, eos, stats, S)
        steps += 1
    return steps


@pytest.mark.parametrize("with_eos", [False, True], ids=["noeos", "eos"])
@pytest.mark.parametrize("draw", sorted(DRAWS))
@pytest.mark.parametrize("source", ["ngram", "table_right", "table_wrong", "table_mixed"])
@pytest.mark.parametrize("S", [2, 4, 8])
def test_tokens_equal_the_plain_loop(model, S, source, draw, with_eos):
    eos = _eos_of(model, draw) if with_eos else None
    want = plain(model, draw, eos)
    truth = want[:, P:]
    if source == "ngram":
        draft = "ngram"
    elif source == "table_right":
        draft = truth.clone()
    elif source == "table_wrong":
        draft = (truth + 1) % 512
    else:
        draft = truth.clone()
        draft[:, [3, 4, 10, 17]] = (draft[:, [3, 4, 10, 17]] + 1) % 512
    got, stats = model.generate(_idx(), N, prompt_lens=PL, sampler="device", seed=SEED, eos_token=eos, speculate=S,
                                draft=draft, return_stats=True, **DRAWS[draw])
    assert torch.equal(got, want)
    assert torch.equal(got[:, :P], _idx())
    assert len(stats["stats"]) == S + 1 and 1 <= stats["verify_steps"] <= N - 1
    if source != "ngram":
        assert stats["verify_steps"] == steps_for(draft, truth, S, eos)
    if eos is None:
        assert sum(e * n for e, n in enumerate(stats["stats"])) == B * (N - 1)
        if source == "table_right":
            assert stats["verify_steps"] == math.ceil((N - 1) / S)
        if source == "table_wrong":
            assert stats["verify_steps"] == N - 1


def test_ngram_lengths_and_default_output(model):
    want = plain(model, "greedy", None)
    for n in (1, 2, 5):
        assert torch.equal(model.generate(_idx(), N, prompt_lens=PL, sampler="device", seed=SEED, temperature=0.0,
                                          speculate=4, ngram=n), want)


def test_one_new_token_needs_no_verify_step(model):
    want = model.generate(_idx(), 1, prompt_lens=PL, sampler="device", seed=SEED)
    got, stats = model.generate(_idx(), 1, prompt_lens=PL, sampler="device", seed=SEED, speculate=2, return_stats=True)
    assert torch.equal(got, want) and stats["verify_steps"] == 0


def test_argument_errors(model):
    idx = _idx()
    ok = dict(sampler="device", seed=1)
    for bad in (1, 9, 0):
        with pytest.raises(ValueError, match="speculate"):
            model.generate(idx, 4, speculate=bad, **ok)
    with pytest.raises(ValueError, match="sampler='device'"):
        model.generate(idx, 4, speculate=2)
    with pytest.raises(ValueError, match="seed"):
        model.generate(idx, 4, speculate=2, sampler="device")
    with pytest.raises(ValueError, match="return_logits"):
        model.generate(idx, 4, speculate=2, return_logits=True, **ok)
    with pytest.raises(ValueError, match="draft"):
        model.generate(idx, 4, speculate=2, draft="model", **ok)
    with pytest.raises(ValueError, match="draft table"):
        model.generate(idx, 4, speculate=2, draft=torch.zeros(B, 5, dtype=torch.int64), **ok)
    with pytest.raises(ValueError, match="draft table"):
        model.generate(idx, 4, speculate=2, draft=torch.zeros(B, 4, dtype=torch.int32), **ok)
    with pytest.raises(ValueError, match="ngram"):
        model.generate(idx, 4, speculate=2, ngram=0, **ok)
    with pytest.raises(ValueError, match="return_stats"):
        model.generate(idx, 4, return_stats=True, **ok)
