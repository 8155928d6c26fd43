"""GPT2.generate(speculate=S) on the GPU (head-dim-64 tiny model: 2 layers, 2 heads, n_embd 128, vocabulary 512,
block_size 256): the tokens are bit for bit those of generate(sampler="device") with the same seed for every S, draft
source, sampling setting, batch size, with and without eos, eager and replayed from a graph, on a reused cache; the
number of verify steps; the cache length; the argument errors of the GPU path."""
import math

import pytest
import torch

from pytorch_distributed_nn_amd.ops.speculate import accept_reference

pytestmark = pytest.mark.gpu
P, N, SEED = 12, 24, 11
PLS = {1: [12], 3: [5, 12, 8]}
DRAWS = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, top_k=20, top_p=0.9)}
SOURCES = ("ngram", "table_right", "table_wrong", "table_mixed")
_PLAIN = {}


@pytest.fixture(scope="module")
def model():
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(0)
    m = build_gpt2("gpt2_tiny", block_size=256)
    with torch.no_grad():                # sharper logits than the 0.02 init gives, so that rows differ
        for p in m.parameters():
            p.mul_(4.0)
    return m.cuda()


def _idx(B):
    base = torch.randint(0, 512, (B, 4), generator=torch.Generator().manual_seed(5))
    return base.repeat(1, 3).cuda()


def plain(model, B, draw, eos):
    """the plain device-sampler tokens, computed once per setting"""
    key = (B, draw, eos)
    if key not in _PLAIN:
        _PLAIN[key] = model.generate(_idx(B), N, prompt_lens=PLS[B], sampler="device", seed=SEED, eos_token=eos,
                                     **DRAWS[draw])
    return _PLAIN[key]


def steps_for(table, truth, pl, S, eos):
    """verify steps the loop needs with drafts from ``table`` when the draws are ``truth`` (CPU tensors): the acceptance
    rule of ops.speculate.accept_reference, step by step"""
    B = truth.shape[0]
    out = torch.zeros(B, P + N, dtype=torch.int64)
    out[:, P] = truth[:, 0]
    ntok = torch.ones(B, dtype=torch.int32)
    lens = torch.tensor(pl, dtype=torch.int32)
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


@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("B", [1, 3])
def test_tokens_equal_the_plain_loop(model, B, graph, S):
    from pytorch_distributed_nn_amd.ops.transformer import KVCache
    pl = PLS[B]
    cache = KVCache(model, B, model.kv_cache_len(P, N + 8), "cuda", S=8)        # one cache, reused by every call below
    for draw in sorted(DRAWS):
        for with_eos in (False, True):
            eos = int(plain(model, B, draw, None)[B - 1, P + N // 2]) if with_eos else None
            want = plain(model, B, draw, eos)
            truth = want[:, P:].cpu()
            for source in SOURCES:
                if source == "ngram":
                    draft = "ngram"
                elif source == "table_right":
                    draft = truth.clone()
                elif source == "table_wrong":
                    draft = (truth + 1) % 512
                else:
                    draft = truth.clone()
                    draft[:, [3, 4, 10, 17]] = (draft[:, [3, 4, 10, 17]] + 1) % 512
                got, stats = model.generate(_idx(B), N, prompt_lens=pl, sampler="device", seed=SEED, eos_token=eos,
                                            speculate=S, draft=draft.cuda() if torch.is_tensor(draft) else draft,
                                            graph=graph, cache=cache, return_stats=True, **DRAWS[draw])
                what = f"{draw} eos={eos} {source}"
                assert torch.equal(got, want), what
                assert torch.equal(got[:, :P], _idx(B)), f"{what}: the prompt columns changed"
                lens = cache.lens.cpu()
                assert bool((lens <= torch.tensor(pl) + N - 1).all()), f"{what}: lens {lens.tolist()}"
                if source != "ngram":
                    assert stats["verify_steps"] == steps_for(draft, truth, pl, S, eos), what
                if eos is None:
                    assert lens.tolist() == [p + N - 1 for p in pl], what
                    assert sum(e * n for e, n in enumerate(stats["stats"])) == B * (N - 1), what
                    if source == "table_right":
                        assert stats["verify_steps"] == math.ceil((N - 1) / S), what
                    if source == "table_wrong":
                        assert stats["verify_steps"] == N - 1, what


def test_fresh_cache_and_ngram_lengths(model):
    want = plain(model, 3, "sampled", None)
    for n in (1, 5):
        got = model.generate(_idx(3), N, prompt_lens=PLS[3], sampler="device", seed=SEED, speculate=4, ngram=n,
                             **DRAWS["sampled"])
        assert torch.equal(got, want)


def test_gpu_argument_errors(model):
    from pytorch_distributed_nn_amd import tuning
    from pytorch_distributed_nn_amd.ops.transformer import KVCache
    ok = dict(sampler="device", seed=1, speculate=4)
    with pytest.raises(ValueError, match="cache"):          # a cache sized for single-query steps
        model.generate(_idx(1), N, cache=KVCache(model, 1, model.kv_cache_len(P, N + 4), "cuda"), **ok)
    with pytest.raises(ValueError, match="cache"):          # no room for the rejected drafts' slots
        model.generate(_idx(1), 200, cache=KVCache(model, 1, model.kv_cache_len(P, 200), "cuda", S=4), **ok)
    big = torch.randint(0, 512, (9, P), generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(ValueError, match="B <= 8"):
        model.generate(big, 4, **ok)
    old = tuning.get("decode_skinny")
    tuning.set("decode_skinny", 0)
    try:
        with pytest.raises(ValueError, match="decode_skinny"):
            model.generate(_idx(1), 4, **ok)
    finally:
        tuning.set("decode_skinny", old)
