"""Every refusal of generation.check_args, through GPT2.generate on the CPU: one row per ``raise`` (a condition of two
halves gets one row per half), each a ValueError whose message is told apart by ``match``; and that a call wrong in two
ways raises the earlier refusal.  The refusals of the GPU path need no GPU: they are decided from ``idx.is_cuda`` before
anything runs, so a CPU tensor that answers True there reaches them."""
import pytest
import torch

from pytorch_distributed_nn_amd import tuning
from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2

B, P, N = 2, 6, 4
DEV = dict(sampler="device", seed=1)
SPEC = dict(speculate=2, **DEV)


class _SaysCuda(torch.Tensor):
    # reaches the GPU refusals only while check_args decides by idx.is_cuda; were it to read idx.device instead, these
    # cases would take the CPU route (and fail here, as no refusal follows there)
    is_cuda = True


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_gpt2("gpt2_tiny")                  # head dim 64, block_size 128


def _idx(b=B, p=P):
    return torch.randint(0, 512, (b, p), generator=torch.Generator().manual_seed(3))


def _gpu(idx):
    return idx.as_subclass(_SaysCuda)


# (match, idx, max_new_tokens, keyword arguments), in the order of the checks
REFUSALS = [
    (r"idx must be \[B\]\[P\]", torch.zeros(6, dtype=torch.int64), N, {}),
    (r"idx must be \[B\]\[P\]", torch.zeros(2, 0, dtype=torch.int64), N, {}),
    ("max_new_tokens must be >= 0", _idx(), -1, {}),
    ("prompt_lens must be 2 lengths", _idx(), N, dict(prompt_lens=[3])),
    ("prompt_lens must be 2 lengths", _idx(), N, dict(prompt_lens=[0, 3])),
    ("prompt_lens must be 2 lengths", _idx(), N, dict(prompt_lens=torch.tensor([3, P + 1]))),
    (r"\+ max_new_tokens 123 > block size 128", _idx(), 123, {}),
    (r"temperature must be >= 0 and top_k >= 1, got -0\.5, None", _idx(), N, dict(temperature=-0.5)),
    ("temperature must be >= 0 and top_k >= 1, got 1.0, 0", _idx(), N, dict(top_k=0)),
    ("top_p must be > 0", _idx(), N, dict(top_p=0.0)),
    ("sampler must be 'torch' or 'device', got 'host'", _idx(), N, dict(sampler="host")),
    ("pass seed, and no generator", _idx(), N, dict(sampler="device")),
    ("pass seed, and no generator", _idx(), N, dict(generator=torch.Generator(), **DEV)),
    (r"speculate must be in \[2, 8\], got 1", _idx(), N, dict(speculate=1, **DEV)),
    (r"speculate must be in \[2, 8\], got 9", _idx(), N, dict(speculate=9, **DEV)),
    ("speculate verifies drafts with the counter-based draw", _idx(), N, dict(speculate=2)),
    ("return_logits is not available with speculate", _idx(), N, dict(return_logits=True, **SPEC)),
    (r"a draft table must be int64 \[2\]\[4\], got torch.int64 \(2, 5\)", _idx(), N,
     dict(draft=torch.zeros(B, N + 1, dtype=torch.int64), **SPEC)),
    (r"a draft table must be int64 \[2\]\[4\], got torch.int32", _idx(), N,
     dict(draft=torch.zeros(B, N, dtype=torch.int32), **SPEC)),
    ("draft must be 'ngram' or an int64", _idx(), N, dict(draft="model", **SPEC)),
    ("ngram must be an int >= 1, got 0", _idx(), N, dict(ngram=0, **SPEC)),
    ("ngram must be an int >= 1, got 2.0", _idx(), N, dict(ngram=2.0, **SPEC)),
    (r"speculate on the GPU needs tuning decode_skinny on, B <= 8 and B \* S <= 64 .*B = 9, S = 2", _gpu(_idx(9)), N, SPEC),
    ("return_stats needs speculate", _idx(), N, dict(return_stats=True)),
]


@pytest.mark.parametrize("match,idx,new,kw", REFUSALS, ids=["-".join([str(i), *sorted(r[3])]) for i, r in enumerate(REFUSALS)])
def test_refusal(model, match, idx, new, kw):
    with pytest.raises(ValueError, match=match):
        model.generate(idx, new, **kw)


def test_gpu_speculate_refusal_of_the_switch(model):
    """(the row above is its B half; B <= 8 and S <= 8 leave B * S <= 64 nothing to refuse)"""
    old = tuning.get("decode_skinny")
    tuning.set("decode_skinny", 0)
    try:
        with pytest.raises(ValueError, match="got decode_skinny = 0, B = 2, S = 2"):
            model.generate(_gpu(_idx()), N, **SPEC)
    finally:
        tuning.set("decode_skinny", old)


def test_head_dim_refusal_is_the_gpu_path_s_alone():
    torch.manual_seed(0)
    m = build_gpt2("gpt2_tiny", n_head=4)           # head dim 32
    with pytest.raises(ValueError, match=r"generation needs the fused kernels \(head dim 64\); got head dim 32"):
        m.generate(_gpu(_idx()), N)
    assert m.generate(_idx(), N, temperature=0.0).shape == (B, P + N)       # the CPU path runs any head dim


def test_the_earlier_refusal_wins(model):
    with pytest.raises(ValueError, match="max_new_tokens must be >= 0"):
        model.generate(_idx(), -1, temperature=-1.0)
    with pytest.raises(ValueError, match="return_logits is not available"):
        model.generate(_idx(), N, return_logits=True, ngram=0, **SPEC)


def test_nothing_to_generate_returns_early(model):
    idx = _idx()
    assert torch.equal(model.generate(idx, 0), idx)
    out, lg = model.generate(idx, 0, return_logits=True)
    assert torch.equal(out, idx) and lg.shape == (B, 0, 512)
    out, stats = model.generate(idx, 0, return_stats=True, **SPEC)
    assert torch.equal(out, idx) and stats == {"verify_steps": 0, "stats": [0, 0, 0]}
