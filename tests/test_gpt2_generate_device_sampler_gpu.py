"""GPT2.generate(sampler="device") on the GPU (gpt2_tiny, V = 512, prompts of 130 columns): every token against the
numpy reference from the GPU's own logits, graph replay against the eager loop, seeds, mixed prompt lengths, and that
generation leaves the training path alone."""
import pytest
import torch

import sample_ref as R

pytestmark = pytest.mark.gpu
NEW, P = 24, 130
KW = dict(temperature=0.9, top_k=40, top_p=0.9, sampler="device")


def _tiny(seed=0):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(seed)
    return build_gpt2("gpt2_tiny", block_size=256)


@pytest.fixture(scope="module")
def gpu():
    return _tiny().cuda()


def _prompts(B):
    return torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(100 + P)).cuda()


@pytest.fixture(scope="module")
def eager(gpu):
    return gpu.generate(_prompts(3), NEW, prompt_lens=[5, 77, 130], seed=11, return_logits=True, **KW)


def test_every_token_is_the_definitions(eager):
    """the logits returned are the fp32 image of the bf16 logits the kernel sampled from"""
    out, lg = eager
    assert lg.shape == (3, NEW, 512) and lg.dtype == torch.float32 and out.shape == (3, P + NEW)
    lg, worst = lg.cpu().numpy(), 0.0
    for i in range(NEW):
        for b in range(3):
            worst = max(worst, R.check_row(lg[b, i], 0.9, 40, 0.9, R.uniform(11, i, b), int(out[b, P + i])))
    print(f"worst distance / EPS {worst:.4f}")


def test_graph_is_bitwise_the_eager_loop_with_eos(gpu, eager):
    out, lg = eager
    eos = int(out[1, P + 5])                                  # an id that occurs
    a = gpu.generate(_prompts(3), NEW, prompt_lens=[5, 77, 130], seed=11, return_logits=True, eos_token=eos, **KW)
    b = gpu.generate(_prompts(3), NEW, prompt_lens=[5, 77, 130], seed=11, return_logits=True, eos_token=eos, graph=True,
                     **KW)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0][1, :P + 6], out[1, :P + 6]) and bool((a[0][1, P + 5:] == eos).all())
    g = gpu.generate(_prompts(3), NEW, prompt_lens=[5, 77, 130], seed=11, return_logits=True, graph=True, **KW)
    assert torch.equal(g[0], out) and torch.equal(g[1], lg)


def test_seeds(gpu, eager):
    again = gpu.generate(_prompts(3), NEW, prompt_lens=[5, 77, 130], seed=11, **KW)
    other = gpu.generate(_prompts(3), NEW, prompt_lens=[5, 77, 130], seed=12, **KW)
    assert torch.equal(again, eager[0]) and not torch.equal(other, eager[0])
    with pytest.raises(ValueError):
        gpu.generate(_prompts(3), 2, **KW)
    with pytest.raises(ValueError):
        gpu.generate(_prompts(3), 2, seed=1, generator=torch.Generator(device="cuda"), **KW)


def test_torch_sampler_takes_top_p(gpu):
    out, lg = gpu.generate(_prompts(2), 6, temperature=1.0, top_p=0.3, return_logits=True,
                           generator=torch.Generator(device="cuda").manual_seed(1))
    for i in range(6):
        for b in range(2):
            sp, si = torch.softmax(lg[b, i].double(), -1).sort(descending=True)
            assert int(out[b, P + i]) in si[:int((sp.cumsum(0) - sp < 0.3).sum()) + 1].tolist()


def test_training_step_is_unchanged_by_generate():
    m = _tiny(seed=1).cuda()
    idx, tgt = _prompts(2)[:, :128], _prompts(2)[:, :128].flip(1)
    m.train()

    def loss():
        m.zero_grad(set_to_none=True)
        l = m(idx, tgt)
        l.backward()
        return l.detach().clone()
    l0 = loss()
    m.generate(idx[:, :5], 8, seed=3, graph=True, **KW)
    assert m.training
    assert torch.equal(l0, loss())
