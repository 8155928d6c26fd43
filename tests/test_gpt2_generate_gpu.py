"""GPT2.generate on the GPU (gpt2_tiny: n_embd 128, n_head 2 = head dim 64; prompts of 5 and 130 tokens, 40 new tokens):
the cached decode path against the CPU fp32 model, graph replay against eager, cache reuse, and that generation leaves
the training path alone."""
import copy

import pytest
import torch

from pytorch_distributed_nn_amd.generation import fused_stepper

pytestmark = pytest.mark.gpu
NEW = 40


def _tiny(seed=0, **kw):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(seed)
    return build_gpt2("gpt2_tiny", block_size=256, **kw)


@pytest.fixture(scope="module")
def models():
    ref = _tiny().float()
    return copy.deepcopy(ref).cuda(), ref


def _prompts(B, P):
    return torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(100 + P))


def _rel(a, b):
    """relative L2 error of every row of a against b -> [rows]"""
    return ((a.double() - b.double()).norm(dim=-1) / b.double().norm(dim=-1))


@pytest.mark.parametrize("P", [5, 130])
def test_teacher_forced_logits_against_cpu_fp32(models, P):
    """The greedy sequence of the fp32 CPU model, fed step by step through the cached GPU decode path (no bf16 near-tie
    can change the sequence); every step's logits against the CPU fp32 logits by relative L2.  The bound is measured
    here against existing code: e0 = the worst relative L2 error of the uncached GPU forward(idx) on the same rows
    (padded to 128) against the same CPU logits; the cached path must stay within 2 e0 + 1e-3 (the two GPU paths round
    independently, with other GEMM row counts and another softmax order, at the same magnitude).

    Recorded on an MI355X: P = 5: e0 = 6.94e-3, cached 7.29e-3; P = 130: e0 = 7.87e-3, cached 7.74e-3."""
    gpu, ref = models
    B = 2
    idx = _prompts(B, P)
    seq, lg_ref = ref.generate(idx, NEW, temperature=0.0, return_logits=True)        # [B][P+NEW], [B][NEW][V]
    # e0: the existing uncached forward on the full rows, padded to a multiple of 128
    T = seq.shape[1]
    Tp = (T + 127) // 128 * 128
    with torch.no_grad():
        full = gpu(torch.nn.functional.pad(seq, (0, Tp - T)).cuda()).float().cpu()
    e0 = _rel(full[:, P - 1:P - 1 + NEW], lg_ref).max().item()
    # the cached path, teacher-forced
    with torch.no_grad():
        pl = torch.full((B,), P, dtype=torch.int32, device="cuda")
        logits, step = fused_stepper(gpu, idx.cuda(), pl, NEW, False, None)
        got = [logits.clone()]
        for i in range(NEW - 1):
            got.append(step(seq[:, P + i].cuda()).clone())
    got = torch.stack(got, 1).cpu()
    err = _rel(got, lg_ref).max().item()
    print(f"P={P}: uncached GPU forward e0 = {e0:.3e}, cached decode path = {err:.3e}, bound = {2 * e0 + 1e-3:.3e}")
    assert err <= 2 * e0 + 1e-3


@pytest.mark.parametrize("sampling", ["greedy", "sampled"])
def test_graph_replay_is_bitwise_the_eager_loop(models, sampling):
    gpu, _ = models
    idx = _prompts(3, 130).cuda()
    kw = dict(temperature=0.0) if sampling == "greedy" else dict(temperature=0.9, top_k=20)
    outs = []
    for graph in (False, True):
        if sampling == "sampled":
            kw["generator"] = torch.Generator(device="cuda").manual_seed(7)
        outs.append(gpu.generate(idx, NEW, prompt_lens=[5, 77, 130], graph=graph, return_logits=True, **kw))
    (t0, l0), (t1, l1) = outs
    assert torch.equal(t0, t1), "graph=True changed the tokens"
    assert torch.equal(l0, l1), "graph=True changed the logits"


def test_second_call_on_a_reset_cache_reproduces_the_first(models):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    gpu, _ = models
    idx = _prompts(2, 5).cuda()
    cache = TX.KVCache(gpu, 2, gpu.kv_cache_len(5, NEW), "cuda")
    a = gpu.generate(idx, NEW, temperature=0.0, return_logits=True, cache=cache, eos_token=3)
    assert bool((cache.lens == 5 + NEW - 1).all())
    cache.reset()
    assert bool((cache.lens == 0).all())
    b = gpu.generate(idx, NEW, temperature=0.0, return_logits=True, cache=cache, eos_token=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = gpu.generate(idx, NEW, temperature=0.0, return_logits=True, eos_token=3)      # and a fresh cache
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    with pytest.raises(ValueError):
        gpu.generate(_prompts(3, 5).cuda(), NEW, cache=cache)


def test_training_step_is_unchanged_by_generate():
    """forward + backward of the same model after a generate call: the same loss, bitwise.  No state is left behind."""
    m = _tiny(seed=1).cuda()
    idx, tgt = _prompts(2, 128).cuda(), _prompts(2, 128).flip(1).cuda()
    m.train()

    def loss_and_grad():
        m.zero_grad(set_to_none=True)
        loss = m(idx, tgt)
        loss.backward()
        return loss.detach().clone(), m.transformer.h[0].attn.c_attn.weight.grad.clone()       # grads: atomics, not compared
    l0, g0 = loss_and_grad()
    m.generate(idx[:, :5], 8, temperature=0.0, graph=True)
    assert m.training
    l1, g1 = loss_and_grad()
    assert torch.equal(l0, l1) and bool(torch.isfinite(g1).all())


def test_head_dim_guard():
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    m = build_gpt2("gpt2_tiny", n_head=4).cuda()                    # head dim 32
    with pytest.raises(ValueError, match="head dim 64"):
        m.generate(_prompts(1, 5).cuda(), 3)
    with pytest.raises(ValueError, match="block size"):
        build_gpt2("gpt2_tiny").cuda().generate(_prompts(1, 100).cuda(), 29)
