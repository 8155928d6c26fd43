"""GPT-2 decode on the skinny-M GEMM (ops.linear.linear_fwd_decode -> ops.kernels.gemm_skinny; gpt2_tiny: n_embd 128,
n_head 2 = head dim 64, block_size 256): which linears are routed there and when, that tuning ``decode_skinny`` = 0 is the
path before the kernel bit for bit, the accuracy of both paths against the CPU fp32 model, graph replay against eager with
mixed prompt lengths, cache reuse, and that training is left alone."""
import copy

import pytest
import torch

from pytorch_distributed_nn_amd.generation import fused_stepper

pytestmark = pytest.mark.gpu
NEW = 24


def _tiny(seed=0, **kw):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(seed)
    return build_gpt2("gpt2_tiny", block_size=256, **kw)


@pytest.fixture(scope="module")
def models():
    ref = _tiny().float()
    return copy.deepcopy(ref).cuda(), ref


@pytest.fixture
def switch():
    """-> set(value); the tuning entry is put back afterwards"""
    from pytorch_distributed_nn_amd import tuning
    old = tuning.get("decode_skinny")
    yield lambda v: tuning.set("decode_skinny", v)
    tuning.set("decode_skinny", old)


def _prompts(B, P):
    return torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(100 + P))


def _rel(a, b):
    return ((a.double() - b.double()).norm(dim=-1) / b.double().norm(dim=-1))


def _teacher_forced(gpu, idx, seq, P, new):
    """the cached decode path fed the given sequence -> logits [B][new][V] on the CPU"""
    with torch.no_grad():
        pl = torch.full((idx.shape[0],), P, dtype=torch.int32, device="cuda")
        logits, step = fused_stepper(gpu, idx.cuda(), pl, new, False, None)
        got = [logits.clone()]
        for i in range(new - 1):
            got.append(step(seq[:, P + i].cuda()).clone())
    return torch.stack(got, 1).cpu()


def test_routing(models, switch, monkeypatch):
    from pytorch_distributed_nn_amd.ops import kernels
    gpu, _ = models
    L = gpu.config.n_layer
    calls = []
    real = kernels.gemm_skinny
    monkeypatch.setattr(kernels, "gemm_skinny", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])

    def one_decode_step(B):
        idx = _prompts(B, 5).cuda()
        with torch.no_grad():
            pl = torch.full((B,), 5, dtype=torch.int32, device="cuda")
            logits, step = fused_stepper(gpu, idx, pl, 2, False, None)
            calls.clear()                                   # the prefill's first-token head is not the step
            step(logits.argmax(-1))
        torch.cuda.synchronize()
        return list(calls)
    assert kernels.SKINNY_MAX_M >= 2
    got = one_decode_step(2)
    assert got == [2] * (4 * L + 1), got
    switch(0)
    assert one_decode_step(2) == []
    switch(1)
    if kernels.SKINNY_MAX_M < 64:                           # (at 64 every batch the kernel takes is routed to it)
        assert one_decode_step(kernels.SKINNY_MAX_M + 1) == []
    else:
        assert one_decode_step(65) == []
    # the first-token head after the prefill has M = B rows too
    calls.clear()
    with torch.no_grad():
        fused_stepper(gpu, _prompts(2, 5).cuda(), torch.full((2,), 5, dtype=torch.int32, device="cuda"), 2, False, None)
    assert calls == [2]


def test_off_switch_is_the_previous_path_bitwise(models, switch, monkeypatch):
    from pytorch_distributed_nn_amd.ops import linear as BL
    gpu, ref = models
    idx = _prompts(2, 5)
    seq = ref.generate(idx, NEW, temperature=0.0)
    switch(0)
    off = _teacher_forced(gpu, idx, seq, 5, NEW)
    switch(1)
    monkeypatch.setattr(BL, "linear_fwd_decode", lambda x, wk, bias=None, act=0, res=None: BL.linear_fwd(x, wk, bias=bias, act=act, res=res))
    old = _teacher_forced(gpu, idx, seq, 5, NEW)
    assert torch.equal(off, old)


@pytest.mark.parametrize("P", [5, 130])
def test_teacher_forced_logits_against_cpu_fp32(models, switch, P):
    """As test_gpt2_generate_gpu.py: the fp32 CPU model's greedy sequence fed through the cached GPU path; every step's
    logits against the CPU fp32 logits by relative L2, held to 2 e0 + 1e-3 with e0 the worst error of the uncached GPU
    forward on the same rows.  Both switch positions are measured; the new path (1) is the one asserted here, the old one
    by the existing test.

    Recorded on an MI355X: P = 5: e0 = 6.94e-3, decode_skinny=1 7.29e-3, decode_skinny=0 7.29e-3; P = 130: e0 = 7.38e-3,
    decode_skinny=1 7.54e-3, decode_skinny=0 7.54e-3 (the two paths differ in few bf16 roundings of the same fp32 sums)."""
    gpu, ref = models
    B = 2
    idx = _prompts(B, P)
    seq, lg_ref = ref.generate(idx, NEW, temperature=0.0, return_logits=True)
    T = seq.shape[1]
    Tp = (T + 127) // 128 * 128
    with torch.no_grad():
        full = gpu(torch.nn.functional.pad(seq, (0, Tp - T)).cuda()).float().cpu()
    e0 = _rel(full[:, P - 1:P - 1 + NEW], lg_ref).max().item()
    err = {}
    for v in (1, 0):
        switch(v)
        err[v] = _rel(_teacher_forced(gpu, idx, seq, P, NEW), lg_ref).max().item()
    print(f"P={P}: uncached GPU forward e0 = {e0:.3e}, decode_skinny=1 {err[1]:.3e}, decode_skinny=0 {err[0]:.3e}, "
          f"bound = {2 * e0 + 1e-3:.3e}")
    assert err[1] <= 2 * e0 + 1e-3


def test_graph_replay_and_reset_cache(models):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    gpu, _ = models
    idx = _prompts(3, 130).cuda()
    outs = [gpu.generate(idx, NEW, prompt_lens=[5, 77, 130], graph=g, return_logits=True, temperature=0.0)
            for g in (False, True)]
    assert torch.equal(outs[0][0], outs[1][0]), "graph=True changed the tokens"
    assert torch.equal(outs[0][1], outs[1][1]), "graph=True changed the logits"
    cache = TX.KVCache(gpu, 3, gpu.kv_cache_len(130, NEW), "cuda")
    a = gpu.generate(idx, NEW, prompt_lens=[5, 77, 130], temperature=0.0, return_logits=True, cache=cache)
    cache.reset()
    b = gpu.generate(idx, NEW, prompt_lens=[5, 77, 130], temperature=0.0, return_logits=True, cache=cache)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], outs[0][0]) and torch.equal(a[1], outs[0][1])


def test_training_step_is_unchanged_by_generate():
    m = _tiny(seed=1).cuda()
    idx, tgt = _prompts(2, 128).cuda(), _prompts(2, 128).flip(1).cuda()
    m.train()

    def loss():
        m.zero_grad(set_to_none=True)
        out = m(idx, tgt)
        out.backward()
        return out.detach().clone()
    l0 = loss()
    m.generate(idx[:, :5], 8, temperature=0.0, graph=True)
    assert m.training
    assert torch.equal(l0, loss())
