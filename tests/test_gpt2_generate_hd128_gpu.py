"""GPT2.generate on the GPU at head dim 128 (gpt2_tiny with n_embd 256, n_head 2; the decode kernels of
csrc/kernels/attention_decode_hd128.hip), after test_gpt2_generate_gpu.py: the cached decode path against the CPU fp32
model, graph replay and speculation exact, quantised decode weights, and what stays at head dim 64 refused."""
import copy

import pytest
import torch

from pytorch_distributed_nn_amd.generation import DecodeWeights, fused_stepper

pytestmark = pytest.mark.gpu
NEW = 40


@pytest.fixture(scope="module")
def models():
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(0)
    ref = build_gpt2("gpt2_tiny", n_embd=256, n_head=2, block_size=256).float()
    return copy.deepcopy(ref).cuda(), ref


def _prompts(B, P):
    return torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(100 + P))


def _rel(a, b):
    return ((a.double() - b.double()).norm(dim=-1) / b.double().norm(dim=-1))


@pytest.mark.parametrize("P,weights", [(5, "bf16"), (130, "bf16"), (5, "fp8")])
def test_teacher_forced_logits_against_cpu(models, P, weights):
    """test_gpt2_generate_gpu.py's test and rule: the CPU model's greedy sequence fed step by step through the cached GPU
    path, every step's logits against the CPU logits by relative L2, within 2 e0 + 1e-3 with e0 the uncached GPU
    forward's error on the same rows against the CPU fp32 model (existing code, not the code under test).  "fp8": both
    sides decode on the same dequantised e4m3 weights (the CPU path's definition); e0 stays the bf16 forward's.

    Recorded on an MI355X: P = 5: e0 = 8.12e-3, cached 7.91e-3; P = 130: e0 = 7.73e-3, cached 8.19e-3; P = 5, fp8:
    e0 = 8.12e-3, cached 7.07e-3."""
    gpu, ref = models
    B = 2
    idx = _prompts(B, P)
    seq, lg_ref = ref.generate(idx, NEW, temperature=0.0, return_logits=True, decode_weights=weights)
    T = seq.shape[1]
    Tp = (T + 127) // 128 * 128
    with torch.no_grad():
        full = gpu(torch.nn.functional.pad(seq, (0, Tp - T)).cuda()).float().cpu()
        base = lg_ref if weights == "bf16" else ref(seq).float()[:, P - 1:P - 1 + NEW]
        e0 = _rel(full[:, P - 1:P - 1 + NEW], base).max().item()
        pl = torch.full((B,), P, dtype=torch.int32, device="cuda")
        dec = None if weights == "bf16" else DecodeWeights(gpu, weights)
        logits, step = fused_stepper(gpu, idx.cuda(), pl, NEW, False, None, dec=dec)
        got = [logits.clone()]
        for i in range(NEW - 1):
            got.append(step(seq[:, P + i].cuda()).clone())
    err = _rel(torch.stack(got, 1).cpu(), lg_ref).max().item()
    print(f"P={P} {weights}: uncached GPU forward e0 = {e0:.3e}, cached decode path = {err:.3e}, bound = {2 * e0 + 1e-3:.3e}")
    assert err <= 2 * e0 + 1e-3


def test_graph_replay_and_speculation_are_exact(models):
    gpu, _ = models
    idx = _prompts(3, 130).cuda()
    kw = dict(prompt_lens=[5, 77, 130], temperature=0.9, top_k=20, sampler="device", seed=7)
    t0, l0 = gpu.generate(idx, NEW, return_logits=True, **kw)
    t1, l1 = gpu.generate(idx, NEW, return_logits=True, graph=True, **kw)
    assert torch.equal(t0, t1), "graph=True changed the tokens"
    assert torch.equal(l0, l1), "graph=True changed the logits"
    assert torch.equal(gpu.generate(idx, NEW, speculate=4, **kw), t0), "speculate=4 changed the tokens"
    fused = dict(decode_fused=True, **kw)
    assert torch.equal(gpu.generate(idx, NEW, graph=True, **fused), gpu.generate(idx, NEW, **fused))


def test_what_stays_at_head_dim_64_is_refused(models):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    gpu, _ = models
    idx = _prompts(2, 5).cuda()
    cache = TX.KVCache(gpu, 2, 256, "cuda")
    assert cache.k.shape[-1] == 128
    for call in (lambda: gpu.generate(idx, 3, kv_cache="fp8"),
                 lambda: gpu.generate(idx, 3, cache=cache, resume=True),
                 lambda: gpu.session(2, 64),
                 lambda: TX.KVCache(gpu, 2, 256, "cuda", dtype="fp8")):
        with pytest.raises(ValueError, match="head dim 128"):
            call()
