"""GPT-2 decode with ``decode_fused=True`` (gpt2_tiny: n_embd 128, n_head 2, block_size 256): the fused step against the
CPU fp32 model by the criterion and margins of test_gpt2_decode_skinny_gpu.py, speculation and graph replay bit for bit,
fp8 weights with an fp8 cache, and the refusal past 16 rows."""
import pytest
import torch

from pytorch_distributed_nn_amd.generation import fused_stepper
from test_gpt2_decode_skinny_gpu import NEW, _prompts, _rel, models   # noqa: F401  (models: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [5, 130])
def test_teacher_forced_logits_against_cpu_fp32(models, P):
    """The unfused path's test with the fused stepper: relative L2 of every step's logits against the CPU fp32 logits,
    held to 2 e0 + 1e-3 with e0 the worst error of the uncached GPU forward on the same rows."""
    gpu, ref = models
    idx = _prompts(2, P)
    seq, lg_ref = ref.generate(idx, NEW, temperature=0.0, return_logits=True)
    T = seq.shape[1]
    Tp = (T + 127) // 128 * 128
    with torch.no_grad():
        full = gpu(torch.nn.functional.pad(seq, (0, Tp - T)).cuda()).float().cpu()
        pl = torch.full((2,), P, dtype=torch.int32, device="cuda")
        logits, step = fused_stepper(gpu, idx.cuda(), pl, NEW, False, None, fused=True)
        got = [logits.clone()] + [step(seq[:, P + i].cuda()).clone() for i in range(NEW - 1)]
    e0 = _rel(full[:, P - 1:P - 1 + NEW], lg_ref).max().item()
    err = _rel(torch.stack(got, 1).cpu(), lg_ref).max().item()
    print(f"P={P}: uncached GPU forward e0 = {e0:.3e}, decode_fused {err:.3e}, bound = {2 * e0 + 1e-3:.3e}")
    assert err <= 2 * e0 + 1e-3


@pytest.mark.parametrize("fmt", [dict(), dict(decode_weights="fp8", kv_cache="fp8")], ids=["bf16", "fp8"])
def test_speculate_and_graph_are_bitwise(models, fmt):
    gpu, _ = models
    idx = _prompts(3, 130).cuda()
    kw = dict(prompt_lens=[5, 77, 130], sampler="device", seed=11, temperature=0.8, top_k=50, decode_fused=True, **fmt)
    plain = gpu.generate(idx, NEW, **kw)
    assert torch.equal(gpu.generate(idx, NEW, speculate=2, **kw), plain), "speculate=2 changed the tokens"
    assert torch.equal(gpu.generate(idx, NEW, graph=True, **kw), plain), "graph=True changed the tokens"
    assert torch.equal(gpu.generate(idx, NEW, speculate=2, graph=True, **kw), plain)


def test_too_many_rows_are_refused(models):
    gpu, ref = models
    idx = _prompts(5, 5)
    with pytest.raises(ValueError, match="decode_fused"):
        gpu.generate(idx.cuda(), 4, sampler="device", seed=1, speculate=4, decode_fused=True)
    with pytest.raises(ValueError, match="decode_fused"):
        gpu.generate(_prompts(17, 5).cuda(), 4, decode_fused=True)
    assert torch.equal(ref.generate(idx, 4, temperature=0.0, decode_fused=True), ref.generate(idx, 4, temperature=0.0))
