"""GPT2.generate(decode_weights="mxfp4") on the GPU (test_gpt2_generate_gpu.py's gpt2_tiny, head dim 64): against the CPU
definition (the same dequantised weights in plain PyTorch), and exact under speculation, graph replay, resume and an fp8
key/value cache."""
import pytest
import torch

from test_gpt2_decode_fp8_gpu import NEW, _prompts, _tolerance
from test_gpt2_generate_gpu import _rel, models          # noqa: F401  (models: the (GPU, CPU fp32) pair fixture)

pytestmark = pytest.mark.gpu
FP4 = dict(decode_weights="mxfp4")
SEED = 13


def test_mxfp4_decode_against_the_cpu_definition(models):
    """Greedy, B = 2, mixed prompt lengths; both sides hold the same dq.  Every step's logits within the bf16 tolerance
    (test_gpt2_decode_fp8_gpu.py's: twice the uncached GPU forward's own error against fp32 on the same rows, plus 1e-3)
    while the tokens before it agree; the tokens equal wherever the reference's top-two margin exceeds what that
    tolerance lets two logits move against each other, sqrt(2) tol |logits|; at most a quarter of the (row, step) pairs
    may be left out.  With this prompt seed the CPU reference alone leaves no pair out up to tol = 0.0328 (smallest
    margin 0.0464 |logits|), above 1.5 times the tolerance recorded below.
    Recorded on an MI355X: worst relative L2 6.43e-3, tolerance 1.62e-2, 0 of 12 left out."""
    gpu, ref = models
    P, pl, idx = 9, [5, 9], _prompts(2, 9, SEED)
    kw = dict(temperature=0.0, return_logits=True, prompt_lens=pl)
    seq_ref, lg_ref = ref.generate(idx, NEW, **kw, **FP4)
    seq, lg = gpu.generate(idx.cuda(), NEW, **kw, **FP4)
    assert not torch.equal(lg, gpu.generate(idx.cuda(), NEW, **kw)[1]), "decode_weights='mxfp4' ran on the bf16 weights"
    assert not torch.equal(lg, gpu.generate(idx.cuda(), NEW, decode_weights="fp8", **kw)[1]), "'mxfp4' ran on the fp8 weights"
    tol = _tolerance(gpu, ref, [torch.cat([idx[b, :pl[b]], seq_ref[b, P:]]) for b in range(2)], pl)
    top = lg_ref.topk(2).values
    sure = (top[..., 0] - top[..., 1]) > 2 ** 0.5 * tol * lg_ref.norm(dim=-1)
    same = seq.cpu()[:, P:] == seq_ref[:, P:]
    valid = torch.cat([torch.ones(2, 1), same[:, :-1].float().cumprod(1)], 1).bool()     # the tokens before the step agree
    err = _rel(lg.cpu(), lg_ref)[valid].max().item()
    print(f"mxfp4 decode vs CPU: relative L2 {err:.3e}, tolerance {tol:.3e}, left out {int((~sure).sum())} of {sure.numel()}")
    assert int((~sure).sum()) * 4 <= sure.numel()
    assert same[sure].all(), "a token differs where the reference's margin exceeds the tolerance"
    assert err <= tol


def test_speculation_graph_resume_and_fp8_cache_stay_exact(models):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    gpu, _ = models
    idx, N = _prompts(2, 6, seed=7).repeat(1, 3).cuda(), 16         # a repeating prompt: the n-gram draft finds something
    skw = dict(temperature=0.8, top_k=50, top_p=0.9, sampler="device", seed=5, **FP4)
    kw = dict(prompt_lens=[18, 11], **skw)
    plain = gpu.generate(idx, N, **kw)
    wrong = (plain[:, 18:] + 1) % 512                            # a draft table that is wrong at every position
    assert torch.equal(gpu.generate(idx, N, speculate=4, draft=wrong, **kw), plain), "speculate (wrong drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, speculate=4, **kw), plain), "speculate (n-gram drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, graph=True, **kw), plain), "graph=True changed the tokens"
    assert torch.equal(gpu.generate(idx, N, speculate=4, graph=True, **kw), plain)
    kv = dict(kv_cache="fp8", **kw)                              # the plain loop of the fp8 cache is another computation
    assert torch.equal(gpu.generate(idx, N, speculate=4, graph=True, **kv), gpu.generate(idx, N, **kv)), "with kv_cache='fp8'"

    def chunked(**more):     # resume=True over two chunks of the prompt
        c = TX.KVCache(gpu, 2, 256, "cuda", S=4)
        gpu.generate(idx[:, :10], 0, cache=c, resume=True, **FP4)
        return gpu.generate(idx[:, 10:], N, cache=c, resume=True, **more)
    assert torch.equal(chunked(speculate=4, **skw), chunked(**skw)), "speculate changed the tokens under resume"
    with pytest.raises(ValueError, match="decode_fused"):
        gpu.generate(idx, 2, decode_fused=True, **kw)
