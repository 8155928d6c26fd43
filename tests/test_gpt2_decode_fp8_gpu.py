"""GPT2.generate(decode_weights="fp8") on the GPU (test_gpt2_generate_gpu.py's gpt2_tiny, head dim 64): against the CPU
definition (the same dequantised weights in plain PyTorch), and exact under speculation, graph replay and resume."""
import pytest
import torch
import torch.nn.functional as F

from test_gpt2_generate_gpu import _rel, models          # noqa: F401  (models: the (GPU, CPU fp32) pair fixture)

pytestmark = pytest.mark.gpu
NEW = 6
FP8 = dict(decode_weights="fp8")


def _prompts(B, P, seed=3):
    return torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(500 + seed))


def _tolerance(gpu, ref, rows, starts):
    """test_gpt2_generate_gpu.py's bound: 2 e0 + 1e-3, e0 = the worst relative L2 error of the uncached GPU forward on
    the same rows (padded to 128) against the CPU fp32 forward at the generated positions"""
    e0 = 0.0
    with torch.no_grad():
        for row, s in zip(rows, starts):
            g = gpu(F.pad(row[None], (0, 128 - len(row))).cuda()).float().cpu()[:, s - 1:s - 1 + NEW]
            e0 = max(e0, _rel(g, ref(row[None]).float()[:, s - 1:s - 1 + NEW]).max().item())
    return 2 * e0 + 1e-3


def test_fp8_decode_against_the_cpu_definition(models):
    """Greedy, B = 2, mixed prompt lengths; both sides hold the same dq.  Every step's logits within the bf16 tolerance
    while the tokens before it agree; the tokens equal wherever the reference's top-two margin exceeds what that
    tolerance lets two logits move against each other, sqrt(2) tol |logits|.  With this prompt seed the CPU reference
    leaves no (row, step) out up to tol = 0.0209 (smallest margin 0.0296 |logits|); at most a quarter may be.
    Recorded on an MI355X: worst relative L2 6.38e-3, tolerance 1.42e-2, 0 of 12 left out."""
    gpu, ref = models
    P, pl, idx = 9, [5, 9], _prompts(2, 9)
    kw = dict(temperature=0.0, return_logits=True, prompt_lens=pl)
    seq_ref, lg_ref = ref.generate(idx, NEW, **kw, **FP8)
    seq, lg = gpu.generate(idx.cuda(), NEW, **kw, **FP8)
    assert not torch.equal(lg, gpu.generate(idx.cuda(), NEW, **kw)[1]), "decode_weights='fp8' ran on the bf16 weights"
    tol = _tolerance(gpu, ref, [torch.cat([idx[b, :pl[b]], seq_ref[b, P:]]) for b in range(2)], pl)
    top = lg_ref.topk(2).values
    sure = (top[..., 0] - top[..., 1]) > 2 ** 0.5 * tol * lg_ref.norm(dim=-1)
    same = seq.cpu()[:, P:] == seq_ref[:, P:]
    valid = torch.cat([torch.ones(2, 1), same[:, :-1].float().cumprod(1)], 1).bool()     # the tokens before the step agree
    err = _rel(lg.cpu(), lg_ref)[valid].max().item()
    print(f"fp8 decode vs CPU: relative L2 {err:.3e}, tolerance {tol:.3e}, left out {int((~sure).sum())} of {sure.numel()}")
    assert int((~sure).sum()) * 4 <= sure.numel()
    assert same[sure].all(), "a token differs where the reference's margin exceeds the tolerance"
    assert err <= tol


def test_speculation_graph_and_resume_stay_exact(models):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    gpu, ref = models
    idx, N = _prompts(2, 6, seed=7).repeat(1, 3).cuda(), 16         # a repeating prompt: the n-gram draft finds something
    skw = dict(temperature=0.8, top_k=50, top_p=0.9, sampler="device", seed=5, **FP8)
    kw = dict(prompt_lens=[18, 11], **skw)
    plain = gpu.generate(idx, N, **kw)
    wrong = (plain[:, 18:] + 1) % 512                            # a draft table that is wrong at every position
    assert torch.equal(gpu.generate(idx, N, speculate=4, draft=wrong, **kw), plain), "speculate (wrong drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, speculate=4, **kw), plain), "speculate (n-gram drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, graph=True, **kw), plain), "graph=True changed the tokens"
    assert torch.equal(gpu.generate(idx, N, speculate=4, graph=True, **kw), plain)

    def chunked(**more):     # resume=True over two chunks of the prompt
        c = TX.KVCache(gpu, 2, 256, "cuda", S=4)
        gpu.generate(idx[:, :10], 0, cache=c, resume=True, **FP8)
        return gpu.generate(idx[:, 10:], N, cache=c, resume=True, **more)
    # against one call on the whole prompt: the first logits within the bf16 tolerance (test_generate_resume_gpu.py)
    one = gpu.generate(idx, NEW, temperature=0.0, return_logits=True, **FP8)[1]
    two = chunked(temperature=0.0, return_logits=True, **FP8)[1]
    tol = _tolerance(gpu, ref, list(ref.generate(idx.cpu(), NEW, temperature=0.0, **FP8)), [18, 18])
    assert _rel(two[:, 0], one[:, 0]).max().item() <= tol
    assert torch.equal(chunked(speculate=4, **skw), chunked(**skw)), "speculate changed the tokens under resume"
