"""GPT2.generate(prefill_weights="decode") on the GPU (test_gpt2_generate_gpu.py's gpt2_tiny, head dim 64), both stored
formats: against the CPU definition (one model on the dequantised weights, prompt included), exact under speculation,
graph replay and an fp8 key/value cache, and independent of how a prompt is cut into resume=True chunks."""
import pytest
import torch

from test_gpt2_decode_fp8_gpu import NEW, _prompts, _tolerance
from test_gpt2_generate_gpu import _rel, models          # noqa: F401  (models: the (GPU, CPU fp32) pair fixture)

pytestmark = pytest.mark.gpu
SEED = 11
FMTS = ["fp8", "mxfp4"]


@pytest.mark.parametrize("fmt", FMTS)
def test_quantised_prefill_against_the_cpu_definition(models, fmt):
    """test_mxfp4_decode_against_the_cpu_definition with prefill_weights="decode" on both sides: greedy, B = 2, mixed
    prompt lengths, logits within its tolerance (twice the uncached GPU forward's own error against fp32, plus 1e-3,
    measured here) while the tokens before agree, tokens equal wherever the reference's top-two margin exceeds sqrt(2) tol
    |logits|, at most a quarter of the (row, step) pairs left out.  With this prompt seed the CPU reference alone
    leaves no pair out up to tol = 0.0360 (fp8) and 0.0248 (mxfp4), above 1.5 x 1.62e-2 = 0.0243.
    Recorded on an MI355X: worst relative L2 5.55e-3 (fp8), 6.01e-3 (mxfp4), tolerance 1.42e-2, 0 of 12 left out."""
    gpu, ref = models
    P, pl, idx = 9, [5, 9], _prompts(2, 9, SEED)
    kw = dict(temperature=0.0, return_logits=True, prompt_lens=pl, decode_weights=fmt)
    seq_ref, lg_ref = ref.generate(idx, NEW, prefill_weights="decode", **kw)
    seq, lg = gpu.generate(idx.cuda(), NEW, prefill_weights="decode", **kw)
    assert not torch.equal(lg, gpu.generate(idx.cuda(), NEW, prefill_weights="bf16", **kw)[1]), "the prefill ran on the bf16 weights"
    tol = _tolerance(gpu, ref, [torch.cat([idx[b, :pl[b]], seq_ref[b, P:]]) for b in range(2)], pl)
    top = lg_ref.topk(2).values
    sure = (top[..., 0] - top[..., 1]) > 2 ** 0.5 * tol * lg_ref.norm(dim=-1)
    same = seq.cpu()[:, P:] == seq_ref[:, P:]
    valid = torch.cat([torch.ones(2, 1), same[:, :-1].float().cumprod(1)], 1).bool()     # the tokens before the step agree
    err = _rel(lg.cpu(), lg_ref)[valid].max().item()
    print(f"{fmt} prefill + decode vs CPU: relative L2 {err:.3e}, tolerance {tol:.3e}, left out {int((~sure).sum())} of {sure.numel()}")
    assert int((~sure).sum()) * 4 <= sure.numel()
    assert same[sure].all(), "a token differs where the reference's margin exceeds the tolerance"
    assert err <= tol


@pytest.mark.parametrize("fmt", FMTS)
def test_speculation_graph_and_fp8_cache_stay_exact(models, fmt):
    gpu, _ = models
    idx, N = _prompts(2, 6, seed=7).repeat(1, 3).cuda(), 16         # a repeating prompt: the n-gram draft finds something
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, sampler="device", seed=5, prompt_lens=[18, 11], decode_weights=fmt,
              prefill_weights="decode")
    plain = gpu.generate(idx, N, **kw)
    wrong = (plain[:, 18:] + 1) % 512                            # a draft table that is wrong at every position
    assert torch.equal(gpu.generate(idx, N, speculate=4, draft=wrong, **kw), plain), "speculate (wrong drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, speculate=4, **kw), plain), "speculate (n-gram drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, graph=True, **kw), plain), "graph=True changed the tokens"
    kv = dict(kv_cache="fp8", **kw)                              # the plain loop of the fp8 cache is another computation
    assert torch.equal(gpu.generate(idx, N, speculate=4, graph=True, **kv), gpu.generate(idx, N, **kv)), "with kv_cache='fp8'"


@pytest.mark.parametrize("fmt", FMTS)
def test_ingest_does_not_depend_on_the_chunking(models, fmt):
    """18 tokens through resume=True as 10 + 8 and as one chunk of 18 (both Engine.extend on 64-row padded chunks, the
    first an ingest-only call, which builds its own snapshot): every later logit is bit-equal, which needs the GEMM's
    and attn_extend's row bits to be independent of the rows around them."""
    from pytorch_distributed_nn_amd.ops import transformer as TX
    gpu, _ = models
    idx = _prompts(2, 18, seed=7).cuda()
    kw = dict(temperature=0.0, return_logits=True, decode_weights=fmt, prefill_weights="decode", resume=True)
    c1, c2 = (TX.KVCache(gpu, 2, 256, "cuda") for _ in range(2))
    gpu.generate(idx[:, :10], 0, cache=c1, **kw)
    seq1, lg1 = gpu.generate(idx[:, 10:], NEW, cache=c1, **kw)
    seq2, lg2 = gpu.generate(idx, NEW, cache=c2, **kw)
    assert torch.equal(seq1[:, 8:], seq2[:, 18:]) and torch.equal(lg1, lg2), "the chunking of the prompt reached the logits"
