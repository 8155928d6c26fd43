"""GPT2.generate(kv_cache="fp8") on the GPU (test_gpt2_generate_gpu.py's gpt2_tiny, head dim 64): against the CPU
definition (K / V rows round-tripped through e4m3 when stored, plain PyTorch), exact under speculation, graph replay and
resume with either decode_weights, and a Session turn."""
import pytest
import torch

from pytorch_distributed_nn_amd.generation import Engine, Reference
from test_gpt2_decode_fp8_gpu import NEW, _prompts, _tolerance
from test_gpt2_generate_gpu import _rel, models          # noqa: F401  (models: the (GPU, CPU fp32) pair fixture)

pytestmark = pytest.mark.gpu


def _forced(ref, idx, pl, toks, kv):
    """the CPU Reference, teacher-forced: prefill, then one step per column of toks -> fp32 logits [B][1 + n][V]"""
    r = Reference(ref, idx.shape[0], 64, kv=kv)
    with torch.no_grad():
        return torch.stack([r.prefill(idx, torch.tensor(pl))] + [r.step(t) for t in toks.unbind(1)], 1)


def test_teacher_forced_logits_against_the_cpu_definition(models):
    """B = 2, prompts of 5 and 9 tokens, six fixed random tokens per row, all fed: seven logits per row, every one
    compared.  Tolerance 2 e0 + 1e-3 + e_q: the project's bound (_tolerance, over both windows of NEW = 6 positions that
    cover the seven) plus e_q, the relative
    L2 between the CPU reference with kv="fp8" and with the bf16 cache on the same tokens, the quantisation's own effect:
    the two devices' K / V differ at bf16 rounding level before they are quantised, so a few elements land on adjacent
    e4m3 codes, each at most one quantisation step apart.
    Recorded on an MI355X: err 1.06e-2, e0 6.61e-3, e_q 1.10e-2 (tolerance 2.52e-2)."""
    gpu, ref = models
    pl, idx, toks = [5, 9], _prompts(2, 9), _prompts(2, NEW, seed=11)
    want = _forced(ref, idx, pl, toks, "fp8")
    e_q = _rel(want, _forced(ref, idx, pl, toks, "bf16")).max().item()
    rows = [torch.cat([idx[b, :pl[b]], toks[b]]) for b in range(2)]
    tol0 = max(_tolerance(gpu, ref, rows, pl), _tolerance(gpu, ref, rows, [p + 1 for p in pl]))
    got = {}
    with torch.no_grad():
        for kv in ("fp8", "bf16"):
            eng = Engine(gpu, 2, 9, NEW + 1, kv=kv)
            lg = [eng.prefill(idx.cuda(), torch.tensor(pl, dtype=torch.int32, device="cuda")).float()]
            for t in toks.unbind(1):
                lg.append(eng.rows(t.cuda(), eng.cache.lens).float())
                eng.cache.lens.add_(1)
            got[kv] = torch.stack(lg, 1).cpu()
            assert eng.cache.k.dtype == (torch.uint8 if kv == "fp8" else torch.bfloat16)
    assert not torch.equal(got["fp8"][:, 1:], got["bf16"][:, 1:]), "kv_cache='fp8' ran on a bf16 cache"
    err = _rel(got["fp8"], want).max().item()
    print(f"kv fp8 vs CPU: err {err:.3e}, e0 {(tol0 - 1e-3) / 2:.3e}, e_q {e_q:.3e}, tolerance {tol0 + e_q:.3e}")
    assert err <= tol0 + e_q


@pytest.mark.parametrize("decode_weights", ["bf16", "fp8"])
def test_speculation_graph_and_resume_stay_exact(models, decode_weights):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    gpu, _ = models
    idx, N = _prompts(2, 6, seed=7).repeat(1, 3).cuda(), 16         # a repeating prompt: the n-gram draft finds something
    fp8 = dict(kv_cache="fp8", decode_weights=decode_weights)
    skw = dict(temperature=0.8, top_k=50, top_p=0.9, sampler="device", seed=5, **fp8)
    kw = dict(prompt_lens=[18, 11], **skw)
    plain = gpu.generate(idx, N, **kw)
    wrong = (plain[:, 18:] + 1) % 512                            # a draft table that is wrong at every position
    assert torch.equal(gpu.generate(idx, N, speculate=4, draft=wrong, **kw), plain), "speculate (wrong drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, speculate=4, **kw), plain), "speculate (n-gram drafts) changed the tokens"
    assert torch.equal(gpu.generate(idx, N, graph=True, **kw), plain), "graph=True changed the tokens"
    assert torch.equal(gpu.generate(idx, N, speculate=4, graph=True, **kw), plain)

    def chunked(**more):     # resume=True over two chunks of the prompt; the calls follow the cache's dtype
        c = TX.KVCache(gpu, 2, 256, "cuda", S=4, dtype="fp8")
        gpu.generate(idx[:, :10], 0, cache=c, resume=True, decode_weights=decode_weights)
        return gpu.generate(idx[:, 10:], N, cache=c, resume=True, **more)
    assert torch.equal(chunked(speculate=4, **skw), chunked(**skw)), "speculate changed the tokens under resume"


def test_session_turn_against_the_cpu_definition(models):
    """The first logits of a second turn on the kept fp8 cache against the CPU session's definition, generate(kv_cache=
    "fp8") on the whole history, within the tolerance above (e_q over the session's own tokens, teacher-forced).
    Recorded on an MI355X: err 1.05e-2, tolerance 2.49e-2."""
    gpu, ref = models
    s = gpu.session(2, 256, kv_cache="fp8")
    assert s.cache.k.dtype == torch.uint8 and s.cache.ks.dtype == torch.float32
    t1, t2 = _prompts(2, 7, seed=1), _prompts(2, 4, seed=2)
    s.generate(list(t1), NEW, temperature=0.0)
    hist = torch.tensor(s.history)
    # turn 2 as the session runs it: the uncached tail of the history, then the turn; here with the logits kept
    rows = torch.cat([hist[:, s.cached[0]:], t2], 1).cuda()
    lg = gpu.generate(rows, NEW, temperature=0.0, cache=s.cache, resume=True, return_logits=True)[1][:, 0].cpu()
    full = torch.cat([hist, t2], 1)
    seq, want = ref.generate(full, NEW, temperature=0.0, return_logits=True, kv_cache="fp8")
    forced = torch.cat([hist[:, 7:], t2], 1)
    e_q = _rel(_forced(ref, t1, [7, 7], forced, "fp8"), _forced(ref, t1, [7, 7], forced, "bf16")).max().item()
    tol = _tolerance(gpu, ref, list(seq), [full.shape[1]] * 2) + e_q
    err = _rel(lg, want[:, 0]).max().item()
    print(f"session turn 2, kv fp8: err {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
