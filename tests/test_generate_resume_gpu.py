"""generate(resume=True) and generation.Session on the GPU (gpt2_tiny: n_embd 128, n_head 2 = head dim 64, block size
256): the resumed ingest (append + extend kernels) and the decode steps behind it against the CPU fp32 model, chunked
ingest, and the exact properties: graph replay, speculative decoding, a rewound Session, and that resume leaves the
default path alone."""
import copy

import pytest
import torch

from pytorch_distributed_nn_amd.generation import fused_stepper

pytestmark = pytest.mark.gpu
NEW = 10


def _tiny(seed=0, **kw):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(seed)
    return build_gpt2("gpt2_tiny", block_size=256, **kw)


@pytest.fixture(scope="module")
def models():
    ref = _tiny().float()
    return copy.deepcopy(ref).cuda(), ref


def _prompts(B, P, seed=0):
    return torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(300 + P + seed))


def _rel(a, b):
    """relative L2 error of every row of a against b -> [rows]"""
    return ((a.double() - b.double()).norm(dim=-1) / b.double().norm(dim=-1))


def _cache(gpu, B, S=1):
    from pytorch_distributed_nn_amd.ops import transformer as TX
    return TX.KVCache(gpu, B, 256, "cuda", S=S)


def _forced(gpu, cache, idx, seq_new):
    """resume: ingest idx [B][P] behind the cache, then feed seq_new[:, :-1] step by step -> fp32 logits [B][N][V]"""
    B, P = idx.shape
    pl = torch.full((B,), P, dtype=torch.int32, device="cuda")
    logits, step = fused_stepper(gpu, idx.cuda(), pl, seq_new.shape[1], False, cache, resume=True)
    got = [logits.clone()]
    for i in range(seq_new.shape[1] - 1):
        got.append(step(seq_new[:, i].cuda()).clone())
    return torch.stack(got, 1).cpu()


def _uncached(gpu, seq):
    """the existing uncached GPU forward on the rows, padded to a multiple of 128 -> fp32 logits [B][T][V]"""
    T = seq.shape[1]
    with torch.no_grad():
        return gpu(torch.nn.functional.pad(seq, (0, (T + 127) // 128 * 128 - T)).cuda()).float().cpu()[:, :T]


@pytest.mark.parametrize("P1", [5, 70])
def test_two_turns_teacher_forced_against_cpu_fp32(models, P1):
    """Two turns on one kept cache.  The fp32 CPU model generates greedily on the concatenation (turn 1: P1 tokens + 10
    new; turn 2: the last emitted token, which was never run, + 20 tokens, + 10 new), and its tokens are fed through the
    resumed GPU path (turn 1 is a resume behind an empty cache); the logits of every step of both turns against the CPU
    fp32 logits by relative L2.  The bound is test_gpt2_generate_gpu.py's: e0 = the worst relative L2 error of the
    uncached GPU forward(idx) on the same rows (padded to 128) against the same CPU logits; the resumed path must stay
    within 2 e0 + 1e-3.

    Recorded on an MI355X: P1 = 5: e0 = 7.18e-3, resumed turn 1 7.41e-3, turn 2 6.76e-3; P1 = 70: e0 = 7.39e-3,
    resumed turn 1 7.05e-3, turn 2 7.64e-3."""
    gpu, ref = models
    B, P2 = 2, 20
    t1, t2 = _prompts(B, P1), _prompts(B, P2, seed=1)
    seq1, lg1 = ref.generate(t1, NEW, temperature=0.0, return_logits=True)
    seq2, lg2 = ref.generate(torch.cat([seq1, t2], 1), NEW, temperature=0.0, return_logits=True)
    T1 = P1 + NEW
    full = _uncached(gpu, seq2)
    e0 = max(_rel(full[:, P1 - 1:T1 - 1], lg1).max().item(), _rel(full[:, T1 + P2 - 1:T1 + P2 - 1 + NEW], lg2).max().item())
    cache = _cache(gpu, B)
    with torch.no_grad():
        got1 = _forced(gpu, cache, t1, seq1[:, P1:])
        assert cache.lens.tolist() == [T1 - 1] * B
        got2 = _forced(gpu, cache, torch.cat([seq1[:, -1:], t2], 1), seq2[:, T1 + P2:])
        assert cache.lens.tolist() == [T1 + P2 + NEW - 1] * B
    e1, e2 = _rel(got1, lg1).max().item(), _rel(got2, lg2).max().item()
    print(f"P1={P1}: uncached GPU forward e0 = {e0:.3e}, resumed turn 1 = {e1:.3e}, turn 2 = {e2:.3e}, "
          f"bound = {2 * e0 + 1e-3:.3e}")
    assert max(e1, e2) <= 2 * e0 + 1e-3


def test_chunked_ingest_teacher_forced_against_cpu_fp32(models):
    """A 130-token prompt ingested in chunks of 64 (64, 64, 2) by resume=True, max_new_tokens=0, then decoded; the same
    comparison and bound.

    Recorded on an MI355X: e0 = 6.90e-3, chunked ingest + decode 6.78e-3."""
    gpu, ref = models
    B, P = 2, 130
    idx = _prompts(B, P)
    seq, lg = ref.generate(idx, NEW, temperature=0.0, return_logits=True)
    e0 = _rel(_uncached(gpu, seq)[:, P - 1:P - 1 + NEW], lg).max().item()
    cache = _cache(gpu, B)
    with torch.no_grad():
        for c0 in (0, 64):
            out = gpu.generate(idx[:, c0:c0 + 64].cuda(), 0, cache=cache, resume=True)
            assert out.shape == (B, 64) and cache.lens.tolist() == [c0 + 64] * B
        got = _forced(gpu, cache, idx[:, 128:], seq[:, P:])
    err = _rel(got, lg).max().item()
    print(f"chunked: uncached GPU forward e0 = {e0:.3e}, chunked ingest + decode = {err:.3e}, bound = {2 * e0 + 1e-3:.3e}")
    assert err <= 2 * e0 + 1e-3


def _ingested(gpu, B, S=1):
    """a cache that holds a first turn of 70 tokens (ragged: row b has 70 - 9 b)"""
    cache = _cache(gpu, B, S)
    pl = [70 - 9 * b for b in range(B)]
    gpu.generate(_prompts(B, 70).cuda(), 0, prompt_lens=pl, cache=cache, resume=True)
    assert cache.lens.tolist() == pl
    return cache


def test_graph_replay_is_bitwise_the_eager_loop_with_resume(models):
    gpu, _ = models
    idx = _prompts(3, 20, seed=2).cuda()
    outs = []
    for graph in (False, True):
        outs.append(gpu.generate(idx, NEW, prompt_lens=[20, 3, 11], graph=graph, return_logits=True, temperature=0.9, top_k=20,
                                 generator=torch.Generator(device="cuda").manual_seed(7), cache=_ingested(gpu, 3),
                                 resume=True))
    (t0, l0), (t1, l1) = outs
    assert torch.equal(t0, t1), "graph=True changed the tokens"
    assert torch.equal(l0, l1), "graph=True changed the logits"


def test_speculate_is_bitwise_the_plain_loop_with_resume(models):
    gpu, _ = models
    turn = _prompts(2, 6, seed=3).repeat(1, 4).cuda()            # a repeating turn: the n-gram draft has something to find
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, sampler="device", seed=5, prompt_lens=[24, 17])
    plain = gpu.generate(turn, 24, cache=_ingested(gpu, 2, 4), resume=True, **kw)
    spec, stats = gpu.generate(turn, 24, cache=_ingested(gpu, 2, 4), resume=True, speculate=4, return_stats=True, **kw)
    assert torch.equal(plain, spec), "speculate changed the tokens under resume"
    assert stats["verify_steps"] >= 1
    assert torch.equal(gpu.generate(turn, 24, cache=_ingested(gpu, 2, 4), resume=True, speculate=4, graph=True, **kw), plain)


def test_rewound_session_reproduces_the_turn(models):
    gpu, _ = models
    s = gpu.session(2, 256)
    t1 = [_prompts(1, 70)[0].tolist(), _prompts(1, 5)[0].tolist()]
    t2 = [_prompts(1, 20, seed=4)[0].tolist(), _prompts(1, 33, seed=5)[0].tolist()]
    n1 = s.generate(t1, NEW, temperature=0.0)
    len1 = [len(h) for h in s.history]
    assert len1 == [80, 15] and s.cached == [79, 14] and s.cache.lens.tolist() == [79, 14]
    n2 = s.generate(t2, NEW, temperature=0.0)
    assert s.history == [t1[b] + n1[b] + t2[b] + n2[b] for b in range(2)] and s.cached == [109, 57]
    s.truncate(len1)
    assert s.history == [t1[b] + n1[b] for b in range(2)] and s.cache.lens.tolist() == [79, 14]
    assert s.generate(t2, NEW, temperature=0.0) == n2, "the rewound session did not reproduce turn 2"
    # an eos inside a turn: the row is cut after it, and only the cut tokens stay cached
    s.truncate(len1)
    eos = n2[0][3]
    n3 = s.generate(t2, NEW, temperature=0.0, eos_token=eos)
    cut = n2[0][:n2[0].index(eos) + 1]
    assert n3[0] == cut and s.cached[0] == 80 + 20 + len(cut) and s.cache.lens.tolist() == s.cached
    # the refusals that need the cache: a full one, and another batch size
    with pytest.raises(ValueError, match="cached"):
        gpu.generate(_prompts(2, 150).cuda(), 30, cache=s.cache, resume=True)
    with pytest.raises(ValueError, match="resume=True continues a kept cache"):
        gpu.generate(_prompts(3, 5).cuda(), 3, cache=s.cache, resume=True)


def test_default_path_is_unchanged_around_resume(models):
    gpu, _ = models
    idx = _prompts(2, 5).cuda()
    cache = _cache(gpu, 2)
    a = gpu.generate(idx, NEW, temperature=0.0, return_logits=True, cache=cache)
    gpu.generate(_prompts(2, 40).cuda(), 5, temperature=0.0, cache=cache, resume=True)
    assert cache.lens.tolist() == [5 + NEW - 1 + 40 + 4] * 2
    b = gpu.generate(idx, NEW, temperature=0.0, return_logits=True, cache=cache)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = gpu.generate(idx, NEW, temperature=0.0, return_logits=True)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
