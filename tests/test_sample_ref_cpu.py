"""The token draw on the CPU: ops.sampling.sample_reference (torch, the kernel's documented meaning) against the numpy
reference of tests/sample_ref.py on every case, the properties of the definition itself, GPT2.generate(sampler="device")
on gpt2_tiny, and the new flags of tools/generate.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import sample_ref as R
from pytorch_distributed_nn_amd.ops.sampling import sample_reference, sample_row, uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_uniform_matches_the_numpy_generator():
    for seed, step, b in [(0, 0, 0), (20241020, 5, 3), (2 ** 63 - 1, 2 ** 40, 65535), (7, 1, 2 ** 31)]:
        assert uniform(seed, step, b) == R.uniform(seed, step, b)
        assert 0.0 <= uniform(seed, step, b) < 1.0


def test_case_list_covers_every_listed_value():
    cs = R.cases()
    kind = lambda k, V: k if k in (None, 1, 2, 50) and k != V else "V" if k == V else "V+5" if k == V + 5 else "?"   # noqa: E731
    assert 200 <= len(cs) <= 400
    assert {c[0] for c in cs} == set(R.FAMILIES) and {c[2] for c in cs} == set(R.VS) and {c[1] for c in cs} == set(R.BS)
    assert {c[4] for c in cs} == set(R.PS) and {c[5] for c in cs} == set(R.TS)
    assert {kind(c[3], c[2]) for c in cs} == {None, 1, 2, 50, "V", "V+5"}
    for V in R.VS:                                                    # and every k kind and p at every vocabulary size
        mine = [c for c in cs if c[2] == V]
        assert {c[4] for c in mine} == set(R.PS) and {c[3] for c in mine} == set(R.ks_of(V))
    assert sum(1 for c in cs if c[3] == 1 and c[5] > 0) >= 20        # the exact k = 1 branch runs


def test_sample_reference_agrees_with_numpy_on_every_case():
    """thresholds and set sizes equal (either neighbour on ambiguous rows), every token accepted under the CDF rule; at
    most 5 % of the top-p rows are ambiguous"""
    top_p_rows = amb_rows = 0
    worst = 0.0
    for fam, B, V, k, p, T, seed in R.cases():
        x = R.make(fam, B, V, seed)
        tok, thr, nkeep = sample_reference(torch.from_numpy(x), T, k, p, state=R.STATE)
        for b in range(B):
            r = R.analyse(x[b], T, k, p)
            top_p_rows += r["top_p"]
            amb_rows += r["ambiguous"]
            u = R.uniform(*R.STATE, b)
            worst = max(worst, R.check_row(x[b], T, k, p, u, int(tok[b]), float(thr[b]), int(nkeep[b])))
    print(f"worst distance / EPS {worst:.4f}; ambiguous {amb_rows} of {top_p_rows} top-p rows")
    assert top_p_rows > 100 and amb_rows <= 0.05 * top_p_rows


def test_top_k_set_is_the_mask_of_the_torch_sampler(monkeypatch):
    """the set GPT2._sample hands to torch.multinomial (probability > 0) is the definition's kept set"""
    from pytorch_distributed_nn_amd.models.gpt2 import GPT2
    seen = []
    real = torch.multinomial
    monkeypatch.setattr(torch, "multinomial", lambda pr, *a, **kw: (seen.append(pr.clone()), real(pr, *a, **kw))[1])
    for fam, V, k in [("gauss1", 1000, 50), ("bf16_ties", 4099, 50), ("bf16_ties", 64, 2), ("equal", 64, 2)]:
        x = torch.from_numpy(R.make(fam, 3, V, 5))
        GPT2._sample(x, 1.0, k, torch.Generator().manual_seed(0))
        mask = seen[-1] > 0
        _, thr, nkeep = sample_reference(x, 1.0, k, None, state=(1, 0))
        assert torch.equal(mask, x >= thr[:, None]) and torch.equal(nkeep.long(), mask.sum(1))
        assert int(nkeep.min()) >= k
    assert len(seen) == 4


def test_selection_frequency_over_equally_spaced_u():
    """p = None: the tokens sample_reference's row draw returns over 2^16 equally spaced u; every token's frequency equals
    its probability (from the numpy reference) within 2^-16 + EPS"""
    x = R.make("gauss1", 1, 40, 9)
    n = 2 ** 16
    for T, k in [(0.7, 20), (1.0, None), (4.0, 7)]:
        r = R.analyse(x[0], T, k, None)
        _, C = R.final_set(r, r["thrs"][0])
        prob = np.diff(np.r_[0.0, C])
        us = torch.arange(n, dtype=torch.float64) / n
        tok, _, _ = sample_row(torch.from_numpy(x[0]), T, k, None, us)
        counts = np.bincount(tok.numpy(), minlength=40)
        assert counts.sum() == n and np.abs(counts / n - prob).max() <= 2.0 ** -16 + R.EPS
        one, _, _ = sample_reference(torch.from_numpy(x), T, k, None, u=[float(us[12345])])      # the same path as a single draw
        assert int(one) == int(tok[12345])


def test_hash_is_a_uniform_source():
    """a 16-token row over 4096 streams x 4 steps: Pearson's chi-square against the exact probabilities stays below the
    1 - 1e-6 quantile for 15 degrees of freedom (about 56)"""
    x = R.make("gauss1", 1, 16, 3)
    r = R.analyse(x[0], 1.0, None, None)
    _, C = R.final_set(r, R.NINF)
    prob = np.diff(np.r_[0.0, C])
    us = np.array([R.uniform(77, s, b) for s in range(4) for b in range(4096)])
    counts = np.bincount(np.searchsorted(C, us, side="right").clip(max=15), minlength=16)
    chi2 = ((counts - us.size * prob) ** 2 / (us.size * prob)).sum()
    print(f"chi-square {chi2:.2f}")
    assert chi2 < 56.0
    row = torch.from_numpy(x).expand(8, 16).contiguous()              # and sample_reference uses stream = row
    tok, _, _ = sample_reference(row, 1.0, None, None, state=(77, 2))
    assert tok.tolist() == np.searchsorted(C, us[2 * 4096:2 * 4096 + 8], side="right").tolist()


def test_eos_rows_and_guards():
    x = torch.from_numpy(R.make("gauss1", 4, 64, 1))
    fin = torch.tensor([0, 1, 0, 1], dtype=torch.uint8)
    tok, thr, nkeep = sample_reference(x, 0.0, None, None, state=(1, 0), eos_token=int(x[0].argmax()), finished=fin)
    assert tok[1] == tok[3] == tok[0] and fin.tolist() == [1, 1, int(x[2].argmax() == x[0].argmax()), 1]
    assert nkeep.tolist()[1] == 0
    for kw in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=0), dict(top_p=0.0), dict(top_p=-0.5)):
        with pytest.raises(ValueError):
            sample_reference(x, **{"temperature": 1.0, **kw}, state=(1, 0))
    with pytest.raises(ValueError):
        sample_reference(x)


# ------------------------------------------------------------------------------------------------ generate on the CPU
def _tiny():
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(0)
    return build_gpt2("gpt2_tiny", block_size=64).float().eval()


def _old_sample(logits, temperature, top_k, generator):
    """GPT2._sample before top_p existed"""
    if temperature == 0 or top_k == 1:
        return logits.argmax(-1)
    lg = logits / temperature
    if top_k is not None:
        kth = torch.topk(lg, min(int(top_k), lg.shape[-1]), dim=-1).values[:, -1:]
        lg = lg.masked_fill(lg < kth, float("-inf"))
    return torch.multinomial(torch.softmax(lg, -1), 1, generator=generator).squeeze(1)


def test_generate_device_sampler_on_cpu():
    m = _tiny()
    idx = torch.randint(0, 512, (3, 6), generator=torch.Generator().manual_seed(1))
    kw = dict(temperature=0.9, top_k=40, top_p=0.9, sampler="device")
    a, lg = m.generate(idx, 12, seed=5, return_logits=True, **kw)
    b = m.generate(idx, 12, seed=5, **kw)
    c = m.generate(idx, 12, seed=6, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c) and lg.shape == (3, 12, 512) and lg.dtype == torch.float32
    for i in range(12):                                                # every token is the definition's, at (seed, i, b)
        for bb in range(3):
            R.check_row(lg[bb, i].numpy(), 0.9, 40, 0.9, R.uniform(5, i, bb), int(a[bb, 6 + i]))
    eos = int(a[0, 8])
    e = m.generate(idx, 12, seed=5, eos_token=eos, **kw)
    assert torch.equal(e[0, 6:8], a[0, 6:8]) and bool((e[0, 8:] == eos).all())
    for bad in (dict(seed=None), dict(seed=1, generator=torch.Generator())):
        with pytest.raises(ValueError):
            m.generate(idx, 2, **{**kw, **bad})
    with pytest.raises(ValueError):
        m.generate(idx, 2, sampler="host")
    with pytest.raises(ValueError):
        m.generate(idx, 2, top_p=0.0)


def test_torch_sampler_is_unchanged_without_top_p_and_filters_with_it():
    m = _tiny()
    idx = torch.randint(0, 512, (2, 5), generator=torch.Generator().manual_seed(2))
    out, lg = m.generate(idx, 8, temperature=0.8, top_k=30, generator=torch.Generator().manual_seed(3), return_logits=True)
    g = torch.Generator().manual_seed(3)
    want = torch.stack([_old_sample(lg[:, i], 0.8, 30, g) for i in range(8)], 1)
    assert torch.equal(out[:, 5:], want)
    # top_p: every token lies in the nucleus of its step's logits
    out, lg = m.generate(idx, 8, temperature=1.0, top_p=0.3, generator=torch.Generator().manual_seed(3), return_logits=True)
    for i in range(8):
        for b in range(2):
            pr = torch.softmax(lg[b, i].double(), -1)
            sp, si = pr.sort(descending=True)
            n = int((sp.cumsum(0) - sp < 0.3).sum())
            assert int(out[b, 5 + i]) in si[:n + 1].tolist()


def test_tool_flags_parse_and_run():
    spec = importlib.util.spec_from_file_location("pdnn_generate_tool_s", os.path.join(ROOT, "tools", "generate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--network", "gpt2_tiny", "--random-init", "--prompt-ids", "1,2,3", "--max-new-tokens", "6", "--device", "cpu",
            "--top-k", "20", "--top-p", "0.8"]
    a = tool.main(base + ["--sampler", "device", "--seed", "4"])
    b = tool.main(base + ["--sampler", "device", "--seed", "4"])
    assert a.shape == (1, 9) and torch.equal(a, b)
    assert tool.main(base).shape == (1, 9)
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(base + ["--sampler", "host"])
