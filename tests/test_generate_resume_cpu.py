"""generate(resume=True) and generation.Session without a GPU: the refusals of ``resume`` (after every existing one), the
CPU Session against ``generate`` on the concatenated history, its history and eos accounting, and ``tools/generate.py
--chunk``."""
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(0)
    return build_gpt2("gpt2_tiny", block_size=256).float().eval()


def _toks(n, seed):
    return torch.randint(0, 512, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def test_resume_refusals(model):
    idx = torch.tensor([_toks(5, 1), _toks(5, 2)])
    with pytest.raises(ValueError, match="resume=True continues a kept cache"):
        model.generate(idx, 3, resume=True)
    with pytest.raises(ValueError, match="B = 2, got one of B = 3"):
        model.generate(idx, 3, resume=True, cache=SimpleNamespace(B=3))
    with pytest.raises(ValueError, match="Session"):
        model.generate(idx, 3, resume=True, cache=SimpleNamespace(B=2))
    # the existing refusals come first and keep their text
    with pytest.raises(ValueError, match="temperature must be >= 0"):
        model.generate(idx, 3, resume=True, temperature=-1.0)
    with pytest.raises(ValueError, match="block size"):
        model.generate(idx, 252, resume=True)
    with pytest.raises(ValueError, match="max_new_tokens must be >= 0"):
        model.generate(idx, -1, resume=True)
    # and the default is the call as it was
    assert torch.equal(model.generate(idx, 3, temperature=0.0), model.generate(idx, 3, temperature=0.0, resume=False))


def test_session_on_the_cpu_is_generate_on_the_concatenated_history(model):
    s = model.session(2, 256)
    assert s.cache is None and s.history == [[], []]
    t1 = [_toks(5, 3), _toks(9, 4)]
    n1 = s.generate(t1, 6, temperature=0.0)
    P = 9
    idx = torch.tensor([t1[0] + [0] * 4, t1[1]])
    want1 = model.generate(idx, 6, temperature=0.0, prompt_lens=[5, 9])[:, P:]
    assert torch.equal(torch.tensor(n1), want1)
    assert s.history == [t1[0] + n1[0], t1[1] + n1[1]] and s.cached == [0, 0]
    t2 = [_toks(7, 5), _toks(2, 6)]
    n2 = s.generate(t2, 4, temperature=0.0)
    h = [t1[0] + n1[0] + t2[0], t1[1] + n1[1] + t2[1]]
    P = max(len(r) for r in h)
    idx = torch.tensor([r + [0] * (P - len(r)) for r in h])
    want2 = model.generate(idx, 4, temperature=0.0, prompt_lens=[len(r) for r in h])[:, P:]
    assert torch.equal(torch.tensor(n2), want2)
    assert s.history == [h[0] + n2[0], h[1] + n2[1]]
    # the device sampler's reference goes through as well
    s2 = model.session(1, 64)
    a = s2.generate([_toks(4, 7)], 5, temperature=0.8, top_k=50, top_p=0.9, sampler="device", seed=11)
    b = model.generate(torch.tensor([_toks(4, 7)]), 5, temperature=0.8, top_k=50, top_p=0.9, sampler="device", seed=11)
    assert a == b[:, 4:].tolist()


def test_session_history_and_eos(model):
    turn = [_toks(6, 8), _toks(6, 9)]
    plain = model.session(2, 64).generate(turn, 8, temperature=0.0)
    eos = plain[0][2]

    def cut(n):
        return n[:n.index(eos) + 1] if eos in n else n
    s = model.session(2, 64)
    new = s.generate(turn, 8, temperature=0.0, eos_token=eos)
    assert new == [cut(plain[0]), cut(plain[1])] and new[0][-1] == eos and len(new[0]) <= 3
    assert s.history == [turn[0] + new[0], turn[1] + new[1]]
    # an empty turn is fine where there is history to run; max_new_tokens = 0 only appends
    assert s.generate([[], [5]], 0) == [[], []]
    assert s.history[0] == turn[0] + new[0] and s.history[1] == turn[1] + new[1] + [5]
    s.truncate(6)
    assert s.history == turn and s.cached == [0, 0]
    s.truncate([3, 6])
    assert s.history == [turn[0][:3], turn[1]]
    with pytest.raises(ValueError, match="2 turns"):
        s.generate([[1]], 2)
    with pytest.raises(ValueError, match="max_len"):
        s.generate([[1], [2]], 64)
    with pytest.raises(ValueError, match="session's own"):
        s.generate([[1], [2]], 2, resume=False)
    with pytest.raises(ValueError, match="every row needs a token"):
        model.session(1, 64).generate([[]], 2)
    with pytest.raises(ValueError, match="max_len"):
        model.session(1, 257)


def test_generate_tool_chunk_on_the_cpu(capsys):
    spec = importlib.util.spec_from_file_location("pdnn_generate_tool_c", os.path.join(ROOT, "tools", "generate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--network", "gpt2_tiny", "--random-init", "--prompt-ids", "9,8,7,6,5,4,3", "--max-new-tokens", "5",
            "--temperature", "0", "--device", "cpu"]
    a = tool.main(base)
    b = tool.main(base + ["--chunk", "3"])
    assert torch.equal(a, b) and a.shape == (1, 12)
    assert "in one piece" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tool.main(base + ["--chunk", "0"])
