"""tools/generate.py on the CPU: argument handling, and a round trip through a gpt2_tiny checkpoint."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("pdnn_generate_tool", os.path.join(ROOT, "tools", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_prompt_parsing(tool, tmp_path):
    assert tool.parse_prompt("1,2,3").tolist() == [[1, 2, 3]]
    assert tool.parse_prompt(" 7 , 8,").tolist() == [[7, 8]]
    np.save(tmp_path / "v.npy", np.array([4, 5, 6], dtype=np.int32))
    np.save(tmp_path / "m.npy", np.array([[1, 2], [3, 4]], dtype=np.int64))
    np.save(tmp_path / "f.npy", np.array([1.5, 2.0]))
    assert tool.parse_prompt(str(tmp_path / "v.npy")).tolist() == [[4, 5, 6]]
    assert tool.parse_prompt(str(tmp_path / "m.npy")).tolist() == [[1, 2], [3, 4]]
    for bad in ("1,x,3", "", str(tmp_path / "f.npy")):
        with pytest.raises(ValueError):
            tool.parse_prompt(bad)


def test_arguments(tool, capsys):
    for argv in (["--prompt-ids", "1,2"],                                                   # neither source
                 ["--random-init", "--checkpoint", "x.pt", "--prompt-ids", "1"],            # both
                 ["--random-init"]):                                                        # no prompt
        with pytest.raises(SystemExit):
            tool.main(argv)
    capsys.readouterr()
    base = ["--network", "gpt2_tiny", "--random-init", "--device", "cpu"]
    for argv, msg in ((["--network", "resnet50", "--random-init", "--prompt-ids", "1"], "expected one of"),
                      (base + ["--prompt-ids", "1,999"], "token ids"),
                      (base + ["--prompt-ids", "1,2", "--max-new-tokens", "127"], "block size"),
                      (base + ["--prompt-ids", "nope.npy"], "nope.npy")):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert msg in str(e.value)


def test_checkpoint_round_trip(tool, tmp_path, capsys):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    from pytorch_distributed_nn_amd.utils.observability import save_checkpoint
    torch.manual_seed(5)
    m = build_gpt2("gpt2_tiny")
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(4.0)
    path = save_checkpoint(str(tmp_path / "ck.pt"), m, arch="gpt2_tiny", step=3)
    want = m.generate(torch.tensor([[9, 8, 7, 6]]), 10, temperature=0.0)
    out = tool.main(["--network", "gpt2_tiny", "--checkpoint", path, "--prompt-ids", "9,8,7,6", "--max-new-tokens", "10",
                     "--temperature", "0", "--device", "cpu"])
    assert torch.equal(out, want)
    printed = capsys.readouterr().out.strip().splitlines()
    assert printed == [",".join(map(str, want[0].tolist()))]
    # a random init is another model; seeded sampling repeats
    a = tool.main(["--network", "gpt2_tiny", "--random-init", "--prompt-ids", "9,8,7,6", "--max-new-tokens", "10",
                   "--top-k", "8", "--seed", "3", "--device", "cpu"])
    b = tool.main(["--network", "gpt2_tiny", "--random-init", "--prompt-ids", "9,8,7,6", "--max-new-tokens", "10",
                   "--top-k", "8", "--seed", "3", "--device", "cpu"])
    assert torch.equal(a, b) and a.shape == (1, 14)
