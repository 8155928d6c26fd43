"""generation.Replay on a unit that counts its own executions (``buf.add_(1)`` on a one-element tensor): eager calls, the
warm-up / capture / replay sequence of ``graph=True`` (a capture executes nothing, so it must not count), one CUDAGraph
per helper; and ops.transformer.block_step's refusal of a row count or an S its cache was not built for, before any
launch."""
import pytest
import torch

from pytorch_distributed_nn_amd.generation import Replay

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_five_calls_run_the_unit_five_times(graph, monkeypatch):
    made = []
    real = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: (made.append(1), real(*a, **k))[1])
    buf = torch.zeros(1, device="cuda")
    run = Replay(lambda: buf.add_(1), graph)
    for n in range(1, 6):
        run()
        assert buf.item() == n
    assert len(made) == (1 if graph else 0)


def test_block_step_refuses_rows_its_cache_cannot_take(monkeypatch):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    from pytorch_distributed_nn_amd.ops import transformer as TX
    m = build_gpt2("gpt2_tiny").cuda()
    c = m.config
    B, S = 2, 4
    cache = TX.KVCache(m, B, 128, "cuda", S=S)
    params, shadows = m.transformer.h[0].fused_params()
    launches = []
    real = TX.K.call                                # every wrapper of ops.kernels launches through it
    monkeypatch.setattr(TX.K, "call", lambda *a, **k: (launches.append(a[0]), real(*a, **k))[1])

    def step(rows, conf_S, S_):
        x = torch.zeros(rows, c.n_embd, device="cuda", dtype=torch.bfloat16)
        return TX.block_step(x, (B, conf_S, c.n_head, c.eps), shadows, params, cache, 0, S_)
    with pytest.raises(ValueError, match=r"16 rows for B = 2, S = 8 \(cache S = 4"):       # S > cache.S
        step(B * 8, 8, 8)
    with pytest.raises(ValueError, match=r"6 rows for B = 2, S = 4"):                      # rows != B * S
        step(6, S, S)
    with pytest.raises(ValueError, match=r"66 rows for B = 33, S = 2 .*at most 64 rows"):  # more than the skinny GEMM takes
        x = torch.zeros(66, c.n_embd, device="cuda", dtype=torch.bfloat16)
        TX.block_step(x, (33, 2, c.n_head, c.eps), shadows, params, cache, 0, 2)
    assert launches == []
    assert step(B * S, S, S).shape == (B * S, c.n_embd) and launches       # and the rows it was built for go through
