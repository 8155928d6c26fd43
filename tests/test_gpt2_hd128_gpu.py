"""GPT-2 at head dim 128 (n_embd = 256, 2 heads) trains through the flash kernels of csrc/kernels/attention_hd128.hip:
loss and every gradient against the fp32 CPU model, at the tolerances of test_transformer_gpu.py's engine test; the
document mask and attention dropout, which those kernels do not have, are refused."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
B, T = 2, 128


def _model(**kw):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(0)
    return build_gpt2("gpt2_tiny", n_embd=256, n_head=2, block_size=128, **kw)


def _batch(m):
    g = torch.Generator().manual_seed(5)
    return (torch.randint(8, m.config.vocab_size, (B, T), generator=g) for _ in range(2))


def test_gpt2_head_dim_128_matches_reference():
    from pytorch_distributed_nn_amd.ops import transformer as TX
    assert TX.use_flash(128, 256, 2)
    m = _model().cuda()
    ref = copy.deepcopy(m).float().cpu()
    idx, tgt = _batch(m)
    loss, lref = m(idx.cuda(), tgt.cuda()), ref(idx, tgt)
    assert abs(loss.item() - lref.item()) / lref.item() < 0.01
    loss.backward()
    lref.backward()
    for (n, p), (_, pr) in zip(m.named_parameters(), ref.named_parameters()):
        a, b = p.grad.cpu().float().flatten(), pr.grad.flatten()
        assert F.cosine_similarity(a, b, dim=0).item() > 0.99, n
        assert ((a - b).norm() / b.norm().clamp_min(1e-12)).item() < 0.1, n


@pytest.mark.parametrize("kw", [{"doc_mask_eot": 7}, {"attn_pdrop": 0.1}], ids=["doc", "dropout"])
def test_gpt2_head_dim_128_refuses_mask_and_dropout(kw):
    m = _model(**kw).cuda().train()
    idx, tgt = _batch(m)
    with pytest.raises(ValueError, match="head-dim-128 flash kernels have neither"):
        m(idx.cuda(), tgt.cuda())
