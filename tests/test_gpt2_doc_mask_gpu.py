"""GPT-2 with packed-document attention on the GPU (DOC flash kernels in every block, bounds from one kernel per
forward) against the CPU fp32 reference with the equivalent boolean mask, at the tolerances test_transformer_gpu.py's
test_gpt2_tiny_loss_and_grads holds the unmasked model to; under flat-arena gradients with gpt2_side_wgrad on."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
EOT = 7


def cos(a, b):
    return F.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0).item()


def _tiny(seed=0, **kw):
    from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
    torch.manual_seed(seed)
    return build_gpt2("gpt2_tiny", **kw)


def _packed(B=4, T=128):
    """rows of 1 - 5 documents, one row without any EOT"""
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(8, 512, (B, T), generator=g)
    for b, ends in enumerate(((), (63,), (30, 64, 100), (10, 11, 70, 126))):
        idx[b, list(ends)] = EOT
    return idx, torch.randint(8, 512, (B, T), generator=g)


def test_gpt2_tiny_doc_mask_loss_and_grads():
    from pytorch_distributed_nn_amd import tuning
    from pytorch_distributed_nn_amd.optim import AdamW, flatten_module
    m = _tiny(doc_mask_eot=EOT).cuda()
    ref = copy.deepcopy(m).float().cpu()
    plain = _tiny()
    idx, tgt = _packed()
    old = tuning.set("gpt2_side_wgrad", 1)
    try:
        flatten_module(m)
        opt = AdamW(m.parameters(), lr=1e-3)
        opt.zero_grad()
        loss = m(idx.cuda(), tgt.cuda())
        lref = ref(idx, tgt)
        assert abs(loss.item() - lref.item()) / lref.item() < 0.01
        loss.backward()
        lref.backward()
        torch.cuda.synchronize()
        for (n, p), (_, pr) in zip(m.named_parameters(), ref.named_parameters()):
            assert cos(p.grad.cpu(), pr.grad) > 0.99, n
    finally:
        tuning.set("gpt2_side_wgrad", old)
    # the mask is what was run: the same rows without it give other logits after the first document
    with torch.no_grad():
        a = m(idx.cuda()).float().cpu()
        b = ref(idx)
        c = plain.float()(idx)
    assert (a[1, 64:] - b[1, 64:]).abs().max() < (a[1, 64:] - c[1, 64:]).abs().max()      # nearer the masked reference


def test_explicit_bounds_on_the_gpu_equal_the_derived_ones():
    from pytorch_distributed_nn_amd.ops import transformer as TX
    idx, tgt = _packed()
    masked, plain = _tiny(doc_mask_eot=EOT).cuda(), _tiny().cuda()
    ds, de = TX.doc_bounds_reference(idx, EOT)
    with torch.no_grad():
        a = masked(idx.cuda(), tgt.cuda())
        b = plain(idx.cuda(), tgt.cuda(), doc_bounds=(ds, de))
        c = plain(idx.cuda(), tgt.cuda())
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_unfused_chain_refuses_the_mask():
    idx, tgt = _packed()
    m = _tiny(doc_mask_eot=EOT, n_head=4).cuda()                # head dim 32: the unfused chain
    with pytest.raises(ValueError, match="document"):
        m(idx.cuda(), tgt.cuda())
    m = _tiny(doc_mask_eot=EOT).cuda()                          # T % 128 != 0
    with pytest.raises(ValueError, match="document"):
        m(idx[:, :96].cuda().contiguous(), tgt[:, :96].cuda().contiguous())
    m.config.doc_mask_eot = None                                # without the mask the chain still runs
    assert torch.isfinite(m(idx[:, :96].cuda().contiguous(), tgt[:, :96].cuda().contiguous())).item()
