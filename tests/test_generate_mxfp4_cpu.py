"""decode_weights="mxfp4" on the CPU: the block quantiser's definition (ops/quant.py) by hand, its error bound, and the
CPU generate path, which is the definition the GPU path is tested against."""
import copy

import pytest
import torch

from pytorch_distributed_nn_amd.generation import Reference
from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
from pytorch_distributed_nn_amd.ops.quant import dequantize_blocks, quantize_blocks_reference

BF = torch.bfloat16


def test_quantize_blocks_reference_by_hand_and_bound():
    w = torch.zeros(2, 96)
    w[0, :4] = torch.tensor([0.75, -0.375, 0.0625, -0.0])              # amax 0.75 = 6 * 2^-3: e = -3; w * 8 = 6, -3, 0.5, -0
    w[0, 32:36] = torch.tensor([0.75390625, 0.375, -1e-3, 0.5])        # the next bf16 above: e = -2; w * 4 = 3.02, 1.5, ~0, 2
    # block 2 of row 0 stays zero: e = 0.  Row 1, amax 6 (e = 0): the seven ties, then values next to them
    w[1, :12] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -3.5, 0.251, 4.99])
    q, sc = quantize_blocks_reference(w.to(BF))
    assert q.dtype == sc.dtype == torch.uint8 and q.shape == (2, 48) and sc.shape == (2, 3)
    assert sc.tolist() == [[124, 125, 127], [127, 127, 127]]
    assert q[0, :2].tolist() == [0xD7, 0x81]                           # codes 7, -5 | 1, -0: element 2 i is the low nibble
    assert q[0, 16:18].tolist() == [0x35, 0x48] and not q[0, 2:16].any() and not q[0, 18:].any()
    # 6 -> 7 | 0.25 -> 0, 0.75 -> 2 (1.0), 1.25 -> 2, 1.75 -> 4 (2.0), 2.5 -> 4, 3.5 -> 6 (4.0), 5 -> 6 | -0.25 -> -0, -3.5 -> -4
    assert q[1, :6].tolist() == [0x07, 0x22, 0x44, 0x66, 0xE8, 0x61]
    dq = dequantize_blocks(q, sc)
    assert dq.dtype == BF and dq[0, :4].tolist() == [0.75, -0.375, 0.0625, 0.0] and dq[0, 32:36].tolist() == [0.75, 0.375, 0.0, 0.5]
    assert dq[1, :12].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 0.0, -4.0, 0.5, 4.0]
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(40, 160, generator=g) * torch.logspace(-25, 25, 40)[:, None] * torch.logspace(-2, 2, 160)[None, :]).to(BF)
    w[3] = 0.0
    q, sc = quantize_blocks_reference(w)
    wd, s = w.double(), torch.ldexp(torch.ones(40, 5, dtype=torch.float64), sc.int() - 127).repeat_interleave(32, 1)
    assert (sc[3] == 127).all() and (wd.abs() / s <= 6).all() and ((wd.abs() / s).view(40, 5, 32).amax(2)[sc != 127] > 3).all()
    assert ((dequantize_blocks(q, sc).double() - wd).abs() <= torch.maximum(0.25 * wd.abs(), 0.25 * s)).all()


def test_cpu_generate_mxfp4_is_the_model_with_dq_in_the_step():
    torch.manual_seed(0)
    m = build_gpt2("gpt2_tiny", block_size=64).float()
    B, P, N, pl = 2, 7, 5, torch.tensor([4, 7], dtype=torch.int32)
    idx = torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(2))
    with pytest.raises(ValueError, match="decode_fused"):
        m.generate(idx, 2, decode_weights="mxfp4", decode_fused=True)
    kw = dict(temperature=0.0, return_logits=True, prompt_lens=pl)
    seq, lg = m.generate(idx, N, decode_weights="mxfp4", **kw)
    assert not torch.equal(lg, m.generate(idx, N, **kw)[1]) and not torch.equal(lg, m.generate(idx, N, decode_weights="fp8", **kw)[1])
    dq = lambda w: dequantize_blocks(*quantize_blocks_reference(w.detach().to(BF)), dtype=w.dtype)     # noqa: E731
    m2 = copy.deepcopy(m)                                        # the five weight kinds replaced; the embedding keeps wte
    m2.lm_head.weight = torch.nn.Parameter(dq(m.transformer.wte.weight))
    for blk in m2.transformer.h:
        for lin in (blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj):
            lin.weight.data = dq(lin.weight)
    with torch.no_grad():
        r = Reference(m, B, P + N)                               # the prefill on the original weights, its logits on dq;
        r.head = m2.lm_head.weight
        logits = r.prefill(idx, pl)
        r.model, r.tr = m2, m2.transformer                       # then every step on the copy
        for i in range(N):
            assert torch.equal(lg[:, i], logits) and torch.equal(seq[:, P + i], logits.argmax(-1)), f"step {i}"
            logits = r.step(seq[:, P + i])
