"""decode_weights="fp8" on the CPU: the argument's refusals, the row quantiser's definition (ops/quant.py) and the CPU
generate path, which is the definition the GPU path is tested against."""
import copy

import pytest
import torch

from pytorch_distributed_nn_amd.generation import Reference
from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
from pytorch_distributed_nn_amd.ops.quant import dequantize_rows, quantize_rows_reference

BF = torch.bfloat16


def test_quantize_rows_reference_by_hand_and_bound():
    w = torch.zeros(2, 16)
    w[0, :6] = torch.tensor([56.0, -28.0, 0.109375, 1.0625, 2.0 ** -13, -3.25])     # amax 56 = 0.875 * 2^6: e = -3
    w[1, :4] = torch.tensor([56.25, 1.0, -30.0, 0.0302734375])                      # the next bf16 above: e = -2
    q, inv = quantize_rows_reference(w.to(BF))
    assert inv.tolist() == [0.125, 0.25] and inv.dtype == torch.float32 and q.dtype == torch.uint8
    # w * 8 = 448, -224, 0.875, 8.5 (a tie: to even, 8), 2^-10 (a tie of 0 and the subnormal 2^-9: to 0), -26
    assert q[0, :6].tolist() == [0x7E, 0xF6, 0x36, 0x50, 0x00, 0xDD]
    # w * 4 = 225 (a tie of 224 and 240: to even, 224), 4, -120, 0.12109375 (-> 0.125)
    assert q[1, :4].tolist() == [0x76, 0x48, 0xEF, 0x20] and not q[:, 6:].any()
    w = (torch.randn(40, 144, generator=torch.Generator().manual_seed(1)) * torch.logspace(-30, 30, 40)[:, None]).to(BF)
    w[3] = 0.0
    q, inv = quantize_rows_reference(w)
    dq, wd, s = dequantize_rows(q, inv), w.double(), inv.double()[:, None]
    assert dq.dtype == BF and inv[3].item() == 1.0 and ((wd.abs() / s).amax(1) <= 448).all()
    assert ((dq.double() - wd).abs() <= torch.maximum(2.0 ** -4 * wd.abs(), 2.0 ** -10 * s)).all()


def test_cpu_generate_fp8_is_the_model_with_dq_in_the_step():
    torch.manual_seed(0)
    m = build_gpt2("gpt2_tiny", block_size=64).float()
    B, P, N, pl = 2, 7, 5, torch.tensor([4, 7], dtype=torch.int32)
    idx = torch.randint(0, 512, (B, P), generator=torch.Generator().manual_seed(2))
    for bad in ("int4", "FP8", None, 8):
        with pytest.raises(ValueError, match="decode_weights"):
            m.generate(idx, 2, decode_weights=bad)
    seq, lg = m.generate(idx, N, temperature=0.0, return_logits=True, prompt_lens=pl, decode_weights="fp8")
    assert not torch.equal(lg, m.generate(idx, N, temperature=0.0, return_logits=True, prompt_lens=pl)[1])
    dq = lambda w: dequantize_rows(*quantize_rows_reference(w.detach().to(BF)), dtype=w.dtype)     # noqa: E731
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
