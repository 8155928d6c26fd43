"""prefill_weights="decode" on the CPU, the definition the GPU path is tested against: the whole call is one ordinary
model, the one whose four block linears and LM head hold the dequantised weights.  The copy it is compared with keeps the
original embedding: its ``lm_head.weight`` is a new parameter holding dq(wte), which unties it from ``wte``, so the
embedding lookup still reads the original table, as the feature does; tokens and every step's logits must then be equal."""
import copy

import pytest
import torch

from pytorch_distributed_nn_amd.generation import DecodeWeights
from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_cpu_generate_is_one_model_with_dq(fmt):
    torch.manual_seed(0)
    m = build_gpt2("gpt2_tiny", block_size=64).float()
    idx = torch.randint(0, 512, (2, 7), generator=torch.Generator().manual_seed(2))
    kw = dict(temperature=0.0, return_logits=True, prompt_lens=torch.tensor([4, 7], dtype=torch.int32))
    dec = DecodeWeights(m, fmt)
    seq, lg = m.generate(idx, 5, decode_weights=fmt, prefill_weights="decode", **kw)
    seq2, lg2 = m.generate(idx, 5, decode_weights=dec, prefill_weights="decode", **kw)       # a snapshot is accepted
    assert torch.equal(seq, seq2) and torch.equal(lg, lg2)
    assert not torch.equal(lg, m.generate(idx, 5, decode_weights=fmt, prefill_weights="bf16", **kw)[1])
    m2 = copy.deepcopy(m)
    m2.lm_head.weight = torch.nn.Parameter(dec.dequantize(dec.wte, torch.float32))
    for blk, stored in zip(m2.transformer.h, dec.blocks):
        for lin, w in zip((blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj), stored):
            lin.weight.data = dec.dequantize(w, torch.float32)
    seq_ref, lg_ref = m2.generate(idx, 5, **kw)
    assert torch.equal(seq, seq_ref) and torch.equal(lg, lg_ref)


def test_refusals():
    m = build_gpt2("gpt2_tiny", block_size=64).float()
    idx = torch.zeros(1, 4, dtype=torch.int64)
    for kw in (dict(prefill_weights="decode"), dict(prefill_weights="decode", decode_weights="bf16"),
               dict(prefill_weights="fp8", decode_weights="fp8"), dict(prefill_weights=None)):
        with pytest.raises(ValueError, match="prefill_weights"):
            m.generate(idx, 2, **kw)
        with pytest.raises(ValueError, match="prefill_weights"):
            m.session(1, 16, **kw)
