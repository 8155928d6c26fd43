"""generate(kv_cache="fp8") on the CPU: the refusals, the stored rows of the reference, and that the option takes effect."""
import pytest
import torch

from pytorch_distributed_nn_amd.generation import Reference
from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
from pytorch_distributed_nn_amd.ops.quant import dequantize_rows, quantize_rows_reference


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_gpt2("gpt2_tiny", block_size=64).float().eval()


IDX = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(4))


def test_bad_values_and_a_contradicting_cache_are_refused(model):
    class Cache:        # what check_args reads of an ops.transformer.KVCache
        B, dtype = 2, "bf16"
    with pytest.raises(ValueError, match="kv_cache must be"):
        model.generate(IDX, 2, kv_cache="fp16")
    with pytest.raises(ValueError, match="kv_cache='fp8' with a cache= of dtype 'bf16'"):
        model.generate(IDX, 2, kv_cache="fp8", cache=Cache())
    with pytest.raises(ValueError, match="kv_cache"):
        model.session(2, 32, kv_cache="e5m2")


def test_every_visible_row_of_the_reference_cache_is_its_own_round_trip(model):
    ref = Reference(model, 2, 16, kv="fp8")
    with torch.no_grad():
        ref.prefill(IDX, torch.tensor([5, 9]))
        for t in (IDX[:, 0], IDX[:, 1]):
            ref.step(t)
    for c in ref.ks + ref.vs:
        for b, n in enumerate(ref.lens.tolist()):
            rows = c[b, :, :n].reshape(-1, c.shape[-1])
            assert n in (7, 11) and torch.equal(rows, dequantize_rows(*quantize_rows_reference(rows), dtype=rows.dtype))


def test_generate_runs_and_differs_from_the_default(model):
    kw = dict(temperature=0.0, return_logits=True, prompt_lens=[5, 9])
    (seq, lg), (_, lg16) = model.generate(IDX, 4, kv_cache="fp8", **kw), model.generate(IDX, 4, **kw)
    assert seq.shape == (2, 13) and torch.equal(lg[:, 0], lg16[:, 0]) and not torch.equal(lg[:, 1:], lg16[:, 1:])
    spec = model.generate(IDX, 4, kv_cache="fp8", decode_weights="fp8", sampler="device", seed=1, speculate=2,
                          prompt_lens=[5, 9])
    assert torch.equal(spec, model.generate(IDX, 4, kv_cache="fp8", decode_weights="fp8", sampler="device", seed=1,
                                            prompt_lens=[5, 9]))
