"""GPT-2 dropout through the model layers on the CPU (fp32 reference path): the config fields, the (seed, step) state,
training / eval behaviour and the CLI flags."""
import pytest
import torch

from pytorch_distributed_nn_amd.models.gpt2 import GPT2Config, build_gpt2
from pytorch_distributed_nn_amd.ops import transformer as TX


def _tiny(seed=0, **kw):
    torch.manual_seed(seed)
    return build_gpt2("gpt2_tiny", **kw)


def _batch(B=2, T=32):
    g = torch.Generator().manual_seed(1)
    return torch.randint(0, 512, (B, T), generator=g), torch.randint(0, 512, (B, T), generator=g)


def test_config_defaults_are_off():
    c = GPT2Config()
    assert (c.embd_pdrop, c.attn_pdrop, c.resid_pdrop) == (0.0, 0.0, 0.0)
    m = _tiny()
    assert m.dropout_rates() is None and "_pdnn_drop_state" not in m.__dict__
    idx, tgt = _batch()
    m(idx, tgt)
    assert "_pdnn_drop_state" not in m.__dict__                 # nothing new runs with the rates at 0


def test_training_steps_differ_and_are_reproducible_from_the_state():
    idx, tgt = _batch()
    m = _tiny(embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1)
    m.set_dropout_state(17, 0)
    a, b = m(idx, tgt), m(idx, tgt)
    assert m.dropout_state("cpu").tolist() == [17, 2]           # one step per training forward
    assert a.item() != b.item()
    m.set_dropout_state(17, 0)
    a2 = m(idx, tgt)
    m.set_dropout_state(17, 1)
    b2 = m(idx, tgt)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    m.set_dropout_state(18, 0)
    assert m(idx, tgt).item() != a.item()
    # each rate alone changes the loss, and the gradient reaches every parameter
    plain = _tiny()
    plain.train()
    base = plain(idx, tgt)
    for name in ("embd_pdrop", "attn_pdrop", "resid_pdrop"):
        one = _tiny(**{name: 0.5})
        one.set_dropout_state(3, 0)
        assert one(idx, tgt).item() != base.item(), name
    a2.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_state_is_not_a_buffer_and_seeds_from_torch():
    m = _tiny(resid_pdrop=0.1)
    idx, tgt = _batch()
    torch.manual_seed(1234)
    m(idx, tgt)
    assert m.dropout_state("cpu").tolist() == [1234, 1]
    assert not any("drop" in k for k in m.state_dict()) and not any("drop" in n for n, _ in m.named_buffers())


def test_eval_and_no_grad_run_the_rate_zero_model():
    idx, tgt = _batch()
    m, plain = _tiny(embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1), _tiny()
    m.set_dropout_state(5, 0)
    with torch.no_grad():
        assert torch.equal(m(idx, tgt), plain(idx, tgt))        # training mode, grad mode off
    m.eval(), plain.eval()
    assert torch.equal(m(idx, tgt), plain(idx, tgt)) and torch.equal(m(idx), plain(idx))
    assert m.dropout_state("cpu").tolist() == [5, 0]            # no step was drawn


def test_reference_path_applies_the_generators_masks():
    """one layer, resid only: x1 = x + keep1 attn(..) s, by hand from the exported bits"""
    idx, _ = _batch(1, 8)
    m = _tiny(n_layer=1, resid_pdrop=0.5)
    m.set_dropout_state(9, 4)
    blk = m.transformer.h[0]
    x = m.transformer.wte(idx) + m.transformer.wpe(torch.arange(8))
    k1, k2 = (TX.dropout_keep_reference((9, 4), s, 0.5, rows=(8, 128)).float().view(1, 8, 128) * 2.0 for s in (1, 2))
    x1 = x + blk.attn(blk.ln_1(x)) * k1
    want = m.lm_head(m.transformer.ln_f(x1 + blk.mlp(blk.ln_2(x1)) * k2))
    got = m._forward_reference(idx, None, None, ((0.0, 0.0, 0.5), torch.tensor([9, 4])))
    assert torch.allclose(got, want, atol=1e-6)


def test_bad_rates_are_refused():
    idx, tgt = _batch()
    for kw in (dict(attn_pdrop=1.0), dict(resid_pdrop=-0.1), dict(embd_pdrop=float("nan"))):
        with pytest.raises(ValueError, match="pdrop"):
            _tiny(**kw)(idx, tgt)


def test_cli_flags():
    from pytorch_distributed_nn_amd.cli import dropout_rates, parse_args
    a = parse_args(["--network", "gpt2_tiny", "--dropout", "0.1"])
    assert dropout_rates(a) == (0.1, 0.1, 0.1)
    a = parse_args(["--network", "gpt2_tiny", "--dropout", "0.1", "--attn-pdrop", "0", "--embd-pdrop", "0.2"])
    assert dropout_rates(a) == (0.2, 0.0, 0.1)
    assert dropout_rates(parse_args(["--network", "gpt2_tiny", "--resid-pdrop", "0.3"])) == (0.0, 0.0, 0.3)
    assert dropout_rates(parse_args(["--network", "gpt2_tiny"])) == (0.0, 0.0, 0.0)
    with pytest.raises(SystemExit, match="dropout"):
        parse_args(["--network", "LeNet", "--dropout", "0.1"])
    with pytest.raises(SystemExit, match="dropout"):
        parse_args(["--network", "gpt2_tiny", "--dropout", "1.0"])
    with pytest.raises(SystemExit, match="attn-pdrop"):
        parse_args(["--network", "gpt2_tiny", "--attn-pdrop", "-0.5"])


def test_cli_yaml(tmp_path):
    from pytorch_distributed_nn_amd.cli import dropout_rates, parse_args
    f = tmp_path / "c.yaml"
    f.write_text("network: gpt2_tiny\ndropout: 0.1\nresid-pdrop: 0.2\n")
    assert dropout_rates(parse_args(["--config", str(f)])) == (0.1, 0.1, 0.2)
    assert dropout_rates(parse_args(["--config", str(f), "--dropout", "0.3"])) == (0.3, 0.3, 0.2)
