"""Packed-document attention through the model layers on the CPU (fp32 reference path): GPT2Config.doc_mask_eot and
forward(doc_bounds=), the synthetic packed token generator and the CLI flag."""
import pytest
import torch

from pytorch_distributed_nn_amd.models.gpt2 import build_gpt2
from pytorch_distributed_nn_amd.ops import transformer as TX

EOT = 7


def _tiny(**kw):
    torch.manual_seed(0)
    return build_gpt2("gpt2_tiny", **kw).eval()


def _packed(B=2, T=128, ends=((40, 41, 90), (127,))):
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(8, 512, (B, T), generator=g)
    for b, e in enumerate(ends):
        idx[b, list(e)] = EOT
    return idx


def test_logits_of_a_document_ignore_earlier_documents():
    idx = _packed()
    other = idx.clone()
    other[0, :40] = torch.randint(8, 512, (40,), generator=torch.Generator().manual_seed(2))     # first document only
    masked, plain = _tiny(doc_mask_eot=EOT), _tiny()
    with torch.no_grad():
        a, b = masked(idx), masked(other)
        assert torch.equal(a[0, 41:], b[0, 41:]) and torch.equal(a[1], b[1])       # later documents: not a bit
        assert not torch.equal(a[0, :41], b[0, :41])
        a, b = plain(idx), plain(other)
        assert not torch.equal(a[0, 41:], b[0, 41:])                                # without the mask they do change
    assert torch.equal(plain.transformer.wte.weight, masked.transformer.wte.weight)


def test_explicit_bounds_equal_the_eot_derived_ones_and_win():
    idx = _packed()
    ds, de = TX.doc_bounds_reference(idx, EOT)
    assert ds[0, 40] == 0 and ds[0, 41] == 41 and ds[0, 42] == 42 and de[0, 41] == 42 and de[0, 91] == 128
    assert ds[1].eq(0).all() and de[1].eq(128).all()                                # EOT at T - 1: one document
    masked, plain = _tiny(doc_mask_eot=EOT), _tiny()
    tgt = idx.roll(-1, 1)
    with torch.no_grad():
        assert torch.equal(masked(idx), plain(idx, doc_bounds=(ds, de)))
        assert torch.equal(masked(idx, tgt), plain(idx, tgt, doc_bounds=(ds.long(), de.long())))
        one = (torch.zeros_like(ds), torch.full_like(de, 128))
        assert torch.equal(masked(idx, doc_bounds=one), plain(idx))                 # explicit bounds win over the config
    with pytest.raises(ValueError):
        plain(idx, doc_bounds=(ds[:, :64], de))
    vis = TX.doc_visible(ds)
    assert vis.shape == (2, 128, 128) and bool(vis[0, 41, 41]) and not bool(vis[0, 41, 40]) and not bool(vis[0, 41, 42])


def test_attention_reference_takes_a_mask():
    B, T, H = 2, 16, 2
    qkv = torch.randn(B * T, 3 * H * 8, generator=torch.Generator().manual_seed(3))
    i = torch.arange(T)
    causal = (i[None, :] <= i[:, None]).expand(B, T, T)
    assert torch.allclose(TX.attention_reference(qkv, B, T, H, mask=causal), TX.attention_reference(qkv, B, T, H), atol=1e-6)
    unit = torch.eye(T, dtype=torch.bool).expand(B, T, T)
    v = qkv.view(B, T, 3, H, 8)[:, :, 2].reshape(B * T, H * 8)
    assert torch.allclose(TX.attention_reference(qkv, B, T, H, mask=unit), v, atol=1e-6)


def test_synthetic_tokens_with_eot():
    from pytorch_distributed_nn_amd.data import SyntheticTokens
    a = SyntheticTokens(512, 128, 4, n_batches=2, seed=5, eot=EOT, mean_doc_len=16)
    b = SyntheticTokens(512, 128, 4, n_batches=2, seed=5, eot=EOT, mean_doc_len=16)
    c = SyntheticTokens(512, 128, 4, n_batches=2, seed=6, eot=EOT, mean_doc_len=16)
    for (xa, ya), (xb, yb) in zip(a.batches, b.batches):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
        assert torch.equal(xa[:, 1:], ya[:, :-1])
    assert not torch.equal(a.batches[0][0], c.batches[0][0])
    x = torch.cat([t[0] for t in a.batches])
    n = int((x == EOT).sum())
    assert 0.5 * x.numel() / 16 < n < 2.0 * x.numel() / 16                          # gaps of mean 16, no stray EOT
    e0 = SyntheticTokens(16, 64, 8, seed=1, eot=0, mean_doc_len=1)                  # every token ends a document
    assert bool((e0.batches[0][0] == 0).all())
    plain = SyntheticTokens(512, 128, 4, n_batches=1, seed=5)                       # the unpacked stream is unchanged
    g = torch.Generator().manual_seed(5)
    assert torch.equal(plain.batches[0][0], torch.randint(0, 512, (4, 129), generator=g)[:, :-1])
    with pytest.raises(ValueError):
        SyntheticTokens(512, 128, 4, eot=512)
    with pytest.raises(ValueError):
        SyntheticTokens(512, 128, 4, mean_doc_len=16)


def test_cli_flag():
    from pytorch_distributed_nn_amd.cli import parse_args
    assert parse_args(["--network", "gpt2_tiny", "--doc-mask-eot", "7"]).doc_mask_eot == 7
    assert parse_args(["--network", "GPT2-small", "--doc-mask-eot", "50256"]).doc_mask_eot == 50256
    assert parse_args(["--network", "gpt2_tiny"]).doc_mask_eot is None
    with pytest.raises(SystemExit, match="doc-mask-eot"):
        parse_args(["--network", "LeNet", "--doc-mask-eot", "7"])
    with pytest.raises(SystemExit, match="doc-mask-eot"):
        parse_args(["--network", "gpt2_tiny", "--doc-mask-eot", "-1"])
