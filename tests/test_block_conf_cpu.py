"""ops.transformer.BlockConf: the named form of a block's configuration accepts the plain tuples callers pass."""
from pytorch_distributed_nn_amd.ops.transformer import BlockConf


def test_block_conf_from_plain_tuples():
    metas, doc, drop = object(), (object(), object()), (0.1, 0.2, object(), 3)
    full = (2, 128, 4, 1e-5, metas, doc, drop)
    c4 = BlockConf(*full[:4])
    assert (c4.B, c4.T, c4.H, c4.eps) == (2, 128, 4, 1e-5)
    assert c4.metas is None and c4.doc is None and c4.drop is None
    c6 = BlockConf(*full[:6])
    assert c6.metas is metas and c6.doc is doc and c6.drop is None
    c7 = BlockConf(*full)
    assert c7.metas is metas and c7.doc is doc and c7.drop is drop
    assert BlockConf(*c7) == c7 and BlockConf(*(full[:6] + (None,))) == c6
    for c in (c4, c6, c7):
        assert isinstance(c, tuple) and len(c) == 7
        B, T, H, eps = c[:4]
        assert (B, T, H, eps) == full[:4]
