"""ops/speculate.py on the CPU: prepare_reference and accept_reference against the hand-written cases of
tests/speculate_cases.py (n-gram lookup, table drafts, acceptance, truncation, eos, complete rows)."""
import pytest
import torch

import speculate_cases as C
from pytorch_distributed_nn_amd.ops.sampling import uniform
from pytorch_distributed_nn_amd.ops.speculate import accept_reference, prepare_reference

SEED = 1234


@pytest.mark.parametrize("name", sorted(C.PREPARE_NGRAM))
def test_prepare_ngram(name):
    kw, want = C.prepare_ngram_case(name)
    S, nt, ln = kw["S"], int(kw["ntok"][0]), int(kw["lens"][0])
    before = kw["out"].clone()
    tok_in, pos, u = prepare_reference(seed=SEED, **kw)
    assert tok_in.dtype == torch.int64 and tok_in.tolist() == want
    assert pos.dtype == torch.int32 and pos.tolist() == [ln + j for j in range(S)]
    assert u.dtype == torch.float32 and u.tolist() == [uniform(SEED, nt + j, 0) for j in range(S)]
    assert torch.equal(kw["out"], before)


def test_prepare_table():
    kw, want, pos_want = C.prepare_table_case()
    tok_in, pos, u = prepare_reference(seed=SEED, **kw)
    assert tok_in.tolist() == want and pos.tolist() == pos_want
    S = kw["S"]
    assert u.tolist() == [uniform(SEED, int(kw["ntok"][b]) + j, b) for b in range(2) for j in range(S)]


def test_uniform_is_24_bits_and_depends_on_every_argument():
    us = {(s, i, b): uniform(s, i, b) for s in (1, 2) for i in (0, 1, 5) for b in (0, 1, 7)}
    assert len(set(us.values())) == len(us)
    for v in us.values():
        assert 0.0 <= v < 1.0 and v * 2 ** 24 == int(v * 2 ** 24)


@pytest.mark.parametrize("case", [C.accept_case, C.accept_done_case], ids=["mixed_rows", "done"])
def test_accept(case):
    kw, st, want = case()
    tok_in0, t0 = st["tok_in"].clone(), st["t"].clone()
    done = accept_reference(st["tok_in"], st["t"], st["out"], kw["P"], kw["N"], st["ntok"], st["lens"], st["finished"],
                            kw["eos_token"], st["stats"], kw["S"])
    assert done is want["done"]
    assert st["out"].tolist() == want["out"]
    assert st["ntok"].tolist() == want["ntok"] and st["lens"].tolist() == want["lens"]
    assert st["stats"].tolist() == want["stats"]
    if want["finished"] is not None:
        assert st["finished"].tolist() == want["finished"]
    assert torch.equal(st["tok_in"], tok_in0) and torch.equal(st["t"], t0)
