"""mapreduce.reduce_verify / reduce_aggregate with verify_batch= on one rank, without a GPU: what the callable may return and what it may not.
The verdict must never come from the truthiness of a row, and a leaf without a digest must give False, not an exception."""
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mr(pkg):
    return importlib.import_module(pkg.__name__ + ".mapreduce")


PROOFS = [b"a" * 8, b"b" * 8]


def test_booleans_and_rows(mr):
    assert mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: [True, True]) is True
    assert mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: [True, False]) is False
    assert mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: [np.bool_(True), np.bool_(False)]) is False
    # the rows of PlonkCircuit.verify_batch: a refused proof is a non-empty (truthy) tuple and must still count as refused
    assert mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: [(True, None, None), (False, "x", 3)]) is False
    assert mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: [(True, None, None), (True, None, None)]) is True
    assert mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: ([(True, None, None), (False, "x", 3)], [[1, 2, 3, 4], [5, 6, 7, 8]])) is False
    assert mr.reduce_verify(None, [], verify_batch=lambda ps: pytest.fail("nothing to verify: not called")) is True
    # verify_leaf is not used when verify_batch is given
    assert mr.reduce_verify(lambda p: pytest.fail("not used"), PROOFS, verify_batch=lambda ps: [True, True]) is True


def test_a_leaf_without_a_digest_gives_false_not_an_exception(mr):
    # what Prover.plonk_verify_batch(..., want_digests=True) returns for a leaf whose header does not parse: refused, digest None
    vb = lambda ps: ([True, False], [[1, 2, 3, 4], None])  # noqa: E731
    assert mr.reduce_verify(None, PROOFS, verify_batch=vb) is False
    out = mr.reduce_aggregate(None, None, PROOFS, verify_batch=vb)
    assert out == {"ok": False}
    # digests are kept for ACCEPTED leaves only
    assert mr._verify_share(vb, PROOFS, [0, 1]) == (False, {0: [1, 2, 3, 4]})
    assert mr._verify_share(lambda ps: ([True, True], [[1, 2, 3, 4], None]), PROOFS, [0, 1]) == (True, {0: [1, 2, 3, 4]})


@pytest.mark.parametrize("ret", [[1, 1], ["yes", ""], [None, True], [(True, None), (False, None)], [(1, None, None), (0, "x", 3)], [[True], [False]]])
def test_anything_else_is_refused(mr, ret):
    with pytest.raises(TypeError):
        mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: ret)


def test_wrong_counts_are_refused(mr):
    with pytest.raises(ValueError):
        mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: [True])
    with pytest.raises(ValueError):
        mr.reduce_verify(None, PROOFS, verify_batch=lambda ps: ([True, True], [[1, 2, 3, 4]]))
