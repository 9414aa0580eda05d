"""Row a10 on the GPU: Ed25519 witness records through the C ABI vs the Python big-int oracle on
the OpenSSL / RFC 8032 fixtures, plus a validator-set sized batch signed by OpenSSL-made keys
re-used across messages; and the adversarial families of tests/ed25519_cases.py (torsion, non-canonical
and random encodings, the edges of S, lanes of one wavefront leaving at different exits), every word."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_cases as edc  # noqa: E402
from test_emu_ed25519 import check_records, load_cases  # noqa: E402

pytestmark = pytest.mark.gpu


def test_fixture_records(prover):
    cases = load_cases()
    out = prover.ed25519_witness([bytes.fromhex(c["pub"]) for c in cases], [bytes.fromhex(c["sig"]) for c in cases],
                                 [bytes.fromhex(c["msg"]) for c in cases])
    check_records(cases, out)


def test_batch_of_150_mixed(prover):
    """150 records built from the valid fixtures with every third one corrupted"""
    base = [c for c in load_cases() if c["valid"]]
    cases = []
    for i in range(150):
        c = dict(base[i % len(base)])
        if i % 3 == 2:
            m = bytearray(bytes.fromhex(c["msg"]) or b"\x00")
            m[0] ^= 1 + (i % 7)
            c = {"src": f"corrupt{i}", "pub": c["pub"], "sig": c["sig"], "msg": bytes(m).hex(), "valid": False}
        cases.append(c)
    out = prover.ed25519_witness([bytes.fromhex(c["pub"]) for c in cases], [bytes.fromhex(c["sig"]) for c in cases],
                                 [bytes.fromhex(c["msg"]) for c in cases])
    assert [bool(r[0]) for r in out] == [c["valid"] for c in cases]
    check_records(cases[:12], out[:12])


# ---- adversarial families (tests/ed25519_cases.py): every word of every record against the Python-integer oracle --------------------------------
SENTINEL = 0xA5A5A5A5A5A5A5A5


def launch_raw(prover, triples, overlong=None):
    """the raw ABI on n rows, with the lengths of the `overlong` rows set beyond the row stride; the output buffer holds n + 1 records
    pre-filled with a sentinel.  Returns (the n records, the expected records): the record after the last one must still be the sentinel"""
    n = len(triples)
    pubs, sigs, msgs, lens, stride = edc.marshal(triples)
    expected = [edc.expected_record(*t) for t in triples]
    for i in range(n):
        if overlong is not None and overlong[i]:
            lens[i] = (stride + 1, 0xFFFFFFFF, stride + 64)[i % 3]
            expected[i] = [0] * edc.REC
    bufs = [prover.to_device(a) for a in (pubs, sigs, msgs, lens, np.full((n + 1, edc.REC), SENTINEL, dtype=np.uint64))]
    try:
        prover._chk(prover.lib.glp_ed25519_witness(prover.ctx, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, stride, bufs[3].ptr, n, bufs[4].ptr),
                    "glp_ed25519_witness")
        out = bufs[4].download((n + 1, edc.REC))
    finally:
        for b in bufs:
            b.free()
    assert (out[n] == SENTINEL).all(), "the kernel wrote past the last record"
    return out[:n], expected


def test_families_every_word(prover):
    """one launch per family; all 37 words, zero where the oracle has no value"""
    for name in "abcde":
        triples = edc.FAMILIES[name]()
        out = prover.ed25519_witness([t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples])
        edc.assert_records(triples, out)


def test_mixed_exits_in_every_wavefront(prover):
    """all families shuffled, some rows over-long: every block of 64 rows (asserted by shuffled_rows) has lanes that leave at the length check,
    after a failed decoding, at S >= L and at the end of the full path; n is no multiple of 64"""
    triples, overlong = edc.shuffled_rows()
    assert len(triples) % 64 != 0 and any(overlong)
    out, expected = launch_raw(prover, triples, overlong)
    assert all(not out[i].any() for i in range(len(triples)) if overlong[i])
    edc.assert_records(triples, out, expected)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_grid_edges(prover, n):
    """one lane, a wavefront short of one lane, a full one, and one lane into a second block"""
    triples, overlong = edc.shuffled_rows()
    out, expected = launch_raw(prover, triples[:n], overlong[:n])
    edc.assert_records(triples[:n], out, expected)


def test_records_feed_the_circuit_inputs(prover):
    """the valid rows of the torsion family: the circuit's input vector built from the device's record (verdict, k, x_A, x_R) is the one built
    with Python integers.  No circuit is built"""
    import __graft_entry__ as graft
    ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
    triples = edc.family_d()
    out = prover.ed25519_witness([t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples])
    valid = [i for i, t in enumerate(triples) if edc.expected_record(*t)[0]]
    assert len(valid) >= 10 and [i for i in range(len(triples)) if out[i][0]] == valid
    for i in valid:
        pub, sig, msg = triples[i]
        assert ec.witness_inputs(pub, sig, msg, record=out[i]) == ec.witness_inputs(pub, sig, msg), i
    with pytest.raises(ValueError):
        invalid = next(i for i in range(len(triples)) if i not in valid)
        ec.witness_inputs(*triples[invalid], record=out[invalid])
