"""The signature leaf's input vectors built on the device (glp_ed25519_leaf_inputs, glp_ed25519_half_scalars) against the project's own Python,
ed25519_circuit.witness_inputs(..., record=None) and half_size_pair, word for word, on the cases of tests/ed25519_inputs_cases.py (the ones
tests/test_emu_ed25519_inputs.py runs on the CPU): B = 1, 5 and 65, the three forms, split both ways, a forged neighbour, the launch and
synchronise counts.  Then the signature MapReduce with device_inputs: the same root proof as without, accepted under expected_key, a forged
signature refused with the existing message — once for the 112-byte statement and once for canonical votes of three lengths.  Small parameters
(6 queries, 4 PoW bits, fan-in 2); every recording is made once per module."""
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_inputs_cases as cases  # noqa: E402
from conftest import poseidon_consts  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

BLOCK = hashlib.sha256(b"a block").digest()
FLAGS = [True, True, True, True, False]
SENTINEL = 0x5E5E5E5E5E5E5E5E


def _mod(name):
    graft.load_package()
    return importlib.import_module(graft.PKG_NAME + name)


def run_batch(prover, pkg, b):
    """(rows [n][width], status [n]) of one Prover.ed25519_leaf_inputs call into a buffer a word wider than it needs"""
    layout = pkg.Ed25519InputLayout(b.form, b.lo, b.hi, b.split)
    assert layout.n_words() == b.width
    out = prover.to_device(np.full(b.n * b.width + 1, SENTINEL, dtype=np.uint64))
    slots = range(b.n)
    dummy = None if b.dummy is None else (bytes(b.dummy[:32]), bytes(b.dummy[32:96]), bytes(b.dummy[96:]))
    buf, status = prover.ed25519_leaf_inputs(layout, [bytes(b.pubs[i]) for i in slots], [bytes(b.sigs[i]) for i in slots],
                                             [bytes(b.msgs[i, :b.lens[i]]) for i in slots], None if b.form == cases.PLAIN else list(b.flags), dummy,
                                             out=out)
    assert buf is out and prover.ed25519_last_input_counts() == (2, 1), "two launches and one synchronise whatever n is"
    words = out.download((b.n * b.width + 1,))
    out.free()
    assert words[-1] == SENTINEL
    return words[:-1].reshape(b.n, b.width), status


def assert_batch(b, rows, status):
    assert status.tolist() == b.status.tolist(), b.name
    for i in range(b.n):
        assert np.array_equal(rows[i], b.rows[i]), (b.name, i, np.nonzero(rows[i] != b.rows[i])[0][:8].tolist())
        if status[i] != cases.OK:
            assert not rows[i].any(), (b.name, i)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 65, 513])
def test_half_scalars_equal_half_size_pair(prover, n):
    _, want, ints = cases.half_scalar_cases()
    assert len(ints) == 513
    pick = list(range(n)) if n > 65 else [(7 * i) % 13 for i in range(min(n, 13))] + list(range(13, 13 + max(0, n - 13)))
    got = prover.ed25519_half_scalars([ints[i] for i in pick])
    for row, i in zip(got, pick):
        assert row.tolist() == want[i].tolist(), hex(ints[i])
    if n == 513:
        st = want[:13, 7].tolist()
        assert st.count(cases.INVALID) == 2 and st.count(cases.NO_PAIR) >= 3


@pytest.mark.gpu
def test_plain_form_every_golden_case(prover, pkg):
    for b in cases.plain_batches():
        assert_batch(b, *run_batch(prover, pkg, b))
    assert any(s == cases.REJECT for b in cases.plain_batches() for s in b.status)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.FLAGGED_NAMES)
def test_flagged_and_vote_forms(prover, pkg, name):
    b = cases.flagged_batch(name)
    assert_batch(b, *run_batch(prover, pkg, b))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 65])
def test_forged_slot_is_rejected_and_its_neighbours_stay_right(prover, pkg, B):
    b = cases.flagged_batch(f"b-112-B{B}")
    rows, status = run_batch(prover, pkg, b)
    assert status[3] == cases.REJECT and not rows[3].any() and b.flags[3]
    others = [i for i in range(B) if i != 3]
    assert all(status[i] == cases.OK for i in others) and all(np.array_equal(rows[i], b.rows[i]) and rows[i].any() for i in others)


@pytest.mark.gpu
def test_refused_arguments(prover, pkg):
    with pytest.raises(pkg.GlpError):
        pkg.Ed25519InputLayout(cases.FLAGGED, 48, 49, 1).n_words()
    with pytest.raises(pkg.GlpError):
        pkg.Ed25519InputLayout(7, 48, 48, 1).n_words()
    b = cases.flagged_batch("b-112-B1")
    with pytest.raises(pkg.GlpError):                                            # the flagged form without flags and dummy
        prover.ed25519_leaf_inputs(pkg.Ed25519InputLayout(b.form, b.lo, b.hi, 1), [bytes(32)], [bytes(64)], [bytes(112)])


def _prove_both_ways(sigs, pubs, sg, msgs):
    """prove_set of ONE object (one set of recordings) with device_inputs off, then on; the forged-signature refusal with it on"""
    assert sigs.device_witness and not sigs.device_inputs
    off = sigs.prove_set(pubs, sg, msgs, FLAGS)
    sigs.device_inputs = True
    try:
        calls = []
        sm = _mod(".signature_mr")
        real_wi, real_w = sm.witness_inputs, sigs.prover.ed25519_witness
        sm.witness_inputs = lambda *a, **k: calls.append("witness_inputs") or real_wi(*a, **k)
        sigs.prover.ed25519_witness = lambda *a, **k: calls.append("ed25519_witness") or real_w(*a, **k)
        try:
            on = sigs.prove_set(pubs, sg, msgs, FLAGS)
        finally:
            sm.witness_inputs = real_wi
            del sigs.prover.ed25519_witness
        assert calls == [], "the Map step with device_inputs downloads no record and builds no vector in Python"
        forged = bytearray(sg[1])
        forged[33] ^= 1
        with pytest.raises(ValueError, match=r"the signatures of slots \[1\] do not verify"):
            sigs.prove_set(pubs, [sg[0], bytes(forged)] + sg[2:], msgs, FLAGS)
    finally:
        sigs.device_inputs = False
    return off, on


@pytest.fixture(scope="module")
def leaf112(prover, pkg):
    """the 112-byte signature statement, recorded once"""
    sm, ec = _mod(".signature_mr"), _mod(".ed25519_circuit")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    sigs = sm.SignatureSetMapReduce(prover, consts, msg_len=112, hash_offset=16, fan_in=2, num_queries=6, pow_bits=4, device_witness=True,
                                    device_witness_chunk=4)
    seeds = [hashlib.sha256(b"seed %d" % i).digest() for i in range(5)]
    msgs = [sigs.vote_bytes(BLOCK, i) for i in range(5)]
    keys = [ec.keypair_and_sign(s, m) for s, m in zip(seeds, msgs)]
    yield dict(sigs=sigs, consts=consts, pubs=[k[0] for k in keys], sg=[k[1] if f else None for k, f in zip(keys, FLAGS)], msgs=msgs)
    sigs.free()


@pytest.mark.gpu
def test_signature_set_with_device_inputs(prover, pkg, leaf112):
    sm = _mod(".signature_mr")
    prover.set_poseidon_constants(*leaf112["consts"])
    with pytest.raises(ValueError, match="device_inputs needs device_witness"):
        sm.SignatureSetMapReduce(prover, leaf112["consts"], device_inputs=True)
    sigs = leaf112["sigs"]
    off, on = _prove_both_ways(sigs, leaf112["pubs"], leaf112["sg"], leaf112["msgs"])
    assert on["root_proof"] == off["root_proof"] and on["public"] == off["public"] and on["slots"] == off["slots"]
    vkey = sigs.expected_key(5)
    assert np.array_equal(vkey, on["key"])
    assert sigs.verify_set(on["root_proof"], vkey, on["block_hash"], on["signer_digest"]), prover.last_reject
    assert on["block_hash"] == BLOCK


@pytest.mark.gpu
def test_canonical_votes_with_device_inputs(prover, pkg):
    sm, ec, bs = _mod(".signature_mr"), _mod(".ed25519_circuit"), _mod(".blobstream")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    fmt = bs.VoteFormat.for_commit("celestia", 0)
    with pytest.raises(ValueError, match="device_inputs needs device_witness"):
        sm.CanonicalVoteSetMapReduce(prover, consts, fmt, device_inputs=True)
    sigs = sm.CanonicalVoteSetMapReduce(prover, consts, fmt, fan_in=2, num_queries=6, pow_bits=4, device_witness=True, device_witness_chunk=4)
    try:
        height = 2_500_008
        seeds = [hashlib.sha256(b"seed %d" % i).digest() for i in range(5)]
        msgs = [sigs.vote_bytes(BLOCK, i, height=height) for i in range(5)]
        assert len({len(m) for m in msgs}) >= 3
        keys = [ec.keypair_and_sign(s, m) for s, m in zip(seeds, msgs)]
        off, on = _prove_both_ways(sigs, [k[0] for k in keys], [k[1] if f else None for k, f in zip(keys, FLAGS)], msgs)
        assert on["root_proof"] == off["root_proof"] and on["public"] == off["public"] and on["height"] == height
        vkey = sigs.expected_key(5)
        assert np.array_equal(vkey, on["key"])
        assert sigs.verify_set(on["root_proof"], vkey, BLOCK, on["signer_digest"], height, 0), prover.last_reject
    finally:
        sigs.free()
