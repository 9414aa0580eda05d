"""Canonical votes of differing lengths through the signature MapReduce on the GPU (signature_mr.CanonicalVoteSetMapReduce): one launch of the
Ed25519 witness kernel over messages of mixed lengths, a set of five validators (three distinct vote lengths, one unsigned) in eight slots proved,
folded and verified by both verifiers under the VERIFIER's key, the negative cases, the device-side witness path, and CombinedSkip with the votes'
height tied to the target block.  Small parameters (6 queries, 4 PoW bits, fan-in 2); the recordings are made once per module."""
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_ref as pref  # noqa: E402
from conftest import poseidon_consts, ptr  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

HEIGHT = 2_500_008
BLOCK = hashlib.sha256(b"a block").digest()
FLAGS = [True, True, True, True, False]


def _mod(name):
    graft.load_package()
    return importlib.import_module(graft.PKG_NAME + name)


@pytest.fixture(scope="module")
def cv(prover, pkg):
    """the prover's object, the verifier's (another ctx; it evaluates witnesses on the device), five validators and their votes"""
    sm, ec, bs = _mod(".signature_mr"), _mod(".ed25519_circuit"), _mod(".blobstream")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    fmt = bs.VoteFormat.for_commit("celestia", 0)
    sigs = sm.CanonicalVoteSetMapReduce(prover, consts, fmt, fan_in=2, num_queries=6, pow_bits=4)
    p2 = pkg.Prover(0)
    p2.set_poseidon_constants(*consts)
    other = sm.CanonicalVoteSetMapReduce(p2, consts, fmt, fan_in=2, num_queries=6, pow_bits=4, device_witness=True, device_witness_chunk=4)
    seeds = [hashlib.sha256(b"seed %d" % i).digest() for i in range(5)]
    pubs = [ec.keypair_and_sign(s, b"")[0] for s in seeds]

    def votes(height=HEIGHT, block=BLOCK, vote_type=2):
        msgs = [sigs.vote_bytes(block, i, height=height, vote_type=vote_type) for i in range(5)]
        return [ec.keypair_and_sign(s, m)[1] if f else None for s, m, f in zip(seeds, msgs, FLAGS)], msgs
    s = dict(sm=sm, ec=ec, bs=bs, consts=consts, fmt=fmt, sigs=sigs, other=other, seeds=seeds, pubs=pubs, votes=votes)
    # the recordings (leaf, level-1 node, padded root — on both objects) are made here, once: the set the tests are about, and the verifier's key
    sg, msgs = votes()
    s["out"] = sigs.prove_set(pubs, sg, msgs, FLAGS)
    s["vkey"] = other.expected_key(5)                                          # the verifier's own setup, on its own object and ctx
    yield s
    other.free()
    sigs.free()
    p2.close()


def _set_constants(prover, oracle, consts):
    prover.set_poseidon_constants(*consts)
    oracle.orc_poseidon_set_constants(*(ptr(a) for a in consts))


@pytest.mark.gpu
def test_witness_kernel_over_messages_of_mixed_lengths(prover, pkg):
    """ONE glp_ed25519_witness launch, per-signature lengths either side of the SHA-512 block boundaries of R ‖ A ‖ M (111 | 112 and 239)"""
    ec = _mod(".ed25519_circuit")
    lens = [47, 48, 111, 112, 175]
    msgs = [bytes((7 * i + k) & 0xFF for k in range(n)) for i, n in enumerate(lens)]
    keys = [ec.keypair_and_sign(hashlib.sha256(b"mixed %d" % i).digest(), m) for i, m in enumerate(msgs)]
    recs = prover.ed25519_witness([k[0] for k in keys], [k[1] for k in keys], msgs)
    for (pub, sig), m, r in zip(keys, msgs, recs):
        assert int(r[0]) == 1
        k = sum(int(r[1 + j]) << (64 * j) for j in range(4))
        assert k == int.from_bytes(hashlib.sha512(sig[:32] + pub + m).digest(), "little") % ec.ELL
    # the same signatures over messages shifted by one row: every record is rejected
    recs = prover.ed25519_witness([k[0] for k in keys], [k[1] for k in keys], msgs[1:] + msgs[:1])
    assert not any(int(r[0]) for r in recs)


@pytest.mark.gpu
def test_set_with_three_vote_lengths_and_an_unsigned_slot(prover, oracle, cv):
    _set_constants(prover, oracle, cv["consts"])
    gd = _mod(".gadgets")
    sigs, other = cv["sigs"], cv["other"]
    sg, msgs = cv["votes"]()
    assert len({len(m) for m in msgs}) >= 3 and sg[4] is None
    out, rec = cv["out"], dict(sigs.record_seconds)
    out2 = sigs.prove_set(cv["pubs"], sg, msgs, FLAGS)                          # replays every recording, and is the same proof
    assert sigs.record_seconds == rec and out2["root_proof"] == out["root_proof"] and out2["public"] == out["public"]
    digest = gd.signer_digest_host(cv["consts"], cv["pubs"], FLAGS, pad_to=8)
    words = [int.from_bytes(BLOCK[i:i + 4], "big") for i in range(0, 32, 4)]
    assert out["slots"] == 6 and out["public"] == words + digest + [HEIGHT, 0, 0, 0]
    assert (out["block_hash"], out["signer_digest"], out["height"], out["round"]) == (BLOCK, digest, HEIGHT, 0)
    vkey = cv["vkey"]
    assert np.array_equal(vkey, out["key"])
    assert other.verify_set(out["root_proof"], vkey, BLOCK, digest, HEIGHT, 0), other.prover.last_reject
    pref.verify_plonk(out["root_proof"], oracle, pos_consts=cv["consts"], public=out["public"])
    assert not other.verify_set(out["root_proof"], vkey, BLOCK, digest, HEIGHT + 1, 0)
    assert not other.verify_set(out["root_proof"], vkey, BLOCK, digest, HEIGHT, 1)
    assert not other.verify_set(out["root_proof"], vkey, bytes(32), digest, HEIGHT, 0)


@pytest.mark.gpu
def test_what_cannot_be_proved(prover, oracle, cv):
    _set_constants(prover, oracle, cv["consts"])
    sigs, ec, seeds, pubs = cv["sigs"], cv["ec"], cv["seeds"], cv["pubs"]
    sg, msgs = cv["votes"]()
    forged = bytearray(sg[1])
    forged[33] ^= 1
    with pytest.raises(ValueError):                                           # a forged signature
        sigs.prove_set(pubs, [sg[0], bytes(forged)] + sg[2:], msgs, FLAGS)
    with pytest.raises(ValueError):                                           # a flagged slot without a signature
        sigs.prove_set(pubs, sg[:4] + [bytes(64)], msgs, [True] * 5)

    def one_other(i, **kw):
        m = list(msgs)
        m[i] = sigs.vote_bytes(kw.pop("block", BLOCK), i, **kw)
        s = list(sg)
        s[i] = ec.keypair_and_sign(seeds[i], m[i])[1]
        return pubs, s, m, FLAGS
    with pytest.raises(ValueError):                                           # one validly signed PREVOTE: the leaf refuses it
        sigs.prove_set(*one_other(2, height=HEIGHT, vote_type=1))
    with pytest.raises(ValueError):                                           # one vote at another height: its node refuses the mixed children
        sigs.prove_set(*one_other(3, height=HEIGHT + 1))
    with pytest.raises(ValueError):                                           # one vote naming another block
        sigs.prove_set(*one_other(0, height=HEIGHT, block=hashlib.sha256(b"another block").digest()))
    with pytest.raises(ValueError):                                           # a vote longer than the window
        sigs.prove_set(pubs, sg, msgs[:4] + [msgs[4] + bytes(8)], FLAGS)


@pytest.mark.gpu
def test_device_witness_gives_the_same_root_proof(prover, oracle, cv):
    _set_constants(prover, oracle, cv["consts"])
    sg, msgs = cv["votes"]()
    assert cv["other"].device_witness and not cv["sigs"].device_witness
    out = cv["other"].prove_set(cv["pubs"], sg, msgs, FLAGS)
    assert out["root_proof"] == cv["out"]["root_proof"] and out["public"] == cv["out"]["public"]


@pytest.mark.gpu
def test_combined_skip_with_canonical_votes(prover, oracle, cv):
    """the small tree of test_combined_skip_small_tree_and_negative_cases with the votes in-circuit: the outer circuit equates the signature
    root's height with the target block, so votes for another height — all validly signed, all agreeing — cannot be joined with this skip"""
    _set_constants(prover, oracle, cv["consts"])
    cs, dm, gd = _mod(".combined_skip_mr"), _mod(".data_commitment_mr"), _mod(".gadgets")
    ec, sigs, consts = cv["ec"], cv["sigs"], cv["consts"]
    idx = [0, 1, 2, None, None]
    mr = cs.CombinedSkipMapReduce(prover, consts, skip=8, batch=2, fan_in=2, num_queries=6, pow_bits=4, max_skip=100, signatures=sigs)
    *case, seeds = mr.synthetic_case(4, 5, idx, trusted_height=2_500_000, power_groups=3, seed=11, real_keys=True)
    case[4] = list(FLAGS)
    votes = mr.synthetic_votes(case, seeds)
    assert votes[0][4] is None and len({len(m) for m in votes[1]}) >= 3
    out = mr.prove_skip(*case, votes=votes)
    target_hash = dm.HeaderChainMapReduce.header_hash(case[2][-1])
    assert out["signatures_in_circuit"] and out["target_block"] == 2_500_008 == HEIGHT and out["target_hash"] == target_hash
    assert all(m[1:3] == b"\x08\x02" and int.from_bytes(m[4:12], "little") == out["target_block"] and m[16:48] == target_hash for m in votes[1])
    want = dict(trusted_hash=out["trusted_hash"], target_hash=target_hash, signer_digest=gd.signer_digest_host(consts, case[3][0], case[4], pad_to=8),
                trusted_block=2_500_000, target_block=2_500_008, commitment=out["commitment"])
    assert mr.verify(out["root_proof"], out["key"], **want), prover.last_reject
    pref.verify_plonk(out["root_proof"], oracle, pos_consts=consts, public=out["public"])
    assert not mr.verify(out["root_proof"], out["key"], **dict(want, target_block=2_500_009))
    # votes for target_block + 1
    m2 = [sigs.vote_bytes(target_hash, i, height=out["target_block"] + 1) for i in range(5)]
    s2 = [ec.keypair_and_sign(seeds[i], m2[i])[1] if case[4][i] else None for i in range(5)]
    with pytest.raises(ValueError):
        mr.prove_skip(*case, votes=(s2, m2))
    mr.free()
