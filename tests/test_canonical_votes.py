"""Canonical Tendermint votes of differing lengths in the signature circuit (blobstream.canonical_vote_sign_bytes / VoteFormat,
ed25519_circuit.Sha512Gadget.hash_bytes_var, verify_statement(vote_format=...)): the encoder against byte strings assembled by hand from the
layout, the variable-length SHA-512 against hashlib at the two-block edges, and ONE recorded leaf circuit that replays votes of every length of
its window and refuses prevotes, wrong length prefixes, moved tags, lengths that are not the signed one and forged signatures.  CPU only (the
builder runs on object(), as in tests/test_ed25519_circuit.py)."""
import ctypes
import hashlib
import importlib
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import poseidon_consts  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

NANOS = [0, 1, 127, 128, 16_383, 16_384, 2_097_151, 2_097_152, 268_435_455, 268_435_456, 999_999_999]


def _mods():
    graft.load_package()
    return tuple(importlib.import_module(graft.PKG_NAME + m) for m in (".blobstream", ".ed25519_circuit", ".recursion"))


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------
def test_encoder_against_hand_assembled_bytes():
    bs, _, _ = _mods()
    h, ph = bytes(range(32)), bytes(range(100, 132))
    # round 0, nanos 0, short chain id: both fields omitted
    got = bs.canonical_vote_sign_bytes("ab", 5, 0, h, 1, ph, 1_700_000_000, 0)
    psh = b"\x08\x01" + b"\x12\x20" + ph
    block_id = b"\x0a\x20" + h + b"\x12" + bytes([len(psh)]) + psh
    stamp = b"\x08" + bytes([0x80, 0xE2, 0xCF, 0xAA, 0x06])                    # 1 700 000 000 in base 128, low group first
    assert sum((g & 0x7F) << (7 * i) for i, g in enumerate(stamp[1:])) == 1_700_000_000
    body = b"\x08\x02" + b"\x11" + bytes([5, 0, 0, 0, 0, 0, 0, 0]) + b"\x22" + bytes([len(block_id)]) + block_id + b"\x2a" + bytes([len(stamp)]) + stamp + \
        b"\x32\x02ab"
    assert len(block_id) == 72 and len(body) == 97 and got == bytes([97]) + body
    # round 3, nanos 999 999 999 (a five-byte varint), a prevote, a two-byte part total, a longer chain id: the body needs a two-byte prefix
    got = bs.canonical_vote_sign_bytes(b"osmosis-testnet-42", 0x0102030405, 3, h, 300, ph, 1_700_000_001, 999_999_999, vote_type=1)
    psh = b"\x08\xac\x02" + b"\x12\x20" + ph
    block_id = b"\x0a\x20" + h + b"\x12" + bytes([len(psh)]) + psh
    stamp = b"\x08" + bytes([0x81, 0xE2, 0xCF, 0xAA, 0x06]) + b"\x10" + bytes([0xFF, 0x93, 0xEB, 0xDC, 0x03])
    assert sum((g & 0x7F) << (7 * i) for i, g in enumerate(stamp[7:])) == 999_999_999
    body = b"\x08\x01" + b"\x11" + bytes([5, 4, 3, 2, 1, 0, 0, 0]) + b"\x19" + bytes([3, 0, 0, 0, 0, 0, 0, 0]) + b"\x22" + bytes([len(block_id)]) + block_id + \
        b"\x2a" + bytes([len(stamp)]) + stamp + b"\x32\x12osmosis-testnet-42"
    assert len(body) == 129 and got == bytes([0x81, 0x01]) + body
    for bad in (dict(seconds=-1), dict(nanos=-1), dict(nanos=10**9), dict(block_hash=bytes(31)), dict(part_hash=bytes(33)), dict(height=0), dict(height=-4)):
        kw = dict(chain_id="ab", height=5, round=0, block_hash=h, part_total=1, part_hash=ph, seconds=1, nanos=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            bs.canonical_vote_sign_bytes(**kw)


def test_format_windows():
    bs, _, _ = _mods()
    fmt = bs.VoteFormat.for_commit("celestia", 0)
    assert (fmt.round_present, fmt.min_len, fmt.max_len, fmt.prefix_len, fmt.base, fmt.hash_offset) == (False, 104, 110, 1, 12, 16)
    lens = set()
    for nanos in NANOS:
        n = len(bs.canonical_vote_sign_bytes("celestia", 4_000_000, 0, bytes(32), 1, bytes(32), 1_700_000_000, nanos))
        assert fmt.min_len <= n <= fmt.max_len
        lens.add(n)
    assert lens == {104, 106, 107, 108, 109, 110}
    long_id = "a-chain-with-a-long-name"
    f3 = bs.VoteFormat.for_commit(long_id, 3)                                  # a round and a 24-byte chain id: the two-byte prefix
    assert (f3.round_present, f3.min_len, f3.max_len, f3.prefix_len, f3.base, f3.hash_offset) == (True, 130, 136, 2, 22, 26)
    for nanos in NANOS:
        assert f3.min_len <= len(bs.canonical_vote_sign_bytes(long_id, 7, 3, bytes(32), 1, bytes(32), 1_700_000_000, nanos)) <= f3.max_len
    with pytest.raises(ValueError):
        bs.VoteFormat(False, 125, 131)                                          # straddles the 1-byte / 2-byte length prefix
    with pytest.raises(ValueError):
        bs.VoteFormat.for_commit("a" * 30, 0)                                   # ... and so does this commit's window (bodies of 125 .. 131 bytes)
    with pytest.raises(ValueError):
        bs.VoteFormat(False, 47, 53)
    with pytest.raises(ValueError):
        bs.VoteFormat(True, 170, 176)
    assert bs.VoteFormat(False, 48, 54).prefix_len == 1 and bs.VoteFormat(True, 169, 175).prefix_len == 2


# ---- hash_bytes_var alone ------------------------------------------------------------------------------------------------------------------
def _var_hash_program(ec, rec, lo, hi):
    """a program: inputs = 64 fixed bytes, hi message bytes, L, the one-hot; the digest bytes are its public inputs"""
    b = rec.CircuitBuilder(object(), n_wires=144, n_routed=144)
    g = ec.Sha512Gadget(b)
    fixed = [ec._byte_input(b, g, 0) for _ in range(64)]
    msg = [ec._byte_input(b, g, 0) for _ in range(hi)]
    L = b.var(lo)
    onehot = [b.var(1 if j == 0 else 0) for j in range(hi - lo + 1)]
    digest, length = g.hash_bytes_var([bits for _, bits in fixed], [bits for _, bits in msg], lo, hi, onehot)
    b.assert_equal(length, L)
    for byte in digest:
        b.public_input(g.pack(byte))
    return b.program()


@pytest.mark.parametrize("lo,hi", [(48, 54), (169, 175)])
def test_hash_bytes_var_matches_hashlib_for_every_length(lo, hi):
    _, ec, rec = _mods()
    consts = poseidon_consts("small")
    prog = _var_hash_program(ec, rec, lo, hi)                                  # ONE recording replays every L
    rng = np.random.default_rng(lo)
    fixed = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    msg = rng.integers(0, 256, hi, dtype=np.uint8).tobytes()
    onehot = lambda L: [1 if j == L - lo else 0 for j in range(hi - lo + 1)]
    digest = lambda vals: bytes(int(vals[v]) for v in prog.public_vars)
    for L in range(lo, hi + 1):
        want = hashlib.sha512(fixed + msg[:L]).digest()
        for tail in (msg[L:], bytes(hi - L), bytes([0xFF]) * (hi - L)):        # junk at or beyond L changes nothing
            vals = prog.evaluate(consts, list(fixed) + list(msg[:L] + tail) + [L] + onehot(L), threads=1)
            assert digest(vals) == want, L
    base = list(fixed) + list(msg)
    two = onehot(lo)
    two[-1] = 1
    for L, sel in ((lo, two), (lo + 1, onehot(lo + 2)), (lo, [0] * (hi - lo + 1)), (hi + 1, onehot(hi)), (lo + 1, [2 if j == 1 else (P_MINUS_1 if j == 2 else 0) for j in range(hi - lo + 1)])):
        with pytest.raises(ValueError):
            prog.evaluate(consts, base + [L] + sel, threads=1)


P_MINUS_1 = (1 << 64) - (1 << 32)                                               # selectors 2 and -1 sum to 1 but are no bits


def test_hash_bytes_var_refuses_windows_across_a_block_boundary():
    _, ec, rec = _mods()
    b = rec.CircuitBuilder(object(), n_wires=144, n_routed=144)
    g = ec.Sha512Gadget(b)
    zero_byte = [g.zero] * 8
    for lo, hi in ((47, 50), (170, 176)):
        with pytest.raises(ValueError):
            g.hash_bytes_var([zero_byte] * 64, [zero_byte] * hi, lo, hi, [g.one] + [g.zero] * (hi - lo))


# ---- the leaf, recorded once ---------------------------------------------------------------------------------------------------------------
HEIGHT, CHAIN = 4_000_123, "celestia"
BLOCK = hashlib.sha256(b"a block").digest()


def _vote(bs, nanos, vote_type=2, height=HEIGHT, block=BLOCK):
    return bs.canonical_vote_sign_bytes(CHAIN, height, 0, block, 1, hashlib.sha256(b"parts").digest(), 1_700_000_000, nanos, vote_type=vote_type)


@pytest.fixture(scope="module")
def leaf():
    bs, ec, rec = _mods()
    fmt = bs.VoteFormat.for_commit(CHAIN, 0)
    msg = _vote(bs, 0)
    pub, sig = ec.keypair_and_sign(bytes(32), msg)
    b = rec.CircuitBuilder(object(), n_wires=144, n_routed=144)
    st = ec.verify_statement(b, pub, sig, msg, flag=True, vote_format=fmt)
    hb = st["msg_bytes"][fmt.hash_offset:fmt.hash_offset + 32]
    one = b.constant(1)
    words = [b.arith(1 << 24, 1, 0, hb[k], one, b.arith(1 << 16, 1, 0, hb[k + 1], one, b.arith(1 << 8, 1, 0, hb[k + 2], one, hb[k + 3]))) for k in range(0, 32, 4)]
    for v in st["key_words"] + [st["flag"]] + words + st["height_words"] + st["round_words"]:
        b.public_input(v)
    prog = b.program()
    return dict(fmt=fmt, prog=prog, builder_values=np.array(b.values, dtype=np.uint64), first=(pub, sig, msg), consts=poseidon_consts("small"))


def _public(pub, flag, block, height, rnd=0):
    return list(struct.unpack(">8I", pub)) + [flag] + list(struct.unpack(">8I", block)) + [height & 0xFFFFFFFF, height >> 32, rnd & 0xFFFFFFFF, rnd >> 32]


def test_leaf_is_a_2_16_row_circuit(leaf):
    stats = leaf["prog"].stats
    print("canonical leaf:", {k: stats[k] for k in ("rows", "rows_used", "arith_gates", "sha_rows")})
    assert stats["rows"] == 1 << 16
    pub, sig, msg = leaf["first"]
    _, ec, _ = _mods()
    vals = leaf["prog"].evaluate(leaf["consts"], ec.witness_inputs(pub, sig, msg, True, vote_format=leaf["fmt"]), threads=1)
    assert np.array_equal(vals, leaf["builder_values"])


def test_leaf_replays_votes_of_three_lengths_and_an_unsigned_slot(leaf):
    bs, ec, _ = _mods()
    prog, fmt, consts = leaf["prog"], leaf["fmt"], leaf["consts"]
    seen = set()
    for i, nanos in enumerate((0, 77, 999_999_999)):
        msg = _vote(bs, nanos)
        seen.add(len(msg))
        pub, sig = ec.keypair_and_sign(hashlib.sha256(b"validator %d" % i).digest(), msg)
        vals = prog.evaluate(consts, ec.witness_inputs(pub, sig, msg, True, vote_format=fmt), threads=1)
        assert [int(vals[v]) for v in prog.public_vars] == _public(pub, 1, BLOCK, HEIGHT)
    assert seen == {104, 106, 110}
    # an unflagged slot: no signature, the dummy triple is verified in its place; its own vote is still read (and must be well-formed)
    msg = _vote(bs, 300)
    pub, _ = ec.keypair_and_sign(hashlib.sha256(b"validator 9").digest(), msg)
    vals = prog.evaluate(consts, ec.witness_inputs(pub, bytes(64), msg, False, vote_format=fmt), threads=1)
    assert [int(vals[v]) for v in prog.public_vars] == _public(pub, 0, BLOCK, HEIGHT)


def test_leaf_refuses_what_is_not_a_signed_precommit_of_this_format(leaf):
    bs, ec, _ = _mods()
    prog, fmt, consts = leaf["prog"], leaf["fmt"], leaf["consts"]
    seed = hashlib.sha256(b"validator 3").digest()
    refused = lambda inputs: pytest.raises(ValueError, prog.evaluate, consts, inputs, threads=1)
    o_msg, o_len, o_hot = 33, 33 + fmt.max_len, 34 + fmt.max_len                # input positions: flag, key (32), message, L, one-hot
    W = fmt.max_len - fmt.min_len + 1

    def signed_inputs(msg):
        pub, sig = ec.keypair_and_sign(seed, msg)
        return ec.witness_inputs(pub, sig, msg, True, vote_format=fmt)
    good = _vote(bs, 77)
    prog.evaluate(consts, signed_inputs(good), threads=1)
    # a prevote, validly signed
    refused(signed_inputs(_vote(bs, 77, vote_type=1)))
    # a wrong length prefix, validly signed
    wrong = bytearray(good)
    wrong[0] += 1
    refused(signed_inputs(bytes(wrong)))
    # the tag 0a 20 of the block hash one byte later (validly signed bytes of the same length)
    moved = bytearray(good)
    moved[fmt.base + 2:fmt.base + 5] = bytes([moved[fmt.base + 4], 0x0A, 0x20])
    refused(signed_inputs(bytes(moved)))
    # a claimed length that is not the signed one: L + 1, with the prefix and the selectors saying so consistently, the extra byte zero
    inputs = signed_inputs(good)
    claimed = len(good) + 1
    inputs[o_msg] += 1
    inputs[o_len] = claimed
    inputs[o_hot:o_hot + W] = [1 if j == claimed - fmt.min_len else 0 for j in range(W)]
    refused(inputs)
    # lengths outside the window: no input vector exists, and a hand-made one (L = min_len - 1 / max_len + 1, whatever the selectors) is refused
    with pytest.raises(ValueError):
        ec.witness_inputs(bytes(32), bytes(64), bytes(fmt.max_len + 1), False, vote_format=fmt)
    with pytest.raises(ValueError):
        ec.witness_inputs(bytes(32), bytes(64), bytes(fmt.min_len - 1), False, vote_format=fmt)
    short = _vote(bs, 0)
    for L, sel in ((fmt.min_len - 1, [0] * W), (fmt.min_len - 1, [1] + [0] * (W - 1)), (fmt.max_len + 1, [0] * (W - 1) + [1])):
        inputs = signed_inputs(short)
        inputs[o_msg] = L - 1
        inputs[o_len] = L
        inputs[o_hot:o_hot + W] = sel
        refused(inputs)
    # a forged S
    pub, sig = ec.keypair_and_sign(seed, good)
    forged = bytearray(sig)
    forged[40] ^= 1
    refused(ec.witness_inputs(pub, bytes(forged), good, True, vote_format=fmt))
    # a vote at another height is a valid leaf of its own (the nodes compare heights); its public inputs say so
    other = _vote(bs, 77, height=HEIGHT + 1)
    vals = prog.evaluate(consts, signed_inputs(other), threads=1)
    assert [int(vals[v]) for v in prog.public_vars][17:19] == [HEIGHT + 1, 0]


def test_leaf_plan_on_the_host_equals_the_evaluator(leaf):
    """the level-scheduled plan of the device evaluator, run serially on the host, gives the evaluator's bytes for a vote of another length"""
    bs, ec, _ = _mods()
    prog, fmt, consts = leaf["prog"], leaf["fmt"], leaf["consts"]
    lib = graft.load_package().load_library()
    msg = _vote(bs, 16_384)
    pub, sig = ec.keypair_and_sign(hashlib.sha256(b"validator 5").digest(), msg)
    inputs = np.ascontiguousarray(ec.witness_inputs(pub, sig, msg, True, vote_format=fmt), dtype=np.uint64)
    want = prog.evaluate(consts, inputs, threads=1)
    words, eq = np.ascontiguousarray(prog.prog, dtype=np.uint64), np.ascontiguousarray(prog.eq_pairs, dtype=np.uint64)
    h = ctypes.c_void_p()
    assert lib.glp_witness_plan_create(words.ctypes.data, words.size, prog.n_inputs, prog.n_values, eq.ctypes.data, eq.size // 2, ctypes.byref(h)) == 0
    try:
        vals = np.zeros(prog.n_values, dtype=np.uint64)
        bad = ctypes.c_size_t(0)
        rc = lib.glp_witness_plan_run_host(h, *(a.ctypes.data for a in consts), inputs.ctypes.data, inputs.size, vals.ctypes.data, vals.size, ctypes.byref(bad))
        assert rc == 0 and vals.tobytes() == np.ascontiguousarray(want, dtype=np.uint64).tobytes()
    finally:
        lib.glp_witness_plan_destroy(h)


def test_leaf_with_a_round_and_the_two_byte_prefix():
    """the other form of every format-dependent constraint: a round field (tag 19, round words exported) and a body of 128 bytes or more"""
    bs, ec, rec = _mods()
    chain = "a-chain-with-a-long-name"
    fmt = bs.VoteFormat.for_commit(chain, 3)
    height = (7 << 32) | 4_000_123
    msg = bs.canonical_vote_sign_bytes(chain, height, 3, BLOCK, 1, bytes(32), 1_700_000_000, 16_384)
    assert fmt.prefix_len == 2 and fmt.min_len < len(msg) < fmt.max_len and msg[fmt.hash_offset:fmt.hash_offset + 32] == BLOCK
    pub, sig = ec.keypair_and_sign(bytes(32), msg)
    b = rec.CircuitBuilder(object(), n_wires=144, n_routed=144)
    st = ec.verify_statement(b, pub, sig, msg, flag=True, vote_format=fmt)
    assert [b.value(v) for v in st["height_words"]] == [4_000_123, 7] and [b.value(v) for v in st["round_words"]] == [3, 0]
    assert bytes(b.value(v) for v in st["msg_bytes"]) == msg.ljust(fmt.max_len, b"\0") and b.value(st["length"]) == len(msg)
    # refused while the format constraints are laid down (validly signed bytes): a second prefix byte that is not 1, the round's tag missing
    for pos, byte in ((1, 2), (fmt.prefix_len + 11, 0x18)):
        bad = bytearray(msg)
        bad[pos] = byte
        pub2, sig2 = ec.keypair_and_sign(bytes(32), bytes(bad))
        with pytest.raises(ValueError):
            ec.verify_statement(rec.CircuitBuilder(object(), n_wires=144, n_routed=144), pub2, sig2, bytes(bad), flag=True, vote_format=fmt)
