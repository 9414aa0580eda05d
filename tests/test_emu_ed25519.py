"""Row a10 on the CPU emulation: the Ed25519 witness kernel vs the Python big-int oracle
(oracle/ed25519_oracle.py), on OpenSSL-generated and RFC 8032 fixtures (tests/golden/ed25519.json)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_oracle as edo  # noqa: E402
from test_emu_hash import k_tables  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
REC = 37


def load_cases():
    with open(os.path.join(G, "ed25519.json")) as f:
        return json.load(f)["cases"]


def marshal(cases):
    n = len(cases)
    stride = max(1, max(len(bytes.fromhex(c["msg"])) for c in cases))
    pubs = np.zeros((n, 32), dtype=np.uint8)
    sigs = np.zeros((n, 64), dtype=np.uint8)
    msgs = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    for i, c in enumerate(cases):
        m = bytes.fromhex(c["msg"])
        pubs[i] = np.frombuffer(bytes.fromhex(c["pub"]), dtype=np.uint8)
        sigs[i] = np.frombuffer(bytes.fromhex(c["sig"]), dtype=np.uint8)
        msgs[i, :len(m)] = np.frombuffer(m, dtype=np.uint8)
        lens[i] = len(m)
    return pubs, sigs, msgs, lens, stride


def int_of(words):
    return sum(int(w) << (64 * k) for k, w in enumerate(words))


def check_records(cases, out):
    for i, c in enumerate(cases):
        w = edo.witness(bytes.fromhex(c["pub"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]))
        rec = out[i]
        assert bool(rec[0]) == w["valid"] == c["valid"], c["src"]
        for name, off in (("A", 5), ("R", 13)):
            if w[name] is not None:
                assert (int_of(rec[off:off + 4]), int_of(rec[off + 4:off + 8])) == w[name], (c["src"], name)
        if w["P1"] is not None:
            assert int_of(rec[1:5]) == w["k"], c["src"]
            assert (int_of(rec[21:25]), int_of(rec[25:29])) == w["P1"], c["src"]
            assert (int_of(rec[29:33]), int_of(rec[33:37])) == w["P2"], c["src"]


def test_oracle_is_pinned_by_openssl_and_rfc_vectors():
    for c in load_cases():
        assert edo.verify(bytes.fromhex(c["pub"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"])) == c["valid"], c["src"]


def test_emulated_ed25519_witness(emu):
    cases = load_cases()
    pubs, sigs, msgs, lens, stride = marshal(cases)
    _, k512 = k_tables()
    out = np.zeros((len(cases), REC), dtype=np.uint64)
    assert emu.emu_ed25519_witness(pubs.ctypes.data, sigs.ctypes.data, msgs.ctypes.data, stride, lens.ctypes.data, len(cases),
                                   k512.ctypes.data, out.ctypes.data) == 0
    check_records(cases, out)


def test_adversarial_families_every_word(emu):
    """tests/ed25519_cases.py: valid signatures at every SHA-512 block boundary, random byte strings as encodings, edge and non-canonical y,
    torsion and mixed-order points, the edges of S — every record equals the oracle's on all 37 words, zero where the oracle has no value"""
    import ed25519_cases as edc
    _, k512 = k_tables()
    for name in "abcde":
        triples = edc.FAMILIES[name]()
        pubs, sigs, msgs, lens, stride = edc.marshal(triples)
        out = np.full((len(triples), REC), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        assert emu.emu_ed25519_witness(pubs.ctypes.data, sigs.ctypes.data, msgs.ctypes.data, stride, lens.ctypes.data, len(triples),
                                       k512.ctypes.data, out.ctypes.data) == 0
        edc.assert_records(triples, out)


def test_invalid_encodings(emu):
    """non-canonical y, a y with no square root, x = 0 with the sign bit set"""
    base = load_cases()[0]
    bad_pubs = [(2**255 - 19).to_bytes(32, "little"),                   # y = p (non-canonical)
                (2).to_bytes(32, "little"),                              # y = 2: is it on the curve?
                ((1 << 255) | 1).to_bytes(32, "little")]                  # y = 1 -> x = 0, sign = 1: invalid
    cases = [{"src": f"badpub{i}", "pub": b.hex(), "msg": base["msg"], "sig": base["sig"],
              "valid": False} for i, b in enumerate(bad_pubs)]
    pubs, sigs, msgs, lens, stride = marshal(cases)
    _, k512 = k_tables()
    out = np.zeros((len(cases), REC), dtype=np.uint64)
    assert emu.emu_ed25519_witness(pubs.ctypes.data, sigs.ctypes.data, msgs.ctypes.data, stride, lens.ctypes.data, len(cases),
                                   k512.ctypes.data, out.ctypes.data) == 0
    for i, c in enumerate(cases):
        w = edo.witness(bytes.fromhex(c["pub"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]))
        assert not w["valid"] and out[i][0] == 0
        assert (w["A"] is None) == (int_of(out[i][5:9]) == 0 and int_of(out[i][9:13]) == 0), c["src"]
