"""Adversarial Ed25519 inputs for the witness kernel and the in-circuit verifier (a helper module, not a conftest).

Everything here is built on the arithmetic of oracle/ed25519_oracle.py (Python integers, pinned by OpenSSL and RFC 8032 vectors) and hashlib:
an RFC 8032 §5.1.6 signer, a derived generator T8 of the 8-torsion, the expected 37-word record of a triple, and five families of
(pub, sig, msg) triples with fixed seeds.  The package's own signer appears once, as a cross-check of it."""
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ed25519_oracle as edo  # noqa: E402

p, L = edo.p, edo.L
REC = 37
B = (edo.Bx, edo.By)
IDENTITY = (0, 1)


# ---- points ----------------------------------------------------------------------------------------------------------------------------------
def encode(point):
    """RFC 8032 §5.1.2: y little-endian with the parity of x in the top bit"""
    return (point[1] | ((point[0] & 1) << 255)).to_bytes(32, "little")


def encode_y(y, sign):
    """any 255-bit y, canonical or not, with a sign bit"""
    assert 0 <= y < 1 << 255
    return (y | (sign << 255)).to_bytes(32, "little")


def mul(s, point):
    return edo._affine(edo._mul(s, edo._ext(point)))


def add(P1, P2):
    return edo._affine(edo._add(edo._ext(P1), edo._ext(P2)))


def hash_k(R32, A32, msg):
    return int.from_bytes(hashlib.sha512(R32 + A32 + msg).digest(), "little") % L


# ---- RFC 8032 §5.1.5 / §5.1.6 ------------------------------------------------------------------------------------------------------------------
def secret_of(seed32):
    """(the clamped scalar a, the nonce prefix) of a 32-byte seed"""
    h = hashlib.sha512(bytes(seed32)).digest()
    return (int.from_bytes(h[:32], "little") & ((1 << 254) - 8)) | (1 << 254), h[32:]


def sign(seed32, msg):
    """(public key, signature)"""
    a, prefix = secret_of(seed32)
    A = encode(mul(a, B))
    r = int.from_bytes(hashlib.sha512(prefix + bytes(msg)).digest(), "little") % L
    R = encode(mul(r, B))
    return A, R + ((r + hash_k(R, A, bytes(msg)) * a) % L).to_bytes(32, "little")


_checked = {}


def check_signer():
    """once per process: the oracle accepts the signer's output, and the package's keypair_and_sign gives the same bytes for one seed"""
    if "signer" not in _checked:
        seed, msg = hashlib.sha256(b"ed25519_cases signer").digest(), b"cross-check of the two signers"
        pub, sig = sign(seed, msg)
        assert edo.verify(pub, msg, sig)
        import __graft_entry__ as graft
        graft.load_package()
        ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
        assert ec.keypair_and_sign(seed, msg) == (pub, sig)
        _checked["signer"] = True


# ---- the 8-torsion ---------------------------------------------------------------------------------------------------------------------------------
T8_MULTIPLES_HEX = [
    "0100000000000000000000000000000000000000000000000000000000000000",
    "c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a",
    "0000000000000000000000000000000000000000000000000000000000000080",
    "26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05",
    "ecffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
    "26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc85",
    "0000000000000000000000000000000000000000000000000000000000000000",
    "c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac03fa",
]


def _derive_t8():
    y = 2
    while True:
        P0 = edo.decode_point(y.to_bytes(32, "little"))
        if P0 is not None:
            T = mul(L, P0)                                                      # the torsion component of P0
            if mul(4, T) != IDENTITY:                                           # of order exactly 8
                return T
        y += 1


T8 = _derive_t8()
TORSION = [mul(j, T8) for j in range(8)]
assert [encode(T).hex() for T in TORSION] == T8_MULTIPLES_HEX
assert mul(8, T8) == IDENTITY and all(edo.decode_point(encode(T)) == T for T in TORSION)


# ---- expected records -------------------------------------------------------------------------------------------------------------------------
def _words(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


_records = {}


def expected_record(pub, sig, msg):
    """the 37 words the kernel must write: [0] verdict [1..4] k [5..12] A [13..20] R [21..28] P1 [29..36] P2; zero wherever the oracle has no
    value (a point that does not decode; k, P1, P2 unless both points decode and S < L).  Cached: the oracle runs once per triple and process."""
    key = (bytes(pub), bytes(sig), bytes(msg))
    rec = _records.get(key)
    if rec is None:
        w = edo.witness(key[0], key[2], key[1])
        rec = [0] * REC
        rec[0] = 1 if w["valid"] else 0
        for name, off in (("A", 5), ("R", 13)):
            if w[name] is not None:
                rec[off:off + 8] = _words(w[name][0]) + _words(w[name][1])
        if w["P1"] is not None:
            rec[1:5] = _words(w["k"])
            rec[21:29] = _words(w["P1"][0]) + _words(w["P1"][1])
            rec[29:37] = _words(w["P2"][0]) + _words(w["P2"][1])
        else:
            assert w["k"] == 0 and w["P2"] is None and not w["valid"]
        _records[key] = rec
    return rec


def exit_class(pub, sig, msg):
    """which return of the kernel a row with an in-range length takes: 'decode', 's_ge_l' or 'full'"""
    if edo.decode_point(pub) is None or edo.decode_point(sig[:32]) is None:
        return "decode"
    return "full" if int.from_bytes(sig[32:], "little") < L else "s_ge_l"


# ---- families ---------------------------------------------------------------------------------------------------------------------------------
_families = {}


def _cached(fn):
    def wrapper():
        if fn.__name__ not in _families:
            check_signer()
            _families[fn.__name__] = fn()
        return list(_families[fn.__name__])
    wrapper.__name__ = fn.__name__
    wrapper.__doc__ = fn.__doc__
    return wrapper


BOUNDARY_LENGTHS = [0, 1, 46, 47, 48, 49, 63, 64, 65, 174, 175, 176, 177, 303, 304]      # both sides of every SHA-512 block boundary of R || A || M


@_cached
def family_a():
    """64 valid signatures: every boundary length, then random lengths below 200"""
    rng = np.random.default_rng(1)
    lengths = BOUNDARY_LENGTHS + [int(v) for v in rng.integers(0, 200, 64 - len(BOUNDARY_LENGTHS))]
    out = []
    for n in lengths:
        seed, msg = rng.bytes(32), rng.bytes(n)
        pub, sig = sign(seed, msg)
        out.append((pub, sig, msg))
    assert len(out) == 64 and all(edo.verify(pub, msg, sig) for pub, sig, msg in out)
    return out


@_cached
def family_b():
    """256 triples with random 32-byte strings as A and R, S random below L, a random message"""
    rng = np.random.default_rng(2)
    out = []
    for _ in range(256):
        pub, R = rng.bytes(32), rng.bytes(32)
        S = int.from_bytes(rng.bytes(40), "little") % L
        out.append((pub, R + S.to_bytes(32, "little"), rng.bytes(int(rng.integers(0, 100)))))
    classes = [(edo.decode_point(pub) is not None, edo.decode_point(sig[:32]) is not None) for pub, sig, _ in out]
    for c in ((True, True), (True, False), (False, True), (False, False)):
        assert classes.count(c) >= 32, (c, classes.count(c))                       # expectation 64, sigma 6.9: 32 is 4.6 sigma below
    return out


EDGE_Y = ([0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, (1 << 26) - 1, 1 << 26, (1 << 51) - 1, 1 << 51,
           (1 << 254) - 1, 1 << 254, (1 << 255) - 1 - (1 << 26)] + [p + j for j in range(19)])       # p + 18 = 2^255 - 1: every non-canonical y


@_cached
def family_c():
    """every edge y, with both sign bits, in the place of A and in the place of R of a valid triple"""
    msg = b"edge y values"
    pub, sig = sign(hashlib.sha256(b"family c").digest(), msg)
    out = []
    for y in EDGE_Y:
        for s in (0, 1):
            e = encode_y(y, s)
            out.append((e, sig, msg))
            out.append((pub, e + sig[32:], msg))
    assert len(out) == 4 * 35
    return out


TORSION_S = [0, 1, 2, L - 2, L - 1, (1 << 252) - 1, 1 << 252]


@_cached
def torsion_groups():
    """[(i, S, [triple for j in 0, 1, 2])]: A = [i]T8, R = [S]B + [j]T8.  Valid exactly when j + k i = 0 (mod 8): the oracle says which"""
    out = []
    for i, A in enumerate(TORSION):
        for si, S in enumerate(TORSION_S):
            SB = mul(S, B)
            msg = b"torsion key %d, scalar %d" % (i, si)
            out.append((i, S, [(encode(A), encode(add(SB, TORSION[j])) + S.to_bytes(32, "little"), msg) for j in range(3)]))
    return out


MIXED_TORSION = [(1, 3), (3, 5), (2, 4), (4, 4), (7, 1), (5, 0)]                  # (tA, tR): each pair admits k with tR + k tA = 0 (mod 8)


@_cached
def mixed_order():
    """[(triple, cofactorless_valid)]: A = [a]B + [tA]T8, R = [r]B + [tR]T8, S = r + k a.  [8][S]B = [8]R + [8][k]A always holds (the cofactored
    check passes); the RFC's cofactorless equation holds exactly when tR + k tA = 0 (mod 8).  The message counter is ground for one of each kind
    per (tA, tR)"""
    out = []
    for n, (tA, tR) in enumerate(MIXED_TORSION):
        a, prefix = secret_of(hashlib.sha256(b"mixed order %d" % n).digest())
        A = encode(add(mul(a, B), TORSION[tA]))
        found = {}
        counter = 0
        while len(found) < 2:
            msg = b"mixed-order key %d, message %d" % (n, counter)
            counter += 1
            r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
            R = encode(add(mul(r, B), TORSION[tR]))
            k = hash_k(R, A, msg)
            kind = (tR + k * tA) % 8 == 0
            if kind not in found:
                found[kind] = (A, R + ((r + k * a) % L).to_bytes(32, "little"), msg)
        out += [(found[True], True), (found[False], False)]
    for (pub, sig, msg), kind in out:
        assert edo.verify(pub, msg, sig) == kind
        w = edo.witness(pub, msg, sig)                                          # ... and the cofactored equation holds for both kinds
        assert mul(8, w["P1"]) == add(mul(8, w["R"]), mul(8, w["P2"]))
    assert sum(kind for _, kind in out) >= 3 and sum(not kind for _, kind in out) >= 3
    return out


@_cached
def family_d():
    """torsion keys and mixed-order keys"""
    out = [t for _, _, group in torsion_groups() for t in group] + [t for t, _ in mixed_order()]
    verdicts = [edo.verify(pub, msg, sig) for pub, sig, msg in out]
    assert any(verdicts) and not all(verdicts)
    return out


@_cached
def family_e():
    """the S edges on one valid signature"""
    msg = b"edges of the scalar S"
    pub, sig = sign(hashlib.sha256(b"family e").digest(), msg)
    S =int.from_bytes(sig[32:], "little")
    edges = [L - 1, L, L + 1, S + L, (1 << 253) - 1, 1 << 253, 1 << 255, (1 << 256) - 1, S | (1 << 255), 0]
    return [(pub, sig[:32] + v.to_bytes(32, "little"), msg) for v in edges]


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}


def all_triples():
    return [t for name in "abcde" for t in FAMILIES[name]()]


SHUFFLE_SEED = 1            # the first seed of numpy's default_rng for which shuffled_rows' assertion on the blocks holds


def shuffled_rows(seed=None):
    """(triples, overlong): every family, shuffled with a fixed seed, for launches in which the lanes of each wavefront leave the kernel at
    different exits.  overlong[i] says that the test gives row i a length beyond the row stride (every 16th row: such a row's record is all
    zero).  The families hold only eight rows that decode and have S >= L — fewer than there are wavefronts —, so family A's 64 signatures are
    added once more with S + L in the place of S.  Asserted here: n is no multiple of 64, and every block of 64 consecutive rows (the last,
    shorter one included) holds all four exits: over-long length, decode failure, S >= L, the full path."""
    key = ("shuffled", SHUFFLE_SEED if seed is None else seed)
    if key not in _families:
        rows = all_triples()
        for pub, sig, msg in family_a():
            rows.append((pub, sig[:32] + (int.from_bytes(sig[32:], "little") + L).to_bytes(32, "little"), msg))
        order = np.random.default_rng(key[1]).permutation(len(rows))
        rows = [rows[int(i)] for i in order]
        overlong = [i % 16 == 7 for i in range(len(rows))]
        assert len(rows) % 64 != 0
        for lo in range(0, len(rows), 64):
            exits = {"overlong" if overlong[i] else exit_class(*rows[i]) for i in range(lo, min(lo + 64, len(rows)))}
            assert exits == {"overlong", "decode", "s_ge_l", "full"}, (lo, exits)
        _families[key] = (rows, overlong)
    rows, overlong = _families[key]
    return list(rows), list(overlong)


def marshal(triples):
    """(pubs [n][32], sigs [n][64], msgs [n][stride], lens [n], stride) as the kernel's ABI takes them"""
    n = len(triples)
    stride = max(1, max(len(m) for _, _, m in triples))
    pubs, sigs = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint8)
    msgs, lens = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    for i, (pub, sig, msg) in enumerate(triples):
        pubs[i], sigs[i] = np.frombuffer(pub, dtype=np.uint8), np.frombuffer(sig, dtype=np.uint8)
        msgs[i, :len(msg)] = np.frombuffer(msg, dtype=np.uint8)
        lens[i] = len(msg)
    return pubs, sigs, msgs, lens, stride


def assert_records(triples, out, expected=None):
    """every record equals the expected one on all 37 words (expected: a list that overrides expected_record, for rows whose length the test
    made over-long)"""
    assert len(out) == len(triples)
    for i, (pub, sig, msg) in enumerate(triples):
        want = expected_record(pub, sig, msg) if expected is None else expected[i]
        got = [int(v) for v in out[i]]
        if got != want:
            bad = [k for k in range(REC) if got[k] != want[k]]
            raise AssertionError(f"row {i} (A {pub.hex()}, sig {sig.hex()}, {len(msg)}-byte message): words {bad} differ; "
                                 f"got {[hex(got[k]) for k in bad]}, want {[hex(want[k]) for k in bad]}")
