"""Cases and references shared by tests/test_emu_ed25519_inputs.py (the kernels on the CPU) and tests/test_gpu_ed25519_inputs.py (the C ABI on
the device): the scalars of the half-size reduction with what ed25519_circuit.half_size_pair makes of them, and slot batches of the three forms
of ed25519_circuit.witness_inputs with their expected rows and statuses.  The reference is the project's own Python, nothing here computes
an expectation another way.  Everything is built once per process (functools.lru_cache) and never changed."""
import functools
import importlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as graft  # noqa: E402
import ed25519_oracle as edo  # noqa: E402

ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
ELL = ec.ELL
OK, REJECT, NO_PAIR, INVALID = 0, 1, 2, 3
PLAIN, FLAGGED, VOTE = 0, 1, 2
EDGE_LENGTHS = (47, 48, 111, 112, 175)            # SHA-512 of R || A || M changes its block count at 47 -> 48 and 175 -> 176


class Window:
    """the two fields of a blobstream.VoteFormat that witness_inputs reads (a VoteFormat itself refuses windows below 48 bytes)"""

    def __init__(self, min_len, max_len):
        self.min_len, self.max_len = min_len, max_len


def words4(k):
    return [(k >> (64 * j)) & (2**64 - 1) for j in range(4)]


@functools.lru_cache(maxsize=None)
def half_scalar_cases():
    """(ks [n][4] u64, expected [n][8] u64: u[3] v[3] neg status)"""
    rng = random.Random(20261020)
    ks = [0, 1, 2, 3, 1 << 126, (1 << 127) + 1, 1 << 200, ELL - 3, ELL - 1, ELL - 2, (ELL + 1) // 2, ELL, (1 << 256) - 1]
    ks += [rng.randrange(ELL) for _ in range(500)]
    want = np.zeros((len(ks), 8), dtype=np.uint64)
    for i, k in enumerate(ks):
        if k >= ELL:
            want[i, 7] = INVALID
            continue
        try:
            u, v, neg = ec.half_size_pair(k)
        except ValueError:
            want[i, 7] = NO_PAIR
            continue
        want[i, :3], want[i, 3:6], want[i, 6] = words4(u)[:3], words4(v)[:3], int(neg)
    return np.array([words4(k) for k in ks], dtype=np.uint64), want, ks


class Batch:
    """one call's worth of slots: the arrays glp_ed25519_leaf_inputs takes, and rows / status as witness_inputs gives them"""

    def __init__(self, name, form, lo, hi, split, slots, dummy=None, fmt=None):
        self.name, self.form, self.lo, self.hi, self.split = name, form, lo, hi, int(bool(split))
        n = self.n = len(slots)
        self.stride = max(1, max(len(s[2]) for s in slots))
        self.pubs, self.sigs = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint8)
        self.msgs, self.lens = np.zeros((n, self.stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
        self.flags = np.zeros(n, dtype=np.uint8)
        self.dummy = None if dummy is None else np.frombuffer(b"".join(dummy), dtype=np.uint8).copy()
        head = {PLAIN: 96 + hi, FLAGGED: 1 + 32 + hi + 64, VOTE: 1 + 32 + hi + 1 + (hi - lo + 1) + 64}[form]
        self.width = head + 44 + (38 if split else 0)
        self.rows, self.status = np.zeros((n, self.width), dtype=np.uint64), np.zeros(n, dtype=np.int32)
        for i, (pub, sig, msg, flag) in enumerate(slots):
            self.pubs[i], self.sigs[i] = np.frombuffer(pub, dtype=np.uint8), np.frombuffer(sig, dtype=np.uint8)
            self.msgs[i, :len(msg)], self.lens[i], self.flags[i] = np.frombuffer(msg, dtype=np.uint8), len(msg), int(bool(flag))
            if not lo <= len(msg) <= hi:
                self.status[i] = INVALID
            elif (form == PLAIN or flag) and not edo.verify(pub, msg, sig):
                self.status[i] = REJECT
            else:
                try:
                    row = ec.witness_inputs(pub, sig, msg, None if form == PLAIN else bool(flag), record=None, split_scalars=bool(split),
                                            vote_format=fmt if form == VOTE else None)
                    assert len(row) == self.width, (name, len(row), self.width)
                    self.rows[i] = row
                except ValueError as e:
                    assert "half-size" in str(e), e
                    self.status[i] = NO_PAIR


def signed(seed, msg):
    pub, sig = ec.keypair_and_sign(bytes([seed]) * 32, msg)
    return pub, sig, msg


def vote_like(length, salt):
    return bytes((salt * 31 + 7 * k) & 0xFF for k in range(length))


def forged(slot):
    pub, sig, msg = slot
    s = (int.from_bytes(sig[32:], "little") + 1) % ELL
    return pub, sig[:32] + s.to_bytes(32, "little"), msg


@functools.lru_cache(maxsize=None)
def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "ed25519.json")) as f:
        return [(bytes.fromhex(c["pub"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bool(c["valid"])) for c in json.load(f)["cases"]]


@functools.lru_cache(maxsize=None)
def plain_batches():
    """form (a): every case of tests/golden/ed25519.json, one batch per message length (a program is recorded for one length), split both ways"""
    by_len = {}
    for pub, sig, msg, _ in golden_cases():
        by_len.setdefault(len(msg), []).append((pub, sig, msg, True))
    out = []
    for k, (ln, slots) in enumerate(sorted(by_len.items())):
        out.append(Batch(f"golden-len{ln}", PLAIN, ln, ln, k % 2 == 0, slots))
    ln, slots = max(by_len.items(), key=lambda kv: len(kv[1]))
    out.append(Batch(f"golden-len{ln}-other-split", PLAIN, ln, ln, False, slots))
    return out


@functools.lru_cache(maxsize=None)
def flagged_batches():
    """forms (b) and (c) at the SHA-512 block edges, flags 1 and 0, a forged neighbour; B = 1, 5, 65; a real commit window with three lengths"""
    from importlib import import_module
    bs = import_module(graft.PKG_NAME + ".blobstream")
    out = []
    for n, ln in enumerate(EDGE_LENGTHS):
        a, b = signed(1 + n, vote_like(ln, n)), signed(11 + n, vote_like(ln, n + 5))
        unsigned_ = (b[0], bytes(64), vote_like(ln, n + 9))
        dummy = ec.dummy_signature(ln)
        out.append(Batch(f"b-len{ln}", FLAGGED, ln, ln, n % 2 == 0, [a + (1,), unsigned_ + (0,), b + (1,)], dummy))
        lo, hi = ln - 2, ln + 1
        short = signed(21 + n, vote_like(lo, n))
        out.append(Batch(f"c-len{ln}", VOTE, lo, hi, n % 2 == 1, [a + (1,), unsigned_ + (0,), short + (1,), (b[0], bytes(64), vote_like(hi, 3), 0)],
                         ec.dummy_signature(lo), Window(lo, hi)))
    # B = 1, 5 and 65 (one slot past a 64-lane block) of the 112-byte flagged form; slot 3 of each larger batch carries a forged S
    base = [signed(40 + j, vote_like(112, j)) for j in range(6)]
    for B in (1, 5, 65):
        slots = []
        for i in range(B):
            s = base[i % 6]
            if i == 3:
                slots.append(forged(s) + (1,))
            elif i % 4 == 2:
                slots.append((s[0], bytes(64), s[2], 0))
            else:
                slots.append(s + (1,))
        out.append(Batch(f"b-112-B{B}", FLAGGED, 112, 112, True, slots, ec.dummy_signature(112)))
    # a commit's window: three true lengths in one call, one length outside it
    fmt = bs.VoteFormat.for_commit("celestia", 0)
    lo, hi = fmt.min_len, fmt.max_len
    slots = [signed(60, vote_like(lo, 1)) + (1,), signed(61, vote_like(lo + 3, 2)) + (1,), signed(62, vote_like(hi, 3)) + (1,),
             signed(63, vote_like(hi + 1, 4)) + (1,), (bytes(32), bytes(64), vote_like(lo + 1, 5), 0), signed(64, vote_like(lo - 1, 6)) + (0,)]
    for split in (True, False):
        out.append(Batch(f"c-commit-split{int(split)}", VOTE, lo, hi, split, slots, ec.dummy_signature(lo), fmt))
    assert [b.name for b in out] == FLAGGED_NAMES
    return out


# the names of flagged_batches(), spelled out so that collecting a test module signs nothing
FLAGGED_NAMES = ([f"{form}-len{ln}" for ln in EDGE_LENGTHS for form in "bc"] + [f"b-112-B{B}" for B in (1, 5, 65)]
                 + ["c-commit-split1", "c-commit-split0"])


def flagged_batch(name):
    return next(b for b in flagged_batches() if b.name == name)


def all_batches():
    return plain_batches() + flagged_batches()
