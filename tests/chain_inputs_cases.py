"""Cases and references shared by tests/test_emu_chain_inputs.py (the kernels on the CPU) and tests/test_gpu_chain_inputs.py (the C ABI on the
device): calls of the batched Tendermint tree with their roots by a recursive hashlib restatement, and header chains with the rows
data_commitment_mr._chain_leaf_inputs builds, the hashes HeaderChainMapReduce.header_hash gives and the status _map_chain's tests imply.
Everything is built once per process (functools.lru_cache) and never changed."""
import functools
import hashlib
import importlib
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

dcm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
bs = importlib.import_module(graft.PKG_NAME + ".blobstream")

OK, BAD_LINK, BAD_HEIGHT, BAD_DATA_FIELD = 0, 1, 2, 3
MAX_LEAVES = 512
LEAF_COUNTS = (0, 1, 2, 3, 5, 7, 8, 9, 14, 100, 127, 128, 129, MAX_LEAVES)
# the hashed message is 00 || leaf: 54 fills one block to the last byte that leaves room for the padding, 55 and 56 spill into a second block,
# 118 / 119 / 120 do the same at two blocks, 300 takes five
LEAF_LENS = (0, 1, 54, 55, 56, 118, 119, 120, 300)
FIELD_LENGTHS = (4, 12, 5, 13, 72, 34, 34, 34, 34, 34, 34, 34, 34, 22)
SENTINEL = 0x5E5E5E5E5E5E5E5E


def tm_root(items):
    """RFC 6962 / Tendermint simple tree by recursion (split at the largest power of two below n)"""
    if not items:
        return hashlib.sha256(b"").digest()
    if len(items) == 1:
        return hashlib.sha256(b"\x00" + items[0]).digest()
    k = 1 << ((len(items) - 1).bit_length() - 1)
    return hashlib.sha256(b"\x01" + tm_root(items[:k]) + tm_root(items[k:])).digest()


class TreeCall:
    """one call: trees (lists of leaves), the flat arrays the C form takes, the expected roots"""

    def __init__(self, name, trees):
        self.name, self.trees = name, trees
        leaves = [x for t in trees for x in t]
        self.data = np.frombuffer(b"".join(leaves), dtype=np.uint8).copy()
        self.offs = np.zeros(len(leaves) + 1, dtype=np.uint64)
        self.offs[1:] = np.cumsum([len(x) for x in leaves])
        self.first = np.zeros(len(trees) + 1, dtype=np.uint64)
        self.first[1:] = np.cumsum([len(t) for t in trees])
        self.total, self.B = len(leaves), len(trees)
        self.roots = [tm_root(t) for t in trees]


def _leaves(rng, count, lens, at=0):
    return [rng.randbytes(lens[(at + i) % len(lens)]) for i in range(count)]


@functools.lru_cache(maxsize=None)
def tree_calls():
    rng = random.Random(20261020)
    calls = [TreeCall(f"B1-n{c}", [_leaves(rng, c, LEAF_LENS, c)]) for c in LEAF_COUNTS]
    calls += [TreeCall(f"B1-len{ln}", [_leaves(rng, 3, (ln,))]) for ln in LEAF_LENS]
    calls.append(TreeCall("B2", [_leaves(rng, 129, LEAF_LENS), _leaves(rng, 5, LEAF_LENS, 4)]))          # 256 lanes, a small tree beside a big one
    calls.append(TreeCall("B65", [_leaves(rng, LEAF_COUNTS[(5 * t + 1) % 12], LEAF_LENS, t) for t in range(65)]))     # up to 128 leaves: 64 lanes
    calls.append(TreeCall("B130", [_leaves(rng, LEAF_COUNTS[(5 * t + 1) % 9], LEAF_LENS, t) for t in range(130)]))
    calls.append(TreeCall("B3-max", [_leaves(rng, 2, (40,)), _leaves(rng, MAX_LEAVES, (1, 54, 55)), []]))
    return calls


def refused_tree_calls():
    """(name, data_len, offs, first, total, B, expected return code)"""
    ok_offs, ok_first = np.array([0, 2, 4, 10], dtype=np.uint64), np.array([0, 1, 3], dtype=np.uint64)
    big = MAX_LEAVES + 1
    return [("descending offsets", 10, np.array([0, 4, 2, 10], dtype=np.uint64), ok_first, 3, 2, -1),
            ("tree_first does not end at total_leaves", 10, ok_offs, np.array([0, 1, 2], dtype=np.uint64), 3, 2, -1),
            ("tree_first descends", 10, ok_offs, np.array([0, 4, 3], dtype=np.uint64), 3, 2, -1),
            ("last offset past data_len", 9, ok_offs, ok_first, 3, 2, -1),
            ("a tree over the maximum", 10, np.zeros(big + 1, dtype=np.uint64), np.array([0, big], dtype=np.uint64), big, 1, -5)]


# ---- chains ----
def varint_field(value, n_bytes=None):
    """08 || varint(value); n_bytes: padded to that many varint bytes by continuation groups of zero (a NON-minimal encoding)"""
    v = bs.encode_varint(value)
    if n_bytes is not None and len(v) < n_bytes:
        v = bytes(b | 0x80 for b in v) + bytes([0x80] * (n_bytes - len(v) - 1)) + b"\x00"
    return b"\x08" + v


def make_chain(rng, field_lengths, n, first_height, start):
    """n headers with random opaque bytes and real links, heights and data-hash prefixes"""
    prev, out = bytes(start), []
    for k in range(n):
        f = [rng.randbytes(ln) for ln in field_lengths]
        f[2] = varint_field(first_height + k)
        f[4] = b"\x0a\x20" + prev + f[4][34:]
        f[6] = b"\x0a\x20" + f[6][2:]
        assert len(f[2]) == field_lengths[2]
        out.append(f)
        prev = dcm.HeaderChainMapReduce.header_hash(f)
    return out


def relink(headers, start, frm):
    """headers[frm:] linked again to the hashes of what now precedes them (a tampered header changes its own hash)"""
    prev = bytes(start) if frm == 0 else dcm.HeaderChainMapReduce.header_hash(headers[frm - 1])
    for k in range(frm, len(headers)):
        headers[k][4] = b"\x0a\x20" + prev + headers[k][4][34:]
        prev = dcm.HeaderChainMapReduce.header_hash(headers[k])


TAMPERS = ("link-bit", "link-prefix", "height+1", "varint-nonminimal", "varint-overlong", "data-prefix")


def tamper(headers, start, first_height, at, kind, n_groups):
    """one tamper on header `at`; the headers behind it are linked to the tampered header's hash, so only header `at` is refused.  Returns the
    status expected at `at`."""
    f = headers[at]
    if kind == "link-bit":
        b = bytearray(f[4]); b[2 + 17] ^= 0x10; f[4] = bytes(b)
        want = BAD_LINK
    elif kind == "link-prefix":
        f[4] = b"\x0a\x21" + f[4][2:]
        want = BAD_LINK
    elif kind == "height+1":
        f[2] = varint_field(first_height + at + 1)
        want = BAD_HEIGHT
    elif kind == "varint-nonminimal":                  # the height with one group less, padded back by a zero group: same value, other bytes
        f[2] = varint_field((first_height + at) & ((1 << (7 * (n_groups - 1))) - 1), n_groups)
        want = BAD_HEIGHT
    elif kind == "varint-overlong":                    # a continuation bit on the last byte: the varint runs past the field
        b = bytearray(f[2]); b[-1] |= 0x80; f[2] = bytes(b)
        want = BAD_HEIGHT
    elif kind == "data-prefix":
        f[6] = b"\x0a\x21" + f[6][2:]
        want = BAD_DATA_FIELD
    else:
        raise ValueError(kind)
    assert len(f[2]) == len(headers[0][2])
    relink(headers, start, at + 1)
    return want


def python_status(headers, hashes, first_height, k):
    """what _map_chain's two tests say of header k (hashes[k] = the hash before it), as the status the device reports"""
    f = headers[k]
    if bytes(f[4])[:34] != b"\x0a\x20" + hashes[k]:
        return BAD_LINK
    if bytes(f[2]) != b"\x08" + bs.encode_varint(first_height + k):
        return BAD_HEIGHT
    if bytes(f[6])[:2] != b"\x0a\x20":
        return BAD_DATA_FIELD
    return OK


class ChainCase:
    """a chain with what the Python path makes of it: hashes [n + 1], status [n], rows [n / B][width] (zero where a header of the leaf is
    refused)"""

    def __init__(self, name, field_lengths, leaf_headers, n_groups, first_height, headers, start):
        self.name, self.field_lengths, self.B, self.g, self.first, self.headers, self.start = name, tuple(field_lengths), leaf_headers, n_groups, first_height, headers, bytes(start)
        self.n = len(headers)
        self.blob = np.frombuffer(b"".join(bytes(x) for h in headers for x in h), dtype=np.uint8).copy()
        self.hashes = [self.start] + [dcm.HeaderChainMapReduce.header_hash(h) for h in headers]
        self.status = np.array([python_status(headers, self.hashes, first_height, k) for k in range(self.n)], dtype=np.int32)
        rows = []
        for lo in range(0, self.n, leaf_headers):
            if self.status[lo:lo + leaf_headers].any():
                rows.append(None)
            else:
                rows.append(dcm._chain_leaf_inputs(self.hashes[lo], first_height + lo, headers[lo:lo + leaf_headers], n_groups))
        self.width = next(len(r) for r in rows if r is not None) if any(r is not None for r in rows) else None
        self.rows = rows

    def rows_array(self, width):
        return np.array([r if r is not None else [0] * width for r in self.rows], dtype=np.uint64).reshape(len(self.rows), width)


# varint byte counts 1, 2 and 4 with heights at both ends of each: the chain is placed so that its first or its last header has the edge height
HEIGHT_EDGES = ((1, 0, "lo"), (1, 127, "hi"), (2, 128, "lo"), (2, 16383, "hi"), (4, 1 << 21, "lo"), (4, (1 << 28) - 1, "hi"))


def _lengths(g):
    fl = list(FIELD_LENGTHS)
    fl[2] = 1 + g
    return tuple(fl)


@functools.lru_cache(maxsize=None)
def good_chains():
    rng = random.Random(7)
    out = []
    for g, edge, side in HEIGHT_EDGES:
        for B in (1, 2, 8):
            for leaves in (1, 2, 3):
                if (B, leaves) not in ((1, 1), (1, 3), (2, 2), (8, 1), (8, 3)) and g != 4:
                    continue                                   # every (B, leaves) pair at 4 varint bytes, a spread of them at 1 and 2
                n = B * leaves
                first = edge if side == "lo" else edge - (n - 1)
                start = rng.randbytes(32)
                out.append(ChainCase(f"g{g}-{side}-B{B}-L{leaves}", _lengths(g), B, g, first, make_chain(rng, _lengths(g), n, first, start), start))
    return out


@functools.lru_cache(maxsize=None)
def nonminimal_chain():
    """heights 100 .. 103 under a 2-byte layout: every height field spells the RIGHT height in two groups (e4 00 ...), which is not the canonical
    varint — only the test of the top group can refuse it.  Every header is BAD_HEIGHT, both rows are zero."""
    rng = random.Random(13)
    start, first, fl = rng.randbytes(32), 100, _lengths(2)
    prev, headers = start, []
    for k in range(4):
        f = [rng.randbytes(ln) for ln in fl]
        f[2] = varint_field(first + k, 2)
        f[4] = b"\x0a\x20" + prev + f[4][34:]
        f[6] = b"\x0a\x20" + f[6][2:]
        headers.append(f)
        prev = dcm.HeaderChainMapReduce.header_hash(f)
    c = ChainCase("g2-nonminimal-all", fl, 2, 2, first, headers, start)
    assert c.status.tolist() == [BAD_HEIGHT] * 4 and bytes(headers[0][2]) == b"\x08\xe4\x00"
    return c


@functools.lru_cache(maxsize=None)
def truncated_chains():
    """the first height that no longer FITS the layout's varint bytes, on the last header of the last leaf of three: 16384 under the 2-byte
    layout with the field 08 80 00, 128 under the 1-byte layout with 08 00 — the low groups of the height, every per-group comparison agrees,
    and only the test that nothing lies above the top group can refuse it (encode_varint gives three and two bytes).  BAD_HEIGHT at that
    header, a zero row for its leaf, the two leaves before it untouched."""
    rng = random.Random(17)
    out = []
    for g, B in ((2, 2), (1, 2)):
        limit, n, fl = 1 << (7 * g), 3 * B, _lengths(g)
        first, start = limit - (n - 1), rng.randbytes(32)
        headers = make_chain(rng, fl, n - 1, first, start)
        f = [rng.randbytes(ln) for ln in fl]
        f[2] = b"\x08" + bytes([0x80] * (g - 1)) + b"\x00"                 # the g low groups of `limit`: all zero
        f[4] = b"\x0a\x20" + dcm.HeaderChainMapReduce.header_hash(headers[-1]) + f[4][34:]
        f[6] = b"\x0a\x20" + f[6][2:]
        headers.append(f)
        c = ChainCase(f"g{g}-truncated-{limit}", fl, B, g, first, headers, start)
        assert first + n - 1 == limit and c.status.tolist() == [OK] * (n - 1) + [BAD_HEIGHT] and [r is None for r in c.rows] == [False, False, True]
        out.append(c)
    assert bytes(out[0].headers[-1][2]) == b"\x08\x80\x00" and bytes(out[1].headers[-1][2]) == b"\x08\x00"
    return out


@functools.lru_cache(maxsize=None)
def tampered_chains():
    """every tamper on the first, a middle and the last header of the MIDDLE leaf of three (8-header leaves at 4 varint bytes; 2-header leaves
    at 2 varint bytes, where first and middle coincide with the leaf's two headers)"""
    rng = random.Random(11)
    out = []
    for g, B, first in ((4, 8, 1 << 21), (2, 2, 300)):
        for kind in TAMPERS:
            for at in sorted({B, B + B // 2, 2 * B - 1}):
                start = rng.randbytes(32)
                headers = make_chain(rng, _lengths(g), 3 * B, first, start)
                want = tamper(headers, start, first, at, kind, g)
                c = ChainCase(f"g{g}-B{B}-{kind}@{at}", _lengths(g), B, g, first, headers, start)
                assert c.status.tolist() == [want if k == at else OK for k in range(3 * B)], c.name
                assert [r is None for r in c.rows] == [False, True, False], c.name
                out.append(c)
    return out
