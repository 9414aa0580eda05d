"""Cases and references shared by tests/test_emu_tm_proofs.py (the kernels on the CPU) and tests/test_gpu_tm_proofs.py (the C ABI on the device).
The reference is a hashlib restatement of the RECURSIVE definitions — RFC 6962 MTH and PATH (split at the largest power of two below n) and
Tendermint's computeHashFromAunts, recalled — and deliberately not the level-wise form the kernels use.  The tree calls are those of
chain_inputs_cases.tree_calls() (B = 1, 2, 65, 130, mixed and empty trees, leaf lengths at the SHA-256 padding edges) plus single trees of 511,
512, 513 (the LDS boundary of the top kernel), 1024, 1025 (the smallest count that needs two level launches before the top kernel) and 4096
leaves.  The negative matrix is built over trees of pairwise DISTINCT leaves: with equal neighbouring leaves a proof legitimately verifies at the
neighbour's index.  Everything is built once per process (functools.lru_cache) and never changed."""
import functools
import hashlib
import random

import numpy as np

import chain_inputs_cases as cic

OK, BAD_SHAPE, BAD_ROOT = 0, 1, 2
BIG_COUNTS = (511, 512, 513, 1024, 1025, 4096)
SENTINEL = 0xEE


def leaf_hash(x):
    return hashlib.sha256(b"\x00" + bytes(x)).digest()


def inner_hash(l, r):
    return hashlib.sha256(b"\x01" + l + r).digest()


def split_point(n):
    return 1 << ((n - 1).bit_length() - 1)


class RefTree:
    """one tree by recursion, subtree roots memoised on (lo, hi)"""

    def __init__(self, leaves):
        self.leaves, self.memo = leaves, {}

    def root(self, lo=0, hi=None):
        hi = len(self.leaves) if hi is None else hi
        if hi == lo:
            return hashlib.sha256(b"").digest()
        if hi - lo == 1:
            return leaf_hash(self.leaves[lo])
        if (lo, hi) not in self.memo:
            k = split_point(hi - lo)
            self.memo[lo, hi] = inner_hash(self.root(lo, lo + k), self.root(lo + k, hi))
        return self.memo[lo, hi]

    def path(self, m, lo=0, hi=None):
        """RFC 6962 PATH(m, D[lo:hi)) in bottom-up order: the path inside the half that holds m, then the other half's root"""
        hi = len(self.leaves) if hi is None else hi
        if hi - lo <= 1:
            return []
        k = split_point(hi - lo)
        if m < k:
            return self.path(m, lo, lo + k) + [self.root(lo + k, hi)]
        return self.path(m - k, lo + k, hi) + [self.root(lo, lo + k)]


def hash_from_aunts(index, total, lh, aunts):
    """Tendermint's computeHashFromAunts, recalled: None = refused"""
    if index >= total or total == 0:
        return None
    if total == 1:
        return lh if not aunts else None
    if not aunts:
        return None
    k = split_point(total)
    if index < k:
        left = hash_from_aunts(index, k, lh, aunts[:-1])
        return None if left is None else inner_hash(left, aunts[-1])
    right = hash_from_aunts(index - k, total - k, lh, aunts[:-1])
    return None if right is None else inner_hash(aunts[-1], right)


def ref_status(root, leaf, index, total, aunts, n_aunts, stride):
    """the verdict on one proof: `aunts` is the whole row (stride entries), n_aunts the proof's own count"""
    if n_aunts > stride:
        return BAD_SHAPE
    got = hash_from_aunts(index, total, leaf_hash(leaf), list(aunts[:n_aunts]))
    if got is None:
        return BAD_SHAPE
    return OK if got == root else BAD_ROOT


def queries_of(trees):
    """every leaf of trees <= 130; the first, last, middle and both sides of the split point of larger ones"""
    out = []
    for t, leaves in enumerate(trees):
        n = len(leaves)
        which = range(n) if n <= 130 else sorted({0, n - 1, n // 2, split_point(n) - 1, split_point(n)})
        out += [(t, i) for i in which]
    return out


class ProofCase:
    """a tree call with its queries and what the reference says of them"""

    def __init__(self, call):
        self.name, self.call, self.trees = call.name, call, call.trees
        self.refs = [RefTree(t) for t in call.trees]
        self.roots = [r.root() for r in self.refs]
        self.queries = queries_of(call.trees)
        self.aunts = [self.refs[t].path(i) for t, i in self.queries]
        self.leaf_hashes = [leaf_hash(call.trees[t][i]) for t, i in self.queries]
        self.max_aunts = max([len(a) for a in self.aunts], default=0)
        self.qt = np.array([q[0] for q in self.queries], dtype=np.uint64)
        self.ql = np.array([q[1] for q in self.queries], dtype=np.uint64)

    def aunts_array(self, stride):
        out = np.zeros((len(self.queries), stride, 32), dtype=np.uint8)
        for q, a in enumerate(self.aunts):
            for k, x in enumerate(a):
                out[q, k] = np.frombuffer(x, dtype=np.uint8)
        return out


def distinct_leaves(rng, count, lens, tag):
    """leaves whose first bytes spell (tag, i): pairwise distinct within a call whatever the random rest is"""
    out = []
    for i in range(count):
        ln = max(3, lens[i % len(lens)])
        out.append(bytes([tag, i & 0xFF, i >> 8]) + rng.randbytes(ln - 3))
    return out


@functools.lru_cache(maxsize=None)
def proof_cases():
    rng = random.Random(20261021)
    calls = list(cic.tree_calls())
    calls += [cic.TreeCall(f"big-n{c}", [distinct_leaves(rng, c, (64,) if c > 600 else cic.LEAF_LENS, 0)]) for c in BIG_COUNTS]
    # a wide tree beside small ones: the small ones sit the level launches out, the empty one has only its root
    calls.append(cic.TreeCall("B4-wide", [distinct_leaves(rng, 2, (40,), 1), distinct_leaves(rng, 1025, (3, 55), 2), [], distinct_leaves(rng, 7, (1, 54), 3)]))
    cases = [ProofCase(c) for c in calls]
    for c in cases:                                            # the recursive tree agrees with chain_inputs_cases' own recursion
        assert c.roots == c.call.roots, c.name
    return cases


def case(name):
    return next(c for c in proof_cases() if c.name == name)


TAMPERS = ("valid", "aunt-bit", "leaf-bit", "root-bit", "index-neighbour", "total+1", "total-1", "n_aunts+1", "n_aunts-1", "n_aunts>stride",
           "index>=total", "total=0", "inner-node-as-leaf")


class NegativeMatrix:
    """every tamper on every leaf of small trees of distinct leaves (1, 2, 3, 5, 8, 13 leaves) and on five leaves of a 513-leaf tree: the arrays
    glp_tm_verify_inclusion_batch takes and the reference's verdict on each proof.  A tampered root is a further entry of the root array."""

    def __init__(self):
        rng = random.Random(77)
        self.trees = [distinct_leaves(rng, c, (3, 54, 55, 64, 120), t) for t, c in enumerate((1, 2, 3, 5, 8, 13, 513))]
        refs = [RefTree(t) for t in self.trees]
        self.roots = [r.root() for r in refs]
        self.stride = 11                                       # ceil(log2 513) = 10, and one slot to spare
        self.kind, self.leaves, self.index, self.total, self.n_aunts, self.root_of, rows, self.want = [], [], [], [], [], [], [], []
        for t, i in queries_of(self.trees):
            n, path = len(self.trees[t]), refs[t].path(i)
            for kind in TAMPERS:
                leaf, idx, tot, aunts, cnt, ro = self.trees[t][i], i, n, list(path), len(path), t
                if kind == "aunt-bit":
                    if not aunts:
                        continue
                    k = rng.randrange(len(aunts))
                    aunts[k] = _flip(aunts[k], rng)
                elif kind == "leaf-bit":
                    leaf = _flip(leaf, rng)
                elif kind == "root-bit":
                    ro = len(self.roots)
                    self.roots.append(_flip(self.roots[t], rng))
                elif kind == "index-neighbour":
                    if n == 1:
                        continue
                    idx = i + 1 if i + 1 < n else i - 1
                elif kind == "total+1":
                    tot = n + 1
                elif kind == "total-1":
                    tot = n - 1
                elif kind == "n_aunts+1":
                    cnt += 1
                elif kind == "n_aunts-1":
                    if cnt == 0:
                        continue
                    cnt -= 1
                elif kind == "n_aunts>stride":
                    cnt = self.stride + 1 + rng.randrange(3)
                elif kind == "index>=total":
                    idx = n + rng.randrange(3)
                elif kind == "total=0":
                    tot = 0
                elif kind == "inner-node-as-leaf":
                    # the level-1 node above leaves (2j, 2j + 1) offered as leaf j of a tree of ceil(n / 2) leaves, with the path of its parent
                    if i % 2 or i + 1 >= n:
                        continue
                    leaf = leaf_hash(self.trees[t][i]) + leaf_hash(self.trees[t][i + 1])
                    idx, tot, aunts, cnt = i // 2, (n + 1) // 2, aunts[1:], cnt - 1
                row = (aunts + [bytes(32)] * self.stride)[:self.stride]
                self.kind.append(kind); self.leaves.append(leaf); self.index.append(idx); self.total.append(tot); self.n_aunts.append(cnt)
                self.root_of.append(ro); rows.append(row)
                self.want.append(ref_status(self.roots[ro], leaf, idx, tot, row, cnt, self.stride))
        self.aunts = np.frombuffer(b"".join(b"".join(r) for r in rows), dtype=np.uint8).reshape(len(rows), self.stride, 32).copy()
        self.n = len(rows)
        for kind, want in zip(self.kind, self.want):           # what the matrix must show whatever the code under test does
            if kind == "valid":
                assert want == OK
            if kind in ("aunt-bit", "leaf-bit", "root-bit", "inner-node-as-leaf"):
                assert want == BAD_ROOT, kind
            if kind in ("n_aunts+1", "n_aunts-1", "n_aunts>stride", "index>=total", "total=0"):
                assert want == BAD_SHAPE, kind
            if kind == "index-neighbour":
                assert want != OK
        assert set(self.kind) == set(TAMPERS)


def _flip(b, rng):
    b = bytearray(b)
    b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def negative_matrix():
    return NegativeMatrix()
