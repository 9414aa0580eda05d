"""glp_merkle_batch on the CPU (tests/emu_merkle_batch): the three batched Merkle kernel bodies under the product's own launch plan
(csrc/merkle_plan.h), against the oracle's tree, per tree.  Every tree of a batch holds independent random data, so a wrong tree offset
cannot pass.  An emulated fused workgroup is 256 threads meeting at some 10^4 wave barriers and costs seconds, so settings that resolve to
one and the same plan share a run, and the constant kinds and the leaf layouts are varied on the shapes where one run is a few workgroups."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, oracle_merkle, poseidon_consts, ptr, rand_field, u64p

D = os.path.join(ROOT, "tests", "emu_merkle_batch")
DEFAULT = 0xFFFFFFFF
DEFAULT_LOG = 15        # what GLP_MERKLE_FUSE_DEFAULT resolves to (csrc/merkle_plan.h: GLP_MERKLE_FUSE_LOG_MEASURED)
SENTINEL = np.uint64(0x5E5E5E5E5E5E5E5E)

# log_leaves, cap_h, B, leaf_len (B and leaf_len chosen here where the issue's table leaves them open)
SHAPES = [(0, 0, 2, 7), (5, 5, 2, 9), (3, 0, 3, 3), (9, 0, 2, 8), (10, 2, 2, 135), (12, 0, 1, 5), (12, 3, 1, 5)]


@pytest.fixture(scope="module")
def emb():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_merkle_batch.so"))
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.emu_merkle_batch.argtypes = [u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_uint32, u64p, ctypes.c_uint64, u64p, u64p, ctypes.c_int, u32p, u32p]
    return lib


def consts384(kind):
    rc, circ, diag = poseidon_consts(kind)
    return np.concatenate([rc, circ, diag]).astype(np.uint64), (rc, circ, diag)


def hand_plan(log_leaves, cap_h, fuse):
    """(launches, fused) worked out from the header comment of glp_merkle_batch alone: one leaf launch; going down from the leaves, a level
    of more than 2^fuse nodes is one launch; from the first level of at most 2^fuse nodes on, launches of up to 9 levels each — as many as
    the slice of min(nodes of the input level, 512) digests has above it — down to the cap"""
    launches, fused, lvl = 1, 0, log_leaves
    while lvl > cap_h:
        if fuse and lvl - 1 <= fuse:
            lvl -= min(9, lvl, lvl - cap_h)
            fused += 1
        else:
            lvl -= 1
        launches += 1
    return launches, fused


# launch counts written down by hand for the table's shapes: {(log_leaves, cap_h): {fuse_max_log: (launches, fused launches)}}; "own" = the
# shape's log_leaves.  The default (fusion from the level of 2^15 nodes) fuses every level of these shapes, as "own" does.
PLANS = {
    (0, 0): {0: (1, 0), 6: (1, 0), "own": (1, 0), "default": (1, 0)},
    (5, 5): {0: (1, 0), 6: (1, 0), "own": (1, 0), "default": (1, 0)},
    (3, 0): {0: (4, 0), 6: (2, 1), "own": (2, 1), "default": (2, 1)},
    (9, 0): {0: (10, 0), 6: (4, 1), "own": (2, 1), "default": (2, 1)},          # 6: levels of 256 and 128 nodes on their own, then 7 levels fused
    (10, 2): {0: (9, 0), 6: (5, 1), "own": (2, 1), "default": (2, 1)},          # own: 8 levels in one launch of two slices per tree
    (12, 0): {0: (13, 0), 6: (7, 1), "own": (3, 2), "default": (3, 2)},         # own: 9 levels, then the last 3 from a slice of 8 digests
    (12, 3): {0: (10, 0), 6: (7, 1), "own": (2, 1), "default": (2, 1)},
}


def test_plan_launch_counts(pkg):
    lib = pkg.load_library()
    for (log_leaves, cap_h), want in PLANS.items():
        for fuse, counts in want.items():
            f = log_leaves if fuse == "own" else None if fuse == "default" else fuse
            assert pkg.Prover.merkle_batch_plan(log_leaves, cap_h, f) == counts, (log_leaves, cap_h, fuse)
            assert hand_plan(log_leaves, cap_h, DEFAULT_LOG if f is None else f) == counts
        assert pkg.Prover.merkle_batch_plan(log_leaves, cap_h) == pkg.Prover.merkle_batch_plan(log_leaves, cap_h, DEFAULT_LOG)
    # the signature leaf's trees (2^19 leaves, cap 4): 16 launches one level at a time; at the default the three widest levels, then 9 + 3 levels fused
    assert pkg.Prover.merkle_batch_plan(19, 4, 0) == (16, 0)
    assert pkg.Prover.merkle_batch_plan(19, 4, 19) == (3, 2)
    assert pkg.Prover.merkle_batch_plan(19, 4) == (6, 2)
    n = ctypes.c_uint32()
    assert lib.glp_merkle_batch_plan(3, 4, 0, ctypes.byref(n), None) == -1        # cap_h > log_leaves
    assert lib.glp_merkle_batch_plan(41, 0, 0, ctypes.byref(n), None) == -1


def run_emu(emb, src, src_tree_stride, poly_major, poly_stride, leaf_len, log_leaves, cap_h, B, fuse, small, digest_tree_stride=None, fill=None):
    nd = 4 * ((2 << log_leaves) - (1 << cap_h))
    stride = nd if digest_tree_stride is None else digest_tree_stride
    dig = np.zeros((B, stride), dtype=np.uint64) if fill is None else np.full((B, stride), fill, dtype=np.uint64)
    caps = np.zeros((B, 1 << cap_h, 4), dtype=np.uint64)
    nl, nf = ctypes.c_uint32(), ctypes.c_uint32()
    c384 = run_emu.c384
    assert emb.emu_merkle_batch(ptr(src), src_tree_stride, poly_major, poly_stride, leaf_len, log_leaves, cap_h, B, fuse, ptr(dig), stride, ptr(caps),
                                ptr(c384), small, ctypes.byref(nl), ctypes.byref(nf)) == 0
    return dig, caps, (nl.value, nf.value)


def effective(fuse, log_leaves, cap_h):
    """two settings with the same value here give the same plan: fusion starts at the level of 2^min(fuse, log_leaves - 1) nodes, and not
    at all when that is the cap level or above it"""
    f = DEFAULT_LOG if fuse == DEFAULT else fuse
    f = min(f, log_leaves - 1)
    return f if f > 0 and f >= cap_h else 0


@pytest.mark.parametrize("log_leaves,cap_h,B,leaf_len", SHAPES)
def test_emulated_merkle_batch(emb, oracle, log_leaves, cap_h, B, leaf_len):
    """every shape under fuse_max_log = 0, 6, its own log_leaves and the default; leaf-major; small constants with the grouped partial rounds"""
    c384, (rc, circ, diag) = consts384("small")
    run_emu.c384 = c384
    oracle.orc_poseidon_set_constants(ptr(rc), ptr(circ), ptr(diag))
    rng = np.random.default_rng(1000 * log_leaves + 10 * cap_h + B)
    leaves = rand_field(rng, (B, 1 << log_leaves, leaf_len))
    refs = [oracle_merkle(oracle, leaves[b], cap_h) for b in range(B)]
    done = {}
    for fuse in (0, 6, log_leaves, DEFAULT):
        key = effective(fuse, log_leaves, cap_h)
        if key not in done:
            done[key] = run_emu(emb, leaves, (1 << log_leaves) * leaf_len, 0, 0, leaf_len, log_leaves, cap_h, B, fuse, 2)
        dig, caps, counts = done[key]
        # the launches that really ran: the hand-written counts
        want = PLANS[(log_leaves, cap_h)]["default" if fuse == DEFAULT else "own" if fuse == log_leaves else fuse]
        assert counts == want, fuse
        for b in range(B):
            assert np.array_equal(dig[b].reshape(-1, 4), refs[b][0]), (fuse, b)
            assert np.array_equal(caps[b], refs[b][1]), (fuse, b)


@pytest.mark.parametrize("kind,small", [("small", 1), ("medium", 1), ("big", 0)])
def test_emulated_merkle_batch_constant_kinds(emb, oracle, kind, small):
    """the plain partial rounds, the largest fast-path MDS and the generic MDS: one full slice per tree, all nine levels in one launch"""
    log_leaves, cap_h, B, leaf_len = 9, 0, 2, 8
    c384, (rc, circ, diag) = consts384(kind)
    run_emu.c384 = c384
    oracle.orc_poseidon_set_constants(ptr(rc), ptr(circ), ptr(diag))
    leaves = rand_field(np.random.default_rng(77), (B, 1 << log_leaves, leaf_len))
    dig, caps, counts = run_emu(emb, leaves, (1 << log_leaves) * leaf_len, 0, 0, leaf_len, log_leaves, cap_h, B, log_leaves, small)
    assert counts == (2, 1)
    for b in range(B):
        dig_ref, cap_ref = oracle_merkle(oracle, leaves[b], cap_h)
        assert np.array_equal(dig[b].reshape(-1, 4), dig_ref) and np.array_equal(caps[b], cap_ref), b


@pytest.mark.parametrize("log_leaves,cap_h,B,leaf_len,fuse", [(3, 0, 3, 3, 3), (10, 2, 2, 135, 6)])
def test_emulated_merkle_batch_poly_major_with_gaps(emb, oracle, log_leaves, cap_h, B, leaf_len, fuse):
    """polynomial-major leaves with poly_stride > 2^log_leaves, and both tree strides larger than a tree: the digest gap is pre-filled with a
    sentinel that must survive, the source gap holds other random words"""
    c384, (rc, circ, diag) = consts384("small")
    run_emu.c384 = c384
    oracle.orc_poseidon_set_constants(ptr(rc), ptr(circ), ptr(diag))
    rng = np.random.default_rng(5 + log_leaves)
    n = 1 << log_leaves
    poly_stride, gap = n + 3, 11
    src_tree_stride = leaf_len * poly_stride + gap
    src = rand_field(rng, (B, src_tree_stride))
    nd = 4 * ((2 << log_leaves) - (1 << cap_h))
    dig, caps, counts = run_emu(emb, src, src_tree_stride, 1, poly_stride, leaf_len, log_leaves, cap_h, B, fuse, 2, digest_tree_stride=nd + 9,
                                fill=SENTINEL)
    assert counts[1] == 1
    for b in range(B):
        polys = src[b, :leaf_len * poly_stride].reshape(leaf_len, poly_stride)[:, :n]
        dig_ref, cap_ref = oracle_merkle(oracle, np.ascontiguousarray(polys.T), cap_h)
        assert np.array_equal(dig[b, :nd].reshape(-1, 4), dig_ref) and np.array_equal(caps[b], cap_ref), b
        assert np.all(dig[b, nd:] == SENTINEL), b
    # the same trees from leaf-major rows with a gap between the trees' sources
    rows = np.zeros((B, n * leaf_len + gap), dtype=np.uint64)
    for b in range(B):
        rows[b, :n * leaf_len] = src[b, :leaf_len * poly_stride].reshape(leaf_len, poly_stride)[:, :n].T.reshape(-1)
        rows[b, n * leaf_len:] = rand_field(rng, gap)
    dig2, caps2, _ = run_emu(emb, rows, n * leaf_len + gap, 0, 0, leaf_len, log_leaves, cap_h, B, 0, 2, digest_tree_stride=nd + 9, fill=SENTINEL)
    assert np.array_equal(dig2, dig) and np.array_equal(caps2, caps)


def test_emulation_refuses_what_the_product_refuses(emb):
    """glp_merkle_batch_check (csrc/merkle_plan.h) is the one rule both the product and the emulation apply; the product's use of it is
    checked on the GPU (tests/test_gpu_merkle_batch.py)"""
    c384, _ = consts384("small")
    src = np.zeros(4096, dtype=np.uint64)
    dig = np.zeros(4096, dtype=np.uint64)
    nd = 4 * ((2 << 3) - 1)

    def call(src_stride, pm, pstride, leaf_len, log_leaves, cap_h, dstride):
        return emb.emu_merkle_batch(ptr(src), src_stride, pm, pstride, leaf_len, log_leaves, cap_h, 2, 0, ptr(dig), dstride, None, ptr(c384), 1, None, None)

    assert call(8 * 5, 0, 0, 5, 3, 0, nd) == 0
    assert call(8 * 5, 0, 0, 5, 3, 0, nd - 1) == -1          # digest_tree_stride short
    assert call(8 * 5 - 1, 0, 0, 5, 3, 0, nd) == -1          # src_tree_stride short
    assert call(4 * 9 + 8, 1, 9, 5, 3, 0, nd) == 0           # the last polynomial row needs only its first 8 words
    assert call(4 * 9 + 7, 1, 9, 5, 3, 0, nd) == -1
    assert call(64, 1, 7, 5, 3, 0, nd) == -1                 # poly_stride < leaves
    assert call(64, 0, 0, 5, 3, 4, nd) == -1                 # cap_h > log_leaves
    assert call(64, 0, 0, 0, 3, 0, nd) == -1                 # leaf_len == 0
    assert call(2**64 - 1, 1, 1 << 63, 5, 3, 0, nd) == -1    # 4 rows of 2^63 words: the footprint does not fit 64 bits


def test_sanitized_standalone_program():
    """the same source as an ordinary executable under AddressSanitizer + UBSan: fused plans against the unfused one, word for word"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_merkle_batch_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
