"""The forest, audit-path and inclusion-check kernels without a GPU (tests/emu_tm_proofs: the kernel bodies of csrc/tm_proof_kernels.cuh on the
CPU with the driver's checks, plan and grids, and the host forms beside them) against the RECURSIVE hashlib reference of tests/tm_proof_cases.py:
aunts, their counts, leaf hashes and roots for every leaf of trees up to 130 leaves and the first, last, middle and split-point leaves of trees of
511 .. 4096; zeroed unused slots and untouched words behind the rows; the launch counts the plan gives; the forest's roots against the batched-root
kernels; refused calls that write nothing; the negative matrix of the verifier; the product library's host forms; the strict-C99 declarations; the
same source as a stand-alone program under AddressSanitizer + UBSan, built and run directly."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_inputs_cases as cic  # noqa: E402
import tm_proof_cases as cases  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_emu_hash import k_tables  # noqa: E402

D = os.path.join(ROOT, "tests", "emu_tm_proofs")
PAD = 96                                                       # sentinel bytes behind every output array


@pytest.fixture(scope="module")
def tmp_lib():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_tm_proofs.so"))
    c32, c64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    for f in (lib.emu_tm_forest_proofs, lib.emu_tm_forest_proofs_host):
        f.argtypes = [vp, c64, vp, vp, c64, c64, vp, vp, vp, c64, vp, vp, c32, vp, vp, vp]
    for f in (lib.emu_tm_verify, lib.emu_tm_verify_host):
        f.argtypes = [vp, c64, vp, vp, c64, vp, vp, vp, vp, c32, vp, c64, vp, vp]
    return lib


def padded(n_bytes):
    return np.full(n_bytes + PAD, cases.SENTINEL, dtype=np.uint8)


def run_forest(fn, c, stride, all_leaves=False):
    """(rc, roots, aunts [nq][stride][32], n_aunts, leaf hashes, launches) of one call; every output lies in a sentinel-filled block PAD bytes
    longer than it, and the bytes behind it must stay untouched"""
    k256, _ = k_tables()
    call = c.call
    nq = call.total if all_leaves else len(c.queries)
    roots, aunts, na, lh = padded(call.B * 32), padded(nq * stride * 32), padded(nq * 4), padded(nq * 32)
    launches = np.zeros(2, dtype=np.uint32)
    data = call.data if call.data.size else np.zeros(1, dtype=np.uint8)
    qt, ql = (None, None) if all_leaves else (c.qt.ctypes.data, c.ql.ctypes.data)
    rc = fn(data.ctypes.data, call.data.size, call.offs.ctypes.data, call.first.ctypes.data, call.total, call.B, k256.ctypes.data, qt, ql, nq,
            roots.ctypes.data, aunts.ctypes.data, stride, na.ctypes.data, lh.ctypes.data, launches.ctypes.data)
    for name, a, n in (("roots", roots, call.B * 32), ("aunts", aunts, nq * stride * 32), ("n_aunts", na, nq * 4), ("leaf hashes", lh, nq * 32)):
        assert np.all(a[n:] == cases.SENTINEL), f"{c.name}: the call wrote behind its {name}"
    return (rc, [roots[32 * t:32 * t + 32].tobytes() for t in range(call.B)], aunts[:nq * stride * 32].reshape(nq, stride, 32),
            na[:nq * 4].view(np.uint32), lh[:nq * 32].reshape(nq, 32), tuple(int(v) for v in launches))


def expected_create_launches(c):
    biggest = max((len(t) for t in c.trees), default=0)
    return (1 if c.call.total else 0) + max(0, (biggest - 1).bit_length() - 9 if biggest > 1 else 0) + 1


@pytest.mark.parametrize("name", [c.name for c in cases.proof_cases()])
def test_paths_equal_the_recursive_reference(tmp_lib, name):
    c = cases.case(name)
    stride = c.max_aunts + 2                                   # two slots more than any row needs: they come back zero
    for fn in (tmp_lib.emu_tm_forest_proofs, tmp_lib.emu_tm_forest_proofs_host):
        rc, roots, aunts, na, lh, launches = run_forest(fn, c, stride)
        assert rc == 0 and roots == c.roots
        assert na.tolist() == [len(a) for a in c.aunts]
        assert np.array_equal(aunts, c.aunts_array(stride)), np.nonzero((aunts != c.aunts_array(stride)).any(axis=(1, 2)))[0][:8].tolist()
        assert [lh[q].tobytes() for q in range(len(c.queries))] == c.leaf_hashes
        if fn is tmp_lib.emu_tm_forest_proofs:
            assert launches == (expected_create_launches(c), 1 if c.queries else 0)
            assert launches[0] <= 2 + max(0, c.max_aunts - 9)


def test_launch_counts_at_the_stated_sizes(tmp_lib):
    want = {"B1-n8": 2, "B1-n512": 2, "big-n512": 2, "big-n513": 3, "big-n1024": 3, "big-n1025": 4, "big-n4096": 5, "B4-wide": 4, "B1-n0": 1}
    for name, n in want.items():
        c = cases.case(name)
        assert run_forest(tmp_lib.emu_tm_forest_proofs, c, c.max_aunts)[5][0] == n, name


@pytest.mark.parametrize("name", ["B1-n5", "B65", "B3-max", "B4-wide"])
def test_every_leaf_in_numbering_order(tmp_lib, name):
    """both query arrays NULL with n_queries == total_leaves"""
    c = cases.case(name)
    flat = [(t, i) for t, leaves in enumerate(c.trees) for i in range(len(leaves))]
    stride = max((max(0, (len(t) - 1).bit_length()) if len(t) > 1 else 0 for t in c.trees), default=0)
    for fn in (tmp_lib.emu_tm_forest_proofs, tmp_lib.emu_tm_forest_proofs_host):
        rc, roots, aunts, na, lh, _ = run_forest(fn, c, stride, all_leaves=True)
        assert rc == 0 and roots == c.roots
        for q in sorted({0, len(flat) // 3, len(flat) // 2, len(flat) - 1} | set(range(min(40, len(flat))))):
            t, i = flat[q]
            path = c.refs[t].path(i)
            assert int(na[q]) == len(path) and [aunts[q, k].tobytes() for k in range(len(path))] == path, (name, q)
            assert not aunts[q, len(path):].any() and lh[q].tobytes() == cases.leaf_hash(c.trees[t][i])


def test_forest_roots_equal_the_batched_root_kernels(tmp_lib):
    """the same calls through the emulated kernels of glp_tm_merkle_root_batch (tests/emu_chain_inputs)"""
    d = os.path.join(ROOT, "tests", "emu_chain_inputs")
    subprocess.run(["make", "-s"], cwd=d, check=True)
    chi = ctypes.CDLL(os.path.join(d, "libglp_emu_chain_inputs.so"))
    vp, c64 = ctypes.c_void_p, ctypes.c_uint64
    chi.emu_tm_root_batch.argtypes = [vp, c64, vp, vp, c64, c64, vp, vp]
    k256, _ = k_tables()
    for name in ("B2", "B65", "B130", "B3-max", "big-n511", "B1-n512"):
        c = cases.case(name)
        call = c.call
        roots = np.zeros((call.B, 32), dtype=np.uint8)
        assert chi.emu_tm_root_batch(call.data.ctypes.data, call.data.size, call.offs.ctypes.data, call.first.ctypes.data, call.total, call.B,
                                     k256.ctypes.data, roots.ctypes.data) == 0
        got = run_forest(tmp_lib.emu_tm_forest_proofs, c, c.max_aunts)[1]
        assert got == [roots[t].tobytes() for t in range(call.B)], name


def test_cases_cover_what_they_claim():
    cs = cases.proof_cases()
    assert {c.name for c in cs} >= {c.name for c in cic.tree_calls()}
    singles = {len(c.trees[0]) for c in cs if c.call.B == 1}
    assert singles >= set(cic.LEAF_COUNTS) | set(cases.BIG_COUNTS)
    big = cases.case("big-n1025")
    assert big.queries == [(0, 0), (0, 512), (0, 1023), (0, 1024)] and [len(a) for a in big.aunts] == [11, 11, 11, 1]
    five = cases.case("B1-n5")
    assert [len(a) for a in five.aunts] == [3, 3, 3, 3, 1]
    m = cases.negative_matrix()
    for tree in m.trees:
        assert len(set(tree)) == len(tree)
    assert {cases.OK, cases.BAD_SHAPE, cases.BAD_ROOT} == set(m.want)


def test_refused_calls_write_nothing(tmp_lib):
    k256, _ = k_tables()
    data = np.ones(16, dtype=np.uint8)
    q0 = np.zeros(1, dtype=np.uint64)

    def attempt(fn, data_len, offs, first, total, B, qt, ql, nq, stride):
        roots, aunts, na, lh = padded(B * 32), padded(max(1, nq) * max(1, stride) * 32), padded(max(1, nq) * 4), padded(max(1, nq) * 32)
        rc = fn(data.ctypes.data, data_len, offs.ctypes.data, first.ctypes.data, total, B, k256.ctypes.data, None if qt is None else qt.ctypes.data,
                None if ql is None else ql.ctypes.data, nq, roots.ctypes.data, aunts.ctypes.data, stride, na.ctypes.data, lh.ctypes.data, None)
        untouched = all(np.all(a == cases.SENTINEL) for a in (roots, aunts, na, lh))
        return rc, untouched

    for fn in (tmp_lib.emu_tm_forest_proofs, tmp_lib.emu_tm_forest_proofs_host):
        for name, data_len, offs, first, total, B, want in cic.refused_tree_calls():
            rc, untouched = attempt(fn, data_len, offs, first, total, B, q0, q0, 1, 12)
            if name == "a tree over the maximum":          # 513 leaves of no bytes: refused by the 512-leaf call, built here
                assert rc == 0 and not untouched, name
            else:
                assert rc == want == -1 and untouched, name
        ok_offs, ok_first = np.array([0, 2, 4, 10], dtype=np.uint64), np.array([0, 1, 3], dtype=np.uint64)
        u = lambda *v: np.array(v, dtype=np.uint64)
        for what, qt, ql, nq, stride in (("a query leaf equal to the tree's count", u(0, 1), u(0, 2), 2, 4),
                                         ("a query leaf equal to the count of a one-leaf tree", u(0), u(1), 1, 4),
                                         ("a query tree equal to n_trees", u(1, 2), u(0, 0), 2, 4),
                                         ("a stride too small", u(0, 1), u(0, 1), 2, 0),
                                         ("one query array without the other", u(0, 1), None, 2, 4),
                                         ("every leaf, but not total_leaves queries", None, None, 2, 4),
                                         ("every leaf, a stride too small", None, None, 3, 0)):
            rc, untouched = attempt(fn, 10, ok_offs, ok_first, 3, 2, qt, ql, nq, stride)
            assert rc == -1 and untouched, what
        rc, untouched = attempt(fn, 10, ok_offs, ok_first, 3, 2, u(0), u(0), 1, 0)       # the one-leaf tree needs no aunt: stride 0 is enough
        assert rc == 0 and not untouched
        # more than 2^24 leaves in one tree: refused as unsupported from the tree_first array alone (the offsets are sound: all zero)
        big = (1 << 24) + 1
        rc, untouched = attempt(fn, 10, np.zeros(big + 1, dtype=np.uint64), np.array([0, big], dtype=np.uint64), big, 1, q0, q0, 1, 30)
        assert rc == -5 and untouched


def run_verify(fn, m, roots=None, stride=None, n_aunts=None):
    k256, _ = k_tables()
    offs = np.zeros(m.n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in m.leaves])
    blob = np.frombuffer(b"".join(m.leaves), dtype=np.uint8)
    r = np.frombuffer(b"".join(m.roots), dtype=np.uint8)
    index, total = np.array(m.index, dtype=np.uint64), np.array(m.total, dtype=np.uint64)
    na, ro = np.array(m.n_aunts, dtype=np.uint32), np.array(m.root_of, dtype=np.uint32)
    status = np.full(m.n + 4, -7, dtype=np.int32)
    rc = fn(r.ctypes.data, len(m.roots), ro.ctypes.data, blob.ctypes.data, blob.size, offs.ctypes.data, index.ctypes.data, total.ctypes.data,
            m.aunts.ctypes.data, m.stride, na.ctypes.data, m.n, k256.ctypes.data, status.ctypes.data)
    assert np.all(status[m.n:] == -7)
    return rc, status[:m.n]


def test_verifier_statuses_equal_the_reference(tmp_lib):
    m = cases.negative_matrix()
    for fn in (tmp_lib.emu_tm_verify, tmp_lib.emu_tm_verify_host):
        rc, status = run_verify(fn, m)
        assert rc == 0
        bad = [(p, m.kind[p], int(status[p]), m.want[p]) for p in range(m.n) if status[p] != m.want[p]]
        assert not bad, bad[:8]


def test_verifier_refuses_unsound_arrays(tmp_lib):
    k256, _ = k_tables()
    root, leaf = np.zeros(32, dtype=np.uint8), np.ones(8, dtype=np.uint8)
    one, aunts = np.zeros(2, dtype=np.uint64), np.zeros((2, 1, 32), dtype=np.uint8)
    na = np.zeros(2, dtype=np.uint32)
    for fn in (tmp_lib.emu_tm_verify, tmp_lib.emu_tm_verify_host):
        for what, offs, ro, n_roots in (("descending offsets", [0, 5, 4], [0, 0], 1), ("offsets past the data", [0, 4, 9], [0, 0], 1),
                                        ("a root index equal to n_roots", [0, 4, 8], [0, 1], 1), ("no root", [0, 4, 8], [0, 0], 0)):
            status = np.full(2, -7, dtype=np.int32)
            rc = fn(root.ctypes.data, n_roots, np.array(ro, dtype=np.uint32).ctypes.data, leaf.ctypes.data, 8, np.array(offs, dtype=np.uint64).ctypes.data,
                    one.ctypes.data, one.ctypes.data, aunts.ctypes.data, 1, na.ctypes.data, 2, k256.ctypes.data, status.ctypes.data)
            assert rc == -1 and np.all(status == -7), what
        assert fn(None, 0, None, None, 0, None, None, None, None, 0, None, 0, k256.ctypes.data, None) == 0       # n == 0


def test_host_forms_of_the_library(pkg):
    """glp_tm_forest_proofs_host and glp_tm_verify_inclusion_batch_host of the product library (no ctx, no GPU) on one mixed call, on the
    negative matrix and on refused calls"""
    lib = pkg.load_library()
    c = cases.case("B65")
    call, nq, stride = c.call, len(c.queries), c.max_aunts + 1
    roots, aunts = np.zeros((call.B, 32), dtype=np.uint8), np.full((nq, stride, 32), cases.SENTINEL, dtype=np.uint8)
    na, lh = np.zeros(nq, dtype=np.uint32), np.zeros((nq, 32), dtype=np.uint8)
    assert lib.glp_tm_forest_proofs_host(call.data.ctypes.data, call.data.size, call.offs.ctypes.data, call.first.ctypes.data, call.total, call.B,
                                         c.qt.ctypes.data, c.ql.ctypes.data, nq, roots.ctypes.data, aunts.ctypes.data, stride, na.ctypes.data,
                                         lh.ctypes.data) == 0
    assert [roots[t].tobytes() for t in range(call.B)] == c.roots and na.tolist() == [len(a) for a in c.aunts]
    assert np.array_equal(aunts, c.aunts_array(stride)) and [lh[q].tobytes() for q in range(nq)] == c.leaf_hashes
    before = aunts.copy()
    assert lib.glp_tm_forest_proofs_host(call.data.ctypes.data, call.data.size, call.offs.ctypes.data, call.first.ctypes.data, call.total, call.B,
                                         c.qt.ctypes.data, c.ql.ctypes.data, nq, roots.ctypes.data, aunts.ctypes.data, c.max_aunts - 1, na.ctypes.data,
                                         lh.ctypes.data) == -1 and np.array_equal(aunts, before)
    m = cases.negative_matrix()
    offs = np.zeros(m.n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in m.leaves])
    blob, r = np.frombuffer(b"".join(m.leaves), dtype=np.uint8), np.frombuffer(b"".join(m.roots), dtype=np.uint8)
    index, total = np.array(m.index, dtype=np.uint64), np.array(m.total, dtype=np.uint64)
    na, ro = np.array(m.n_aunts, dtype=np.uint32), np.array(m.root_of, dtype=np.uint32)
    status = np.full(m.n, -7, dtype=np.int32)
    assert lib.glp_tm_verify_inclusion_batch_host(r.ctypes.data, len(m.roots), ro.ctypes.data, blob.ctypes.data, blob.size, offs.ctypes.data,
                                                  index.ctypes.data, total.ctypes.data, m.aunts.ctypes.data, m.stride, na.ctypes.data, m.n,
                                                  status.ctypes.data) == 0
    assert status.tolist() == m.want
    assert (pkg.TM_INCLUSION_OK, pkg.TM_INCLUSION_BAD_SHAPE, pkg.TM_INCLUSION_BAD_ROOT) == (cases.OK, cases.BAD_SHAPE, cases.BAD_ROOT)


def test_declarations_are_plain_c_and_the_host_forms_need_no_gpu(pkg, tmp_path):
    """tests/cpp/abi_c99_tm_proofs.c as strict C99 against the library: it links the device calls and runs both host forms on five leaves"""
    pkg.load_library()
    exe = tmp_path / "abi_c99_tm_proofs"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "abi_c99_tm_proofs.c"), "-o", str(exe), "-L", libdir, "-lglprover",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    leaves = [bytes([i] * (i + 1)) for i in range(5)]
    root = cases.RefTree(leaves).root()
    assert r.stdout.strip() == f"aunts 3 3 3 3 1 root {root.hex()} status 0 0 0 0 0 tampered 2 shape 1 refused 1"


def test_sanitized_program():
    """both forms over a corpus of forests, paths and tampered proofs under ASan + UBSan, as a program of their own: builds, runs, exits 0"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_tm_proofs_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "emu_tm_proofs_san ok" in r.stdout, r.stdout[-2000:]
