"""The batched Tendermint tree kernels and the header-chain leaf's input kernels without a GPU (tests/emu_chain_inputs: the kernel bodies of
csrc/tm_batch_kernels.cuh and csrc/chain_inputs.cuh on the CPU with the driver's grids, and the host forms beside them).  Trees against a
recursive hashlib restatement and against the single-tree kernels of glp_tm_merkle_root_var: leaf counts 0 .. 129 and the maximum 512, leaf
lengths at the SHA-256 padding edges, B = 1, 2, 65, 130 with mixed trees, the refusals.  Chain inputs against the project's own Python
(_chain_leaf_inputs, header_hash, the tests of _map_chain): leaves of 1, 2 and 8 headers, 1 to 3 leaves, 1, 2 and 4 varint bytes at both ends of
their height ranges, the first height past the 1- and 2-byte ranges (128, 16384) spelled in the layout's bytes, and every tamper on the first, a
middle and the last header of a leaf.  The strict-C99 declarations, and the same source as
a stand-alone program under AddressSanitizer + UBSan, built and run directly."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_inputs_cases as cases  # noqa: E402
from conftest import ROOT, ptr  # noqa: E402
from test_emu_hash import k_tables  # noqa: E402

D = os.path.join(ROOT, "tests", "emu_chain_inputs")


@pytest.fixture(scope="module")
def chi():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_chain_inputs.so"))
    c32, c64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    for f in (lib.emu_tm_root_batch, lib.emu_tm_root_batch_host):
        f.argtypes = [vp, c64, vp, vp, c64, c64, vp, vp]
    lib.emu_chain_input_words.restype = c64
    lib.emu_chain_input_words.argtypes = [vp, c32, c32]
    for f in (lib.emu_chain_inputs, lib.emu_chain_inputs_host):
        f.argtypes = [vp, c32, c32, vp, vp, c64, c64, vp, vp, c64, vp, vp]
    return lib


def run_trees(fn, call):
    k256, _ = k_tables()
    roots = np.full((call.B, 32), 0xEE, dtype=np.uint8)
    data = call.data if call.data.size else np.zeros(1, dtype=np.uint8)
    assert fn(data.ctypes.data, call.data.size, call.offs.ctypes.data, call.first.ctypes.data, call.total, call.B, k256.ctypes.data, roots.ctypes.data) == 0
    return [roots[t].tobytes() for t in range(call.B)]


@pytest.mark.parametrize("name", [c.name for c in cases.tree_calls()])
def test_batched_trees_equal_the_recursive_tree(chi, name):
    call = next(c for c in cases.tree_calls() if c.name == name)
    assert run_trees(chi.emu_tm_root_batch, call) == call.roots
    assert run_trees(chi.emu_tm_root_batch_host, call) == call.roots


def test_batched_trees_equal_the_single_tree_kernels(chi, emu):
    """tree by tree against the kernels of glp_tm_merkle_root_var (tests/emu), for the mixed calls"""
    k256, _ = k_tables()
    for name in ("B2", "B65"):
        call = next(c for c in cases.tree_calls() if c.name == name)
        got = run_trees(chi.emu_tm_root_batch, call)
        for t, leaves in enumerate(call.trees):
            if not leaves:
                continue
            offs = np.zeros(len(leaves) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(x) for x in leaves])
            out = ctypes.create_string_buffer(32)
            assert emu.emu_tm_merkle_root_var(b"".join(leaves) or b"\0", ptr(offs), len(leaves), k256.ctypes.data, out) == 0
            assert out.raw == got[t], (name, t)


def test_tree_cases_cover_what_they_claim():
    calls = cases.tree_calls()
    assert {c.B for c in calls} >= {1, 2, 65, 130}
    assert {len(c.trees[0]) for c in calls if c.B == 1} >= set(cases.LEAF_COUNTS)
    assert {len(x) for c in calls for t in c.trees for x in t} >= set(cases.LEAF_LENS)
    for name in ("B65", "B130"):
        c = next(x for x in calls if x.name == name)
        assert len({len(t) for t in c.trees}) > 3 and len({len(x) for t in c.trees for x in t}) > 3
    assert any(len(t) == cases.MAX_LEAVES for c in calls for t in c.trees) and any(len(t) == 0 for c in calls if c.B > 1 for t in c.trees)


def test_refused_tree_calls_write_nothing(chi):
    k256, _ = k_tables()
    data = np.ones(16, dtype=np.uint8)
    for name, data_len, offs, first, total, B, want in cases.refused_tree_calls():
        for fn in (chi.emu_tm_root_batch, chi.emu_tm_root_batch_host):
            roots = np.full((B, 32), 0xEE, dtype=np.uint8)
            assert fn(data.ctypes.data, data_len, offs.ctypes.data, first.ctypes.data, total, B, k256.ctypes.data, roots.ctypes.data) == want, name
            assert np.all(roots == 0xEE), name


def run_chain(lib, host, c, pad=3):
    """(rows [n / B][width], status [n], hashes [n + 1]) of one call; the rows lie in a wider slab whose other words must stay untouched"""
    k256, _ = k_tables()
    fl = np.array(c.field_lengths, dtype=np.uint32)
    fn = lib.emu_chain_inputs_host if host else lib.emu_chain_inputs
    width = int(lib.emu_chain_input_words(fl.ctypes.data, c.B, c.g))
    stride = width + pad
    out = np.full((c.n // c.B, stride), cases.SENTINEL, dtype=np.uint64)
    status = np.full(c.n, -1, dtype=np.int32)
    hashes = np.full((c.n + 1, 32), 0xEE, dtype=np.uint8)
    start = np.frombuffer(c.start, dtype=np.uint8).copy()
    assert fn(fl.ctypes.data, c.B, c.g, c.blob.ctypes.data, start.ctypes.data, c.first, c.n, k256.ctypes.data, out.ctypes.data, stride,
              hashes.ctypes.data, status.ctypes.data) == 0
    assert np.all(out[:, width:] == cases.SENTINEL), "a row wrote past its width"
    return out[:, :width], status, [hashes[k].tobytes() for k in range(c.n + 1)]


def assert_chain(c, rows, status, hashes):
    assert hashes == c.hashes, c.name
    assert status.tolist() == c.status.tolist(), c.name
    if c.width is not None:
        assert rows.shape[1] == c.width, c.name
    want = c.rows_array(rows.shape[1])
    for l in range(rows.shape[0]):
        assert np.array_equal(rows[l], want[l]), (c.name, l, np.nonzero(rows[l] != want[l])[0][:8].tolist())
        if c.rows[l] is None:
            assert not rows[l].any(), (c.name, l)


@pytest.mark.parametrize("name", [c.name for c in cases.good_chains()])
def test_chain_rows_equal_chain_leaf_inputs(chi, name):
    c = next(x for x in cases.good_chains() if x.name == name)
    assert not c.status.any()
    for host in (False, True):
        assert_chain(c, *run_chain(chi, host, c))


@pytest.mark.parametrize("name", [c.name for c in cases.tampered_chains() + cases.truncated_chains()] + ["g2-nonminimal-all"])
def test_tampered_headers_are_refused_where_they_are(chi, name):
    """the right status at the right index, a zero row for that leaf only, the neighbouring rows word for word"""
    c = cases.nonminimal_chain() if name == "g2-nonminimal-all" else next(x for x in cases.tampered_chains() + cases.truncated_chains() if x.name == name)
    assert c.status.any()
    for host in (False, True):
        assert_chain(c, *run_chain(chi, host, c))


def test_chain_cases_cover_what_they_claim():
    good = cases.good_chains()
    assert {(c.B, c.n // c.B) for c in good} >= {(B, L) for B in (1, 2, 8) for L in (1, 2, 3)}
    assert {c.g for c in good} == {1, 2, 4}
    heights = {h for c in good for h in (c.first, c.first + c.n - 1)}
    assert heights >= {0, 127, 128, 16383, 1 << 21, (1 << 28) - 1}
    # 127/128 and 16383/16384: the last height that fits a layout in the good chains, the first that does not in the truncated ones
    assert {(c.g, c.first + c.n - 1) for c in cases.truncated_chains()} == {(1, 128), (2, 16384)}
    assert {(1, 127), (2, 16383)} <= {(c.g, c.first + c.n - 1) for c in good}
    bad = cases.tampered_chains()
    assert {c.name.split("-", 2)[2].split("@")[0] for c in bad} == set(cases.TAMPERS)
    for B in (8, 2):
        ats = {int(c.name.split("@")[1]) for c in bad if c.B == B}
        assert ats == {B, B + B // 2, 2 * B - 1}


def test_row_widths_and_refused_layouts(chi):
    fl = np.array(cases.FIELD_LENGTHS, dtype=np.uint32)
    per = 4 + 32 + (72 - 34) + sum(cases.FIELD_LENGTHS) - 5 - 72 - 34
    assert chi.emu_chain_input_words(fl.ctypes.data, 8, 4) == 9 + 8 * per
    for j, v in ((4, 33), (6, 33), (6, 35)):
        bad = fl.copy()
        bad[j] = v
        assert chi.emu_chain_input_words(bad.ctypes.data, 8, 4) == 0
    assert chi.emu_chain_input_words(fl.ctypes.data, 0, 4) == 0 and chi.emu_chain_input_words(fl.ctypes.data, 8, 0) == 0
    assert chi.emu_chain_input_words(fl.ctypes.data, 8, 8) == 0


def test_host_forms_of_the_library(pkg):
    """glp_tm_merkle_root_batch_host and glp_header_chain_leaf_inputs_host of the product library (no ctx, no GPU) on one mixed call and one
    tampered chain; the layout's word count through HeaderChainLayout"""
    lib = pkg.load_library()
    call = next(c for c in cases.tree_calls() if c.name == "B65")
    roots = np.zeros((call.B, 32), dtype=np.uint8)
    assert lib.glp_tm_merkle_root_batch_host(call.data.ctypes.data, call.data.size, call.offs.ctypes.data, call.first.ctypes.data, call.total, call.B,
                                             roots.ctypes.data) == 0
    assert [roots[t].tobytes() for t in range(call.B)] == call.roots
    for name, data_len, offs, first, total, B, want in cases.refused_tree_calls():
        r = np.full((B, 32), 0xEE, dtype=np.uint8)
        assert lib.glp_tm_merkle_root_batch_host(np.ones(16, dtype=np.uint8).ctypes.data, data_len, offs.ctypes.data, first.ctypes.data, total, B,
                                                 r.ctypes.data) == want and np.all(r == 0xEE), name
    c = cases.tampered_chains()[0]
    layout = pkg.HeaderChainLayout.of(c.field_lengths, c.B, c.g)
    width = layout.n_words()
    assert width == c.width
    out = np.full((c.n // c.B, width), cases.SENTINEL, dtype=np.uint64)
    status = np.full(c.n, -1, dtype=np.int32)
    hashes = np.zeros((c.n + 1, 32), dtype=np.uint8)
    assert lib.glp_header_chain_leaf_inputs_host(ctypes.byref(layout), c.blob.ctypes.data, c.start, c.first, c.n, out.ctypes.data, width,
                                                 hashes.ctypes.data, status.ctypes.data) == 0
    assert_chain(c, out, status, [hashes[k].tobytes() for k in range(c.n + 1)])
    assert lib.glp_header_chain_leaf_inputs_host(ctypes.byref(layout), c.blob.ctypes.data, c.start, c.first, c.n - 1, out.ctypes.data, width,
                                                 hashes.ctypes.data, status.ctypes.data) == -1
    assert lib.glp_header_chain_leaf_inputs_host(ctypes.byref(layout), c.blob.ctypes.data, c.start, c.first, c.n, out.ctypes.data, width - 1,
                                                 hashes.ctypes.data, status.ctypes.data) == -1
    with pytest.raises(pkg.GlpError):
        pkg.HeaderChainLayout.of((4, 12, 5, 13, 30) + cases.FIELD_LENGTHS[5:], 8, 4).n_words()


def test_device_inputs_needs_device_witness(pkg):
    dcm = cases.dcm
    with pytest.raises(ValueError, match="device_inputs needs device_witness=True"):
        dcm.HeaderChainMapReduce(None, None, device_inputs=True)


def test_declarations_are_plain_c_and_the_word_count_needs_no_gpu(pkg, tmp_path):
    """tests/cpp/abi_c99_chain_inputs.c as strict C99 against the library: it links the device calls, counts the words of the default layout and
    runs both host forms"""
    pkg.load_library()
    exe = tmp_path / "abi_c99_chain_inputs"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "abi_c99_chain_inputs.c"), "-o", str(exe), "-L", libdir, "-lglprover",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    per = 4 + 32 + 38 + sum(cases.FIELD_LENGTHS) - 5 - 72 - 34
    empty = "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    assert r.stdout.strip() == f"words {9 + 8 * per} refused 1 linked 1 empty {empty} status 1"


def test_sanitized_program():
    """both forms over a corpus of trees and chains under ASan + UBSan, as a program of their own: builds, runs, exits 0"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_chain_inputs_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "emu_chain_inputs_san ok" in r.stdout, r.stdout[-2000:]
