"""The signature leaf's input kernels without a GPU (tests/emu_ed25519_inputs: the kernels of csrc/ed25519_inputs.cuh on the CPU with the
driver's grids) against the project's own Python, ed25519_circuit.half_size_pair and witness_inputs(..., record=None), word for word: the
half-size reduction on its edge scalars and 500 random ones, every case of tests/golden/ed25519.json in the plain form, the flagged and the
canonical-vote forms at the SHA-512 block edges with flags 1 and 0, split_scalars both ways, B = 1, 5 and 65, zero rows for every status
that is not OK.  The same source as a stand-alone program under AddressSanitizer + UBSan is built and run directly."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_inputs_cases as cases  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_emu_hash import k_tables  # noqa: E402

D = os.path.join(ROOT, "tests", "emu_ed25519_inputs")
SENTINEL = 0x5E5E5E5E5E5E5E5E


@pytest.fixture(scope="module")
def edi():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_ed25519_inputs.so"))
    c32, c64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.emu_leaf_input_words.restype = c64
    lib.emu_leaf_input_words.argtypes = [c32, c32, c32, c32]
    lib.emu_half_scalars.argtypes = [vp, c64, vp]
    lib.emu_divmod_l.argtypes = [vp, vp, vp]
    lib.emu_leaf_inputs.argtypes = [c32, c32, c32, c32, vp, vp, vp, c32, vp, vp, vp, c64, vp, vp, c64, vp]
    return lib


def run_batch(lib, b, pad=3):
    """(rows [n][width], status [n]) of the emulated call; the rows lie in a wider slab whose other words must stay untouched"""
    _, k512 = k_tables()
    stride = b.width + pad
    out = np.full((b.n, stride), SENTINEL, dtype=np.uint64)
    status = np.full(b.n, -1, dtype=np.int32)
    rc = lib.emu_leaf_inputs(b.form, b.lo, b.hi, b.split, b.pubs.ctypes.data, b.sigs.ctypes.data, b.msgs.ctypes.data, b.stride, b.lens.ctypes.data,
                             b.flags.ctypes.data if b.form != cases.PLAIN else None, b.dummy.ctypes.data if b.dummy is not None else None,
                             b.n, k512.ctypes.data, out.ctypes.data, stride, status.ctypes.data)
    assert rc == 0
    assert np.all(out[:, b.width:] == SENTINEL), "a row wrote past its width"
    return out[:, :b.width], status


def assert_batch(b, rows, status):
    assert status.tolist() == b.status.tolist(), b.name
    for i in range(b.n):
        assert np.array_equal(rows[i], b.rows[i]), (b.name, i, np.nonzero(rows[i] != b.rows[i])[0][:8].tolist())
        if status[i] != cases.OK:
            assert not rows[i].any(), (b.name, i)


def test_half_scalars_equal_half_size_pair(edi):
    ks, want, ints = cases.half_scalar_cases()
    got = np.full(want.shape, SENTINEL, dtype=np.uint64)
    assert edi.emu_half_scalars(ks.ctypes.data, len(ints), got.ctypes.data) == 0
    for i, k in enumerate(ints):
        assert got[i].tolist() == want[i].tolist(), hex(k)
    st = {k: int(want[i, 7]) for i, k in enumerate(ints[:13])}
    assert [st[k] for k in (cases.ELL - 1, cases.ELL - 2, (cases.ELL + 1) // 2)] == [cases.NO_PAIR] * 3
    assert [st[k] for k in (cases.ELL, (1 << 256) - 1)] == [cases.INVALID] * 2
    assert all(st[k] == cases.OK for k in (0, 1, 2, 3, 1 << 126, (1 << 127) + 1, 1 << 200))


def test_divmod_l_equals_divmod(edi):
    import random
    rng = random.Random(7)
    xs = [0, 1, cases.ELL - 1, cases.ELL, cases.ELL + 1, 1 << 64, 1 << 256, (1 << 512) - 1] + [rng.getrandbits(rng.choice((200, 256, 300, 512))) for _ in range(200)]
    for x in xs:
        a = np.array([(x >> (64 * j)) & (2**64 - 1) for j in range(8)], dtype=np.uint64)
        q, r = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        edi.emu_divmod_l(a.ctypes.data, q.ctypes.data, r.ctypes.data)
        assert (sum(int(v) << (64 * j) for j, v in enumerate(q)), sum(int(v) << (64 * j) for j, v in enumerate(r))) == divmod(x, cases.ELL), hex(x)


def test_row_widths(edi):
    for b in cases.all_batches():
        assert edi.emu_leaf_input_words(b.form, b.lo, b.hi, b.split) == b.width, b.name
    assert edi.emu_leaf_input_words(3, 8, 8, 1) == 0 and edi.emu_leaf_input_words(cases.FLAGGED, 8, 9, 1) == 0
    assert edi.emu_leaf_input_words(cases.VOTE, 9, 8, 1) == 0


def test_plain_form_every_golden_case(edi):
    seen = 0
    for b in cases.plain_batches():
        rows, status = run_batch(edi, b)
        assert_batch(b, rows, status)
        seen += b.n
    golden = cases.golden_cases()
    assert seen >= len(golden)
    assert any(not v for *_, v in golden) and any(s == cases.REJECT for b in cases.plain_batches() for s in b.status)


@pytest.mark.parametrize("name", cases.FLAGGED_NAMES)
def test_flagged_and_vote_forms(edi, name):
    b = cases.flagged_batch(name)
    rows, status = run_batch(edi, b)
    assert_batch(b, rows, status)


def test_cases_cover_what_they_claim():
    bs = cases.flagged_batches()
    assert {b.n for b in bs} >= {1, 5, 65}
    assert {b.split for b in bs} == {0, 1} and {b.split for b in cases.plain_batches()} == {0, 1}
    commit = next(b for b in bs if b.name == "c-commit-split1")
    ok_lens = {int(commit.lens[i]) for i in range(commit.n) if commit.status[i] == cases.OK and commit.flags[i]}
    assert len(ok_lens) == 3 and cases.INVALID in commit.status.tolist()
    forged = next(b for b in bs if b.name == "b-112-B5")
    assert forged.status.tolist() == [0, 0, 0, cases.REJECT, 0]
    for ln in cases.EDGE_LENGTHS:
        for form in "bc":
            b = next(x for x in bs if x.name == f"{form}-len{ln}")
            assert {int(f) for f in b.flags} == {0, 1} and ln in b.lens.tolist()


def test_declarations_are_plain_c_and_the_word_count_needs_no_gpu(pkg, tmp_path):
    """tests/cpp/abi_c99_ed25519_inputs.c as strict C99 against the library: it links the two device calls and counts the words of the three forms"""
    pkg.load_library()
    exe = tmp_path / "abi_c99_ed25519_inputs"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "abi_c99_ed25519_inputs.c"), "-o", str(exe), "-L", libdir, "-lglprover",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    plain, flagged, vote = 96 + 112 + 44, 1 + 32 + 112 + 64 + 44 + 38, 1 + 32 + 110 + 1 + 7 + 64 + 44 + 38
    assert r.stdout.strip() == f"words {plain} {flagged} {vote} refused 1 linked 1"
    assert pkg.Ed25519InputLayout(pkg.ED25519_FORM_VOTE, 104, 110, 1).n_words() == vote


def test_sanitized_program():
    """the reduction and both divisions under ASan + UBSan, as a program of their own: builds, runs, exits 0"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_ed25519_inputs_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "emu_ed25519_inputs_san ok" in r.stdout, r.stdout[-2000:]
