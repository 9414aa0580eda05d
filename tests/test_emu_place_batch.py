"""The kernels of glp_witness_place_batch on the CPU (tests/emu_place_batch): every batched body of csrc/place_batch_kernels.cuh, launched with
the grids the driver uses, against the single-instance bodies it replaces — glp_witness_place_kernel (glp_gather_u64), glp_poseidon_gate_fill_kernel<0>
and <1>, glp_sha_gate_fill_kernel — word for word.  Every slab row holds independent random canonical values and the instances read rows
[2, 0, 2], so a wrong instance offset or slab row cannot pass; sentinel words behind every slab row and behind every wire matrix must be left
alone.  Then the refusals of glp_witness_layout_create (host code of the product library; no GPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, poseidon_consts, ptr, rand_field, u64p

D = os.path.join(ROOT, "tests", "emu_place_batch")
SENTINEL = np.uint64(0x5E5E5E5E5E5E5E5E)
UNUSED = 0xFFFFFFFF
GAP_W, GAP_V = 5, 7
SLAB_ROWS = [2, 0, 2]
POS_WIRES, SHA_WIRES, SWAP_WIRE = 135, 144, 24
u32p = ctypes.POINTER(ctypes.c_uint32)


def p32(a):
    return a.ctypes.data_as(u32p)


@pytest.fixture(scope="module")
def epl():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_place_batch.so"))
    c32, c64, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    lib.emu_place_batch.argtypes = [u64p, c64, u64p, c64, u32p, c32, u32p, c64]
    lib.emu_place_single.argtypes = [u64p, u64p, c64, u32p, c64, u32p]
    lib.emu_public_batch.argtypes = [u64p, u64p, c64, u32p, c32, u32p, c32]
    lib.emu_pos_fill_batch.argtypes = [u64p, c64, c32, u32p, c32, c32, u64p, ci]
    lib.emu_pos_fill_single.argtypes = [u64p, c32, u32p, c32, u64p, ci]
    lib.emu_sha_fill_batch.argtypes = [u64p, c64, c32, u32p, u32p, c32, c32]
    lib.emu_sha_fill_single.argtypes = [u64p, c32, u32p, u32p, c32]
    return lib


def make_case(log_n, W, with_pos, with_sha, seed):
    """a layout and a slab of three rows: (cell index, n_src, Poseidon rows, SHA rows, kinds, slab [3][n_src + GAP_V])"""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    cells = W * n
    n_src = cells // 3 + 11
    n_pos = n * 3 // 8 + 1 if with_pos else 0                  # 4 at 2^3; 193 at 2^9: no multiple of 64
    n_sha = n // 2 - 1 if with_sha else 0                      # 3 at 2^3; 255 at 2^9
    pos_rows = np.arange(n_pos, dtype=np.uint32)
    sha_rows = np.arange(n_pos, n_pos + n_sha, dtype=np.uint32)
    kinds = (np.arange(n_sha) & 3).astype(np.uint32)           # all four kinds
    index = rng.integers(0, n_src, size=(W, n), dtype=np.uint32)
    index[rng.random((W, n)) < 0.2] = UNUSED                   # unused cells
    slab = np.full((3, n_src + GAP_V), SENTINEL, dtype=np.uint64)
    slab[:, :n_src] = rand_field(rng, (3, n_src))
    # what the row fillers read must be in range: the swap bit is 0 / 1, SHA words are 32-bit
    slab[:, 0] = [0, 1, 1]
    slab[:, 1:3] = rng.integers(0, 1 << 32, size=(3, 2), dtype=np.uint64)
    index[SWAP_WIRE, pos_rows] = 0
    for j in range(12):
        index[j, sha_rows] = 1 + ((np.arange(n_sha) + j) & 1)
    return index, n_src, pos_rows, sha_rows, kinds, slab


def single(epl, index, n_src, slab_row):
    one = np.full(index.size, SENTINEL, dtype=np.uint64)
    flag = np.zeros(1, dtype=np.uint32)
    epl.emu_place_single(ptr(one), ptr(np.ascontiguousarray(slab_row)), n_src, p32(index), index.size, p32(flag))
    assert flag[0] == 0
    return one


# (log_n, W, Poseidon rows, SHA rows): 2^3 x 136 = 1088 cells is no multiple of 256; a layout without SHA rows, one without Poseidon rows, one with both
SHAPES = [(3, 136, True, False), (3, 144, False, True), (3, 144, True, True), (9, 136, True, False), (9, 144, False, True), (9, 144, True, True)]


# both MDS kinds where the layout has Poseidon rows (without them the kind selects nothing), B = 1 and 3
CASES = [s + (B, kind) for s in SHAPES for B in (1, 3) for kind in (("small", "big") if s[2] else ("small",))]


@pytest.mark.parametrize("log_n,W,with_pos,with_sha,B,kind", CASES)
def test_batched_equals_single(epl, log_n, W, with_pos, with_sha, B, kind):
    index, n_src, pos_rows, sha_rows, kinds, slab = make_case(log_n, W, with_pos, with_sha, 100 * log_n + W + 7 * B)
    cells = index.size
    rows = np.array(SLAB_ROWS[:B], dtype=np.uint32)
    consts = np.concatenate(poseidon_consts(kind)).astype(np.uint64)
    small = 1 if kind == "small" else 0
    slab_before = slab.copy()
    got = np.full((B, cells + GAP_W), SENTINEL, dtype=np.uint64)
    epl.emu_place_batch(ptr(got), cells + GAP_W, ptr(slab), slab.shape[1], p32(rows), B, p32(index), cells)
    # placement alone: the recorded cells, zeros in the unused ones
    for i in range(B):
        one = single(epl, index, n_src, slab[rows[i]])
        assert np.array_equal(got[i, :cells], one), i
        assert np.all(one[index.ravel() == UNUSED] == 0) and np.any(index == UNUSED)
    if with_pos:
        epl.emu_pos_fill_batch(ptr(got), cells + GAP_W, log_n, p32(pos_rows), pos_rows.size, B, ptr(consts), small)
    if with_sha:
        epl.emu_sha_fill_batch(ptr(got), cells + GAP_W, log_n, p32(sha_rows), p32(kinds), sha_rows.size, B)
    ref = []
    for i in range(B):
        one = single(epl, index, n_src, slab[rows[i]])
        if with_pos:
            epl.emu_pos_fill_single(ptr(one), log_n, p32(pos_rows), pos_rows.size, ptr(consts), small)
        if with_sha:
            epl.emu_sha_fill_single(ptr(one), log_n, p32(sha_rows), p32(kinds), sha_rows.size)
        assert np.array_equal(got[i, :cells], one), i
        ref.append(one)
    assert np.all(got[:, cells:] == SENTINEL)                     # the gap behind every wire matrix
    assert np.array_equal(slab, slab_before)                      # the slab, its gaps included, is only read
    if B == 3:
        assert np.array_equal(ref[0], ref[2]) and not np.array_equal(ref[0], ref[1])      # rows [2, 0, 2]
    # the row fillers wrote something: a derived wire of a filled row is not what placement left there
    placed = single(epl, index, n_src, slab[rows[0]]).reshape(W, -1)
    if with_pos:
        assert not np.array_equal(ref[0].reshape(W, -1)[12:24, pos_rows], placed[12:24, pos_rows])
    if with_sha:
        assert not np.array_equal(ref[0].reshape(W, -1)[12:, sha_rows], placed[12:, sha_rows])


@pytest.mark.parametrize("B,n_pub", [(1, 12), (3, 12), (3, 300)])
def test_public_values(epl, B, n_pub):
    """out[b][j] = slab[row_b][public_vars[j]]; 3 * 300 = 900 values: more than one workgroup, no multiple of 256"""
    rng = np.random.default_rng(B + n_pub)
    n_src = 1000
    slab = rand_field(rng, (3, n_src + GAP_V))
    pv = rng.integers(0, n_src, size=n_pub, dtype=np.uint32)
    rows = np.array(SLAB_ROWS[:B], dtype=np.uint32)
    out = np.full(B * n_pub + 2, SENTINEL, dtype=np.uint64)
    epl.emu_public_batch(ptr(out), ptr(slab), slab.shape[1], p32(rows), B, p32(pv), n_pub)
    assert np.array_equal(out[:B * n_pub].reshape(B, n_pub), slab[rows][:, pv])
    assert np.all(out[B * n_pub:] == SENTINEL)


def test_sanitized_standalone_program():
    """the same source as an ordinary executable under AddressSanitizer + UBSan: every batched body against the single one, word for word"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_place_batch_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


# ---- glp_witness_layout_create: every range check, once, on the host ------------------------------------------------------------------------
def create_layout(lib, log_n, W, cell, n_src, pos=(), sha=(), kinds=(), public=()):
    cell, pos, sha, kinds, public = (np.ascontiguousarray(a, dtype=np.uint32) for a in (cell, pos, sha, kinds, public))
    h, err = ctypes.c_void_p(), ctypes.create_string_buffer(256)
    arg = lambda a: a.ctypes.data if a.size else None
    rc = lib.glp_witness_layout_create(log_n, W, cell.ctypes.data, n_src, arg(pos), pos.size, arg(sha), arg(kinds), sha.size, arg(public), public.size,
                                       ctypes.byref(h), err, len(err))
    return rc, h.value, err.value.decode()


def test_layout_refusals(pkg):
    lib = pkg.load_library()
    log_n, n_src = 3, 50
    n = 1 << log_n
    rng = np.random.default_rng(5)
    good = lambda W: rng.integers(0, n_src, size=W * n, dtype=np.uint32)
    cell = good(SHA_WIRES)
    cell[::5] = UNUSED
    rc, h, err = create_layout(lib, log_n, SHA_WIRES, cell, n_src, pos=[0, 1], sha=[2, 3, 4, 7], kinds=[0, 1, 2, 3], public=[0, n_src - 1])
    assert rc == 0 and h and err == ""
    info = [ctypes.c_uint32() for _ in range(2)] + [ctypes.c_uint64()] + [ctypes.c_uint32() for _ in range(3)]
    assert lib.glp_witness_layout_info(h, *[ctypes.byref(x) for x in info]) == 0
    assert [x.value for x in info] == [log_n, SHA_WIRES, n_src, 2, 4, 2]
    lib.glp_witness_layout_destroy(h)                                    # never placed on a device: host memory only
    bad_cell = cell.copy()
    bad_cell[SHA_WIRES * n - 1] = n_src
    refusals = {
        "cell index = n_src": dict(W=SHA_WIRES, cell=bad_cell),
        "Poseidon row = n": dict(W=SHA_WIRES, cell=cell, pos=[0, n]),
        "SHA row = n": dict(W=SHA_WIRES, cell=cell, sha=[n], kinds=[0]),
        "kind 4": dict(W=SHA_WIRES, cell=cell, sha=[1], kinds=[4]),
        "public var = n_src": dict(W=SHA_WIRES, cell=cell, public=[3, n_src]),
        "W too narrow for a Poseidon row": dict(W=POS_WIRES - 1, cell=good(POS_WIRES - 1), pos=[0]),
        "W too narrow for a SHA row": dict(W=SHA_WIRES - 1, cell=good(SHA_WIRES - 1), sha=[0], kinds=[0]),
    }
    for what, kw in refusals.items():
        W = kw.pop("W")
        rc, h, err = create_layout(lib, log_n, W, kw.pop("cell"), n_src, **kw)
        print(f"{what}: rc {rc}, {err!r}")
        assert rc == -1 and h is None and err.startswith("glp_witness_layout_create: "), what
    # the same widths are accepted when the layout has no such rows
    rc, h, err = create_layout(lib, log_n, 8, good(8), n_src)
    assert rc == 0 and h
    lib.glp_witness_layout_destroy(h)


def test_recorded_program_layout(epl, pkg, oracle):
    """WitnessProgram.layout() on a recorded verifier circuit (the golden proof of the Poseidon-row circuit): made once and cached, it reports the
    recording's shape; the batched bodies, fed the arrays it was made from, lay out what numpy lays out from the builder's values and the
    Poseidon rows come out as the single filler leaves them; release() destroys it; a recording whose cell map names a missing variable is
    refused with the library's reason"""
    import importlib
    import json
    rec, vc = (importlib.import_module(pkg.__name__ + m) for m in (".recursion", ".verifier_circuit"))
    consts = poseidon_consts("small")
    oracle.orc_poseidon_set_constants(*(ptr(a) for a in consts))

    class OracleProver:
        def poseidon_permute(self, states):
            s = np.ascontiguousarray(states, dtype=np.uint64).copy()
            for i in range(s.shape[0]):
                row = s[i].copy()
                oracle.orc_poseidon_permute(ptr(row))
                s[i] = row
            return s
    with open(os.path.join(ROOT, "tests", "golden", "proofs.json")) as f:
        g = json.load(f)["plonk"]
    proof = bytes.fromhex(g["proof"])
    b = rec.CircuitBuilder(OracleProver())
    vc.verify_in_circuit(b, proof, g["circuit_cap"], g["queries"], g["pow_bits"], g["W"], n_routed=g.get("R"), n_public=g.get("n_public", 0))
    b.public_input(5)
    b.public_input(7)
    prog = b.program()
    lib = pkg.load_library()
    lay = prog.layout()
    assert lay and prog.layout() == lay
    info = [ctypes.c_uint32() for _ in range(2)] + [ctypes.c_uint64()] + [ctypes.c_uint32() for _ in range(3)]
    assert lib.glp_witness_layout_info(lay, *[ctypes.byref(x) for x in info]) == 0
    n_src = prog.n_values + prog.fixed_values.size
    assert [x.value for x in info] == [prog.log_n, prog.W, n_src, prog.pos_row_ids.size, prog.sha_row_ids.size, 2]
    assert prog.pos_row_ids.size
    inputs, _ = prog.inputs_from_words([proof])
    vals = prog.evaluate(consts, inputs)
    slab = np.zeros((2, n_src + GAP_V), dtype=np.uint64)
    slab[0, :n_src] = np.concatenate((vals, prog.fixed_values))
    slab[1, :n_src] = slab[0, :n_src][::-1]                       # any other canonical words: only placement reads row 1 below
    cells = prog.W << prog.log_n
    index = np.ascontiguousarray(prog.cell_index, dtype=np.uint32)
    rows = np.array([1, 0], dtype=np.uint32)
    got = np.full((2, cells + GAP_W), SENTINEL, dtype=np.uint64)
    epl.emu_place_batch(ptr(got), cells + GAP_W, ptr(slab), slab.shape[1], p32(rows), 2, p32(index), cells)
    for i in range(2):
        want = np.where(index.ravel() == UNUSED, np.uint64(0), slab[rows[i], :n_src][np.minimum(index.ravel(), n_src - 1)])
        assert np.array_equal(got[i, :cells], want), i
    pv = np.ascontiguousarray(prog.public_vars, dtype=np.uint32)
    out = np.zeros(2 * pv.size, dtype=np.uint64)
    epl.emu_public_batch(ptr(out), ptr(slab), slab.shape[1], p32(rows), 2, p32(pv), pv.size)
    assert out[pv.size:].tolist() == [int(v) for v in vals[prog.public_vars]]
    # instance 1 (slab row 0) is a satisfying witness: its Poseidon rows through the batched filler equal the single filler's
    pc = np.concatenate(consts).astype(np.uint64)
    one = got[1, :cells].copy()
    mat = got[1:2].copy()
    epl.emu_pos_fill_batch(ptr(mat), cells + GAP_W, prog.log_n, p32(prog.pos_row_ids), prog.pos_row_ids.size, 1, ptr(pc), 1)
    epl.emu_pos_fill_single(ptr(one), prog.log_n, p32(prog.pos_row_ids), prog.pos_row_ids.size, ptr(pc), 1)
    assert np.array_equal(mat[0, :cells], one) and np.all(mat[0, cells:] == SENTINEL)
    prog.release()
    assert prog.__dict__.get("_layout") is None
    lay2 = prog.layout()
    assert lay2
    prog.release()
    prog.cell_index = prog.cell_index.copy()
    prog.cell_index[0, 0] = n_src
    with pytest.raises(ValueError, match="glp_witness_layout_create: cell 0 .* names source"):
        prog.layout()
