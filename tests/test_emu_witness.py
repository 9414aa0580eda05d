"""The witness-evaluation kernel body (csrc/witness_kernels.cuh) on the CPU (tests/emu_witness: workgroups of 64 emulated lanes) against the
host evaluator glp_witness_eval: the three golden verifier circuits in a batch of (valid, valid, tampered) on FEWER workgroups than instances,
and a synthetic program that holds every op kind, with operands in range and out of range.  Accepted instances: byte-identical values.
Refused ones: the host's verdict and copy-constraint index."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import P, poseidon_consts, rand_field  # noqa: E402
import __graft_entry__ as graft  # noqa: E402
from test_witness_plan import golden_verifier_program, tampered_inputs  # noqa: E402

NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def emu_witness():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_witness")
    subprocess.run(["make", "-s"], cwd=d, check=True)                      # a no-op after __graft_entry__.build()
    lib = ctypes.CDLL(os.path.join(d, "libglp_emu_witness.so"))
    vp = ctypes.c_void_p
    lib.emu_witness_eval.argtypes = [vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_size_t, vp, ctypes.c_int, vp, vp, ctypes.c_size_t,
                                     ctypes.c_uint32, ctypes.c_uint, ctypes.c_uint, vp, vp]
    return lib


def host_eval(prog, n_values, eq, consts, inputs):
    lib = graft.load_package().load_library()
    inp = np.ascontiguousarray(inputs, dtype=np.uint64)
    vals = np.zeros(n_values, dtype=np.uint64)
    bad = ctypes.c_size_t(0)
    rc = lib.glp_witness_eval(*(a.ctypes.data for a in consts), prog.ctypes.data, prog.size, inp.ctypes.data if inp.size else None, inp.size,
                              vals.ctypes.data, vals.size, eq.ctypes.data if eq.size else None, eq.size // 2, ctypes.byref(bad))
    return rc, (NONE if bad.value == ctypes.c_size_t(-1).value else bad.value), vals


def emu_eval(lib, prog, n_inputs, n_values, eq, consts, batch, grid, block=64, pad=3):
    """the kernel's verdicts turned into the ABI's the way glp_witness_eval_device does: a refused op first, then the lowest failing pair"""
    c384 = np.concatenate(consts).astype(np.uint64)
    small = int(all(int(v) < (1 << 24) for v in np.concatenate(consts[1:])))
    inp = np.ascontiguousarray(batch, dtype=np.uint64).reshape(len(batch), n_inputs)
    B, stride = inp.shape[0], n_values + pad
    vals = np.full((B, stride), 0xABCD, dtype=np.uint64)
    status, bad = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint64)
    rc = lib.emu_witness_eval(prog.ctypes.data, prog.size, n_inputs, n_values, eq.ctypes.data if eq.size else None, eq.size // 2, c384.ctypes.data, small,
                              inp.ctypes.data, vals.ctypes.data, stride, B, grid, block, status.ctypes.data, bad.ctypes.data)
    assert rc == 0
    assert np.all(vals[:, n_values:] == 0xABCD)                            # words past n_values are left alone
    out = []
    for b in range(B):
        if status[b] != 0:
            out.append((int(status[b]), NONE, vals[b, :n_values]))
        elif int(bad[b]) != NONE:
            out.append((-7, int(bad[b]), vals[b, :n_values]))
        else:
            out.append((0, NONE, vals[b, :n_values]))
    return out


def compare(lib, prog, n_inputs, n_values, eq, consts, batch, grid, want):
    prog, eq = np.ascontiguousarray(prog, dtype=np.uint64), np.ascontiguousarray(eq, dtype=np.uint64)
    got = emu_eval(lib, prog, n_inputs, n_values, eq, consts, batch, grid)
    for b, (inputs, (rc_d, bad_d, vals_d)) in enumerate(zip(batch, got)):
        rc_h, bad_h, vals_h = host_eval(prog, n_values, eq, consts, inputs)
        assert (rc_d, bad_d) == (rc_h, bad_h), f"instance {b}"
        assert rc_h == want[b], f"instance {b}"
        if rc_h == 0 or bad_h != NONE:                                     # every op ran on the host too
            assert vals_d.tobytes() == vals_h.tobytes(), f"instance {b}"


@pytest.mark.parametrize("which", ["plonk", "gates", "sha"])
def test_emulated_kernel_on_the_golden_verifier_circuits(emu_witness, oracle, which):
    consts = poseidon_consts("small")
    _, prog, proof = golden_verifier_program(oracle, which, consts)
    inputs, _ = prog.inputs_from_words([proof])
    bad = tampered_inputs(prog, proof, 3)[-1]
    compare(emu_witness, prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs, consts, [inputs, inputs, bad], 2, [0, 0, -7])


def synthetic_program():
    """every op kind, deliberately NOT in level order, a level wider than the workgroup and a chain deeper than a few levels"""
    prog, nv = [], [62]                                                    # v0..v61 = the inputs

    def new(n=1):
        v = nv[0]
        nv[0] += n
        return v
    for i in reversed(range(62)):
        prog += [1, i, i]
    chain = new()
    prog += [0, chain, 0, 1, 2, 3, 5, 7]                                   # ARITH
    for _ in range(40):                                                    # a dependent chain: 40 levels of width 1
        nxt = new()
        prog += [0, nxt, chain, chain, 0, 1, P - 1, 9]
        chain = nxt
    z = new(); prog += [5, z]                                              # ZERO
    bit = new(); prog += [2, bit, chain, 5]                                # BIT
    b1, b2 = new(), new(); prog += [11, b1, chain, 3, 17, 11, b2, chain, 0, 64]        # BITS
    inv = new(); prog += [3, inv, 58]                                      # INV
    e0, e1 = new(), new(); prog += [4, e0, e1, 59, 60]                     # EINV
    pos = new(12); prog += [6] + list(range(pos, pos + 12)) + list(range(12))           # POSEIDON
    sw = new(12); prog += [12] + list(range(sw, sw + 12)) + list(range(pos, pos + 12)) + [12]        # POSEIDON_SWAP, swap bit = v12
    t1, en = new(), new(); prog += [7, t1, en, 13, 14, 15, 16, 17, 18, 0x428A2F98]     # SHA_E
    an = new(); prog += [8, an, 19, 20, 21, t1]                            # SHA_A on the computed T1
    an2 = new(); prog += [8, an2, 19, 20, 21, 61]                          # SHA_A on a free T1 (up to 35 bits)
    wn = new(); prog += [9, wn, 22, 23, 24, 25]                            # SHA_W
    s = new(); prog += [10, s, 26, 27]                                     # ADD32
    x0, x1 = new(), new(); prog += [13, x0, x1, 50, 51, 52, 53, 54, 55]    # EXTMULADD
    first = new(44); prog += [14, first] + list(range(28, 50))             # NNF_MUL
    for k in range(150):                                                   # one level wider than 64 lanes, reading late results
        w = new()
        prog += [0, w, first + (k % 44), sw + (k % 12), s, 1 + k, 2, 3]
    new(3)                                                                 # variables no op writes: 0, as in the host's zeroed value vector
    eq = [56, 57, inv, inv, 0, 0]
    return np.array(prog, dtype=np.uint64), nv[0], np.array(eq, dtype=np.uint64)


def synthetic_cases(rng):
    """(batch, expected verdicts) for synthetic_program(): an accepted base instance, accepted variants, and every way an instance is refused"""
    base = rand_field(rng, 62)
    base[12] = 1                                                       # swap bit
    base[13:28] = rng.integers(0, 1 << 32, 15, dtype=np.uint64)       # SHA words
    base[61] = (1 << 35) - 1                                           # T1
    base[28:50] = rng.integers(0, 1 << 24, 22, dtype=np.uint64)       # limbs
    base[28], base[39] = (1 << 27) - 1, (1 << 28) - 1                  # ... loose ones
    base[57] = base[56]
    base[58] = 0                                                       # INV of 0 is 0
    batch, want = [base.copy()], [0]

    def case(idx, value, rc):
        v = base.copy()
        v[idx] = value
        batch.append(v)
        want.append(rc)
    case(12, 0, 0)                       # no swap
    case(58, 12345, 0)                   # a real inverse
    case(59, 0, 0); batch[-1][60] = 0    # EINV of 0
    case(12, 2, -7)                      # swap bit above 1
    case(13, 1 << 32, -7)                # SHA_E operand above 32 bits
    case(19, 1 << 40, -7)                # SHA_A operand
    case(61, 1 << 35, -7)                # T1 above 35 bits
    case(23, 1 << 32, -7)                # SHA_W operand
    case(27, 1 << 33, -7)                # ADD32 operand
    case(30, 1 << 28, -7)                # NNF limb out of range
    case(57, int(base[56]) ^ 1, -7)      # copy constraint 0 fails
    case(5, P, -1)                       # an input that is not a field element
    case(5, P, -1); batch[-1][12] = 2    # ... together with a refused row: the malformed input decides, as on the host (INPUT ops come first)
    return batch, want


def test_emulated_kernel_on_every_op_kind(emu_witness):
    prog, n_values, eq = synthetic_program()
    rng = np.random.default_rng(14)
    for kind in ("small", "big"):
        consts = poseidon_consts(kind)
        batch, want = synthetic_cases(rng)
        compare(emu_witness, prog, 62, n_values, eq, consts, batch, 3, want)
