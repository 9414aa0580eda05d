"""The segmented witness evaluation on the CPU (tests/emu_witness_seg: every work-item a thread, __syncthreads() a barrier): the three launches
glp_witness_eval_device issues for a segmented plan — prefix, all segments with a workgroup per (instance, segment) pair, tail with the copy
constraints — against the host evaluator, on the 4-child `gates` node with a tampered child in one instance and on a hand-written program
that holds every op kind; and the word-check kernel against WitnessProgram.check_words."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import P, poseidon_consts, rand_field  # noqa: E402
from test_emu_witness import NONE, host_eval  # noqa: E402
from test_witness_segments import check_word_cases, node_program, tampered_children  # noqa: E402


@pytest.fixture(scope="module")
def emu_seg():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_witness_seg")
    subprocess.run(["make", "-s"], cwd=d, check=True)                      # a no-op after __graft_entry__.build()
    lib = ctypes.CDLL(os.path.join(d, "libglp_emu_witness_seg.so"))
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.emu_witness_eval_seg.argtypes = [vp, sz, sz, sz, vp, sz, vp, sz, vp, ctypes.c_int, vp, vp, sz, u32, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, vp, vp]
    lib.emu_witness_check_words.argtypes = [vp, sz, u32, vp, vp, u32, vp, vp, vp, u32, ctypes.c_uint, ctypes.c_uint, vp, vp]
    return lib


@pytest.fixture(scope="module")
def gates_node(oracle):
    return node_program(oracle, "gates", poseidon_consts("small"))


def compare_seg(lib, prog, n_inputs, n_values, eq, seg, consts, batch, want, grid, seg_grid, block, pad=3):
    """the three launches against glp_witness_eval: verdicts (turned into the ABI's the way glp_witness_eval_device does) and bytes"""
    prog, eq, seg = (np.ascontiguousarray(a, dtype=np.uint64) for a in (prog, eq, seg))
    c384 = np.concatenate(consts).astype(np.uint64)
    small = int(all(int(v) < (1 << 24) for v in np.concatenate(consts[1:])))
    inp = np.ascontiguousarray(batch, dtype=np.uint64).reshape(len(batch), n_inputs)
    B, stride = inp.shape[0], n_values + pad
    assert seg_grid < B * (seg.size - 1)                                   # the (instance, segment) loop strides
    vals = np.full((B, stride), 0xABCD, dtype=np.uint64)
    status, bad = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint64)
    rc = lib.emu_witness_eval_seg(prog.ctypes.data, prog.size, n_inputs, n_values, eq.ctypes.data if eq.size else None, eq.size // 2, seg.ctypes.data,
                                  seg.size - 1, c384.ctypes.data, small, inp.ctypes.data, vals.ctypes.data, stride, B, grid, seg_grid, block,
                                  status.ctypes.data, bad.ctypes.data)
    assert rc == 0
    assert np.all(vals[:, n_values:] == 0xABCD)                            # words past n_values are left alone
    for b in range(B):
        got = (int(status[b]), NONE) if status[b] != 0 else (-7, int(bad[b])) if int(bad[b]) != NONE else (0, NONE)
        rc_h, bad_h, vals_h = host_eval(prog, n_values, eq, consts, batch[b])
        assert got == (rc_h, bad_h) and rc_h == want[b], f"instance {b}"
        if rc_h == 0 or bad_h != NONE:                                     # every op ran on the host too
            assert vals[b, :n_values].tobytes() == vals_h.tobytes(), f"instance {b}"


def test_three_launches_on_the_gates_node(emu_seg, gates_node):
    consts = poseidon_consts("small")
    prog, proofs = gates_node
    good, _ = prog.inputs_from_words(proofs)
    bad = tampered_children(prog, proofs, 3)[-1]                           # a word of the last child
    # 2 instances x 4 segments on 3 workgroups
    compare_seg(emu_seg, prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs, prog.seg_bounds, consts, [good, bad], [0, -7], grid=2, seg_grid=3, block=64)


def segmented_synthetic_program():
    """every op kind in prefix | segment | segment | tail: the inputs and a constant in the prefix; each segment a dependent chain, a level wider
    than a workgroup of 64 and its share of the op kinds, reading the prefix and itself; the tail reads both segments.  Deliberately not in
    level order."""
    prog, nv, cuts = [], [62], []                                          # v0..v61 = the inputs

    def new(n=1):
        v = nv[0]
        nv[0] += n
        return v
    for i in reversed(range(62)):
        prog += [1, i, i]
    z = new(); prog += [5, z]                                              # ZERO
    base = new(); prog += [0, base, 0, 1, 2, 3, 5, 7]                      # ARITH
    cuts.append(len(prog))
    # ---- segment A
    chain = base
    for _ in range(20):
        nxt = new()
        prog += [0, nxt, chain, chain, 0, 1, P - 1, 9]
        chain = nxt
    a_chain = chain
    bit = new(); prog += [2, bit, chain, 5]                                # BIT
    b1, b2 = new(), new(); prog += [11, b1, chain, 3, 17, 11, b2, chain, 0, 64]        # BITS
    inv = new(); prog += [3, inv, 58]                                      # INV
    e0, e1 = new(), new(); prog += [4, e0, e1, 59, 60]                     # EINV
    pos = new(12); prog += [6] + list(range(pos, pos + 12)) + list(range(12))           # POSEIDON
    sw = new(12); prog += [12] + list(range(sw, sw + 12)) + list(range(pos, pos + 12)) + [12]        # POSEIDON_SWAP, swap bit = v12
    for k in range(150):
        w = new()
        prog += [0, w, sw + (k % 12), chain, z, 1 + k, 2, 3]
    a_last = w
    cuts.append(len(prog))
    # ---- segment B
    chain = base
    for _ in range(33):
        nxt = new()
        prog += [0, nxt, chain, base, 1, 3, 1, 4]
        chain = nxt
    t1, en = new(), new(); prog += [7, t1, en, 13, 14, 15, 16, 17, 18, 0x428A2F98]     # SHA_E
    an = new(); prog += [8, an, 19, 20, 21, t1]                            # SHA_A on the computed T1
    an2 = new(); prog += [8, an2, 19, 20, 21, 61]                          # SHA_A on a free T1 (up to 35 bits)
    wn = new(); prog += [9, wn, 22, 23, 24, 25]                            # SHA_W
    s = new(); prog += [10, s, 26, 27]                                     # ADD32
    x0, x1 = new(), new(); prog += [13, x0, x1, 50, 51, 52, 53, 54, 55]    # EXTMULADD
    first = new(44); prog += [14, first] + list(range(28, 50))             # NNF_MUL
    for k in range(100):
        w = new()
        prog += [0, w, first + (k % 44), chain, s, 1 + k, 2, 3]
    b_last = w
    cuts.append(len(prog))
    # ---- tail
    t = new(); prog += [0, t, a_last, b_last, a_chain, 1, 1, 0]
    u = new(); prog += [0, u, t, chain, inv, 2, 3, 4]
    new(3)                                                                 # variables no op writes: 0
    eq = [56, 57, inv, inv, 0, 0, u, u]
    return np.array(prog, dtype=np.uint64), nv[0], np.array(eq, dtype=np.uint64), np.array(cuts, dtype=np.uint64)


def segmented_cases(rng):
    """(batch, expected verdicts) for segmented_synthetic_program(): a refusal in each of the three launches"""
    base = rand_field(rng, 62)
    base[12] = 1                                                       # swap bit
    base[13:28] = rng.integers(0, 1 << 32, 15, dtype=np.uint64)       # SHA words
    base[61] = (1 << 35) - 1                                           # T1
    base[28:50] = rng.integers(0, 1 << 24, 22, dtype=np.uint64)       # limbs
    base[57] = base[56]
    batch, want = [base.copy()], [0]

    def case(idx, value, rc):
        v = base.copy()
        v[idx] = value
        batch.append(v)
        want.append(rc)
    case(12, 0, 0)                       # no swap
    case(12, 2, -7)                      # segment A refuses a row: swap bit above 1
    case(27, 1 << 33, -7)                # segment B refuses a row: ADD32 operand
    case(57, int(base[56]) ^ 1, -7)      # copy constraint 0 fails (the tail's launch)
    case(5, P, -1)                       # an input that is not a field element (the prefix's launch)
    case(5, P, -1); batch[-1][12] = 2    # ... together with a refused row in a LATER launch: the malformed input still decides
    return batch, want


@pytest.mark.parametrize("block", [64, 256])
def test_three_launches_on_every_op_kind(emu_seg, block):
    prog, n_values, eq, seg = segmented_synthetic_program()
    rng = np.random.default_rng(15)
    for kind in ("small", "big"):
        consts = poseidon_consts(kind)
        batch, want = segmented_cases(rng)
        compare_seg(emu_seg, prog, 62, n_values, eq, seg, consts, batch, want, grid=3, seg_grid=5, block=block)


def test_word_check_kernel_equals_check_words(emu_seg, gates_node):
    prog, proofs = gates_node

    def run(values, tables, var_want, bit_want):
        B = values.shape[0]
        var_idx, bit_vars, bit_start = tables
        values, var_want, bit_want = (np.ascontiguousarray(a, dtype=np.uint64) for a in (values, var_want, bit_want))
        bad_var, bad_bits = np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
        # 2 workgroups of 64 work-items for B * (n_var + n_bits) checks: the grid-stride loop runs
        assert emu_seg.emu_witness_check_words(values.ctypes.data, values.shape[1], B, var_idx.ctypes.data, var_want.ctypes.data, var_idx.size,
                                               bit_vars.ctypes.data, bit_start.ctypes.data, bit_want.ctypes.data, bit_start.size - 1, 2, 64,
                                               bad_var.ctypes.data, bad_bits.ctypes.data) == 0
        return bad_var, bad_bits
    check_word_cases(prog, proofs, poseidon_consts("small"), run)
