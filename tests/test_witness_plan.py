"""The compiled witness plan (csrc/witness_plan.h, glp_witness_plan_*): the witness program of a recorded circuit reordered into dependency
levels for the device kernel.  CPU only: the REORDERED schedule run serially on the host (glp_witness_plan_run_host) must reproduce
glp_witness_eval byte for byte at full size (signature leaf: 1.2 M ops), the plan's shape must be the one an independent level computation
finds, and malformed programs must be refused when the plan is made (the kernel has no bounds checks)."""
import ctypes
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import P, poseidon_consts, ptr  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# words per op, kind included (the table of verify.hip's program format), and which of the words after the kind are (results, operands)
OP_LEN = [8, 3, 4, 3, 5, 2, 25, 10, 6, 6, 4, 5, 26, 9, 24]
OP_WRITES = {0: [0], 1: [0], 2: [0], 3: [0], 4: [0, 1], 5: [0], 6: list(range(12)), 7: [0, 1], 8: [0], 9: [0], 10: [0], 11: [0], 12: list(range(12)),
             13: [0, 1]}
OP_READS = {0: [1, 2, 3], 1: [], 2: [1], 3: [1], 4: [2, 3], 5: [], 6: list(range(12, 24)), 7: list(range(2, 8)), 8: [1, 2, 3, 4], 9: [1, 2, 3, 4],
            10: [1, 2], 11: [1], 12: list(range(12, 25)), 13: list(range(2, 8)), 14: list(range(1, 23))}


def _lib():
    return graft.load_package().load_library()


def _mods():
    graft.load_package()
    return tuple(importlib.import_module(graft.PKG_NAME + m) for m in (".recursion", ".verifier_circuit", ".ed25519_circuit"))


def python_levels(prog):
    """(number of ops, depth) by the definition of the plan, computed here independently: an op that reads no variable is level 0, any other is
    1 + the highest level among the producers of its operands"""
    prog = [int(w) for w in prog]
    level_of = {}
    pc, n_ops, depth = 0, 0, 0
    while pc < len(prog):
        k = prog[pc]
        a = prog[pc + 1: pc + OP_LEN[k]]
        lvl = max((level_of[a[i]] + 1 for i in OP_READS[k]), default=0)
        for w in ([a[0] + i for i in range(44)] if k == 14 else [a[i] for i in OP_WRITES[k]]):
            level_of[w] = lvl
        depth = max(depth, lvl + 1)
        n_ops += 1
        pc += OP_LEN[k]
    return n_ops, depth


class Plan:
    def __init__(self, prog, n_inputs, n_values, eq_pairs):
        self.lib = _lib()
        self.prog = np.ascontiguousarray(prog, dtype=np.uint64)
        self.eq = np.ascontiguousarray(eq_pairs, dtype=np.uint64)
        self.n_inputs, self.n_values = int(n_inputs), int(n_values)
        h = ctypes.c_void_p()
        self.rc = self.lib.glp_witness_plan_create(self.prog.ctypes.data, self.prog.size, self.n_inputs, self.n_values,
                                                   self.eq.ctypes.data if self.eq.size else None, self.eq.size // 2, ctypes.byref(h))
        self.h = h.value

    def stats(self):
        v = [ctypes.c_uint64() for _ in range(4)]
        assert self.lib.glp_witness_plan_stats(self.h, *(ctypes.byref(x) for x in v)) == 0
        return dict(zip(("ops", "depth", "steps", "stream_bytes"), (int(x.value) for x in v)))

    def run_host(self, consts, inputs):
        inp = np.ascontiguousarray(inputs, dtype=np.uint64)
        vals = np.zeros(self.n_values, dtype=np.uint64)
        bad = ctypes.c_size_t(12345)
        rc = self.lib.glp_witness_plan_run_host(self.h, *(a.ctypes.data for a in consts), inp.ctypes.data if inp.size else None, inp.size,
                                                vals.ctypes.data, vals.size, ctypes.byref(bad))
        return rc, bad.value, vals

    def eval_host(self, consts, inputs):
        inp = np.ascontiguousarray(inputs, dtype=np.uint64)
        vals = np.zeros(self.n_values, dtype=np.uint64)
        bad = ctypes.c_size_t(12345)
        rc = self.lib.glp_witness_eval(*(a.ctypes.data for a in consts), self.prog.ctypes.data, self.prog.size, inp.ctypes.data if inp.size else None,
                                       inp.size, vals.ctypes.data, vals.size, self.eq.ctypes.data if self.eq.size else None, self.eq.size // 2,
                                       ctypes.byref(bad))
        return rc, bad.value, vals

    def close(self):
        if self.h:
            self.lib.glp_witness_plan_destroy(self.h)
            self.h = None


def _same(plan, consts, inputs, want_rc=None):
    rc_h, bad_h, vals_h = plan.eval_host(consts, inputs)
    rc_p, bad_p, vals_p = plan.run_host(consts, inputs)
    assert (rc_p, bad_p) == (rc_h, bad_h)
    if want_rc is not None:
        assert rc_h == want_rc
    if rc_h == 0 or bad_h != ctypes.c_size_t(-1).value:
        # accepted, or refused by a copy constraint: every op ran on both sides, the values are the same bytes
        assert vals_p.tobytes() == vals_h.tobytes()
    return rc_h


def _oracle_prover(oracle):
    class OracleProver:
        def poseidon_permute(self, states):
            s = np.ascontiguousarray(states, dtype=np.uint64).copy()
            for i in range(s.shape[0]):
                row = s[i].copy()
                oracle.orc_poseidon_permute(ptr(row))
                s[i] = row
            return s
    return OracleProver()


def golden_verifier_program(oracle, which, consts):
    rec, vc, _ = _mods()
    oracle.orc_poseidon_set_constants(*(ptr(a) for a in consts))
    with open(os.path.join(G, "proofs.json")) as f:
        g = json.load(f)[which]
    proof = bytes.fromhex(g["proof"])
    b = rec.CircuitBuilder(_oracle_prover(oracle))
    kw = dict(n_routed=g.get("R"), n_public=g.get("n_public", 0), poseidon_consts=consts if which != "plonk" else None, sha=which == "sha")
    vc.verify_in_circuit(b, proof, g["circuit_cap"], g["queries"], g["pow_bits"], g["W"], **kw)
    return b, b.program(), proof


def tampered_inputs(prog, proof, count):
    """input vectors of the proof with one INPUT word flipped each (words the statement shape fixes are refused before any evaluation: skipped)"""
    w = np.frombuffer(proof, dtype="<u8").copy()
    out = []
    for t in prog.input_tags[:: max(1, len(prog.input_tags) // count), 1].tolist():
        bad = w.copy()
        bad[t] ^= np.uint64(1)
        try:
            out.append(prog.inputs_from_words([bad.tobytes()])[0])
        except ValueError:
            pass
    return out


@pytest.fixture(scope="module")
def signature_leaf():
    _, _, ec = _mods()
    msg1 = b"vote: block 4000000 round 0, validator 17".ljust(112, b".")
    pub1, sig1 = ec.keypair_and_sign(bytes(range(32)), msg1)
    b, _ = ec.ed25519_circuit(object(), pub1, sig1, msg1)
    prog = b.program()
    plan = Plan(prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs)
    assert plan.rc == 0
    yield ec, prog, plan, (pub1, sig1, msg1)
    plan.close()


def test_plan_equals_host_evaluator_on_the_signature_leaf(signature_leaf):
    ec, prog, plan, (pub1, sig1, msg1) = signature_leaf
    consts = poseidon_consts("small")
    assert _same(plan, consts, ec.witness_inputs(pub1, sig1, msg1), 0) == 0                       # the recorded inputs
    msg2 = b"vote: block 4000001 round 0, validator 99".ljust(112, b".")
    pub2, sig2 = ec.keypair_and_sign(hashlib.sha256(b"other").digest(), msg2)
    assert _same(plan, consts, ec.witness_inputs(pub2, sig2, msg2), 0) == 0                       # a second valid input set
    forged = bytearray(sig2)
    forged[40] ^= 1
    assert _same(plan, consts, ec.witness_inputs(pub2, bytes(forged), msg2), -7) == -7            # another S
    assert _same(plan, consts, ec.witness_inputs(pub2, sig2, msg1), -7) == -7                     # the signature of another message
    bad_in = np.array(ec.witness_inputs(pub2, sig2, msg2), dtype=np.uint64)
    bad_in[3] = np.uint64(P)                                                                      # not a field element
    assert _same(plan, consts, bad_in, -1) == -1


def test_plan_shape_of_the_signature_leaf(signature_leaf):
    _, prog, plan, _ = signature_leaf
    st = plan.stats()
    n_ops, depth = python_levels(prog.prog)
    print(f"signature leaf: {n_ops} ops, {prog.n_values} variables, depth {depth}, plan {st}")
    assert st["ops"] == n_ops and st["depth"] == depth
    assert prog.stats["variables"] == prog.n_values
    assert depth <= st["steps"] <= depth + (n_ops + 255) // 256
    assert 0 < st["stream_bytes"] < prog.prog.nbytes / 2            # 32-bit indices + the constant dictionary: under half the host program
    # the library's Python face reports the same plan
    assert prog.plan_stats() == st


@pytest.mark.parametrize("which", ["plonk", "gates", "sha"])
def test_plan_equals_host_evaluator_on_the_golden_verifier_circuits(oracle, which):
    consts = poseidon_consts("small")
    b, prog, proof = golden_verifier_program(oracle, which, consts)
    plan = Plan(prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs)
    assert plan.rc == 0
    try:
        inputs, _ = prog.inputs_from_words([proof])
        assert _same(plan, consts, inputs, 0) == 0
        assert np.array_equal(plan.run_host(consts, inputs)[2], np.array(b.values, dtype=np.uint64))
        st = plan.stats()
        assert (st["ops"], st["depth"]) == python_levels(prog.prog)
        # flipped proof words: refused by both with the same copy constraint
        bad = tampered_inputs(prog, proof, 12)
        assert len(bad) >= 6 and all(_same(plan, consts, i2) == -7 for i2 in bad)
        # (a fixed golden proof has no second valid input set.)  Under the generic-MDS constants the same program text takes the other
        # permutation path; whatever the verdict, both evaluators give the same one
        _same(plan, poseidon_consts("big"), inputs)
    finally:
        plan.close()


def _refused(prog, n_inputs, n_values, inputs, serial_host_too=True):
    consts = poseidon_consts("small")
    plan = Plan(prog, n_inputs, n_values, [])
    try:
        assert plan.rc == -1 and not plan.h
        if serial_host_too:
            assert plan.eval_host(consts, inputs)[0] == -1
    finally:
        plan.close()


def test_malformed_programs_are_refused_at_create():
    ok = [1, 0, 0, 1, 1, 1, 0, 2, 0, 1, 1, 3, 0, 5]          # INPUT v0 <- in0; INPUT v1 <- in1; ARITH v2 = 3*v0*v1 + 0*v1 + 5
    good = Plan(ok, 2, 3, [])
    assert good.rc == 0 and good.stats()["ops"] == 3 and good.stats()["depth"] == 2
    rc, _, vals = good.run_host(poseidon_consts("small"), [6, 7])
    assert rc == 0 and vals.tolist() == [6, 7, 3 * 6 * 7 + 5]
    good.close()
    _refused(ok[:6] + [0, 2, 0, 1, 3, 3, 0, 5], 2, 3, [6, 7])                       # index >= n_values
    _refused(ok[:6] + [0, 2, 0, 1, 1, P, 0, 5], 2, 3, [6, 7])                       # constant >= p
    _refused(ok[:-1], 2, 3, [6, 7])                                                  # truncated last op
    _refused(ok + [15, 0], 2, 3, [6, 7])                                             # unknown op kind
    _refused(ok[:3] + [1, 1, 2], 2, 3, [6, 7])                                       # input index >= n_inputs
    _refused(ok[:6] + [2, 2, 0, 64], 2, 3, [6, 7])                                   # bit number out of range
    # The serial host evaluator does not track which variables were written; its CHECKED form (the segments of glp_witness_eval_mt, with their
    # owner table) refuses both of the following, and so does the plan:
    lib = _lib()
    consts = poseidon_consts("small")
    for tail in ([0, 3, 0, 4, 1, 1, 0, 0],                   # reads v4, which nobody wrote
                 [0, 1, 0, 0, 0, 1, 0, 0]):                  # writes v1 again
        prog = np.array(ok + tail + [5, 5], dtype=np.uint64)  # prefix | segment 1 = the bad op | segment 2 = ZERO v5
        _refused(prog, 2, 6, [6, 7], serial_host_too=False)
        inp, vals = np.array([6, 7], dtype=np.uint64), np.zeros(6, dtype=np.uint64)
        seg = np.array([len(ok), len(ok) + 8, len(ok) + 10], dtype=np.uint64)
        bad = ctypes.c_size_t(0)
        assert lib.glp_witness_eval_mt(*(a.ctypes.data for a in consts), prog.ctypes.data, prog.size, inp.ctypes.data, 2, vals.ctypes.data, 6, None, 0,
                                       ctypes.byref(bad), seg.ctypes.data, 2, 2) == -1
    p = Plan(ok, 2, 3, [0, 3])                                # a copy constraint outside the variables
    assert p.rc == -1
    p.close()
