"""The SEGMENTED witness plan (csrc/witness_plan.h: glp_witness_plan_create_ex, glp_witness_plan_parts) and the word checks' per-check function
(glp_witness_check_words_host), on the CPU.  A recursion node is one instance of fan-in independent verifier segments; the plan gives the
prefix, every segment and the tail a level schedule of their own.  Here: two 4-child nodes over the golden `gates` and `sha` proofs, recorded
with CircuitBuilder.begin_segment / end_segment on the oracle's permutation.  The parts run in order on the host must reproduce both host
evaluators byte for byte, the parts' shape must be the one an independent computation finds, false structural claims must be refused when the
plan is made (the kernel has no checks), and the word checks must give check_words' verdicts."""
import ctypes
import json
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import poseidon_consts, ptr  # noqa: E402
from test_witness_plan import G, OP_LEN, OP_READS, OP_WRITES, Plan, _lib, _mods, _oracle_prover  # noqa: E402

NONE = (1 << 64) - 1
FAN = 4


def node_program(oracle, which, consts):
    """the witness program of a FAN-child node over the golden proof `which`: FAN verifier segments, then the Poseidon tree over the digests and
    the public inputs (a non-empty tail).  Returns (program, the FAN proofs)."""
    rec, vc, _ = _mods()
    oracle.orc_poseidon_set_constants(*(ptr(a) for a in consts))
    with open(os.path.join(G, "proofs.json")) as f:
        g = json.load(f)[which]
    proof = bytes.fromhex(g["proof"])
    b = rec.CircuitBuilder(_oracle_prover(oracle))
    kw = dict(n_routed=g.get("R"), n_public=g.get("n_public", 0), poseidon_consts=consts, sha=which == "sha")
    outs = []
    for k in range(FAN):
        b.begin_segment()
        outs.append(vc.verify_in_circuit(b, proof, g["circuit_cap"], g["queries"], g["pow_bits"], g["W"], proof_id=k, **kw))
        b.end_segment()
    level = [o["digest"] for o in outs]
    while len(level) > 1:
        level = [b.two_to_one(level[2 * k], level[2 * k + 1]) for k in range(len(level) // 2)]
    for v in [x for o in outs for x in o["public"] + o["digest"]] + level[0]:
        b.public_input(v)
    return b.program(), [proof] * FAN


@pytest.fixture(scope="module")
def nodes(oracle):
    consts = poseidon_consts("small")
    return {which: node_program(oracle, which, consts) for which in ("gates", "sha")}


class SegPlan(Plan):
    """test_witness_plan.Plan made by glp_witness_plan_create_ex"""

    def __init__(self, prog, n_inputs, n_values, eq_pairs, seg_bounds, n_seg=None):
        self.lib = _lib()
        self.prog = np.ascontiguousarray(prog, dtype=np.uint64)
        self.eq = np.ascontiguousarray(eq_pairs, dtype=np.uint64)
        self.seg = None if seg_bounds is None else np.ascontiguousarray(seg_bounds, dtype=np.uint64)
        self.n_inputs, self.n_values = int(n_inputs), int(n_values)
        self.n_seg = (0 if self.seg is None else self.seg.size - 1) if n_seg is None else n_seg
        h = ctypes.c_void_p()
        self.rc = self.lib.glp_witness_plan_create_ex(self.prog.ctypes.data, self.prog.size, self.n_inputs, self.n_values,
                                                      self.eq.ctypes.data if self.eq.size else None, self.eq.size // 2,
                                                      None if self.seg is None else self.seg.ctypes.data, self.n_seg, ctypes.byref(h))
        self.h = h.value

    def parts(self):
        n = ctypes.c_uint32(0)
        assert self.lib.glp_witness_plan_parts(self.h, ctypes.byref(n), None, None, None) == 0
        arr = [np.full(n.value, 99, dtype=np.uint64) for _ in range(3)]
        assert self.lib.glp_witness_plan_parts(self.h, ctypes.byref(n), *(a.ctypes.data for a in arr)) == 0
        return [tuple(int(a[k]) for a in arr) for k in range(n.value)]

    def eval_mt(self, consts, inputs, threads=4):
        inp = np.ascontiguousarray(inputs, dtype=np.uint64)
        vals = np.zeros(self.n_values, dtype=np.uint64)
        bad = ctypes.c_size_t(12345)
        rc = self.lib.glp_witness_eval_mt(*(a.ctypes.data for a in consts), self.prog.ctypes.data, self.prog.size, inp.ctypes.data if inp.size else None,
                                          inp.size, vals.ctypes.data, vals.size, self.eq.ctypes.data if self.eq.size else None, self.eq.size // 2,
                                          ctypes.byref(bad), self.seg.ctypes.data, self.seg.size - 1, threads)
        return rc, bad.value, vals


def tampered_children(prog, proofs, count):
    """input vectors of the node with ONE word of ONE child flipped, at `count` input_tags positions spread over the children"""
    out = []
    tags = prog.input_tags[:: max(1, len(prog.input_tags) // count)]
    for child, pos in tags.tolist():
        words = [np.frombuffer(p, dtype="<u8").copy() for p in proofs]
        words[child][pos] ^= np.uint64(1)
        try:
            out.append(prog.inputs_from_words([w.tobytes() for w in words])[0])
        except ValueError:
            pass
    return out


@pytest.mark.parametrize("which", ["gates", "sha"])
def test_segmented_plan_equals_both_host_evaluators(nodes, which):
    consts = poseidon_consts("small")
    prog, proofs = nodes[which]
    assert prog.seg_bounds is not None and prog.seg_bounds.size == FAN + 1
    plan = SegPlan(prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs, prog.seg_bounds)
    assert plan.rc == 0
    try:
        good, _ = prog.inputs_from_words(proofs)
        bad = tampered_children(prog, proofs, 6)
        assert len(bad) >= 4
        for inputs, want in [(good, 0)] + [(i2, -7) for i2 in bad]:
            rc_p, bad_p, vals_p = plan.run_host(consts, inputs)
            rc_h, bad_h, vals_h = plan.eval_host(consts, inputs)
            rc_m, bad_m, vals_m = plan.eval_mt(consts, inputs)
            assert (rc_p, bad_p) == (rc_h, bad_h) == (rc_m, bad_m) and rc_p == want
            if rc_h == 0 or bad_h != ctypes.c_size_t(-1).value:             # every op ran on all three sides
                assert vals_p.tobytes() == vals_h.tobytes() == vals_m.tobytes()
    finally:
        plan.close()


def python_parts(prog, seg_bounds):
    """(ops, depth, steps at 256 lanes) per part — prefix, segments, tail — by the definition of the segmented plan, computed here independently:
    inside a part an op that reads nothing THE PART wrote is level 0, any other is 1 + the highest level among the part's producers of its operands"""
    prog = [int(w) for w in prog]
    cuts = [0] + [int(o) for o in seg_bounds] + [len(prog)]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        level_of, width, pc = {}, Counter(), lo
        while pc < hi:
            k = prog[pc]
            a = prog[pc + 1: pc + OP_LEN[k]]
            lvl = max((level_of[a[i]] + 1 for i in OP_READS[k] if a[i] in level_of), default=0)
            for w in ([a[0] + i for i in range(44)] if k == 14 else [a[i] for i in OP_WRITES[k]]):
                level_of[w] = lvl
            width[lvl] += 1
            pc += OP_LEN[k]
        assert pc == hi
        parts.append((sum(width.values()), len(width), sum((w + 255) // 256 for w in width.values())))
    return parts


@pytest.mark.parametrize("which", ["gates", "sha"])
def test_parts_of_the_segmented_plan(nodes, which):
    prog, _ = nodes[which]
    plan = SegPlan(prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs, prog.seg_bounds)
    plain = Plan(prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs)
    try:
        got, want = plan.parts(), python_parts(prog.prog, prog.seg_bounds)
        print(f"{which} x{FAN}: whole program {plain.stats()}, parts (ops, depth, steps) {got}")
        assert len(got) == FAN + 2 and got == want
        assert got[1] == got[2] == got[3] == got[4]                         # four copies of one verifier
        assert got[0][0] > 0 and got[-1][0] > 0                             # constants before the segments, the digest tree after them
        st = plan.stats()
        assert st["ops"] == sum(p[0] for p in got) == plain.stats()["ops"]
        assert st["depth"] == sum(p[1] for p in got) and st["steps"] == sum(p[2] for p in got)
        # a segment on a workgroup of its own has far fewer steps to walk than the whole program on one
        assert max(p[2] for p in got[1:-1]) < plain.stats()["steps"]
        # the library's Python face reports the same parts
        assert [tuple(d[k] for k in ("ops", "depth", "steps")) for d in prog.plan_parts()] == got
        assert len(prog.plan_parts(segments=False)) == 1
    finally:
        plan.close()
        plain.close()


# INPUT v0 <- in0; INPUT v1 <- in1 | ARITH v2 = 3 v0 v1 + 5 | ARITH v3 = 2 v0 v0 + v1 | ARITH v4 = v2 v3 + 7 v0
HAND = [1, 0, 0, 1, 1, 1,  0, 2, 0, 1, 1, 3, 0, 5,  0, 3, 0, 0, 1, 2, 1, 0,  0, 4, 2, 3, 0, 1, 7, 0]
HAND_SEG = [6, 14, 22]


def test_structural_claims_are_checked_at_create():
    consts = poseidon_consts("small")
    good = SegPlan(HAND, 2, 5, [], HAND_SEG)
    assert good.rc == 0 and good.parts() == [(2, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1)]
    rc, _, vals = good.run_host(consts, [6, 7])
    assert rc == 0 and vals.tolist() == [6, 7, 131, 79, 131 * 79 + 42]
    good.close()
    for seg in ([6, 15, 22],          # an offset inside an op
                [7, 14, 22],
                [6, 14, 29],          # ... inside the last one
                [14, 6, 22],          # descending
                [6, 14, 31]):         # beyond the program
        p = SegPlan(HAND, 2, 5, [], seg)
        assert p.rc == -1 and not p.h, seg
    # the second segment reads v2, which the first one writes: both the plan and the checked host evaluator refuse the claim
    cross = HAND[:14] + [0, 3, 2, 0, 1, 2, 1, 0] + HAND[22:]
    p = SegPlan(cross, 2, 5, [], HAND_SEG)
    assert p.rc == -1 and not p.h
    lib = _lib()
    prog, seg = np.array(cross, dtype=np.uint64), np.array(HAND_SEG, dtype=np.uint64)
    inp, vals, bad = np.array([6, 7], dtype=np.uint64), np.zeros(5, dtype=np.uint64), ctypes.c_size_t(0)
    assert lib.glp_witness_eval_mt(*(a.ctypes.data for a in consts), prog.ctypes.data, prog.size, inp.ctypes.data, 2, vals.ctypes.data, 5, None, 0,
                                   ctypes.byref(bad), seg.ctypes.data, 2, 2) == -1
    # ... while the same program is a fine PLAIN plan, and the tail may read every segment
    plain = Plan(cross, 2, 5, [])
    assert plain.rc == 0
    # n_seg of 0 or 1: the plain plan
    for seg, n_seg in ((None, 0), ([6, 14], 1), ([6, 14, 22], 0)):
        p = SegPlan(cross, 2, 5, [], seg, n_seg)
        assert p.rc == 0 and p.stats() == plain.stats() and p.parts() == [(5, 4, 4)] == [tuple(plain.stats()[k] for k in ("ops", "depth", "steps"))]
        p.close()
    plain.close()


def word_tables(prog):
    nb = prog.wc_bits[:, 2].astype(np.int64)
    return (prog.wc_var[:, 2].astype(np.uint32), prog.wc_bit_vars.astype(np.uint32), np.concatenate(([0], np.cumsum(nb))).astype(np.uint32))


def wanted_words(prog, proofs):
    """(wc_var words, wc_bits words) of one instance's proofs"""
    ws = [np.frombuffer(p, dtype="<u8") for p in proofs]
    return (np.array([ws[k][pos] for k, pos in prog.wc_var[:, :2].tolist()], dtype=np.uint64),
            np.array([ws[k][pos] for k, pos in prog.wc_bits[:, :2].tolist()], dtype=np.uint64))


def word_check_cases(prog, proofs):
    """[(the instance's proofs, expected lowest failing wc_var index, ... wc_bits index)]: the recorded proofs; two copies flipped; two query
    indices flipped; one of each (the flips sit in the LAST child and, with two of a kind, out of table order)"""
    n_var, n_bits = prog.wc_var.shape[0], prog.wc_bits.shape[0]
    assert n_var >= 2 and n_bits >= 2

    def flipped(var_rows, bit_rows):
        words = [np.frombuffer(p, dtype="<u8").copy() for p in proofs]
        for k, pos in [prog.wc_var[r, :2].tolist() for r in var_rows] + [prog.wc_bits[r, :2].tolist() for r in bit_rows]:
            words[k][pos] ^= np.uint64(1)
        return [w.tobytes() for w in words]
    return [(list(proofs), NONE, NONE),
            (flipped([n_var - 1, n_var - 3], []), n_var - 3, NONE),
            (flipped([], [n_bits - 1, n_bits - 2]), NONE, n_bits - 2),
            (flipped([n_var - 2], [n_bits - 1]), n_var - 2, n_bits - 1)]


def check_word_cases(prog, proofs, consts, run):
    """run(values [B][n_values], tables, var_want [B][n_var], bit_want [B][n_bits]) -> (first_bad_var[B], first_bad_bits[B]) against
    WitnessProgram.check_words on the same words"""
    cases = word_check_cases(prog, proofs)
    inputs, _ = prog.inputs_from_words(proofs)
    vals = prog.evaluate(consts, inputs, threads=2)                         # the flipped words are not inputs: one evaluation serves every case
    want = [wanted_words(prog, c[0]) for c in cases]
    got_var, got_bits = run(np.tile(vals, (len(cases), 1)), word_tables(prog), np.array([w[0] for w in want]), np.array([w[1] for w in want]))
    for i, (words, bad_var, bad_bits) in enumerate(cases):
        assert (int(got_var[i]), int(got_bits[i])) == (bad_var, bad_bits), f"case {i}"
        _, ws = prog.inputs_from_words(words)
        text = prog.word_check_refusal(int(got_var[i]), int(got_bits[i]))
        if bad_var == NONE and bad_bits == NONE:
            prog.check_words(vals, ws)
            assert text is None
        else:
            with pytest.raises(ValueError) as e:
                prog.check_words(vals, ws)
            assert str(e.value) == text


@pytest.mark.parametrize("which", ["gates", "sha"])
def test_word_checks_equal_check_words(nodes, which):
    prog, proofs = nodes[which]
    lib = _lib()

    def run(values, tables, var_want, bit_want):
        B = values.shape[0]
        var_idx, bit_vars, bit_start = tables
        values, var_want, bit_want = (np.ascontiguousarray(a, dtype=np.uint64) for a in (values, var_want, bit_want))
        bad_var, bad_bits = np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
        assert lib.glp_witness_check_words_host(values.ctypes.data, values.shape[1], B, var_idx.ctypes.data, var_want.ctypes.data, var_idx.size,
                                                bit_vars.ctypes.data, bit_start.ctypes.data, bit_want.ctypes.data, bit_start.size - 1,
                                                bad_var.ctypes.data, bad_bits.ctypes.data) == 0
        return bad_var, bad_bits
    check_word_cases(prog, proofs, poseidon_consts("small"), run)
