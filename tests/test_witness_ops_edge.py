"""The witness evaluator's op kinds at their value edges against tests/witness_ref.py, an interpreter in Python integers that shares nothing
with the product — where the other witness tests compare one of the product's evaluators with another (they share glp_wit_exec,
glp_nnf::mul_hints and the glp_sha_* helpers, so a wrong value they agree on passes).  CPU only: the host entry points glp_witness_eval,
glp_witness_eval_mt and glp_witness_plan_run_host (plain and segmented plan), the emulated kernels of tests/emu_witness and
tests/emu_witness_seg, the builder's own nnf_mul_hints / bit_field, and csrc/nnf25519.h alone as a program under AddressSanitizer + UBSan.
The program and the ~300 instances are tests/witness_cases.py's; tests/test_gpu_witness_ops.py runs the same on the MI355X.  Every
comparison is equality of 64-bit words."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import poseidon_consts  # noqa: E402
import __graft_entry__ as graft  # noqa: E402
import witness_cases as wc  # noqa: E402
import witness_ref as ref  # noqa: E402
from test_emu_witness import NONE, emu_eval, emu_witness  # noqa: E402,F401
from test_emu_witness_segments import emu_seg  # noqa: E402,F401
from test_witness_plan import Plan  # noqa: E402
from test_witness_segments import SegPlan  # noqa: E402

KINDS = ["small", "big"]


def same_words(got, want, what):
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    if got.tobytes() != want.tobytes():
        k = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: variable {k} is {int(got[k]):#x}, the reference says {int(want[k]):#x} ({int((got != want).sum())} words differ)")


def test_reference_reaches_every_path():
    """what the reference alone says about the NNF_MUL cases, before anything is compared with them"""
    classes = wc.nnf_classes()
    groups, stats = wc.nnf_paths()
    print(stats, {g: len(c) for g, c in groups.items()}, {n: len(c) for n, c in classes.items()})
    assert all(n > 0 for n in stats["folds"])                              # 0, 1, 2 and 3 folds
    assert stats["subtract"] >= 20 and stats["three_folds"] >= 16 and stats["negative_carry"] >= 30
    assert len(classes["N3"]) >= 19 and all(ref.nnf_path(a, b)[:2] == (2, True) for a, b in classes["N3"])
    assert len(classes["N4"]) >= 16 and all(ref.nnf_path(a, b)[0] == 3 for a, b in classes["N4"])
    assert len(classes["N5"]) >= 100
    n2 = [ref.nnf_path(a, b) for a, b in classes["N2"]]
    assert any(p[:2] == (0, False) for p in n2) and any(p[:2] == (0, True) for p in n2)
    assert any(all(w == 0 for w in ref.nnf_mul(a, b)[:11]) for a, b in classes["N2"])          # r = 0
    assert len(classes["N7_refused"]) == 22 and all(ref.nnf_mul(a, b) is None for a, b in classes["N7_refused"])
    assert all(ref.nnf_mul(a, b) is not None for a, b in classes["N7_accepted"] + classes["N1"] + classes["N0"])
    # the verdicts of the batch: every kind of refusal, and most instances accepted
    batch, notes = wc.edge_batch()
    verdicts = [(rc, bad) for rc, bad, _ in wc.reference("small", poseidon_consts("small"), "device")]
    assert len(batch) == 300 and sum(v == (0, NONE) for v in verdicts) >= 200
    assert {(-1, NONE), (-7, NONE), (-7, 0), (-7, 2)} <= set(verdicts)
    for note, v in zip(notes, verdicts):
        if note.startswith("INPUT 0x"):
            assert v == (-1, NONE), note                                   # the malformed input decides, with and without a refused row
        if "2^28" in note or "2^35" == note[-4:] or "SHA word 2^32" in note or "2^63" in note:
            assert v == (-7, NONE), note
        if note in ("free T1 2^35 - 1", "free T1 2^32", "SHA words all 0xFFFFFFFF", "SHA words all 0", "INPUT p - 1 everywhere a field element goes"):
            assert v == (0, NONE), note


@pytest.mark.parametrize("kind", KINDS)
def test_host_entry_points_equal_the_reference(kind):
    """glp_witness_eval, glp_witness_eval_mt on 2 threads with the segment bounds, glp_witness_plan_run_host on the plain and the segmented plan"""
    consts = poseidon_consts(kind)
    prog, n_inputs, n_values, eq, seg, _ = wc.edge_program()
    batch, notes = wc.edge_batch()
    want = wc.reference(kind, consts, "host")
    plain, segmented = Plan(prog, n_inputs, n_values, eq), SegPlan(prog, n_inputs, n_values, eq, seg)
    assert plain.rc == 0 and segmented.rc == 0 and len(segmented.parts()) == 4
    try:
        for b, (inputs, (rc, bad, values)) in enumerate(zip(batch, want)):
            for name, got in (("glp_witness_eval", plain.eval_host(consts, inputs)), ("glp_witness_eval_mt", segmented.eval_mt(consts, inputs, threads=2)),
                              ("plan_run_host", plain.run_host(consts, inputs)), ("plan_run_host segmented", segmented.run_host(consts, inputs))):
                assert (got[0], got[1]) == (rc, bad), f"{name}, instance {b} ({notes[b]})"
                if rc == 0 or bad != NONE:                                 # every op ran
                    same_words(got[2], values, f"{name}, instance {b} ({notes[b]})")
    finally:
        plain.close()
        segmented.close()


def emu_seg_eval(lib, prog, n_inputs, n_values, eq, seg, consts, batch, grid, seg_grid, block=64, pad=3):
    """the three launches of a segmented plan on the emulated kernel; verdicts turned into the ABI's like test_emu_witness.emu_eval"""
    c384 = np.concatenate(consts).astype(np.uint64)
    small = int(all(int(v) < (1 << 24) for v in np.concatenate(consts[1:])))
    inp = np.ascontiguousarray(batch, dtype=np.uint64).reshape(len(batch), n_inputs)
    B, stride = inp.shape[0], n_values + pad
    vals = np.full((B, stride), wc.SENTINEL, dtype=np.uint64)
    status, bad = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint64)
    rc = lib.emu_witness_eval_seg(prog.ctypes.data, prog.size, n_inputs, n_values, eq.ctypes.data, eq.size // 2, seg.ctypes.data, seg.size - 1,
                                  c384.ctypes.data, small, inp.ctypes.data, vals.ctypes.data, stride, B, grid, seg_grid, block, status.ctypes.data,
                                  bad.ctypes.data)
    assert rc == 0
    assert np.all(vals[:, n_values:] == wc.SENTINEL)                       # words past n_values are left alone
    return [((int(status[b]), NONE) if status[b] != 0 else (-7, int(bad[b])) if int(bad[b]) != NONE else (0, NONE)) + (vals[b, :n_values],)
            for b in range(B)]


def check_device_form(got, want, notes, what):
    """every instance, refused ones included: verdict, first failing pair and every word"""
    _, _, _, _, _, slots = wc.edge_program()
    assert len(got) == len(want)
    for b, ((rc_d, bad_d, vals_d), (rc, bad, values)) in enumerate(zip(got, want)):
        assert (rc_d, bad_d) == (rc, bad), f"{what}, instance {b} ({notes[b]})"
        same_words(vals_d, values, f"{what}, instance {b} ({notes[b]})")
        assert all(int(vals_d[u]) == 0 for u in slots["unwritten"])


@pytest.mark.parametrize("kind", KINDS)
def test_emulated_kernels_equal_the_reference(emu_witness, emu_seg, kind):  # noqa: F811
    """tests/emu_witness (glp_witness_eval_kernel) and tests/emu_witness_seg (the three launches of glp_witness_eval_part_kernel) on fewer
    workgroups than instances"""
    consts = poseidon_consts(kind)
    prog, n_inputs, n_values, eq, seg, _ = wc.edge_program()
    batch, notes = wc.edge_batch()
    want = wc.reference(kind, consts, "device")
    assert emu_eval.__defaults__ == (64, 3)                                # block, pad: emu_eval fills with 0xABCD and checks the words past n_values
    check_device_form(emu_eval(emu_witness, prog, n_inputs, n_values, eq, consts, batch, grid=7), want, notes, "emu_witness")
    check_device_form(emu_seg_eval(emu_seg, prog, n_inputs, n_values, eq, seg, consts, batch, grid=5, seg_grid=11), want, notes, "emu_witness_seg")


def test_builder_values_equal_the_reference():
    """CircuitBuilder.nnf_mul_hints and bit_field compute their witness values a third way: all NNF classes and the BITS grid"""
    graft.load_package()
    rec = importlib.import_module(graft.PKG_NAME + ".recursion")
    classes = wc.nnf_classes()
    for name, cases in classes.items():
        for n, (a, b) in enumerate(cases):
            bld = rec.CircuitBuilder(object())
            av, bv = [bld.var(v) for v in a], [bld.var(v) for v in b]
            if name == "N7_refused":
                with pytest.raises(ValueError, match="out of range"):
                    bld.nnf_mul_hints(av, bv)
                continue
            r, k, c = bld.nnf_mul_hints(av, bv)
            assert tuple(bld.values[v] for v in r + k + c) == ref.nnf_mul(a, b), f"{name}[{n}]"
    bld = rec.CircuitBuilder(object())
    for x in wc.BIT_EDGES + wc.FIELD_EDGES:
        xv = bld.var(x)
        for shift, bits in wc.BITS_GRID:
            assert bld.values[bld.bit_field(xv, shift, bits)] == (x >> shift) % (1 << bits), (x, shift, bits)
        for k in wc.BIT_KS:
            assert bld.values[bld.bit(xv, k)] == (x >> k) & 1, (x, k)


def test_nnf_header_alone_under_sanitizers():
    """csrc/nnf25519.h as a stand-alone program built with AddressSanitizer + UBSan: every NNF case, refused ones included"""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_witness")
    subprocess.run(["make", "-s", "sanitized"], cwd=d, check=True)
    cases = [ab for cs in wc.nnf_classes().values() for ab in cs]
    text = "".join(" ".join(str(v) for v in a + b) + "\n" for a, b in cases)
    r = subprocess.run([os.path.join(d, "nnf_hints_san")], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for n, ((a, b), line) in enumerate(zip(cases, lines)):
        want = ref.nnf_mul(a, b)
        got = [int(w) for w in line.split()]
        assert got == ([1] + list(want) if want is not None else [0] * 45), f"case {n}: {a} x {b}"
