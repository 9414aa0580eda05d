"""The witness kernels on the MI355X at the value edges of every op kind, against tests/witness_ref.py (Python integers, nothing shared with
the product): glp_witness_eval_kernel<true> / <false> on tests/witness_cases.py's edge program and glp_witness_eval_part_kernel<true> /
<false> on its segmented twin, all ~300 instances in one call each.  The slab is filled with a sentinel and value_stride is n_values + 3;
status, first failing pair and EVERY word of EVERY instance — refused ones too: a refused op writes 0 and the kernel goes on — must equal
the reference, the three variables no op writes must read 0 and the words past n_values must keep the sentinel.  The CPU twin of every
test here is in tests/test_witness_ops_edge.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import poseidon_consts  # noqa: E402
import witness_cases as wc  # noqa: E402
from test_gpu_witness_device import raw_device_eval  # noqa: E402


def check(prover, kind, rows, segmented):
    """the instances `rows` of the edge batch in one call; raw_device_eval fills the slab with 0xABCD and asserts the words past n_values"""
    consts = poseidon_consts(kind)
    prog, n_inputs, n_values, eq, seg, slots = wc.edge_program()
    batch, notes = wc.edge_batch()
    want = wc.reference(kind, consts, "device")
    prover.set_poseidon_constants(*consts)
    try:
        status, bad, vals = raw_device_eval(prover, prog, n_inputs, n_values, eq, batch[rows], pad=3, seg=seg if segmented else None)
    finally:
        prover.set_poseidon_constants(*poseidon_consts("small"))
    assert vals.shape == (len(rows), n_values)
    for n, b in enumerate(rows):
        rc, first_bad, values = want[b]
        # glp_witness_eval_device orders the kernel's flags the host's way: a refused op first (no pair index), then the lowest failing pair
        assert (int(status[n]), int(bad[n])) == (rc, first_bad), f"instance {b} ({notes[b]})"
        if vals[n].tobytes() != values.tobytes():
            k = int(np.flatnonzero(vals[n] != values)[0])
            nnf = [s for s, first in enumerate(slots["nnf_first"]) if first <= k < first + 44]
            raise AssertionError(f"instance {b} ({notes[b]}): variable {k} is {int(vals[n][k]):#x}, the reference says {int(values[k]):#x}; "
                                 f"{int((vals[n] != values).sum())} words differ" + (f"; NNF_MUL slot {nnf[0]}, word {k - slots['nnf_first'][nnf[0]]}" if nnf else ""))
        assert all(int(vals[n][u]) == 0 for u in slots["unwritten"]), f"instance {b}"


@pytest.mark.gpu
@pytest.mark.parametrize("segmented", [False, True], ids=["plain", "segmented"])
@pytest.mark.parametrize("kind", ["small", "big"])
def test_edge_batch_equals_the_reference(prover, kind, segmented):
    check(prover, kind, list(range(len(wc.edge_batch()[0]))), segmented)


@pytest.mark.gpu
@pytest.mark.parametrize("segmented", [False, True], ids=["plain", "segmented"])
@pytest.mark.parametrize("rows", [[0], [0, 1], [298], [299]], ids=["B1", "B2", "three-folds", "subtract"])
def test_grid_edges_and_uniform_wavefronts(prover, rows, segmented):
    """the batch cut to B = 1 and B = 2; and the two last instances alone, which hold ONE path in all 70 NNF_MUL slots — three folds in 298, the
    final subtraction in 299: wavefronts that do not diverge, where the whole batch's neighbouring lanes all take different paths"""
    _, notes = wc.edge_batch()
    assert "three times" in notes[298] and "final subtraction" in notes[299]
    check(prover, "small", rows, segmented)
