"""Dependency depth of the witness programs this repository records (CPU only; run from the repository root after build()):
    python profiles/witness_depth.py
Level of an op = 0 when it reads no variable, else 1 + the highest level among the producers of its operands.  Prints one table row per
program: ops, variables, depth, median and widest level, barrier-separated steps at 64 / 256 / 1024 lanes (sum over levels of
ceil(width / lanes)), and what glp_witness_plan_stats reports for the same program."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

OP_LEN = [8, 3, 4, 3, 5, 2, 25, 10, 6, 6, 4, 5, 26, 9, 24]
OP_NAME = ["ARITH", "INPUT", "BIT", "INV", "EINV", "ZERO", "POSEIDON", "SHA_E", "SHA_A", "SHA_W", "ADD32", "BITS", "POSEIDON_SWAP", "EXTMULADD", "NNF_MUL"]
WRITES = {0: [0], 1: [0], 2: [0], 3: [0], 4: [0, 1], 5: [0], 6: list(range(12)), 7: [0, 1], 8: [0], 9: [0], 10: [0], 11: [0], 12: list(range(12)), 13: [0, 1]}
READS = {0: [1, 2, 3], 1: [], 2: [1], 3: [1], 4: [2, 3], 5: [], 6: list(range(12, 24)), 7: list(range(2, 8)), 8: [1, 2, 3, 4], 9: [1, 2, 3, 4], 10: [1, 2],
         11: [1], 12: list(range(12, 25)), 13: list(range(2, 8)), 14: list(range(1, 23))}


def levels(prog, n_values):
    prog = prog.tolist()
    lvl = [0] * n_values
    widths, kinds, pc = {}, [0] * 15, 0
    while pc < len(prog):
        k = prog[pc]
        a = prog[pc + 1: pc + OP_LEN[k]]
        m = max((lvl[a[i]] + 1 for i in READS[k]), default=0)
        for w in (range(a[0], a[0] + 44) if k == 14 else (a[i] for i in WRITES[k])):
            lvl[w] = m
        widths[m] = widths.get(m, 0) + 1
        kinds[k] += 1
        pc += OP_LEN[k]
    return np.array([widths[i] for i in range(len(widths))]), kinds


def row(name, prog):
    w, kinds = levels(prog.prog, prog.n_values)
    steps = {lanes: int(np.sum((w + lanes - 1) // lanes)) for lanes in (64, 256, 1024)}
    print(json.dumps({"program": name, "ops": int(w.sum()), "variables": prog.n_values, "depth": int(w.size), "median_width": float(np.median(w)),
                      "max_width": int(w.max()), "steps": steps, "kinds": {OP_NAME[k]: c for k, c in enumerate(kinds) if c}, "plan": prog.plan_stats()}))


def main():
    from conftest import poseidon_consts
    from test_witness_plan import golden_verifier_program
    graft.load_package()
    ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
    msg = b"vote: block 4000000 round 0, validator 17".ljust(112, b".")
    pub, sig = ec.keypair_and_sign(bytes(range(32)), msg)
    b, _ = ec.ed25519_circuit(object(), pub, sig, msg)
    row("ed25519 signature leaf, 112-byte message", b.program())
    oracle = graft.load_oracle()
    import ctypes
    u64p = ctypes.POINTER(ctypes.c_uint64)
    oracle.orc_poseidon_set_constants.argtypes = [u64p, u64p, u64p]
    oracle.orc_poseidon_permute.argtypes = [u64p]
    consts = poseidon_consts("small")
    for which in ("plonk", "gates", "sha"):
        _, prog, _ = golden_verifier_program(oracle, which, consts)
        row(f"verifier circuit of golden proof {which}", prog)


if __name__ == "__main__":
    main()
