#!/usr/bin/env python3
"""tests/golden/gen_verify_batch_l2.py — writes tests/golden/verify_batch_l2.json ON AN MI355X: one proof of the build-defined W = 8 circuit at
log_n = 13 with 4 queries, made by the GPU prover from seeded inputs with the package's default Poseidon constants.  At the prover's default
arity (4 bits) and final polynomial (5 bits) it has L = 2 fold layers of 16-to-1 — the shape every real proof has and none of the proofs in
proofs.json has — in a few tens of KB.  The batched verifier's tests (tests/verify_batch_cases.py) tamper it at every 7th word.
Usage (GPU box, repo root):  python tests/golden/gen_verify_batch_l2.py [out.json]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import __graft_entry__ as graft  # noqa: E402
import plonk_ref as pref  # noqa: E402
from conftest import poseidon_consts  # noqa: E402

L2 = {"seed": 20261020, "log_n": 13, "W": 8, "queries": 4, "pow_bits": 4}


def make(pkg, prover):
    rc, circ, diag = poseidon_consts("small")
    prover.set_poseidon_constants(rc, circ, diag)
    c = pref.build_circuit(np.random.default_rng(L2["seed"]), L2["log_n"], L2["W"])
    ck = pkg.PlonkCircuit(prover, c["consts"], c["sigmas"])
    proof = ck.prove(c["wires"], L2["queries"], L2["pow_bits"])
    assert ck.verify(proof, L2["queries"], L2["pow_bits"]), prover.last_reject
    cap = ck.cap()
    ck.free()
    return dict(L2, note="made by tests/golden/gen_verify_batch_l2.py on an MI355X; Poseidon constants = poseidon_constants.default_constants()",
                circuit_cap=[int(v) for v in cap], proof=proof.hex())


if __name__ == "__main__":
    pkg = graft.load_package()
    pr = pkg.Prover(0)
    out = make(pkg, pr)
    pr.close()
    for path in sys.argv[1:] or [os.path.join(HERE, "verify_batch_l2.json")]:
        with open(path, "w") as f:
            json.dump(out, f)
    print("wrote verify_batch_l2.json:", len(out["proof"]) // 2, "bytes")
