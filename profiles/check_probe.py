"""What the witness checker costs beside the proof of the same witnesses (one MI355X, one process; run from the repository root after build(),
under a time limit of its own):
    timeout 600 python profiles/check_probe.py [out.json]            # default: profiles/check_witness.json
Shape: the data-commitment leaf of the bench (64 blocks per leaf: 2^16 rows x 144 wires, SHA rows and Poseidon rows), 28 queries, 16 PoW bits;
B = 1 and B = 8 different witnesses of the recorded leaf program, laid side by side on the device once.
  first check : glp_plonk_check_witness[_batch] on a key that has not been checked yet — with the once-per-key decode of sigma (a fresh commitment
                of the same circuit per sample)
  check       : the same call on a key whose sigma is decoded (steady state)
  prove       : glp_plonk_prove_ex (B = 1) / glp_plonk_prove_batch (B = 8) on the same witnesses
check and prove are warmed up, then alternate for REPEATS rounds, a host clock around each (both end in a stream synchronise); medians and
min - max.  The yardstick: the K7 + K7s stage of that proof (glp_last_stage_ms, profiling on: 'quotient(K7)+to_coeffs', which also holds the
public-input LDE and the way back to coefficients) evaluates the same gate bodies on 8n points where the checker evaluates them on n.  Every
checked witness must be satisfied (a probe of a failing path would time something else).  No retries: a failing step ends the run."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

QUERIES, POW, LEAF_BLOCKS, REPEATS, FIRST_SAMPLES = 28, 16, 64, 12, 3


def med(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "check_witness.json")
    import torch
    pkg = graft.load_package()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    pr = pkg.Prover(0)
    pr.set_poseidon_constants(*consts)
    mr = dm.DataCommitmentMapReduce(pr, consts, leaf_blocks=LEAF_BLOCKS, num_queries=QUERIES, pow_bits=POW)
    mr._record_leaf()
    prog, ck = mr.leaf_program, mr.leaf_circuit
    words = prog.W << prog.log_n
    Bmax = 8
    rng = np.random.default_rng(1)
    heights = [3_000_000 + k for k in range(Bmax * LEAF_BLOCKS)]
    roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
    slab = pkg.DeviceBuffer(pr, Bmax * words * 8)
    addrs, pubs = [], []
    for i in range(Bmax):
        inp = [w for h, r in zip(heights[i * LEAF_BLOCKS:(i + 1) * LEAF_BLOCKS], roots[i * LEAF_BLOCKS:(i + 1) * LEAF_BLOCKS]) for w in dm.tuple_words(h, r)]
        addrs.append(slab.ptr + i * words * 8)
        pubs.append(prog.device_witness(pr, prog.evaluate(consts, inp, threads=1), out=addrs[-1])[1])
    pr.sync()

    def check(key, B):
        res = key.check_batch_(addrs[:B], pubs[:B], max_list=4) if B > 1 else [key.check_(addrs[0], pubs[0], max_list=4)]
        if not all(r.ok for r in res):
            raise SystemExit(f"B = {B}: a witness of the recorded leaf program is refused: {res}")

    def prove(B):
        return ck.prove_batch_(addrs[:B], pubs[:B], QUERIES, POW) if B > 1 else [ck.prove_(addrs[0], QUERIES, POW, public=pubs[0])]

    rows = []
    for B in (1, 8):
        first = []
        for _ in range(FIRST_SAMPLES):
            fresh = prog.setup(pr)                      # the same circuit committed again: a key that has never been checked
            pr.sync()
            t0 = time.perf_counter()
            check(fresh, B)
            first.append((time.perf_counter() - t0) * 1e3)
            first_counts = pr.plonk_last_check_counts()
            fresh.free()
        check(ck, B)                                    # (the first one of this key decodes its sigma)
        check(ck, B)
        counts = pr.plonk_last_check_counts()
        prove(B)
        t = {"check": [], "prove": []}
        for _ in range(REPEATS):
            for name, fn in (("check", lambda: check(ck, B)), ("prove", lambda: prove(B))):
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        pr.set_profiling(1)
        try:
            prove(B)
            stages = {name: round(ms, 3) for name, ms in pr.last_stage_ms()}
        finally:
            pr.set_profiling(0)
        k7 = stages.get("quotient(K7)+to_coeffs")
        row = {"B": B, "repeats": REPEATS, "first_check_ms": med(first), "check_ms": med(t["check"]), "prove_ms": med(t["prove"]),
               "first_check_counts": {"launches": first_counts[0], "host_syncs": first_counts[1]},
               "check_counts": {"launches": counts[0], "host_syncs": counts[1]},
               "prove_stage_ms": stages, "k7_stage_ms": k7,
               "check_over_prove": round(statistics.median(t["check"]) / statistics.median(t["prove"]), 4),
               "check_over_k7_stage": round(statistics.median(t["check"]) / k7, 4) if k7 else None}
        print(json.dumps(row), flush=True)
        rows.append(row)
    slab.free()
    mr.free()
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0),
                   "shape": {"leaf": "data commitment, 64 blocks", "log_n": prog.log_n, "n_wires": prog.W, "n_routed": ck.n_routed, "num_queries": QUERIES,
                             "pow_bits": POW},
                   "timing": "host clock around calls that end in a stream synchronise; check and prove warmed up, then alternating", "rows": rows}, f, indent=1)
        f.write("\n")
    pr.close()


if __name__ == "__main__":
    main()
