"""B single native verifications on one host thread against ONE batched call (one MI355X, one process; run from the repository root after
build(), under a time limit of its own):
    timeout 600 python profiles/verify_batch_probe.py [out.json]            # default: profiles/verify_batch.json
Proofs: the data-commitment leaf of the bench (64 blocks per leaf: 2^16 rows x 144 wires, SHA rows and Poseidon rows), 28 queries, 16 PoW bits;
8 different witnesses of the recorded leaf program proved in one batched prover call, the B = 104 set holding each of them 13 times (as
separate byte strings).  Per B in (1, 8, 104):
  single : B calls of Prover.plonk_verify (glp_plonk_verify_ex), one after the other on this thread
  batch  : one Prover.plonk_verify_batch (glp_plonk_verify_batch), digests included
Both are warmed up, then alternate for REPEATS rounds; around each a host clock (wall) and the process's CPU seconds (user + system, every
thread of the process: the HIP runtime's included).  Medians and min - max.  Every proof must be accepted both ways, and one tampered proof
in the B = 8 set must be refused both ways with the same reason, before anything is timed.  No retries: a failing step ends the run."""
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

QUERIES, POW, LEAF_BLOCKS, REPEATS, NPROOFS = 28, 16, 64, 5, 8


def med(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verify_batch.json")
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
    rng = np.random.default_rng(1)
    heights = [3_000_000 + k for k in range(NPROOFS * LEAF_BLOCKS)]
    roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
    slab = pkg.DeviceBuffer(pr, NPROOFS * words * 8)
    addrs, pubs = [], []
    for i in range(NPROOFS):
        inp = [w for h, r in zip(heights[i * LEAF_BLOCKS:(i + 1) * LEAF_BLOCKS], roots[i * LEAF_BLOCKS:(i + 1) * LEAF_BLOCKS]) for w in dm.tuple_words(h, r)]
        addrs.append(slab.ptr + i * words * 8)
        pubs.append(prog.device_witness(pr, prog.evaluate(consts, inp, threads=1), out=addrs[-1])[1])
    pr.sync()
    proofs = [bytes(p) for p in ck.prove_batch_(addrs, pubs, QUERIES, POW)]
    slab.free()
    cap = ck.cap()
    publics = [[int(v) for v in p] for p in pubs]

    def single(ps, pbs):
        return [pr.plonk_verify(p, cap, QUERIES, POW, public=pb) for p, pb in zip(ps, pbs)]

    def batch(ps, pbs):
        return pr.plonk_verify_batch(ps, cap, QUERIES, POW, publics=pbs, want_digests=True)[0]

    bad = np.frombuffer(proofs[3], dtype="<u8").copy()
    bad[-7] ^= np.uint64(1)
    mixed = proofs[:3] + [bad.tobytes()] + proofs[4:]
    res = batch(mixed, publics)
    oks = single(mixed, publics[:3] + [publics[3]] + publics[4:])
    pr.plonk_verify(mixed[3], cap, QUERIES, POW, public=publics[3])
    if [r[0] for r in res] != oks or oks.count(False) != 1 or "proof rejected: " + res[3][1] != pr.last_reject:
        raise SystemExit(f"the two verifiers disagree: {res} / {oks} / {pr.last_reject}")
    rows = []
    for B in (1, 8, 104):
        ps = [bytes(bytearray(proofs[k % NPROOFS])) for k in range(B)]
        pbs = [publics[k % NPROOFS] for k in range(B)]
        if not all(single(ps, pbs)) or not all(r[0] for r in batch(ps, pbs)):          # the warm-up of both paths
            raise SystemExit(f"B = {B}: a proof of the recorded leaf is refused")
        counts = pr.verify_last_batch_counts()
        t = {"single": {"wall": [], "cpu": []}, "batch": {"wall": [], "cpu": []}}
        for _ in range(REPEATS):
            for name, fn in (("single", single), ("batch", batch)):
                c0, t0 = time.process_time(), time.perf_counter()
                fn(ps, pbs)
                t[name]["wall"].append((time.perf_counter() - t0) * 1e3)
                t[name]["cpu"].append((time.process_time() - c0) * 1e3)
        row = {"B": B, "repeats": REPEATS, "proof_bytes": len(ps[0]), "counts": counts,
               "single_wall_ms": med(t["single"]["wall"]), "single_cpu_ms": med(t["single"]["cpu"]),
               "batch_wall_ms": med(t["batch"]["wall"]), "batch_cpu_ms": med(t["batch"]["cpu"]),
               "wall_batch_over_single": round(statistics.median(t["batch"]["wall"]) / statistics.median(t["single"]["wall"]), 4),
               "cpu_batch_over_single": round(statistics.median(t["batch"]["cpu"]) / statistics.median(t["single"]["cpu"]), 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    mr.free()
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0),
                   "shape": {"leaf": "data commitment, 64 blocks", "log_n": prog.log_n, "n_wires": prog.W, "num_queries": QUERIES, "pow_bits": POW},
                   "timing": "host clock and process CPU seconds around B Prover.plonk_verify calls / one Prover.plonk_verify_batch call, both "
                             "through the Python wrappers (each copies the proof bytes once); warmed up, then alternating",
                   "rows": rows}, f, indent=1)
        f.write("\n")
    pr.close()


if __name__ == "__main__":
    main()
