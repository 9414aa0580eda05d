"""One glp_plonk_prove_batch call against B sequential glp_plonk_prove_ex calls (one MI355X, one process; run from the repository root after
build(), under a time limit of its own):
    timeout 900 python profiles/plonk_batch_probe.py [out.json]            # default: profiles/plonk_batch.json
    timeout 300 python profiles/plonk_batch_probe.py --only batched --B 8 --reps 5        # one configuration alone, for a kernel trace
Shape: the data-commitment leaf of the bench (64 blocks per leaf: 2^16 rows x 144 wires, SHA rows and Poseidon rows), 28 queries, 16 PoW bits;
B different witnesses of the recorded leaf program, laid side by side on the device once.
  baseline  : B sequential glp_plonk_prove_ex calls on the same ctx (the single-proof path, unchanged: the reference)
  candidate : one glp_plonk_prove_batch call
Both are warmed up, then alternate for REPEATS rounds; a host clock around each (both end in a stream synchronise).  Reported: median and
min - max of both, the baseline's spread, `gain` = the medians differ by more than the baseline's own spread (max - min), the launches and
synchronises per batched call from the two counts entry points, and the stage times (glp_last_stage_ms, profiling on, one extra call each) of
B single calls summed against one batched call.  The proofs of both paths are compared byte for byte before anything is timed.
Then the Map step of 64 such leaves, three ways: three ctxs with prove_batch = 0 (the bench's configuration), one ctx with prove_batch = 8,
three ctxs with prove_batch = 8.  No retries: a failing step ends the run."""
import argparse
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

QUERIES, POW, LEAF_BLOCKS, REPEATS, MAP_LEAVES = 28, 16, 64, 12, 64


def ranges(n_leaves, seed):
    rng = np.random.default_rng(seed)
    heights = [3_000_000 + k for k in range(n_leaves * LEAF_BLOCKS)]
    return heights, [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]


def stage_sum(pr, calls):
    """stage name -> ms, summed over the calls (each a thunk), with profiling on"""
    pr.set_profiling(1)
    out = {}
    try:
        for call in calls:
            call()
            for name, ms in pr.last_stage_ms():
                out[name] = out.get(name, 0.0) + ms
    finally:
        pr.set_profiling(0)
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "plonk_batch.json"))
    ap.add_argument("--only", choices=["sequential", "batched"])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-map", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    provers = [pkg.Prover(0) for _ in range(3)]
    for p in provers:
        p.set_poseidon_constants(*consts)
    pr = provers[0]
    Bs = [args.B] if args.only else [1, 2, 4, 8]
    Bmax = max(Bs)

    mr = dm.DataCommitmentMapReduce(pr, consts, leaf_blocks=LEAF_BLOCKS, num_queries=QUERIES, pow_bits=POW)
    mr._record_leaf()
    prog, ck = mr.leaf_program, mr.leaf_circuit
    words = prog.W << prog.log_n
    heights, roots = ranges(Bmax, 1)
    slab = pkg.DeviceBuffer(pr, Bmax * words * 8)
    addrs, pubs = [], []
    for i in range(Bmax):
        inp = [w for h, r in zip(heights[i * LEAF_BLOCKS:(i + 1) * LEAF_BLOCKS], roots[i * LEAF_BLOCKS:(i + 1) * LEAF_BLOCKS]) for w in dm.tuple_words(h, r)]
        addrs.append(slab.ptr + i * words * 8)
        pubs.append(prog.device_witness(pr, prog.evaluate(consts, inp, threads=1), out=addrs[-1])[1])
    pr.sync()

    def sequential(B):
        return [ck.prove_(addrs[i], QUERIES, POW, public=pubs[i]) for i in range(B)]

    def batched(B):
        return ck.prove_batch_(addrs[:B], pubs[:B], QUERIES, POW)

    if args.only:
        fn = sequential if args.only == "sequential" else batched
        for _ in range(args.reps):
            fn(args.B)
        print(json.dumps({"only": args.only, "B": args.B, "calls": args.reps}))
        return
    rows = []
    for B in Bs:
        ref = sequential(B)                                            # warm-up, and the same bytes from both paths
        if batched(B) != ref or len(set(ref)) != B:
            raise SystemExit(f"B = {B}: the batched proofs differ from glp_plonk_prove_ex's")
        counts = pr.plonk_last_batch_counts(), pr.fri_last_batch_counts()
        t = {"sequential": [], "batched": []}
        for _ in range(REPEATS):
            for name, fn in (("sequential", sequential), ("batched", batched)):
                t0 = time.perf_counter()
                fn(B)
                t[name].append((time.perf_counter() - t0) * 1e3)
        row = {"B": B, "repeats": REPEATS, "ms": {},
               "batched_call_counts": {"plonk_launches": counts[0][0], "plonk_host_syncs": counts[0][1], "fri_launches": counts[1][0],
                                       "fri_host_syncs": counts[1][1], "pow_windows": counts[1][2]}}
        for name, v in t.items():
            row["ms"][name] = {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
        spread = row["ms"]["sequential"]["max"] - row["ms"]["sequential"]["min"]
        row["baseline_spread_ms"] = round(spread, 3)
        row["ms_per_proof"] = {k: round(row["ms"][k]["median"] / B, 3) for k in row["ms"]}
        row["batched_over_sequential"] = round(row["ms"]["batched"]["median"] / row["ms"]["sequential"]["median"], 4)
        row["gain"] = row["ms"]["sequential"]["median"] - row["ms"]["batched"]["median"] > spread
        row["stage_ms"] = {"sequential": stage_sum(pr, [lambda i=i: ck.prove_(addrs[i], QUERIES, POW, public=pubs[i]) for i in range(B)]),
                           "batched": stage_sum(pr, [lambda: batched(B)])}
        print(json.dumps(row), flush=True)
        rows.append(row)
    slab.free()
    mr.free()

    map_rows = []
    if not args.no_map:
        heights, roots = ranges(MAP_LEAVES, 2)
        for n_ctx, k in ((3, 0), (1, 8), (3, 8)):
            m = dm.DataCommitmentMapReduce(pr, consts, leaf_blocks=LEAF_BLOCKS, num_queries=QUERIES, pow_bits=POW, map_provers=provers[1:n_ctx], prove_batch=k)
            m._record_leaf()
            warm = 8 * n_ctx * LEAF_BLOCKS
            first = m.prove_leaves(heights[:warm], roots[:warm])
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                leaves = m.prove_leaves(heights, roots)
                ts.append((time.perf_counter() - t0) * 1e3)
            if leaves[:len(first)] != first or (map_rows and leaves[0] != map_rows[0]["_first"]):
                raise SystemExit("the Map step's leaf proofs differ between configurations")
            map_rows.append({"ctxs": n_ctx, "prove_batch": k, "leaves": MAP_LEAVES, "ms": {"min": round(min(ts), 1), "median": round(statistics.median(ts), 1),
                                                                                         "max": round(max(ts), 1)},
                             "ms_per_leaf": round(statistics.median(ts) / MAP_LEAVES, 2), "_first": leaves[0]})
            print(json.dumps({k2: v for k2, v in map_rows[-1].items() if k2 != "_first"}), flush=True)
            m.free()
        for r in map_rows:
            del r["_first"]
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0),
                   "shape": {"leaf": "data commitment, 64 blocks", "log_n": prog.log_n, "n_wires": prog.W, "num_queries": QUERIES, "pow_bits": POW},
                   "timing": "host clock around calls that end in a stream synchronise; both paths warmed up, then alternating", "rows": rows,
                   "map_step": map_rows}, f, indent=1)
        f.write("\n")
    for p in provers:
        p.close()


if __name__ == "__main__":
    main()
