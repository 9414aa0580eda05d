"""What batched placement and batched proving of Reduce levels gain (one MI355X, one process; run from the repository root after build(), under a
time limit of its own):
    timeout 1500 python profiles/reduce_batch_probe.py [out.json]                    # default: profiles/reduce_batch.json
    timeout 600 python profiles/reduce_batch_probe.py --only placement               # one part alone: placement | chain | range
Three parts, each with the two paths alternated REPEATS (>= 5) times after a warm-up, host clock around calls that end in a stream synchronise.
The comparison is always against prove_batch = 0 IN THE SAME RUN — the code path before batched Reduce levels existed, unchanged by them.
  placement : a resident slab of 8 data-commitment leaves (2^16 x 144) -> 8 resident wire matrices: eight DeviceWitnessBatch.device_witness calls
              against one device_witness_batch call
  chain     : reduce_seconds of the header-chain Reduce over 128 leaves of 8 headers (16 + 2 + 1 nodes; the chain of CombinedSkip(1024)),
              three provers, prove_batch = 0 against 8, host witnesses and device witnesses
  range     : reduce_seconds of the DataCommitment(4096) Reduce (64 leaves of 64 blocks: 8 + 1 nodes), three provers, prove_batch = 0 against
              k in {2, 4, 8}
28 queries, 16 PoW bits.  Reported per row: median and min - max of both paths, the baseline's own spread (max - min), and `gain` = the medians
differ by more than that spread.  The root proofs of both paths are compared byte for byte before anything is timed.  No retries: a failing
step ends the run."""
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

QUERIES, POW, REPEATS = 28, 16, 5


def summary(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def compare(base_ms, cand_ms):
    row = {"repeats": len(base_ms), "ms": {"baseline": summary(base_ms), "candidate": summary(cand_ms)}}
    spread = row["ms"]["baseline"]["max"] - row["ms"]["baseline"]["min"]
    row["baseline_spread_ms"] = round(spread, 3)
    row["candidate_over_baseline"] = round(row["ms"]["candidate"]["median"] / row["ms"]["baseline"]["median"], 4)
    row["gain"] = row["ms"]["baseline"]["median"] - row["ms"]["candidate"]["median"] > spread
    return row


def alternate(base, cand):
    t = ([], [])
    for _ in range(REPEATS):
        for k, fn in enumerate((base, cand)):
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return compare(*t)


def reduce_rows(mr, leaves, ks, witness_modes):
    """reduce(leaves) with prove_batch = 0 against each k, per witness mode; the same root proof from every configuration"""
    rows = []
    mr.prove_batch, mr.device_witness = 0, False
    ref = mr.reduce(leaves)                                                   # records the node circuits
    for dev in witness_modes:
        mr.device_witness = dev
        for k in ks:
            def run(kk):
                mr.prove_batch = kk
                levels = []
                out = mr.reduce(leaves, levels)
                return out, levels
            for kk in (0, k):                                                 # warm-up: replicas, group buffers, slabs
                out, levels = run(kk)
                if out[0] != ref[0] or not np.array_equal(out[2], ref[2]):
                    raise SystemExit(f"prove_batch = {kk}, device_witness = {dev}: the root proof differs")
            row = alternate(lambda: run(0), lambda k=k: run(k))
            row.update({"prove_batch": k, "device_witness": dev, "provers": 1 + len(mr.map_provers),
                        "nodes_per_level": [lv["nodes"] for lv in levels], "rows_per_level": [lv["rows"] for lv in levels]})
            print(json.dumps(row), flush=True)
            rows.append(row)
    mr.prove_batch, mr.device_witness = 0, False
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "reduce_batch.json"))
    ap.add_argument("--only", choices=["placement", "chain", "range"])
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
    res = {"device": torch.cuda.get_device_name(0), "num_queries": QUERIES, "pow_bits": POW,
           "timing": "host clock around calls that end in a stream synchronise; both paths warmed up, then alternating; baseline = prove_batch 0"}
    rng = np.random.default_rng(31)

    if args.only in (None, "placement", "range"):
        mr = dm.DataCommitmentMapReduce(pr, consts, leaf_blocks=64, fan_in=8, num_queries=QUERIES, pow_bits=POW, map_provers=provers[1:])
        heights = [3_000_000 + k for k in range(4096)]
        roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
        mr._record_leaf()
        if args.only in (None, "placement"):
            prog = mr.leaf_program
            words = prog.W << prog.log_n
            inputs = [[w for h, r in zip(heights[64 * k:64 * k + 64], roots[64 * k:64 * k + 64]) for w in dm.tuple_words(h, r)] for k in range(8)]
            slab = prog.evaluate_device(pr, inputs)
            out = pkg.DeviceBuffer(pr, 8 * words * 8)

            def eight_calls():
                pubs = [slab.device_witness(pr, i, out=out.ptr + i * words * 8)[1] for i in range(8)]
                pr.sync()
                return pubs

            def one_call():
                pubs = slab.device_witness_batch(pr, range(8), out)
                pr.sync()
                return pubs
            want = eight_calls()
            ref = out.download((8, words)).copy()
            out.upload(np.zeros((8, words), dtype=np.uint64))
            if one_call() != want or not np.array_equal(out.download((8, words)), ref):
                raise SystemExit("device_witness_batch differs from eight device_witness calls")
            row = alternate(eight_calls, one_call)
            row.update({"instances": 8, "log_n": prog.log_n, "n_wires": prog.W, "batched_call_counts": dict(zip(("launches", "host_syncs"), pr.witness_last_place_counts()))})
            print(json.dumps(row), flush=True)
            res["placement_8_leaves"] = row
            slab.free()
            out.free()
        if args.only in (None, "range"):
            leaves = mr.prove_leaves(heights, roots)
            res["data_commitment_4096_reduce"] = reduce_rows(mr, leaves, (2, 4, 8), (False,))
        mr.free()

    if args.only in (None, "chain"):
        ch = dm.HeaderChainMapReduce(pr, consts, leaf_headers=8, fan_in=8, num_queries=QUERIES, pow_bits=POW, map_provers=provers[1:])
        headers, _ = ch.synthetic_chain(1024)
        first = 1 << (7 * (ch.n_groups - 1))
        ch._record_leaf()
        hashes = [bytes(32)] + [ch.header_hash(h) for h in headers]
        leaves = ch._map_chain(hashes, first, headers, 0, len(headers))
        res["header_chain_128_leaves_reduce"] = reduce_rows(ch, leaves, (8,), (False, True))
        ch.free()

    if args.only is None:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for p in provers:
        p.close()


if __name__ == "__main__":
    main()
