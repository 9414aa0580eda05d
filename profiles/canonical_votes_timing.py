"""The Map of 104 signature leaves at 28 queries / 16 PoW bits on one MI355X, for canonical votes of differing lengths
(signature_mr.CanonicalVoteSetMapReduce, format for_commit("celestia", 0): 104 .. 110 bytes) against the fixed-length form
(SignatureSetMapReduce(msg_len=112), the code path before canonical votes).  Run from the repository root after build():
    python profiles/canonical_votes_timing.py [leaves]
Both objects live in the same process on the same three provers and alternate three times (as profiles/witness_device_timing.py does); the
Map is timed through _map: the Ed25519 witness kernel launch, the witness programs on the host pool, and the leaf proofs.  Both leaves are
2^16 rows x 144 wires, so the expectation is "equal within run-to-run spread": a record, not a gate.  Prints one JSON line per measurement."""
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 104
    pkg = graft.load_package()
    sm = importlib.import_module(graft.PKG_NAME + ".signature_mr")
    ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
    bs = importlib.import_module(graft.PKG_NAME + ".blobstream")
    rc, circ, diag = importlib.import_module(graft.PKG_NAME + ".poseidon_constants").default_constants()
    consts = tuple(np.array(a, dtype=np.uint64) for a in (rc, circ, diag))
    provers = [pkg.Prover(0) for _ in range(3)]
    for p in provers:
        p.set_poseidon_constants(*consts)
    fmt = bs.VoteFormat.for_commit("celestia", 0)
    objs = {"fixed_112": sm.SignatureSetMapReduce(provers[0], consts, msg_len=112, hash_offset=16, fan_in=8, map_provers=provers[1:]),
            "canonical": sm.CanonicalVoteSetMapReduce(provers[0], consts, fmt, fan_in=8, map_provers=provers[1:])}
    block = hashlib.sha256(b"block").digest()
    slots = {}
    for name, mr in objs.items():
        mr._record_leaf()
        st = mr.leaf_stats
        print(json.dumps({"leaf": name, "rows": st["rows"], "rows_used": st["rows_used"], "arith_gates": st["arith_gates"], "sha_rows": st["sha_rows"],
                          "field_products": st["field_products"], "record_seconds": mr.record_seconds["leaf"]}), flush=True)
        msgs = [mr.vote_bytes(block, i, height=4_000_000) if name == "canonical" else mr.vote_bytes(block, i) for i in range(n)]
        seeds = [hashlib.sha256(b"validator %d" % i).digest() for i in range(n)]
        signed = [ec.keypair_and_sign(s, m) for s, m in zip(seeds, msgs)]
        slots[name] = ([k[0] for k in signed], [k[1] for k in signed], msgs, [True] * n)
        if name == "canonical":
            print(json.dumps({"vote_lengths": sorted({len(m) for m in msgs})}), flush=True)
        mr._map(slots[name], 0, min(n, 6))                                      # warm-up: resident buffers, first launches
    times = {name: [] for name in objs}
    for rep in range(3):
        for name, mr in objs.items():
            t0 = time.perf_counter()
            proofs = mr._map(slots[name], 0, n)
            times[name].append(time.perf_counter() - t0)
            print(json.dumps({"rep": rep, "leaf": name, "leaves": len(proofs), "map_seconds": round(times[name][-1], 4),
                              "ms_per_leaf": round(1e3 * times[name][-1] / n, 3)}), flush=True)
    print(json.dumps({"leaves": n, "queries": 28, "pow_bits": 16,
                      **{f"{name}_median_s": round(statistics.median(t), 4) for name, t in times.items()},
                      **{f"{name}_spread_s": round(max(t) - min(t), 4) for name, t in times.items()}}), flush=True)
    for mr in objs.values():
        mr.free()
    for p in provers:
        p.close()


if __name__ == "__main__":
    main()
