"""One glp_fri_prove_batch call against B sequential glp_fri_prove calls (one MI355X, one process; run from the repository root after
build(), under a time limit of its own):
    timeout 900 python profiles/fri_batch_probe.py [out.json]            # default: profiles/fri_batch.json
    timeout 300 python profiles/fri_batch_probe.py --only sequential --B 1 --reps 5     # one configuration alone, for a kernel trace
    timeout 300 python profiles/fri_batch_probe.py --only batched --B 8 --reps 5
Shape: the opening proof of a 2^16-row x 144-wire leaf as plonk.hip hands it to FRI — four batches (preprocessed: 10 constant + 144 sigma
columns, ONE commitment shared by all instances; 144 wires; 2 x 18 partial products; 2 << 3 quotient chunks), masks 1, 1, 3, 1, points
(1, w_n), rate 3, cap 4, arity 4, final 5, 28 queries, 16 PoW bits.  The committed data is random (an opening proof does not care).
  baseline  : B sequential glp_fri_prove calls on the same ctx (the single-proof path, unchanged)
  candidate : one glp_fri_prove_batch call
Both are warmed up, then alternate for REPEATS rounds; a host clock around each (both end in a stream synchronise).  Reported: median and
min - max of both, the baseline's spread, and `gain` = the medians differ by more than the baseline's own spread (max - min).  The proofs
of both paths are compared byte for byte before anything is timed.  No retries: a failing step ends the run."""
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

LOG_N, RB, CAP, ARITY, FINAL, QUERIES, POW = 16, 3, 4, 4, 5, 28, 16
N_POLYS = [10 + 144, 144, 2 * 18, 2 << RB]
MASKS = [1, 1, 3, 1]
REPEATS = 20


def commit(pkg, pr, torch, gen, B, k):
    """B commitments of k random polynomials through glp_commit_values_batch -> B PolynomialBatch views (+ the tensors that own the memory)"""
    n, N = 1 << LOG_N, 1 << (LOG_N + RB)
    nd = pkg.Prover.merkle_digest_len(LOG_N + RB, CAP)
    vals = torch.randint(0, 1 << 62, (B * k, n), dtype=torch.int64, device="cuda", generator=gen)      # canonical: < p
    lde = torch.empty((B * k, N), dtype=torch.int64, device="cuda")
    dig = torch.empty((B, nd), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    caps = np.zeros((B, 1 << CAP, 4), dtype=np.uint64)
    pr._chk(pr.lib.glp_commit_values_batch(pr.ctx, vals.data_ptr(), k, LOG_N, RB, CAP, B, lde.data_ptr(), dig.data_ptr(), nd, caps.ctypes.data),
            "glp_commit_values_batch")
    views = []
    for b in range(B):
        pb = pkg.PolynomialBatch(pr, k, LOG_N, RB, CAP)
        pb.coeffs, pb.lde, pb.digests, pb.cap = vals.data_ptr() + b * k * n * 8, lde.data_ptr() + b * k * N * 8, dig.data_ptr() + b * nd * 8, caps[b]
        views.append(pb)
    return views, (vals, lde, dig)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "fri_batch.json"))
    ap.add_argument("--only", choices=["sequential", "batched"])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = graft.load_package()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    pr = pkg.Prover(0)
    pr.set_poseidon_constants(*(np.array(a, dtype=np.uint64) for a in pc.default_constants()))
    gen = torch.Generator(device="cuda").manual_seed(16)
    w_n = pow(pkg.field_params()[0], 1 << (32 - LOG_N), pkg.P)
    kw = dict(arity_bits=ARITY, final_poly_bits=FINAL, num_queries=QUERIES, pow_bits=POW, point_mults=(1, w_n), open_masks=MASKS)
    Bs = [args.B] if args.only else [1, 2, 4, 8, 16]
    Bmax = max(Bs)
    pre, keep = commit(pkg, pr, torch, gen, 1, N_POLYS[0])
    cols = [[pre[0]] * Bmax]
    for k in N_POLYS[1:]:
        v, own = commit(pkg, pr, torch, gen, Bmax, k)
        cols.append(v)
        keep = keep + own
    instances = [[col[i] for col in cols] for i in range(Bmax)]

    def sequential(B):
        return [pr.fri_prove(instances[i], RB, CAP, **kw) for i in range(B)]

    def batched(B):
        return pr.fri_prove_batch(instances[:B], RB, CAP, **kw)

    if args.only:
        fn = sequential if args.only == "sequential" else batched
        for _ in range(args.reps):
            fn(args.B)
        print(json.dumps({"only": args.only, "B": args.B, "calls": args.reps}))
        pr.close()
        return
    plan = pkg.Prover.fri_prove_batch_plan(LOG_N, RB, CAP, MASKS, arity_bits=ARITY, final_poly_bits=FINAL, num_queries=QUERIES, pow_bits=POW,
                                           point_mults=(1, w_n))
    rows = []
    for B in Bs:
        ref = sequential(B)                                            # warm-up, and the same bytes from both paths
        if batched(B) != ref:
            raise SystemExit(f"B = {B}: the batched proofs differ from glp_fri_prove's")
        counts = pr.fri_last_batch_counts()
        t = {"sequential": [], "batched": []}
        for _ in range(REPEATS):
            for name, fn in (("sequential", sequential), ("batched", batched)):
                t0 = time.perf_counter()
                fn(B)
                t[name].append((time.perf_counter() - t0) * 1e3)
        row = {"B": B, "repeats": REPEATS, "ms": {}, "batched_call_counts": {"launches": counts[0], "host_syncs": counts[1], "pow_windows": counts[2]}}
        for name, v in t.items():
            row["ms"][name] = {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
        spread = row["ms"]["sequential"]["max"] - row["ms"]["sequential"]["min"]
        row["baseline_spread_ms"] = round(spread, 3)
        row["ms_per_proof"] = {k: round(row["ms"][k]["median"] / B, 3) for k in row["ms"]}
        row["batched_over_sequential"] = round(row["ms"]["batched"]["median"] / row["ms"]["sequential"]["median"], 4)
        row["gain"] = row["ms"]["sequential"]["median"] - row["ms"]["batched"]["median"] > spread
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "shape": {"log_n": LOG_N, "n_polys": N_POLYS, "open_masks": MASKS, "points": "(1, w_n)",
                   "rate_bits": RB, "cap_height": CAP, "arity_bits": ARITY, "final_poly_bits": FINAL, "num_queries": QUERIES, "pow_bits": POW},
                   "plan_per_call": {"launches": plan[0], "host_syncs": plan[1]},
                   "timing": "host clock around calls that end in a stream synchronise; both paths warmed up, then alternating", "rows": rows}, f, indent=1)
        f.write("\n")
    pr.close()


if __name__ == "__main__":
    main()
