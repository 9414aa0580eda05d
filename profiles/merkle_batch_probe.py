"""B Merkle trees per call against B calls: which levels are worth fusing (one MI355X; run from the repository root after build(), under a
time limit of its own):
    timeout 600 python profiles/merkle_batch_probe.py [out.json]        # default: profiles/merkle_batch.json
Shapes: the signature leaf's wires and quotient commitments — 2^19 leaves, cap 4, 144 / 16 polynomials — for B = 1, 4, 8 trees.
  baseline   : B sequential glp_merkle_from_polys calls on one ctx, h_cap given (a copy and a synchronise per tree) — how commit_values calls it
  under test : one glp_merkle_batch call, h_caps given, at fuse_max_log 0, 9, 12, 15, 19 and at the library's default
Device events on the ctx's stream around each call (glp_timer_start / glp_timer_stop; the stop synchronises), every configuration warmed up
once, then REPEATS rounds in which the configurations alternate, so a slow stretch of a shared box hits them alike.  Reported per
configuration: min / median / max; for the baseline also its spread over the repeats (interquartile range and max - min).  Every batched
setting's digests are compared with the baseline's on the device before anything is timed.  `accept` = the default's median is no more than
the baseline's median plus the baseline's interquartile range."""
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

LOG_LEAVES, CAP_H = 19, 4
REPEATS = 15
FUSE = [0, 9, 12, 15, LOG_LEAVES, None]          # None = GLP_MERKLE_FUSE_DEFAULT


def launches_today(log_leaves, cap_h, coop_max=16384, top_nodes=64):
    """launches of one glp_merkle / glp_merkle_from_polys call (csrc/hash.hip: merkle_impl), leaf hashing included"""
    n, lvl = 1, log_leaves
    while lvl > cap_h:
        out = 1 << (lvl - 1)
        n += 1
        if out <= top_nodes and out <= coop_max:
            break
        lvl -= 1
    return n


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merkle_batch.json")
    pkg = graft.load_package()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    pr = pkg.Prover(0)
    pr.set_poseidon_constants(*(np.array(a, dtype=np.uint64) for a in pc.default_constants()))
    N = 1 << LOG_LEAVES
    nd = pkg.Prover.merkle_digest_len(LOG_LEAVES, CAP_H)
    gen = torch.Generator(device="cuda").manual_seed(19)
    results = []
    for leaf_len in (144, 16):
        # canonical field elements need only be < p: 62 random bits
        src = torch.randint(0, 1 << 62, (8 * leaf_len, N), dtype=torch.int64, device="cuda", generator=gen)
        ref = torch.zeros((8, nd), dtype=torch.int64, device="cuda")
        got = torch.zeros((8, nd), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        cap = np.zeros((1 << CAP_H, 4), dtype=np.uint64)
        caps = np.zeros((8, 1 << CAP_H, 4), dtype=np.uint64)
        for B in (1, 4, 8):
            def baseline():
                for b in range(B):
                    pr._chk(pr.lib.glp_merkle_from_polys(pr.ctx, src.data_ptr() + b * leaf_len * N * 8, N, leaf_len, LOG_LEAVES, CAP_H,
                                                         ref.data_ptr() + b * nd * 8, cap.ctypes.data), "glp_merkle_from_polys")

            def batched(fuse):
                pr._chk(pr.lib.glp_merkle_batch(pr.ctx, src.data_ptr(), leaf_len * N, 1, N, leaf_len, LOG_LEAVES, CAP_H, B,
                                                pkg.MERKLE_FUSE_DEFAULT if fuse is None else fuse, got.data_ptr(), nd, caps.ctypes.data),
                        "glp_merkle_batch")

            configs = [("baseline", baseline)] + [("default" if f is None else f"fuse_{f}", (lambda f=f: batched(f))) for f in FUSE]
            # warm-up, and the same digests from every setting
            baseline()
            for name, fn in configs[1:]:
                got.zero_()
                torch.cuda.synchronize()
                fn()
                pr.sync()
                if not torch.equal(got[:B], ref[:B]):
                    raise SystemExit(f"{name}: digests differ from the baseline's at leaf_len {leaf_len}, B {B}")
            times = {name: [] for name, _ in configs}
            for _ in range(REPEATS):
                for name, fn in configs:
                    pr.timer_start()
                    fn()
                    times[name].append(pr.timer_stop())
            row = {"log_leaves": LOG_LEAVES, "cap_h": CAP_H, "leaf_len": leaf_len, "B": B, "repeats": REPEATS, "ms": {}}
            for name, t in times.items():
                t = sorted(t)
                row["ms"][name] = {"min": round(t[0], 4), "median": round(statistics.median(t), 4), "max": round(t[-1], 4)}
            q = statistics.quantiles(times["baseline"], n=4)
            row["baseline_spread_ms"] = {"iqr": round(q[2] - q[0], 4), "max_minus_min": round(max(times["baseline"]) - min(times["baseline"]), 4)}
            row["launches_per_tree"] = {"baseline": launches_today(LOG_LEAVES, CAP_H), "baseline_copies_and_syncs": 1}
            row["launches_per_call"] = {}
            for f in FUSE:
                n, nf = pkg.Prover.merkle_batch_plan(LOG_LEAVES, CAP_H, f)
                row["launches_per_call"]["default" if f is None else f"fuse_{f}"] = {"launches": n, "fused": nf}
            best = min((k for k in row["ms"] if k.startswith("fuse_")), key=lambda k: row["ms"][k]["median"])
            row["best"] = best
            row["default_over_baseline"] = round(row["ms"]["default"]["median"] / row["ms"]["baseline"]["median"], 4)
            row["accept"] = row["ms"]["default"]["median"] <= row["ms"]["baseline"]["median"] + row["baseline_spread_ms"]["iqr"]
            print(json.dumps(row), flush=True)
            results.append(row)
        del src, ref, got
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "timing": "device events on one stream, configurations alternating", "rows": results}, f,
                  indent=1)
        f.write("\n")
    pr.close()


if __name__ == "__main__":
    main()
