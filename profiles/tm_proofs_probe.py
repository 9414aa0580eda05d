"""Inclusion proofs on the device: forest build, audit paths and batched verification against what the library had before (one MI355X; run from
the repository root after build(), under a time limit of its own):
    timeout 600 python profiles/tm_proofs_probe.py [out.json]        # default: profiles/tm_proofs.json
Shapes: one range of 4096 DataRootTuples (64-byte leaves); 64 ranges of 64 tuples in one call; verification of 4096 proofs in one call.
  forest        : glp_tm_forest_create (no host roots) + glp_tm_forest_proofs of EVERY leaf, the leaf bytes resident on the device
  root_var      : (a) the only way to the same roots before: glp_tm_merkle_root_var per tree (it keeps no level, so it gives no path)
  hashlib_paths : (b) the level-wise hashlib loop on the host that keeps every level and reads every leaf's aunts
  verify        : glp_tm_verify_inclusion_batch of all the proofs, arrays resident
  hashlib_verify: (b) the same walk in hashlib, one proof after the other
The device configurations are timed by device events on the ctx's stream (glp_timer_start / glp_timer_stop; the stop synchronises) AND by the
host clock around the same call; the hashlib ones by the host clock.  Every configuration is warmed up once, then REPEATS rounds in which the
configurations alternate, so a slow stretch of a shared machine hits them alike.  Reported: min / median / max and the interquartile range.
The only condition is correctness, checked before anything is timed: the forest's roots equal root_var's byte for byte, its aunts equal the
hashlib loop's, and every proof is accepted.  Nothing is gated on the times."""
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

REPEATS = 15


def hashlib_levels(leaves):
    levels = [[hashlib.sha256(b"\x00" + x).digest() for x in leaves]]
    while len(levels[-1]) > 1:
        lv = levels[-1]
        levels.append([hashlib.sha256(b"\x01" + lv[i] + lv[i + 1]).digest() if i + 1 < len(lv) else lv[i] for i in range(0, len(lv), 2)])
    return levels


def hashlib_paths(trees):
    roots, paths = [], []
    for leaves in trees:
        levels = hashlib_levels(leaves)
        roots.append(levels[-1][0])
        for i in range(len(leaves)):
            aunts, idx = [], i
            for lv in levels[:-1]:
                if (idx ^ 1) < len(lv):
                    aunts.append(lv[idx ^ 1])
                idx >>= 1
            paths.append(aunts)
    return roots, paths


def hashlib_verify(root, leaf, index, total, aunts):
    h, used = hashlib.sha256(b"\x00" + leaf).digest(), 0
    while total > 1:
        if (index ^ 1) < total:
            h = hashlib.sha256(b"\x01" + (aunts[used] + h if index & 1 else h + aunts[used])).digest()
            used += 1
        index, total = index >> 1, (total + 1) // 2
    return h == root and used == len(aunts)


def summary(t):
    t = sorted(t)
    q = statistics.quantiles(t, n=4)
    return {"min": round(t[0], 4), "median": round(statistics.median(t), 4), "max": round(t[-1], 4), "iqr": round(q[2] - q[0], 4)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tm_proofs.json")
    pkg = graft.load_package()
    pr = pkg.Prover(0)
    lib = pr.lib
    rng = np.random.default_rng(4096)
    rows = []
    for n_trees, per_tree in ((1, 4096), (64, 64)):
        total = n_trees * per_tree
        trees = [[(1_000_000 + t * per_tree + i).to_bytes(32, "big") + rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for i in range(per_tree)]
                 for t in range(n_trees)]
        flat = [x for t in trees for x in t]
        offs = np.arange(total + 1, dtype=np.uint64) * 64
        first = np.arange(n_trees + 1, dtype=np.uint64) * per_tree
        stride = (per_tree - 1).bit_length()
        d_data = pr.to_device(np.frombuffer(b"".join(flat), dtype=np.uint8))
        d_offs = pr.to_device(offs)
        d_aunts, d_na, d_lh = pr.alloc(total * stride * 32), pr.alloc(total * 4), pr.alloc(total * 32)
        root = ctypes.create_string_buffer(32)
        state = {}

        def forest():
            h = ctypes.c_void_p()
            pr._chk(lib.glp_tm_forest_create(pr.ctx, d_data.ptr, total * 64, offs.ctypes.data, first.ctypes.data, total, n_trees, None, ctypes.byref(h)),
                    "glp_tm_forest_create")
            state["create"] = pr.tm_forest_last_counts()
            pr._chk(lib.glp_tm_forest_proofs(pr.ctx, h, None, None, total, d_aunts.ptr, stride, d_na.ptr, d_lh.ptr), "glp_tm_forest_proofs")
            state["proofs"] = pr.tm_forest_last_counts()
            if "forest" in state:
                lib.glp_tm_forest_destroy(state["forest"])
            state["forest"] = h

        def root_var():
            out = []
            for t in range(n_trees):
                pr._chk(lib.glp_tm_merkle_root_var(pr.ctx, d_data.ptr + t * per_tree * 64, per_tree * 64, d_offs.ptr, per_tree, root), "glp_tm_merkle_root_var")
                out.append(root.raw)
            state["roots_var"] = out

        def host_paths():
            state["host"] = hashlib_paths(trees)

        configs = [("forest", forest, True), ("root_var", root_var, True), ("hashlib_paths", host_paths, False)]
        for _, fn, _dev in configs:                                     # warm-up, then correctness before anything is timed
            fn()
        pr.sync()

        def roots_ptr():                                                # of the forest that is alive now: every forest() call replaces it
            p = ctypes.c_void_p()
            pr._chk(lib.glp_tm_forest_roots(state["forest"], ctypes.byref(p)), "glp_tm_forest_roots")
            return p.value

        got_roots = np.zeros((n_trees, 32), dtype=np.uint8)
        pr._chk(lib.glp_d2h(pr.ctx, got_roots.ctypes.data, roots_ptr(), n_trees * 32), "glp_d2h")
        got_roots = [got_roots[t].tobytes() for t in range(n_trees)]
        if got_roots != state["roots_var"] or got_roots != state["host"][0]:
            raise SystemExit(f"{n_trees} x {per_tree}: the forest's roots differ from glp_tm_merkle_root_var's")
        aunts, na = d_aunts.download((total, stride, 32), dtype=np.uint8), d_na.download(total, dtype=np.uint32)
        for q, path in enumerate(state["host"][1]):
            if int(na[q]) != len(path) or [aunts[q, k].tobytes() for k in range(len(path))] != path:
                raise SystemExit(f"{n_trees} x {per_tree}: the aunts of leaf {q} differ from the hashlib loop's")
        # verification of all the proofs: arrays resident
        d_index = pr.to_device(np.tile(np.arange(per_tree, dtype=np.uint64), n_trees))
        d_total = pr.to_device(np.full(total, per_tree, dtype=np.uint64))
        root_of = np.repeat(np.arange(n_trees, dtype=np.uint32), per_tree)
        status = np.zeros(total, dtype=np.int32)

        def verify():
            pr._chk(lib.glp_tm_verify_inclusion_batch(pr.ctx, roots_ptr(), n_trees, root_of.ctypes.data, d_data.ptr, total * 64, offs.ctypes.data,
                                                      d_index.ptr, d_total.ptr, d_aunts.ptr, stride, d_na.ptr, total, status.ctypes.data),
                    "glp_tm_verify_inclusion_batch")
            state["verify"] = pr.tm_forest_last_counts()

        def host_verify():
            roots, paths = state["host"]
            state["host_ok"] = all(hashlib_verify(roots[q // per_tree], flat[q], q % per_tree, per_tree, paths[q]) for q in range(total))

        configs += [("verify", verify, True), ("hashlib_verify", host_verify, False)]
        verify()
        host_verify()
        if status.any() or not state["host_ok"]:
            raise SystemExit(f"{n_trees} x {per_tree}: a valid proof was refused")
        dev_ms, wall_ms = {name: [] for name, _, dev in configs if dev}, {name: [] for name, _, _ in configs}
        for _ in range(REPEATS):
            for name, fn, dev in configs:
                if dev:
                    pr.sync()
                t0 = time.perf_counter()
                if dev:
                    pr.timer_start()
                fn()
                if dev:
                    dev_ms[name].append(pr.timer_stop())
                wall_ms[name].append((time.perf_counter() - t0) * 1e3)
        info = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()]
        pr._chk(lib.glp_tm_forest_info(state["forest"], *[ctypes.byref(x) for x in info]), "glp_tm_forest_info")
        row = {"trees": n_trees, "leaves_per_tree": per_tree, "leaf_bytes": 64, "proofs": total, "repeats": REPEATS,
               "device_event_ms": {k: summary(v) for k, v in dev_ms.items()}, "host_clock_ms": {k: summary(v) for k, v in wall_ms.items()},
               "launches_syncs": {"forest_create": state["create"], "forest_proofs": state["proofs"], "verify": state["verify"]},
               "forest_bytes": info[3].value, "roots_equal_root_var": True, "aunts_equal_hashlib": True}
        row["forest_over_root_var"] = round(row["device_event_ms"]["forest"]["median"] / row["device_event_ms"]["root_var"]["median"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        lib.glp_tm_forest_destroy(state["forest"])
        for b in (d_data, d_offs, d_aunts, d_na, d_lh, d_index, d_total):
            b.free()
    import torch
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0),
                   "timing": "device events on one stream and the host clock around the same calls, configurations alternating; hashlib on the host clock",
                   "rows": rows}, f, indent=1)
        f.write("\n")
    pr.close()


if __name__ == "__main__":
    main()
