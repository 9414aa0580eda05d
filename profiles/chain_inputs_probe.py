"""What building the header-chain leaves' input vectors on the device costs against building them in Python (one MI355X, one process; run from
the repository root after build(), under a time limit of its own):
    timeout 600 python profiles/chain_inputs_probe.py [out.json]                   # default: profiles/chain_inputs.json
    timeout 1500 python profiles/chain_inputs_probe.py --map [out.json]            # also the Map step of 128 leaves, both ways
Chains of 1024 and 4096 headers of the default field lengths (400 bytes a header), 8 headers a leaf, 4 varint bytes.  The two paths are alternated
REPEATS (5) times after a warm-up, host clock around calls that end in a stream synchronise:
  parent   : what prove_chain does with device_witness on and device_inputs off before the evaluator runs — the header_hash loop, the
             validation loop of _map_chain, _chain_leaf_inputs per leaf, and the upload of the [n / 8][2913] vectors that evaluate_device does
  device   : ONE Prover.header_chain_leaf_inputs call on resident header bytes (4 launches, the statuses back, one synchronise)
  device+up: the same with the join and the upload of the headers' bytes included (what _map_chain_device does before the evaluator runs)
The rows and hashes of both paths are compared before anything is timed.  With --map: the Map step of a 1024-header chain (128 leaves, 28
queries, 16 PoW bits, one prover, device_witness on) with device_inputs off and on, alternated MAP_REPEATS (3) times after one warm-up of each —
exactly what prove_chain's map_seconds brackets (the parent's header_hash loop runs before that bracket, as in prove_chain, and is reported
beside it) — with the host CPU seconds (user + system of the process) of each run, and the leaf proofs compared byte for byte.  No threshold, no
retries: a failing step ends the run."""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

REPEATS, MAP_REPEATS, LEAF_HEADERS, GROUPS = 5, 3, 8, 4


def summary(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def cpu_seconds():
    t = os.times()
    return t.user + t.system


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "chain_inputs.json"))
    ap.add_argument("--map", action="store_true")
    args = ap.parse_args()
    pkg = graft.load_package()
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    bs = importlib.import_module(graft.PKG_NAME + ".blobstream")
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    prover = pkg.Prover(0)
    prover.set_poseidon_constants(*consts)
    mr = dm.HeaderChainMapReduce(prover, consts, leaf_headers=LEAF_HEADERS, fan_in=8, height_varint_bytes=GROUPS, device_witness=True)
    layout = pkg.HeaderChainLayout.of(mr.field_lengths, LEAF_HEADERS, GROUPS)
    width = layout.n_words()
    rng = random.Random(1)
    first, start = 2_500_000, rng.randbytes(32)
    res = {"header_bytes": layout.header_bytes(), "leaf_headers": LEAF_HEADERS, "row_words": width, "repeats": REPEATS, "build_inputs_ms": {}}

    def chain(n):
        prev, out = start, []
        for k in range(n):
            f = [rng.randbytes(ln) for ln in mr.field_lengths]
            f[2] = b"\x08" + bs.encode_varint(first + k)
            f[4] = b"\x0a\x20" + prev + f[4][34:]
            f[6] = b"\x0a\x20" + f[6][2:]
            out.append(f)
            prev = mr.header_hash(f)
        return out

    def parent(headers):
        n = len(headers)
        hashes = [start] + [mr.header_hash(h) for h in headers]
        for k in range(n):                                               # the validation loop of _map_chain
            f = headers[k]
            if bytes(f[4])[:34] != b"\x0a\x20" + hashes[k]:
                raise ValueError(k)
            if bytes(f[2]) != b"\x08" + bs.encode_varint(first + k) or bytes(f[6])[:2] != b"\x0a\x20":
                raise ValueError(k)
        rows = np.ascontiguousarray([dm._chain_leaf_inputs(hashes[k], first + k, headers[k:k + LEAF_HEADERS], GROUPS) for k in range(0, n, LEAF_HEADERS)],
                                    dtype=np.uint64)
        return prover.to_device(rows), rows, hashes

    for n in (1024, 4096):
        headers = chain(n)
        buf, want, hashes = parent(headers)
        buf.free()
        blob = np.frombuffer(b"".join(x for h in headers for x in h), dtype=np.uint8)
        d_hdr = prover.to_device(blob)
        d_in, status, d_hashes = prover.header_chain_leaf_inputs(layout, d_hdr, start, first, n)
        counts = prover.header_chain_last_input_counts()
        assert not status.any() and np.array_equal(d_in.download((n // LEAF_HEADERS, width)), want), "the device rows differ from _chain_leaf_inputs"
        assert d_hashes.download((n + 1, 32), dtype=np.uint8).tobytes() == b"".join(hashes), "the device hashes differ from header_hash"
        t_parent, t_dev, t_dev_up = [], [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            b, _, _ = parent(headers)
            t_parent.append(1e3 * (time.perf_counter() - t0))
            b.free()
            t0 = time.perf_counter()
            prover.header_chain_leaf_inputs(layout, d_hdr, start, first, n, out=d_in, hashes=d_hashes)
            t_dev.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            up = prover.to_device(np.frombuffer(b"".join(x for h in headers for x in h), dtype=np.uint8))
            prover.header_chain_leaf_inputs(layout, up, start, first, n, out=d_in, hashes=d_hashes)
            t_dev_up.append(1e3 * (time.perf_counter() - t0))
            up.free()
        res["build_inputs_ms"][str(n)] = {"parent_python": summary(t_parent), "device_call_resident": summary(t_dev),
                                          "device_call_with_upload": summary(t_dev_up), "launches": counts[0], "synchronises": counts[1],
                                          "rows_and_hashes_equal": True}
        for b in (d_hdr, d_in, d_hashes):
            b.free()
        if n == 1024:
            map_headers = headers
    if args.map:
        headers, n = map_headers, 1024
        outs, times, cpu, t_hash = {}, {False: [], True: []}, {False: [], True: []}, []

        def run(on):
            mr.device_inputs = on
            if on:
                c0, t0 = cpu_seconds(), time.perf_counter()
                leaves = mr._map_chain_device(start, first, headers, 0, n)[0]
            else:
                t_h = time.perf_counter()
                hashes = [start] + [mr.header_hash(h) for h in headers]          # outside prove_chain's bracket, as in prove_chain
                t_hash.append(1e3 * (time.perf_counter() - t_h))
                c0, t0 = cpu_seconds(), time.perf_counter()
                leaves = mr._map_chain(hashes, first, headers, 0, n)
            return leaves, 1e3 * (time.perf_counter() - t0), cpu_seconds() - c0
        mr._record_leaf()
        for on in (False, True):
            run(on)                                                              # warm-up of each path
        t_hash.clear()
        for _ in range(MAP_REPEATS):
            for on in (False, True):
                outs[on], ms, c = run(on)
                times[on].append(ms)
                cpu[on].append(c)
        assert outs[True] == outs[False], "the leaf proofs differ"
        off, on_ = summary(times[False]), summary(times[True])
        res["map"] = {"leaves": n // LEAF_HEADERS, "repeats": MAP_REPEATS, "map_ms_device_inputs_off": off, "map_ms_device_inputs_on": on_,
                      "header_hash_loop_before_the_bracket_ms_off": summary(t_hash),
                      "host_cpu_seconds_off": summary(cpu[False]), "host_cpu_seconds_on": summary(cpu[True]), "leaf_proofs_equal": True,
                      "difference_of_medians_ms": round(off["median"] - on_["median"], 3), "baseline_spread_ms": round(off["max"] - off["min"], 3),
                      "difference_exceeds_baseline_spread": abs(off["median"] - on_["median"]) > off["max"] - off["min"]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    mr.free()
    prover.close()


if __name__ == "__main__":
    main()
