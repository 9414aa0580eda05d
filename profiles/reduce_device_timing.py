"""Host evaluator versus device-side witness generation for the Reduce step (one MI355X; run from the repository root after build(), every
step under a time limit of its own):
    timeout 600 python profiles/reduce_device_timing.py node 16            # (a) one 16-child node of 2^16 x 80 leaf proofs
    timeout 900 python profiles/reduce_device_timing.py reduce chain       # (b) the chain Reduce: 128 leaves of 8 headers, fan-in 8
    timeout 900 python profiles/reduce_device_timing.py reduce signatures  # (b) the signature Reduce: 104 leaves, fan-in 8, padded root
    timeout 600 rocprofv3 --kernel-trace --stats -d DIR -- python profiles/reduce_device_timing.py kernels 16     # (c) kernel time per launch
The host and device paths alternate three times in one process; one JSON line per measurement, medians in the last line."""
import hashlib
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


def setup(n_provers):
    pkg = graft.load_package()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    provers = [pkg.Prover(0) for _ in range(n_provers)]
    for p in provers:
        p.set_poseidon_constants(*consts)
    return pkg, consts, provers


def bench_node(pkg, consts, pr, fan):
    """the node of recursion_witness_breakdown.py: `fan` proofs of the bench's 2^16 x 80 leaf circuit under one RecursionProgram"""
    import bench
    vcm = importlib.import_module(graft.PKG_NAME + ".verifier_circuit")
    cs, sigmas, wires = bench.synthetic_circuit(pr, 16, 80)
    ck = pkg.PlonkCircuit(pr, cs, sigmas)
    dw = pr.to_device(wires)
    proofs = [ck.prove_(dw, 28, 16) for _ in range(fan)]
    return vcm.RecursionProgram(pr, proofs, ck.cap(), 28, 16, 80, consts), proofs


def node(fan):
    pkg, consts, (pr,) = setup(1)
    rp, proofs = bench_node(pkg, consts, pr, fan)
    prog = rp.program
    t0 = time.perf_counter()
    parts = prog.plan_parts()
    print(json.dumps({"fan": fan, "stats": rp.stats, "plan_seconds": round(time.perf_counter() - t0, 3), "single_workgroup_plan": prog.plan_stats(),
                      "parts_ops_depth_steps": [tuple(p.values()) for p in parts]}), flush=True)

    def host_path():
        c0, t0 = time.process_time(), time.perf_counter()
        inputs, ws = prog.inputs_from_words(proofs)
        vals = prog.evaluate(rp.consts, inputs)
        prog.check_words(vals, ws)
        dw, pub = prog.device_witness(pr, vals, reuse=True)
        pr.sync()
        return time.perf_counter() - t0, time.process_time() - c0, pub

    def device_path():
        c0, t0 = time.process_time(), time.perf_counter()
        dw, pub = rp.witness_batch([proofs]).device_witness(pr, 0, reuse=True)
        pr.sync()
        return time.perf_counter() - t0, time.process_time() - c0, pub
    host_path(), device_path()                                    # warm-up: the plan's upload, the slab, the wire buffer
    rows = []
    for rep in range(3):
        hw, hc, hp = host_path()
        dw, dc, dp = device_path()
        assert hp == dp
        rows.append((hw, dw, hc, dc))
        print(json.dumps({"rep": rep, "wires_resident_host_ms": round(1e3 * hw, 3), "wires_resident_device_ms": round(1e3 * dw, 3),
                          "cpu_host_s": round(hc, 4), "cpu_device_s": round(dc, 4)}), flush=True)
    med = [statistics.median(r[k] for r in rows) for k in range(4)]
    assert rp.prove(proofs) == rp.prove(proofs, device_witness=True)
    print(json.dumps({"median": True, "wires_resident_host_ms": round(1e3 * med[0], 3), "wires_resident_device_ms": round(1e3 * med[1], 3),
                      "cpu_host_s": round(med[2], 4), "cpu_device_s": round(med[3], 4)}), flush=True)


def kernels(fan):
    """one evaluation of the node through each device path (the segmented plan's three launches, the single-workgroup kernel), for a kernel trace"""
    pkg, consts, (pr,) = setup(1)
    rp, proofs = bench_node(pkg, consts, pr, fan)
    inputs, _ = rp.program.inputs_from_words(proofs)
    for segments in (True, False, True, False):
        t0 = time.perf_counter()
        slab = rp.program.evaluate_device(pr, [inputs], segments=segments)
        print(json.dumps({"segments": segments, "wall_ms_first_call_includes_upload": round(1e3 * (time.perf_counter() - t0), 3)}), flush=True)
        slab.free()


def reduce(what):
    pkg, consts, provers = setup(3)
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    if what == "chain":
        mr = dm.HeaderChainMapReduce(provers[0], consts, leaf_headers=8, fan_in=8, map_provers=provers[1:])
        headers, _ = mr.synthetic_chain(8 * 128)
        first = 1 << (7 * (mr.n_groups - 1))
        run = lambda: mr.prove_chain(bytes(32), first, headers)
    else:
        sm = importlib.import_module(graft.PKG_NAME + ".signature_mr")
        ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
        mr = sm.SignatureSetMapReduce(provers[0], consts, msg_len=112, hash_offset=16, fan_in=8, map_provers=provers[1:])
        block = hashlib.sha256(b"block").digest()
        msgs = [mr.vote_bytes(block, i) for i in range(104)]
        keys = [ec.keypair_and_sign(hashlib.sha256(b"validator %d" % i).digest(), m) for i, m in enumerate(msgs)]
        run = lambda: mr.prove_set([k[0] for k in keys], [k[1] for k in keys], msgs, [True] * 104)
    roots = {}
    for on in (False, True):                                      # warm-up of both paths: every circuit recorded, every plan made and resident
        mr.device_witness = on
        roots[on] = run()["root_proof"]
    assert roots[False] == roots[True]
    rows = []
    for rep in range(3):
        row = {"what": what, "rep": rep}
        for on in (False, True):
            mr.device_witness = on
            c0 = time.process_time()
            out = run()
            row["reduce_seconds_device" if on else "reduce_seconds_host"] = out["reduce_seconds"]
            row["process_cpu_s_device" if on else "process_cpu_s_host"] = round(time.process_time() - c0, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"what": what, "median": True, "levels": out["levels"],
                      "reduce_seconds_host": statistics.median(r["reduce_seconds_host"] for r in rows),
                      "reduce_seconds_device": statistics.median(r["reduce_seconds_device"] for r in rows)}), flush=True)
    mr.free()


if __name__ == "__main__":
    {"node": lambda: node(int(sys.argv[2])), "kernels": lambda: kernels(int(sys.argv[2])), "reduce": lambda: reduce(sys.argv[2])}[sys.argv[1]]()
