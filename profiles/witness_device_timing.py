"""Host evaluator pool versus device-side witness evaluation for one Map step (MI355X; run from the repository root after build()):
    python profiles/witness_device_timing.py signatures 104      # 104 signature leaves, 112-byte votes
    python profiles/witness_device_timing.py chain 128           # 128 header-chain leaves of 8 headers
The two paths alternate three times.  Per pair: witness wall time (inputs on the host -> every variable resident on the device), host CPU
seconds spent evaluating, and the whole Map (witness + prove) with the keyword off and on.  Prints one JSON line per measurement."""
import hashlib
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def main():
    what, n = sys.argv[1], int(sys.argv[2])
    map_too = len(sys.argv) < 4 or sys.argv[3] != "witness-only"
    pkg = graft.load_package()
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    sm = importlib.import_module(graft.PKG_NAME + ".signature_mr")
    ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
    rc, circ, diag = importlib.import_module(graft.PKG_NAME + ".poseidon_constants").default_constants()
    consts = tuple(np.array(a, dtype=np.uint64) for a in (rc, circ, diag))
    provers = [pkg.Prover(0) for _ in range(3)]
    for p in provers:
        p.set_poseidon_constants(*consts)
    if what == "signatures":
        mr = sm.SignatureSetMapReduce(provers[0], consts, msg_len=112, hash_offset=16, fan_in=8, map_provers=provers[1:])
        mr._record_leaf()
        block = hashlib.sha256(b"block").digest()
        inputs = []
        for i in range(n):
            msg = mr.vote_bytes(block, i)
            pub, sig = ec.keypair_and_sign(hashlib.sha256(b"validator %d" % i).digest(), msg)
            inputs.append(ec.witness_inputs(pub, sig, msg, True))
    else:
        mr = dm.HeaderChainMapReduce(provers[0], consts, leaf_headers=8, fan_in=8, map_provers=provers[1:])
        mr._record_leaf()
        headers, _ = mr.synthetic_chain(8 * n)
        first = 1 << (7 * (mr.n_groups - 1))
        hashes = [bytes(32)] + [mr.header_hash(h) for h in headers]
        inputs = [dm._chain_leaf_inputs(hashes[k], first + k, headers[k:k + 8], mr.n_groups) for k in range(0, 8 * n, 8)]
    prog = mr.leaf_program
    t0 = time.perf_counter()
    stats = prog.plan_stats()
    print(json.dumps({"what": what, "leaves": n, "variables": prog.n_values, "plan": stats, "plan_seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    stride = prog.n_values + prog.fixed_values.size
    pr = provers[0]
    dst = pkg.DeviceBuffer(pr, n * stride * 8)

    def host_path():
        """the pool of 12 single-thread evaluators + one upload per leaf into a [n][stride] device block"""
        cpu = []

        def ev(inp):
            c0 = time.thread_time()
            v = prog.evaluate(consts, inp, threads=1)
            cpu.append(time.thread_time() - c0)
            return v
        t0 = time.perf_counter()
        with ThreadPoolExecutor(12) as pool:
            futs = [pool.submit(ev, inp) for inp in inputs]
            for i, f in enumerate(futs):
                v = f.result()
                pr._chk(pr.lib.glp_h2d(pr.ctx, dst.ptr + i * stride * 8, v.ctypes.data, v.nbytes), "glp_h2d")
        pr.sync()
        return time.perf_counter() - t0, sum(cpu)

    def device_path(slab):
        c0, t0 = time.process_time(), time.perf_counter()
        slab = prog.evaluate_device(pr, inputs, slab=slab)
        pr.sync()
        return time.perf_counter() - t0, time.process_time() - c0, slab

    slab = prog.evaluate_device(pr, inputs)                      # warm-up: the plan's upload, the slab's allocation
    host_path()
    for rep in range(3):
        hw, hc = host_path()
        dw, dc, slab = device_path(slab)
        print(json.dumps({"what": what, "rep": rep, "witness_wall_host_s": round(hw, 4), "witness_wall_device_s": round(dw, 4),
                          "witness_cpu_host_s": round(hc, 4), "witness_cpu_device_s": round(dc, 4),
                          "device_ms_per_instance": round(1e3 * dw / n, 3)}), flush=True)
    check = slab.download(n - 1)
    assert np.array_equal(check, prog.evaluate(consts, inputs[-1], threads=1))
    slab.free()
    dst.free()
    if map_too:
        for rep in range(3):
            row = {"what": what, "rep": rep}
            for on in (False, True):
                mr.device_witness = on
                t0 = time.perf_counter()
                proofs = mr._map_inputs(inputs)
                row["map_wall_device_s" if on else "map_wall_host_s"] = round(time.perf_counter() - t0, 4)
                row["proofs"] = len(proofs)
            print(json.dumps(row), flush=True)
    mr.free()
    for p in provers:
        p.close()


if __name__ == "__main__":
    main()
