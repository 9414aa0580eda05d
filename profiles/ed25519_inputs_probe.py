"""What building the signature leaves' input vectors on the device costs against building them in Python (one MI355X, one process; run from
the repository root after build(), under a time limit of its own):
    timeout 600 python profiles/ed25519_inputs_probe.py [out.json]                   # default: profiles/ed25519_inputs.json
    timeout 1500 python profiles/ed25519_inputs_probe.py --map [out.json]            # also map_seconds of prove_set, both ways
The set is the one of bench.py's combined_skip leg: 100 validators (89 signed), 112-byte votes, fan-in 8 -> 104 slots.  The two paths are
alternated REPEATS (5) times after a warm-up, host clock around calls that end in a stream synchronise:
  parent : Prover.ed25519_witness over the verified triples (launch + download of the 37-word records), ed25519_circuit.witness_inputs per slot
           in Python, and the upload of the [104][291] vectors that WitnessProgram.evaluate_device does
  device : one Prover.ed25519_leaf_inputs call (one upload of the raw bytes, the witness kernel, the input kernel, the statuses back)
Also: the device call on RESIDENT byte arrays (glp_ed25519_leaf_inputs alone) against glp_ed25519_witness + a synchronise on the same arrays —
their difference is the input kernel's own time — and, with --map, map_seconds of SignatureSetMapReduce.prove_set with device_inputs off and
on (28 queries, 16 PoW bits, one prover), root proofs compared byte for byte.  The rows of both paths are compared word for word before
anything is timed.  No threshold, no retries: a failing step ends the run."""
import argparse
import ctypes
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

REPEATS, N_VALIDATORS, SLOTS, MSG_LEN = 5, 100, 104, 112


def summary(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "ed25519_inputs.json"))
    ap.add_argument("--map", action="store_true")
    args = ap.parse_args()
    pkg = graft.load_package()
    sm = importlib.import_module(graft.PKG_NAME + ".signature_mr")
    ec = importlib.import_module(graft.PKG_NAME + ".ed25519_circuit")
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    prover = pkg.Prover(0)
    prover.set_poseidon_constants(*consts)
    sigs = sm.SignatureSetMapReduce(prover, consts, msg_len=MSG_LEN, hash_offset=16, fan_in=8, device_witness=True)
    block = hashlib.sha256(b"a block").digest()
    flags = [bool(i % 9) for i in range(N_VALIDATORS)]
    msgs = [sigs.vote_bytes(block, i) for i in range(N_VALIDATORS)]
    keys = [ec.keypair_and_sign(hashlib.sha256(b"validator %d" % i).digest(), m) for i, m in enumerate(msgs)]
    pubs, sg = [k[0] for k in keys], [k[1] if f else None for k, f in zip(keys, flags)]
    slots = sigs._slots(pubs, sg, msgs, flags, total=SLOTS)
    dummy = ec.dummy_signature(MSG_LEN)
    layout = sigs._input_layout()
    width = layout.n_words()

    def parent():
        triples = [(slots[0][i], slots[1][i], slots[2][i]) if slots[3][i] else dummy for i in range(SLOTS)]
        recs = prover.ed25519_witness([bytes(t[0]) for t in triples], [bytes(t[1]) for t in triples], [bytes(t[2]) for t in triples])
        rows = np.array([ec.witness_inputs(slots[0][i], slots[1][i] if slots[3][i] else bytes(64), slots[2][i], slots[3][i], record=recs[i])
                         for i in range(SLOTS)], dtype=np.uint64)
        buf = prover.to_device(rows)
        return buf, rows

    def device(out=None):
        return prover.ed25519_leaf_inputs(layout, slots[0], [s if f else None for s, f in zip(slots[1], slots[3])], slots[2], slots[3], dummy, out=out)

    buf, want = parent()
    buf.free()
    dbuf, status = device()
    got = dbuf.download((SLOTS, width))
    assert not status.any() and np.array_equal(got, want), "the device rows differ from witness_inputs"
    res = {"slots": SLOTS, "signed": sum(flags), "vote_bytes": MSG_LEN, "row_words": width, "repeats": REPEATS, "rows_equal_witness_inputs": True}
    t_parent, t_device = [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        b, _ = parent()
        t_parent.append(1e3 * (time.perf_counter() - t0))
        b.free()
        t0 = time.perf_counter()
        device(out=dbuf)
        t_device.append(1e3 * (time.perf_counter() - t0))
    res["build_inputs_ms"] = {"parent_python": summary(t_parent), "device_call": summary(t_device)}
    # the C call alone on resident bytes, against the witness kernel alone
    P = np.frombuffer(b"".join(bytes(x) for x in slots[0]), dtype=np.uint8)
    S = np.frombuffer(b"".join(bytes(x) if f else bytes(64) for x, f in zip(slots[1], slots[3])), dtype=np.uint8)
    M = np.frombuffer(b"".join(bytes(x) for x in slots[2]), dtype=np.uint8)
    d = [prover.to_device(a) for a in (P, S, M, np.full(SLOTS, MSG_LEN, dtype=np.uint32), np.array(slots[3], dtype=np.uint8),
                                       np.frombuffer(b"".join(dummy), dtype=np.uint8))]
    recs = prover.alloc(SLOTS * 37 * 8)
    st = np.zeros(SLOTS, dtype=np.int32)
    t_call, t_wit = [], []
    for r in range(REPEATS + 1):
        t0 = time.perf_counter()
        prover._chk(prover.lib.glp_ed25519_leaf_inputs(prover.ctx, ctypes.byref(layout), d[0].ptr, d[1].ptr, d[2].ptr, MSG_LEN, d[3].ptr, d[4].ptr,
                                                       d[5].ptr, SLOTS, dbuf.ptr, width, st.ctypes.data), "glp_ed25519_leaf_inputs")
        t1 = time.perf_counter()
        prover._chk(prover.lib.glp_ed25519_witness(prover.ctx, d[0].ptr, d[1].ptr, d[2].ptr, MSG_LEN, d[3].ptr, SLOTS, recs.ptr), "glp_ed25519_witness")
        prover.sync()
        t2 = time.perf_counter()
        if r:
            t_call.append(1e3 * (t1 - t0))
            t_wit.append(1e3 * (t2 - t1))
    res["resident_ms"] = {"leaf_inputs_call": summary(t_call), "witness_kernel_alone": summary(t_wit),
                          "input_kernel_by_difference": round(statistics.median(t_call) - statistics.median(t_wit), 3)}
    if args.map:
        outs, times = {}, {False: [], True: []}
        sigs.prove_set(pubs, sg, msgs, flags)                                       # records every circuit
        for _ in range(REPEATS):
            for on in (False, True):
                sigs.device_inputs = on
                outs[on] = sigs.prove_set(pubs, sg, msgs, flags)
                times[on].append(1e3 * outs[on]["map_seconds"])
        assert outs[True]["root_proof"] == outs[False]["root_proof"]
        res["map_ms"] = {"device_inputs_off": summary(times[False]), "device_inputs_on": summary(times[True]), "root_proofs_equal": True}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sigs.free()
    prover.close()


if __name__ == "__main__":
    main()
