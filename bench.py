#!/usr/bin/env python3
"""bench.py — Goldilocks NTT GB/s on MI355X (BASELINE.json metric, second half).

A "step" is one forward NTT over the whole batch, in place, natural order in and out, with
the inputs already resident in HBM.  Default workload: n = 2^20, batch = 128 — the wires
commitment shape of BASELINE.json configs[1] ("~2^20 gates", ~128 wire polynomials).
Algorithmic bytes per step = 16 * n * batch (every element read once and
written once).  value = algorithmic bytes of all ranks / max-over-ranks time.

Multi-GPU (launched by torch.distributed.run, one rank per GPU): the batch dimension is
sharded, every rank transforms its own `batch` polynomials, no data-path collective
 — weak scaling.  torch is used for rendezvous/barrier only.

A plain run sets up, warms up, times exactly --steps transforms and prints one JSON line.
--full adds the extra objects, which take runs of their own: "roofline" (HIP-event time of
the pass kernels of one transform, measured live; HBM peak 8 TB/s), "cpu_baseline" (the CPU
oracle timed on a bounded sample on this box's cores; rank 0, N=1 only), "sizes" (GB/s at
2^20/2^22/2^24) and the optional prove / MapReduce legs, printed on a second, enriched line.

--dump-outputs DIR writes what the last timed step left in the batch (see dump_outputs) for
output-for-output comparison of two builds: the inputs depend only on the arguments.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

HBM_PEAK_GBPS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# the pass structure the default line runs with; tests/test_gpu_configs.py::test_headline_config_bit_exact checks THIS plan
# bit for bit against the CPU oracle at the full 128 x 2^20 size, and the line reports whether it ran with it
EXPECTED_HEADLINE_PLAN = "strip(R=2^10,C=2^4,E=32)+finalT(R=2^10,C=2^3,E=32)"
TIMING_PROTOCOL = ("value: wall clock over exactly --steps back-to-back transforms between barrier+synchronize pairs (mean per step, max "
                   "over ranks); the rest with --full only: roofline.achieved: HIP events on the ctx stream around the same --steps transforms (no event between passes); pass_ms_profiling_mode: per-pass HIP-event times, mean over 3-10 transforms with every pass bracketed (slower by the event overhead); sizes: mean of 10 after 3 warm-ups; "
                   "median_ms_of_50_single_launch_timings: SURVEY 8(d) protocol, each transform bracketed by its own HIP events")
PMC_TRAFFIC = os.path.join(ROOT, "profiles", "pmc_traffic.json")   # written by profiles/summarize_pmc.py --traffic


def pmc_traffic_bytes(plan_desc, elements):
    """HBM bytes per transform from the committed rocprofv3 PMC passes (FETCH_SIZE x2 + WRITE_SIZE,
    per launch, scaled by element count), or None when a pass of this plan was not profiled."""
    import re
    try:
        with open(PMC_TRAFFIC) as f:
            t = json.load(f)["kernels"]
    except OSError:
        return None
    mode_id = {"strip": 0, "finalT": 1, "finalRows": 2}
    total = 0.0
    for mode, lr, lc, e32 in re.findall(r"(strip|finalT|finalRows)\(R=2\^(\d+),C=2\^(\d+)(,E=32)?\)", plan_desc):
        # kernel names as rocprofv3 prints them: <LOG_R, MODE, INV, LOG_E, PLAIN, CT_LOG_C>; the instantiation the launcher picks for a plain
        # natural-order transform (ntt_inst.hip): radix-32 work-items -> PLAIN, and the compile-time tile width where one exists
        pre = f"void glp_ntt_pass_kernel<{lr}, {mode_id[mode]}, false, {5 if e32 else 4}, {'true' if e32 and mode != 'finalRows' else 'false'}, "
        ent = t.get(pre + f"{lc}>(GlpNttPassArgs)") or t.get(pre + "-1>(GlpNttPassArgs)")
        if not ent or ent.get("log_c") not in (None, int(lc)):
            return None
        total += (ent["fetch_bytes"] + ent["write_bytes"]) * elements / float(1 << 27)
    return total or None


def splitmix_fill(n_elems, seed):
    """element i = splitmix64(seed + i) mod p (SURVEY.md §8d inputs), vectorised"""
    p = np.uint64(2**64 - 2**32 + 1)
    with np.errstate(over="ignore"):
        z = np.arange(n_elems, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z % p


def time_ntt(pr, d, log_n, batch, steps, warmup):
    for _ in range(warmup):
        pr.ntt_(d, log_n, batch)
    pr.sync()
    pr.timer_start()
    for _ in range(steps):
        pr.ntt_(d, log_n, batch)
    ms = pr.timer_stop()
    return ms / steps


DUMP_SAMPLE = 1 << 21        # elements written by --dump-outputs: two float64 files of 16 MB each
DUMP_SEED = 0x5EED


def dump_outputs(out_dir, d, batch, n):
    """The batch as the caller of ntt_ receives it after the last timed step, as DIR/ntt_out_lo32.npy and DIR/ntt_out_hi32.npy: the
    low and high 32-bit halves of every u64 field element, each exact in float64, so the comparison is bit for bit.  A batch of more
    than DUMP_SAMPLE elements is sampled at fixed flat (row-major) indices drawn from DUMP_SEED."""
    vals = d.download((batch * n,))
    if vals.size > DUMP_SAMPLE:
        vals = vals[np.sort(np.random.default_rng(DUMP_SEED).choice(vals.size, DUMP_SAMPLE, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "ntt_out_lo32.npy"), (vals & np.uint64(0xFFFFFFFF)).astype(np.float64))
    np.save(os.path.join(out_dir, "ntt_out_hi32.npy"), (vals >> np.uint64(32)).astype(np.float64))


def effective_cpus():
    """CPUs this job may actually use: the smaller of the affinity mask and the cgroup CPU quota (a GPU box
    shows 256 hardware threads but grants a 16-CPU quota per GPU; 256 OpenMP threads under that quota only
    oversubscribe it)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                      # cgroup v2: "<quota> <period>" or "max <period>"
            q, per = f.read().split()
        if q != "max":
            n = min(n, max(1, int(q) // int(per)))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:     # cgroup v1
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                n = min(n, max(1, q // per))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(log_n, seconds_target=15.0):
    """the CPU oracle (kind "port": the in-repo restatement; the Rust plonky2 prover cannot be
    built here) on a bounded sample: `polys` transforms of size 2^log_n, OpenMP over the batch."""
    orc = graft.load_oracle()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    orc.orc_ntt_fast.argtypes = [u64p, ctypes.c_uint, ctypes.c_uint64, ctypes.c_int]
    orc.orc_num_threads.restype = ctypes.c_int
    orc.orc_set_num_threads.argtypes = [ctypes.c_int]
    orc.orc_set_num_threads(effective_cpus())
    cores = orc.orc_num_threads()
    n = 1 << log_n
    probe = splitmix_fill(n * cores, 1).reshape(cores, n)
    t = time.perf_counter()
    orc.orc_ntt_fast(probe.ctypes.data_as(u64p), log_n, cores, 0)
    dt = time.perf_counter() - t
    rounds = max(1, min(64, int(seconds_target / max(dt, 1e-3))))
    polys = cores * rounds
    x = splitmix_fill(n * polys, 2).reshape(polys, n)
    t = time.perf_counter()
    orc.orc_ntt_fast(x.ctypes.data_as(u64p), log_n, polys, 0)
    dt = time.perf_counter() - t
    return {"value": round(16.0 * n * polys / dt / 1e9, 3), "unit": "GB/s", "cores": cores, "kind": "port",
            "sample": f"{polys} forward NTTs of 2^{log_n} (16*n bytes each) by oracle/gl_fast.c (hand-reduced radix-2, "
                      f"gcc -O3 -march=native), OpenMP over the batch on {cores} threads = the job's CPU quota "
                      f"({os.cpu_count()} hardware threads visible), {dt:.1f} s"}


SWEEP = {
    (20, 128): ["10:3,10:3", "10:2,10:2", "10:4,10:4", "10:2,10:3", "10:3,10:2", "10:4,10:3", "8:4,12:2", "12:2,8:4", "7:5,7:5,6:6", "10:3:5,10:3:5", "10:2:5,10:2:5", "10:4:5,10:4:5", "10:3:5,10:3",
                "10:3,10:3:5", "10:4:5,10:3:5", "10:4:5,10:2:5", "9:3:5,11:3", "8:4,8:4,4:6"],
    (22, 32): ["11:3,11:3", "8:4,7:5,7:5", "12:2,10:3", "12:2,10:3:5", "8:4,8:4,6:6", "10:4:5,6:4,6:4", "8:4,7:5,7:5"],
    (24, 8): ["12:2,12:2", "8:4,8:4,8:4", "10:4:5,7:5,7:5", "8:4,8:4,8:5", "9:3:5,9:3:5,6:6", "10:4:5,10:3:5,4:6"],
    (20, 1): ["10:4,10:4", "10:3,10:3", "10:2,10:2", "8:4,12:2", "12:2,8:4", "7:5,7:5,6:6"],
    (24, 1): ["12:2,12:2", "12:1,12:1", "8:4,8:4,8:4", "10:4,7:5,7:5"],
}


def sweep():
    """tuning aid: one line per (size, plan) with total and per-pass HIP-event times"""
    pkg = graft.load_package()
    pr = pkg.Prover(0)
    for (log_n, batch), plans in SWEEP.items():
        n = 1 << log_n
        d = pr.to_device(splitmix_fill(n * batch, 3).reshape(batch, n))
        for plan in [None] + plans:
            try:
                pr.set_plan(log_n, plan)
            except Exception as e:  # noqa: BLE001
                print(json.dumps({"log_n": log_n, "batch": batch, "plan": plan, "error": str(e)}), flush=True)
                continue
            ms = time_ntt(pr, d, log_n, batch, steps=10, warmup=3)
            pr.set_profiling(True)
            acc = None
            for _ in range(5):
                pr.ntt_(d, log_n, batch)
                pm = pr.last_pass_ms()
                acc = pm if acc is None else [a + b for a, b in zip(acc, pm)]
            pr.set_profiling(False)
            print(json.dumps({"log_n": log_n, "batch": batch, "plan": pr.describe_plan(log_n, batch), "ms": round(ms, 4),
                              "gbps": round(16.0 * n * batch / ms / 1e6, 1), "pass_ms": [round(a / 5, 4) for a in acc]}),
                  flush=True)
        pr.set_plan(log_n, None)
        d.free()
    pr.close()


def hash_bench():
    """tuning aid: Poseidon permutation rate and the configs[1]-shaped commitment stages"""
    import importlib
    pkg = graft.load_package()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    pr = pkg.Prover(0)
    rc, circ, diag = pc.default_constants()
    pr.set_poseidon_constants(np.array(rc, dtype=np.uint64), np.array(circ, dtype=np.uint64), np.array(diag, dtype=np.uint64))
    n = 1 << 22
    d = pr.to_device(splitmix_fill(n * 12, 1))
    pr.poseidon_permute_(d, n)
    pr.sync()
    pr.timer_start()
    for _ in range(5):
        pr.poseidon_permute_(d, n)
    ms = pr.timer_stop() / 5
    print(json.dumps({"stage": "poseidon_permute", "n": n, "ms": round(ms, 3), "Mperm_per_s": round(n / ms / 1e3, 1)}), flush=True)
    d.free()
    for n_polys, log_n, rate_bits in ((128, 17, 3), (135, 20, 3)):
        N = 1 << (log_n + rate_bits)
        co = pr.to_device(splitmix_fill(n_polys << log_n, 2))
        lde = pr.alloc(n_polys * N * 8)
        dig = pr.alloc(8 * pkg.Prover.merkle_digest_len(log_n + rate_bits, 4))
        res = {"stage": "from_coeffs", "n_polys": n_polys, "log_n": log_n, "rate_bits": rate_bits}
        for name, fn in (("lde_bitrev_ms", lambda: pr.lde_coset_(co, lde, log_n, rate_bits, n_polys, 7, pkg.NTT_BITREV)),
                         ("merkle_ms", lambda: pr.merkle_(lde, n_polys, log_n + rate_bits, 4, dig, poly_major=True, poly_stride=N,
                                                          want_cap=False)),
                         ("ifft_ms", lambda: pr.ntt_(co, log_n, n_polys, inverse=True))):
            fn()
            pr.sync()
            pr.timer_start()
            for _ in range(3):
                fn()
            res[name] = round(pr.timer_stop() / 3, 3)
        perms = N * ((n_polys + 7) // 8) + N
        res["merkle_Mperm_per_s"] = round(perms / res["merkle_ms"] / 1e3, 1)
        res["lde_out_GBps"] = round(n_polys * N * 8 / res["lde_bitrev_ms"] / 1e6, 1)
        print(json.dumps(res), flush=True)
        for b in (co, lde, dig):
            b.free()
    # the whole opening proof at configs[1] scale: wires 135 + Z/partial products 20 + quotient 16 polynomials of 2^20
    for log_n, polys in ((16, [135, 20, 16]), (20, [135, 20, 16])):
        t0 = time.perf_counter()
        batches = []
        for k, npol in enumerate(polys):
            d = pr.to_device(splitmix_fill(npol << log_n, 10 + k).reshape(npol, 1 << log_n))
            pr.ntt_(d, log_n, npol, inverse=True)
            batches.append(pkg.PolynomialBatch.from_coeffs(pr, d, npol, log_n, 3, 4))
        pr.sync()
        t1 = time.perf_counter()
        proof = pr.fri_prove(batches, 3, 4, arity_bits=4, final_poly_bits=5, num_queries=28, pow_bits=16)
        t2 = time.perf_counter()
        proof2 = pr.fri_prove(batches, 3, 4, arity_bits=4, final_poly_bits=5, num_queries=28, pow_bits=16)
        t3 = time.perf_counter()
        print(json.dumps({"stage": "commit+fri_prove", "log_n": log_n, "polys": polys, "commit_s_incl_h2d": round(t1 - t0, 4),
                          "fri_prove_s_first": round(t2 - t1, 4), "fri_prove_s": round(t3 - t2, 4), "proof_bytes": len(proof),
                          "deterministic": proof == proof2}), flush=True)
        for b in batches:
            b.free()
    pr.close()


def synthetic_circuit(pr, log_n, W, seed=1):
    """a satisfiable instance of the build-defined circuit generated with numpy +
    the GPU's own field ops: random inputs, paired-up input cells as copy constraints (sigma swaps
    each pair), gate outputs w = c0*x*y + c1*z.  Returns (consts[3][n], sigmas[W][n], wires[W][n])."""
    n, G = 1 << log_n, W // 4
    rng = np.random.default_rng(seed)
    p = 2**64 - 2**32 + 1
    consts = np.empty((3, n), dtype=np.uint64)
    consts[0] = 1
    consts[1] = splitmix_fill(n, 11)
    consts[2] = splitmix_fill(n, 12)
    wires = splitmix_fill(W * n, 13).reshape(W, n)
    in_cols = np.array([4 * g + k for g in range(G) for k in range(3)], dtype=np.int64)
    K = len(in_cols) * n
    perm = rng.permutation(K).astype(np.int64)
    a, b = perm[0:K - 1:2], perm[1:K:2]
    col_of = lambda flat: in_cols[flat // n]
    row_of = lambda flat: flat % n
    wires[col_of(b), row_of(b)] = wires[col_of(a), row_of(a)]          # paired cells carry equal values
    for g in range(G):                                                   # outputs on the GPU
        x, y, z = wires[4 * g], wires[4 * g + 1], wires[4 * g + 2]
        xy = pr.field_op("mul", x, y)
        wires[4 * g + 3] = pr.field_op("add", pr.field_op("mul", consts[1], xy), pr.field_op("mul", consts[2], z))
    delta = np.zeros(n, dtype=np.uint64)
    delta[1] = 1
    wpow = pr.fft(delta)                                                 # w_n^i
    ks = np.array([pow(7, j, p) for j in range(W)], dtype=np.uint64)
    tgt_col = np.tile(np.arange(W, dtype=np.int64)[:, None], (1, n))
    tgt_row = np.tile(np.arange(n, dtype=np.int64)[None, :], (W, 1))
    tgt_col[col_of(a), row_of(a)], tgt_row[col_of(a), row_of(a)] = col_of(b), row_of(b)
    tgt_col[col_of(b), row_of(b)], tgt_row[col_of(b), row_of(b)] = col_of(a), row_of(a)
    sigmas = pr.field_op("mul", ks[tgt_col], wpow[tgt_row])
    return consts, sigmas, wires


def prove_bench(sizes, quiet=False):
    """end-to-end prove time of the BUILD'S OWN circuit (not the upstream CombinedStep circuit,
    whose definition is not in the reference mount) sized like BASELINE configs[1]"""
    import importlib
    pkg = graft.load_package()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    pr = pkg.Prover(0)
    rc, circ, diag = pc.default_constants()
    pr.set_poseidon_constants(np.array(rc, dtype=np.uint64), np.array(circ, dtype=np.uint64), np.array(diag, dtype=np.uint64))
    out = []
    for log_n, W in sizes:
        consts, sigmas, wires = synthetic_circuit(pr, log_n, W)
        t0 = time.perf_counter()
        ck = pkg.PlonkCircuit(pr, consts, sigmas)
        pr.sync()
        t1 = time.perf_counter()
        dw = pr.to_device(wires)
        times = []
        proof = None
        for _ in range(3):
            pr.sync()
            ta = time.perf_counter()
            proof = ck.prove_(dw, 28, 16)
            times.append(time.perf_counter() - ta)
        # the proof that was timed must be a VALID proof of this circuit: native verifier, bound to the circuit's
        # verifying key and to the security parameters (host arithmetic, outside the timed region)
        tv = time.perf_counter()
        verified = bool(ck.verify(proof, 28, 16))
        verify_s = time.perf_counter() - tv
        pr.set_profiling(True)                                   # one more proof with stage marks (adds syncs)
        ck.prove_(dw, 28, 16)
        stages = pr.last_stage_ms()
        pr.set_profiling(False)
        res = {"stage": "plonk_prove", "verified": verified, "verify_s": round(verify_s, 4), "stage_ms": dict(stages), "circuit": "build-defined arithmetic+permutation circuit (DESIGN.md 3.6), NOT upstream's",
               "log_n": log_n, "wires": W, "setup_s_incl_h2d": round(t1 - t0, 3), "prove_s": [round(t, 4) for t in times],
               "prove_s_best": round(min(times), 4), "proof_bytes": len(proof), "queries": 28, "pow_bits": 16}
        if not quiet:
            print(json.dumps(res), flush=True)
        out.append(res)
        dw.free()
        ck.free()
    pr.close()
    return out


def _rehearsal():
    """GLP_BENCH_REHEARSE=1: run the multi-rank code path on ONE GPU — every rank on cuda:0, gloo collectives on host
    tensors — to rehearse rank guards, barriers and the MapReduce exchange where only one GPU is available.  Its
    numbers mean nothing (the ranks share a GPU); the driver's multi-GPU runs use RCCL ("nccl") as always."""
    return os.environ.get("GLP_BENCH_REHEARSE") == "1"


def _init_dist(local_rank):
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if _rehearsal():
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))


def _gpu_index(local_rank):
    return 0 if _rehearsal() else local_rank


def _coll_device():
    return "cpu" if _rehearsal() else "cuda"


PMC_VALU = os.path.join(ROOT, "profiles", "pmc_valu.json")      # written from the committed rocprofv3 --pmc SQ_INSTS_VALU pass
SIMDS, PEAK_CLOCK_HZ = 1024, 2.4e9                               # 256 CUs x 4 SIMDs; MI355X_MICROARCH.md max clock


def valu_roofline(perms, ms, kind):
    """the ceiling that actually bounds Poseidon hashing: VALU issue.  peak permutations/s = peak wave-instructions/s x 64 lanes /
    (VALU instructions per permutation, from the committed PMC pass); achieved = permutations of the stage / its time"""
    try:
        with open(PMC_VALU) as f:
            pm = json.load(f)
        per, cyc = pm[kind], pm["avg_issue_cycles"]
    except (OSError, KeyError, ValueError):
        return None
    if not perms or ms <= 0 or not per:
        return None
    peak = SIMDS * PEAK_CLOCK_HZ / cyc * 64.0 / per / 1e9
    ach = perms / (ms * 1e-3) / 1e9
    return {"bound": "valu", "achieved": round(ach, 3), "peak": round(peak, 3), "unit": "G permutations/s", "frac": round(ach / peak, 3),
            "valu_per_permutation": per, "issue_cycles_per_instruction": cyc,
            "note": "stage time includes ifft + LDE + every tree level; peak = 1024 SIMDs x 2.4 GHz / issue cycles per wave-instruction "
                    "(4 for the 64-bit/carry/VOP3 integer class, 2 for v_mov: mix from the ISA) x 64 lanes / VALU instructions per "
                    "permutation (rocprofv3 SQ_INSTS_VALU): profiles/pmc_valu.json"}


def prove_stage_detail(stage_ms, log_n, W, rate_bits=3, cap_h=4):
    """per-stage work of one proof of the build-defined circuit and the rate it was done at (SURVEY.md §5:
    one line per stage with ms, bytes moved, GB/s / permutations per second).  Bytes are ALGORITHMIC (each operand
    column read once, each result column written once); permutations = leaf sponges + tree nodes."""
    n, N = 1 << log_n, 1 << (log_n + rate_bits)
    M = W // 8
    cols = {"pre": 3 + W, "wires": W, "zs": 2 * M, "quotient": 2 << rate_bits}

    def commit(k):     # ifft + LDE by cosets + Merkle of k polynomials
        perms = N * ((k + 7) // 8 if k > 4 else 0) + (N - (1 << cap_h))
        byts = 16 * n * k + 8 * n * k + 8 * N * k + 8 * N * k          # ifft r+w, LDE read + write, leaf-hash read
        return perms, byts

    out = {}
    for name, ms in stage_ms.items():
        d = {"ms": round(ms, 3)}
        if name.startswith("commit_wires"):
            d["perms"], d["bytes"] = commit(cols["wires"])
        elif name.startswith("commit_zs"):
            d["perms"], d["bytes"] = commit(cols["zs"])
        elif name.startswith("commit_quotient"):
            d["perms"], d["bytes"] = commit(cols["quotient"])
        elif name.startswith("perm_products"):
            d["bytes"] = 8 * n * (2 * W + cols["zs"])
        elif name.startswith("quotient(K7)"):
            d["bytes"] = 8 * N * (cols["pre"] + W + cols["zs"] + 2) + 8 * N * 2
        elif name == "fri:combine":
            d["bytes"] = 8 * N * (cols["pre"] + W + cols["zs"] + cols["quotient"]) + 16 * N
        if "bytes" in d and ms > 0:
            d["GBps"] = round(d["bytes"] / (ms * 1e-3) / 1e9, 1)
        if "perms" in d and ms > 0:
            d["Gperm_per_s"] = round(d["perms"] / (ms * 1e-3) / 1e9, 3)
            vr = valu_roofline(d["perms"], ms, "leaf_hash_valu_per_permutation")
            if vr:
                d["roofline"] = vr
        out[name] = d
    return out


def mapreduce_leg(pkg, rank, local_rank, world, leaves_per_rank=16, log_n=16, W=80, provers_per_gpu=3):
    """Map + exchange + Reduce of a MapReduce proof on an already initialised process group: leaf i on rank
    i % world, `provers_per_gpu` concurrent provers per GPU (one ctx = one stream = one host thread each:
    the launch- and latency-bound phases of one leaf overlap the throughput-bound phases of another;
    measured 92 -> 155 leaf proofs/s at 3, profiles/r01_mapreduce_concurrency.txt), one all-gather of the
    padded proofs (RCCL on GPUs), then the distributed native verification.  Every rank must call it;
    returns the result dict (meaningful on rank 0)."""
    import importlib
    import torch
    import torch.distributed as dist
    mr = importlib.import_module(graft.PKG_NAME + ".mapreduce")
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    n_leaves = leaves_per_rank * world                     # skip=1024 / batch=8 -> 128 leaves on 8 GPUs
    rc, circ, diag = pc.default_constants()
    provers, cks, dws = [], [], []
    consts = sigmas = wires = None
    for k in range(provers_per_gpu):
        pr = pkg.Prover(_gpu_index(local_rank))
        pr.set_poseidon_constants(np.array(rc, dtype=np.uint64), np.array(circ, dtype=np.uint64), np.array(diag, dtype=np.uint64))
        if consts is None:
            consts, sigmas, wires = synthetic_circuit(pr, log_n, W)
        provers.append(pr)
        cks.append(pkg.PlonkCircuit(pr, consts, sigmas))
        dws.append(pr.to_device(wires))
    workers = [(lambda i, c=c, d=d: c.prove_(d, 28, 16)) for c, d in zip(cks, dws)]
    verifiers = [(lambda p, c=c: c.verify(p, 28, 16)) for c in cks]
    dev = torch.device("cuda", local_rank) if (world > 1 and not _rehearsal()) else None
    # warm-up: one leaf per prover through the whole map + gather path (first-use costs of the proof
    # pools, torch's host ops and the RCCL communicator are not part of a steady-state MapReduce)
    mr.map_prove_gather(workers, provers_per_gpu * world, padded_len=1 << 18, device=dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    proofs = mr.map_prove_gather(workers, n_leaves, padded_len=1 << 18, device=dev)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the same exchange once more behind the C ABI (glp_comm_init / glp_allgather_proofs: the ctx-owned RCCL communicator a
    # Rust/C++ host would use).  Always at N = 1 (a one-rank communicator cannot wait for anyone); at N > 1 only when asked
    # (GLP_MAPREDUCE_COMM=abi) until a multi-GPU run of it is on record — torch.distributed stays the default exchange.
    abi = None
    if world == 1 or os.environ.get("GLP_MAPREDUCE_COMM") == "abi":
        try:
            ids = [pkg.Prover.comm_unique_id() if rank == 0 else None]
            if world > 1:
                dist.broadcast_object_list(ids, src=0)
            provers[0].comm_init(ids[0], rank, world)
            mine = [(i, proofs[i]) for i in mr.leaves_of_rank(n_leaves, rank, world)]
            ta = time.perf_counter()
            again = mr.allgather_leaf_proofs(mine, n_leaves, 1 << 18, comm=provers[0])
            abi = {"matches_torch_exchange": again == proofs, "seconds": round(time.perf_counter() - ta, 4), "ranks": world}
            provers[0].comm_destroy()
        except Exception as e:  # noqa: BLE001
            abi = {"error": f"{type(e).__name__}: {e}"[:200]}
    # Reduce as far as this build goes: native verification of every gathered leaf, split across ranks
    t1 = time.perf_counter()
    all_ok = mr.reduce_verify(verifiers, proofs, device=dev)
    dt_red = time.perf_counter() - t1
    # ... and its first in-circuit part: ONE root proof, on rank 0's GPU, of the Poseidon tree over the leaf-proof digests
    agg = None
    if rank == 0 and all_ok:
        try:
            rec = importlib.import_module(graft.PKG_NAME + ".recursion")
            t2 = time.perf_counter()
            digests = [provers[0].proof_digest(p) for p in proofs]
            digests += [mr.ZERO_DIGEST] * ((1 << max(1, (len(digests) - 1).bit_length())) - len(digests))
            ckr, dwr, public = rec.build_aggregation_circuit(provers[0], digests)
            t3 = time.perf_counter()
            root_proof = ckr.prove_(dwr, 28, 16, public=public)
            t4 = time.perf_counter()
            root_ok = bool(mr.verify_aggregate(provers[0], root_proof, ckr.cap(), digests, public[-4:]))
            agg = {"reduce_proof_seconds": round(t4 - t2, 4), "build_circuit_seconds": round(t3 - t2, 4), "prove_seconds": round(t4 - t3, 4),
                   "root_proof_bytes": len(root_proof), "root_proof_verifies": root_ok, "rows": 1 << ckr.log_n, "wires": ckr.n_wires,
                   "poseidon_rows": len(digests) - 1, "public_inputs": len(public)}
            dwr.free()
            ckr.free()
            # the hashing half of a recursive verifier for the first two leaves: every Merkle opening of every FRI query re-hashed in-circuit
            t5 = time.perf_counter()
            cko, dwo, pub_o, st = rec.opening_check_circuit(provers[0], proofs[:2])
            t6 = time.perf_counter()
            op_proof = cko.prove_(dwo, 28, 16, public=pub_o)
            t7 = time.perf_counter()
            agg["opening_check_of_2_leaf_proofs"] = dict(st, build_circuit_seconds=round(t6 - t5, 3), prove_seconds=round(t7 - t6, 4),
                                                          verified=bool(cko.verify(op_proof, 28, 16, public=pub_o)), proof_bytes=len(op_proof),
                                                          note="in-circuit: digest = sponge(statement, caps); every opened leaf hashes up its path to "
                                                               "the cap entry its index bits select.  NOT in-circuit: transcript, fold arithmetic, "
                                                               "PLONK identity")
            dwo.free()
            cko.free()
            # ... and as a TREE: pairs of leaves verified by level-1 nodes, pairs of level-1 (recursion) proofs verified by the level-2 node
            t13 = time.perf_counter()
            tree = mr.reduce_tree(provers[0], proofs[:4], {"key": cks[0].cap(), "num_queries": 28, "pow_bits": 16, "n_wires": W},
                                  (np.array(rc, dtype=np.uint64), np.array(circ, dtype=np.uint64), np.array(diag, dtype=np.uint64)), fan_in=2)
            t14 = time.perf_counter()
            agg["reduce_tree_of_4_leaves"] = {"levels": tree["levels"], "seconds_total": round(t14 - t13, 3), "root_proof_bytes": len(tree["root_proof"]),
                                              "root_public_inputs": len(tree["public"]),
                                              "root_verifies": bool(provers[0].plonk_verify(tree["root_proof"], tree["key"], 28, 16, public=tree["public"]))}
        except Exception as e:  # noqa: BLE001
            agg = dict(agg or {}, error=f"{type(e).__name__}: {e}"[:200])
    # ... and the Reduce as a real RECURSION spread over the ranks (mapreduce.reduce_tree_distributed): every rank folds the leaf proofs IT proved
    # into one node proof (a circuit that verifies them completely in-circuit: verifier_circuit.py), ONE all-gather of the node proofs, rank 0
    # folds them into the root.  One rank: the root is the node.  Every rank takes part (collectives inside); GLP_BENCH_TREE=0 skips it.
    rr = None
    pow2 = lambda v: v >= 1 and v & (v - 1) == 0
    if all_ok and pow2(world) and pow2(leaves_per_rank) and os.environ.get("GLP_BENCH_TREE", "1") != "0":
        pconsts = (np.array(rc, dtype=np.uint64), np.array(circ, dtype=np.uint64), np.array(diag, dtype=np.uint64))
        folders = mr.RecursionFolders(provers[0], {"key": cks[0].cap(), "num_queries": 28, "pow_bits": 16, "n_wires": W}, pconsts)
        mine = [proofs[i] for i in mr.leaves_of_rank(n_leaves, rank, world)]
        root_err = []

        def fold_root(nodes):                       # rank 0 only, after the collectives: a failure here must not unbalance the ranks
            try:
                return folders.fold_root(nodes)
            except Exception as e:  # noqa: BLE001
                root_err.append(f"{type(e).__name__}: {e}"[:200])
                return None
        try:
            t0 = time.perf_counter()
            out = mr.reduce_tree_distributed(folders.fold_local, fold_root, mine, 1 << 18, device=dev)   # records the circuits on first use
            t_first = time.perf_counter() - t0
            # steady state: the same steps once more with the recorded programs (local work timed locally; the exchange alone, on every rank)
            t1 = time.perf_counter()
            rp1 = folders.programs[(1, len(mine))]
            dwv, pub_v = rp1.witness(mine)
            provers[0].sync()
            t2 = time.perf_counter()
            node = rp1.circuit.prove_(dwv, 28, 16, public=pub_v)
            t3 = time.perf_counter()
            dwv.free()
            nodes = mr.allgather_leaf_proofs([(rank, node)], world, 1 << 18, device=dev)
            t4 = time.perf_counter()
            rr = dict(rp1.stats, wires=rp1.circuit.n_wires, ranks=world, leaves_per_rank=len(mine),
                      record_circuit_seconds_once=folders.record_seconds.get((1, len(mine))), witness_seconds=round(t2 - t1, 4),
                      prove_seconds=round(t3 - t2, 4), exchange_node_proofs_seconds=round(t4 - t3, 4), node_proof_bytes=len(node),
                      first_call_seconds_including_recording=round(t_first, 3))
            if rank == 0:
                ok_node = bool(provers[0].plonk_verify(out["nodes"][0], folders.local_key, 28, 16, public=pkg.proof_public_inputs(out["nodes"][0])))
                rr.update(node_verifies=ok_node, public_inputs=len(pub_v))
                if world > 1 and not root_err:
                    t5 = time.perf_counter()
                    root2 = folders.fold_root(nodes)
                    t6 = time.perf_counter()
                    rp2 = folders.programs[(2, world)]
                    rr["root"] = dict(rp2.stats, record_circuit_seconds_once=folders.record_seconds.get((2, world)),
                                      witness_and_prove_seconds=round(t6 - t5, 4), proof_bytes=len(root2), public_inputs=len(folders.public),
                                      verified=bool(provers[0].plonk_verify(root2, folders.key, 28, 16, public=folders.public)))
                elif root_err:
                    rr["root"] = {"error": root_err[0]}
                rr["note"] = ("Reduce as a recursion: each rank's node proof verifies that rank's leaf proofs entirely in-circuit (transcript, PoW, Merkle "
                              "openings, FRI, PLONK identity) and hashes their digests to a root; with more ranks ONE all-gather of the node proofs and a "
                              "root proof on rank 0 that verifies them in-circuit.  Circuits are recorded once (host builder); every Reduce after that = "
                              "witness_seconds (glp_witness_eval_mt on host threads + on-device placement) + prove_seconds (+ exchange + root)")
        except Exception as e:  # noqa: BLE001 — raised on EVERY rank (agreement before the collectives) or on none
            rr = {"error": f"{type(e).__name__}: {e}"[:200]}
        folders.free()
    if agg is not None and rr is not None:
        agg["recursive_reduce"] = rr
    if world > 1:
        tt = torch.tensor([dt, dt_red], dtype=torch.float64, device=_coll_device())
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt, dt_red = float(tt[0].item()), float(tt[1].item())
    res = {"stage": "mapreduce", "n_leaves": n_leaves, "leaves_per_gpu": leaves_per_rank, "leaf_log_n": log_n,
           "leaf_wires": W, "n_gpus": world, "provers_per_gpu": provers_per_gpu, "seconds": round(dt, 4),
           "leaf_proofs_per_s": round(n_leaves / dt, 1), "reduce_verify_seconds": round(dt_red, 4), "all_leaves_verify": all_ok,
           "leaf_proof_bytes": len(proofs[0]), "all_present": all(len(p) > 0 for p in proofs), "c_abi_exchange": abi, "aggregation": agg,
           "note": "BASELINE configs[2]/[3] shape with the build-defined leaf circuit (NOT upstream's); seconds = Map + one "
                   "all-gather of padded proofs; Reduce = native verification of every leaf (host arithmetic, split across "
                   "ranks and host threads) + all-reduce of the verdicts, then ONE root proof on rank 0 of the Poseidon Merkle tree over the "
                   "leaf-proof digests (public inputs: digests + root; every two-to-one hash a constrained Poseidon row); "
                   "aggregation.recursive_reduce = the same Reduce as a real recursion: one circuit that verifies leaf proofs entirely "
                   "in-circuit (fan-in GLP_BENCH_RECURSION_LEAVES, default 4)"}
    for d, c, q in zip(dws, cks, provers):
        d.free()
        c.free()
        q.close()
    return res


def data_commitment_leg(pkg, n_blocks=4, n_blocks_rows=64):
    """a circuit whose statement MEANS something: DataCommitment over (height, dataRoot) tuples with every SHA-256 compression of the RFC 6962
    tree constrained in-circuit, public inputs = tuples + root.  Two layouts of the same statement (gadgets.py): `sha_rows` — the SHA row
    gates (plonk_gates.h: 178 rows per compression, bit wires filled on the GPU), on n_blocks_rows blocks; `bit_decomposition` — round 2's first
    form on the arithmetic gate alone (~65.5k gates = 3.3k rows per compression), on n_blocks blocks, kept as the comparison.  Reports circuit
    construction (host Python), proof and verification times, and that the exposed root equals the GPU witness kernel's."""
    import importlib
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    gd = importlib.import_module(graft.PKG_NAME + ".gadgets")
    bs = importlib.import_module(graft.PKG_NAME + ".blobstream")
    pr = pkg.Prover(0)
    rc, circ, diag = pc.default_constants()
    pr.set_poseidon_constants(np.array(rc, dtype=np.uint64), np.array(circ, dtype=np.uint64), np.array(diag, dtype=np.uint64))
    rng = np.random.default_rng(11)

    def one(build, nb):
        heights = [2_000_000 + i for i in range(nb)]
        roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(nb)]
        t0 = time.perf_counter()
        ck, dw, public, root = build(pr, heights, roots)
        pr.sync()
        t1 = time.perf_counter()
        proof = ck.prove_(dw, 28, 16, public=public)
        t2 = time.perf_counter()
        proof = ck.prove_(dw, 28, 16, public=public)
        t3 = time.perf_counter()
        ok = bool(ck.verify(proof, 28, 16, public=public))
        t4 = time.perf_counter()
        r = {"blocks": nb, "sha256_compressions": (2 * nb - 1) * 2, "rows": 1 << ck.log_n, "wires": ck.n_wires, "public_inputs": len(public),
             "build_circuit_seconds": round(t1 - t0, 3), "prove_seconds_first": round(t2 - t1, 4), "prove_seconds": round(t3 - t2, 4),
             "verify_seconds": round(t4 - t3, 4), "verified": ok, "proof_bytes": len(proof),
             "compressions_per_second_proved": round((2 * nb - 1) * 2 / (t3 - t2), 1),
             "root_matches_gpu_witness_kernel": root == bs.data_commitment(pr, heights, roots)}
        dw.free()
        ck.free()
        return r

    res = dict(one(gd.data_commitment_rows_circuit, n_blocks_rows), layout="sha_rows",
               note="build-defined DataCommitment statement (NOT upstream's circuit): SHA-256 Merkle tree over abi.encode(height, dataRoot) on the "
                    "SHA row gates (E/A/W/ADD rows; upstream proves its SHA rounds in a separate STARK); circuit construction is host Python")
    res["bit_decomposition"] = one(gd.data_commitment_circuit, n_blocks)
    pr.close()
    return res


def prove_cpu_baseline(pkg, log_n=16, W=80, rate_bits=3, cap_h=4):
    """CPU and GPU side by side for the prove path too.  The wires commitment (inverse transform + coset LDE x 8 + Poseidon
    Merkle tree: the largest stage of a proof) of a BOUNDED sample — 2^16 rows x 80 wires, 1/16 of the timed proof's stage — by the CPU port
    (oracle/gl_fast.c::orc_commit_fast, OpenMP on the job's CPU quota) and by the GPU on the same values; the two caps must be equal.
    kind "port": the in-repo restatement, never the target."""
    import importlib
    orc = graft.load_oracle()
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    u64p = ctypes.POINTER(ctypes.c_uint64)
    ptr = lambda a: a.ctypes.data_as(u64p)
    orc.orc_fast_set_poseidon(*(ptr(a) for a in consts))
    orc.orc_commit_fast.argtypes = [u64p, ctypes.c_uint, ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint64, u64p]
    orc.orc_commit_fast.restype = ctypes.c_int
    orc.orc_num_threads.restype = ctypes.c_int
    orc.orc_set_num_threads.argtypes = [ctypes.c_int]
    orc.orc_set_num_threads(effective_cpus())
    cores = orc.orc_num_threads()
    vals = splitmix_fill(W << log_n, 77).reshape(W, 1 << log_n)
    pr = pkg.Prover(0)
    pr.set_poseidon_constants(*consts)
    pb = pkg.PolynomialBatch.from_values(pr, vals, rate_bits, cap_h)          # warm-up (tables, pool)
    pb.free()
    pr.sync()
    t0 = time.perf_counter()
    pb = pkg.PolynomialBatch.from_values(pr, vals, rate_bits, cap_h)
    pr.sync()
    t_gpu = time.perf_counter() - t0
    gpu_cap = np.asarray(pb.cap, dtype=np.uint64).reshape(-1).copy()
    pb.free()
    pr.close()
    work, cap = vals.copy(), np.zeros(4 << cap_h, dtype=np.uint64)
    t0 = time.perf_counter()
    rc = orc.orc_commit_fast(ptr(work), log_n, W, rate_bits, cap_h, 7, ptr(cap))
    t_cpu = time.perf_counter() - t0
    perms = (1 << (log_n + rate_bits)) * ((W + 7) // 8) + (1 << (log_n + rate_bits))
    return {"stage": "commit_wires", "kind": "port", "cores": cores, "seconds": round(t_cpu, 3), "gpu_seconds_same_sample_incl_h2d": round(t_gpu, 4),
            "caps_equal": bool(rc == 0 and np.array_equal(cap, gpu_cap)), "poseidon_permutations": perms,
            "cpu_permutations_per_second": round(perms / t_cpu, 1),
            "sample": f"wires commitment of 2^{log_n} rows x {W} wires, rate 1/8, cap height {cap_h} (1/16 of the timed proof's commit_wires stage in "
                      f"rows; the stage is linear in rows up to the transforms' log factor) by oracle/gl_fast.c::orc_commit_fast (hand-reduced "
                      f"Goldilocks arithmetic, radix-2 transforms, naive-structure Poseidon with 128-bit MDS accumulation; gcc -O3 -march=native, "
                      f"OpenMP on {cores} threads = the job's CPU quota)"}


def prove_constrained_leg(pkg, blocks=1024):
    """configs[1] "with constraints that mean something": ONE circuit of 2^20 rows x 144 wires whose rows are SHA-256 row gates — the
    DataCommitment statement over 1024 blocks (4094 constrained compressions, gadgets.data_commitment_rows_circuit), proved and verified, with
    the prover's stage timing tree"""
    import hashlib
    import importlib
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    gd = importlib.import_module(graft.PKG_NAME + ".gadgets")
    pr = pkg.Prover(0)
    pr.set_poseidon_constants(*(np.array(a, dtype=np.uint64) for a in pc.default_constants()))
    rng = np.random.default_rng(11)
    hs = [2_000_000 + i for i in range(blocks)]
    rs = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in hs]
    t0 = time.perf_counter()
    ck, dw, public, root = gd.data_commitment_rows_circuit(pr, hs, rs)
    pr.sync()
    t_build = time.perf_counter() - t0
    times = []
    for _ in range(3):
        t = time.perf_counter()
        proof = ck.prove_(dw, 28, 16, public=public)
        times.append(time.perf_counter() - t)
    t = time.perf_counter()
    ok = bool(ck.verify(proof, 28, 16, public=public))
    t_ver = time.perf_counter() - t
    pr.set_profiling(True)
    ck.prove_(dw, 28, 16, public=public)
    stages = dict(pr.last_stage_ms())
    pr.set_profiling(False)
    lvl = [hashlib.sha256(b"\x00" + int(h).to_bytes(32, "big") + r).digest() for h, r in zip(hs, rs)]
    while len(lvl) > 1:
        lvl = [hashlib.sha256(b"\x01" + lvl[i] + lvl[i + 1]).digest() for i in range(0, len(lvl), 2)]
    res = {"circuit": "DataCommitment over 1024 blocks on SHA-256 row gates (build-defined; NOT upstream's circuit)", "log_n": ck.log_n,
           "wires": ck.n_wires, "sha256_compressions": 2 * (2 * blocks - 1), "seconds": round(min(times), 4), "prove_s": [round(x, 4) for x in times],
           "verified": ok, "verify_seconds": round(t_ver, 4), "commitment_matches_hashlib": root == lvl[0], "proof_bytes": len(proof),
           "build_circuit_seconds_python": round(t_build, 2), "queries": 28, "pow_bits": 16, "stage_ms": {k: round(v, 3) for k, v in stages.items()}}
    dw.free()
    ck.free()
    pr.close()
    return res


def validator_set_leg(pkg, n_validators=150):
    """the non-cryptographic half of a Tendermint commit check as a circuit (gadgets.validator_set_circuit): validators_hash of n validators
    (variable-length protobuf leaves, RFC 6962 tree) on the SHA row gates + the > 2/3 voting-power rule; Ed25519 signatures are NOT constrained
    (flags are witnesses; the GPU witness kernel checks them outside).  BASELINE configs[0]'s "validator-Merkle witness", constrained."""
    import importlib
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    gd = importlib.import_module(graft.PKG_NAME + ".gadgets")
    bs = importlib.import_module(graft.PKG_NAME + ".blobstream")
    pr = pkg.Prover(0)
    pr.set_poseidon_constants(*(np.array(a, dtype=np.uint64) for a in pc.default_constants()))
    rng = np.random.default_rng(13)
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n_validators)]
    powers = [int(rng.integers(1, 1 << 40)) for _ in range(n_validators)]
    signed = [bool(i % 5) for i in range(n_validators)]                      # 80 % of the validators sign
    t0 = time.perf_counter()
    ck, dw, public, digest = gd.validator_set_circuit(pr, keys, powers, signed)
    pr.sync()
    t1 = time.perf_counter()
    proof = ck.prove_(dw, 28, 16, public=public)
    t2 = time.perf_counter()
    proof = ck.prove_(dw, 28, 16, public=public)
    t3 = time.perf_counter()
    ok = bool(ck.verify(proof, 28, 16, public=public))
    res = {"validators": n_validators, "rows": 1 << ck.log_n, "wires": ck.n_wires, "build_circuit_seconds": round(t1 - t0, 3),
           "prove_seconds_first": round(t2 - t1, 4), "prove_seconds": round(t3 - t2, 4), "verified": ok, "proof_bytes": len(proof),
           "hash_matches_gpu_witness_kernel": digest == bs.validator_set_hash(pr, keys, powers),
           "signed_power_over_total": round(public[8] / public[9], 4),
           "note": "build-defined statement: validators_hash + the > 2/3 rule constrained; Ed25519 signatures of the flagged validators NOT constrained"}
    dw.free()
    ck.free()
    pr.close()
    return res


def skip_leg(pkg, n_validators=100):
    """the non-cryptographic statement of a light-client skip as ONE circuit (gadgets.skip_circuit): a trusted and a target header (14 field
    encodings each) bound to their validator sets, > 2/3 of the target power and > 1/3 of the trusted power flagged — CombinedSkip's shape minus
    its Ed25519 half (NOT constrained).  The target set keeps 90 % of the trusted set's members."""
    import importlib
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    gd = importlib.import_module(graft.PKG_NAME + ".gadgets")
    pr = pkg.Prover(0)
    pr.set_poseidon_constants(*(np.array(a, dtype=np.uint64) for a in pc.default_constants()))
    rng = np.random.default_rng(14)
    key = lambda: rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    tk = [key() for _ in range(n_validators)]
    tp = [int(rng.integers(1, 1 << 40)) for _ in range(n_validators)]
    keep = n_validators * 9 // 10
    vk = tk[:keep] + [key() for _ in range(n_validators - keep)]
    vp = [int(rng.integers(1, 1 << 40)) for _ in range(n_validators)]
    idx = list(range(keep)) + [None] * (n_validators - keep)
    signed = [bool(i % 7) for i in range(n_validators)]
    lens = [4, 12, 5, 13, 72, 34, 34, 34, 34, 34, 34, 34, 34, 22]
    fields = lambda: [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    t0 = time.perf_counter()
    ck, dw, public, hb_t, hb_v = gd.skip_circuit(pr, fields(), (tk, tp), fields(), (vk, vp), signed, idx)
    pr.sync()
    t1 = time.perf_counter()
    proof = ck.prove_(dw, 28, 16, public=public)
    t2 = time.perf_counter()
    proof = ck.prove_(dw, 28, 16, public=public)
    t3 = time.perf_counter()
    ok = bool(ck.verify(proof, 28, 16, public=public))
    res = {"validators_per_set": n_validators, "shared_validators": keep, "rows": 1 << ck.log_n, "wires": ck.n_wires,
           "build_circuit_seconds": round(t1 - t0, 3), "prove_seconds_first": round(t2 - t1, 4), "prove_seconds": round(t3 - t2, 4),
           "verified": ok, "proof_bytes": len(proof), "public_inputs": len(public),
           "note": "build-defined statement: both header hashes public; validator-set hashes, header binding and the 2/3 + 1/3 power rules constrained; "
                   "Ed25519 signatures of the flagged validators NOT constrained"}
    dw.free()
    ck.free()
    pr.close()
    return res


def header_chain_leg(pkg, rank, local_rank, world, n_headers=256, leaf_headers=4, fan_in=8):
    """the header-chain form of the data commitment as a MapReduce of proofs (data_commitment_mr.HeaderChainMapReduce): n_headers headers walked from a
    start hash — every last_block_id link, every height field and every data_hash constrained (about 45 SHA-256 compressions per header), nodes that
    verify their children in-circuit and check adjacency.  BASELINE's CombinedSkip range shape with real statements, minus Ed25519.  Rank r proves
    and folds the r-th contiguous part, one all-gather of node proofs, root on rank 0.  Every rank must call it."""
    import hashlib
    import importlib
    import torch
    import torch.distributed as dist
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    bs = importlib.import_module(graft.PKG_NAME + ".blobstream")
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    provers = [pkg.Prover(_gpu_index(local_rank)) for _ in range(3)]
    for p in provers:
        p.set_poseidon_constants(*consts)
    dev = torch.device("cuda", local_rank) if (world > 1 and not _rehearsal()) else None
    rng = np.random.default_rng(21)                                   # the same chain on every rank
    lens = (4, 12, 5, 13, 72, 34, 34, 34, 34, 34, 34, 34, 34, 22)

    def chain(start, first, count):
        prev, out = start, []
        for k in range(count):
            f = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lens]
            f[2] = b"\x08" + bs.encode_varint(first + k)
            f[4] = b"\x0a\x20" + prev + f[4][34:]
            f[6] = b"\x0a\x20" + f[6][2:]
            out.append(f)
            prev = dm.HeaderChainMapReduce.header_hash(f)
        return out, prev
    mr = dm.HeaderChainMapReduce(provers[0], consts, leaf_headers=leaf_headers, fan_in=fan_in, map_provers=provers[1:])
    _maybe_fault("header_chain_range", rank)
    res = {"headers": n_headers, "leaf_headers": leaf_headers, "fan_in": fan_in, "ranks": world, "map_provers_per_gpu": 3}
    for run in ("first_run_records_circuits", "steady_state"):
        start, first = hashlib.sha256(run.encode()).digest(), 4_000_000
        hdrs, end = chain(start, first, n_headers)
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        out = mr.prove_chain_distributed(start, first, hdrs, device=dev)
        dt = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([dt, out["map_seconds"]], dtype=torch.float64, device=_coll_device())
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt, map_s = float(tt[0].item()), float(tt[1].item())
        else:
            map_s = out["map_seconds"]
        if rank == 0:
            lvl = [hashlib.sha256(b"\x00" + int(first + k).to_bytes(32, "big") + hdrs[k][6][2:]).digest() for k in range(n_headers)]
            while len(lvl) > 1:
                lvl = [hashlib.sha256(b"\x01" + lvl[i] + lvl[i + 1]).digest() for i in range(0, len(lvl), 2)]
            ok = out["end_hash"] == end and out["commitment"] == lvl[0] and mr.verify_chain(out["root_proof"], out["key"], start, end, lvl[0], first)
            res[run] = {"seconds": round(dt, 3), "map_seconds_max_over_ranks": round(map_s, 4), "levels_on_rank0": out["levels"],
                        "end_hash_and_commitment_match_hashlib_and_verify": bool(ok), "headers_per_second": round(n_headers / dt, 1),
                        "root_proof_bytes": len(out["root_proof"])}
    if rank == 0:
        res["record_seconds_rank0"] = dict(mr.record_seconds)
        res["leaf"] = {k: v for k, v in mr.leaf_program.stats.items() if k in ("rows", "rows_used", "sha_rows")}
        res["note"] = ("build-defined statement (NOT upstream's circuit): public inputs of the root proof = start header hash, end header hash, data "
                       "commitment, first height; header encodings are opaque byte strings of fixed lengths except the three fields the circuit binds")
    mr.free()
    for p in provers:
        p.close()
    return res


def combined_skip_leg(pkg, rank, local_rank, world, skips=(128, 1024), n_validators=100, shared=90):
    """BASELINE configs[2] / configs[3] with the real statement (combined_skip_mr.CombinedSkipMapReduce): CombinedSkip over `skip` headers as a
    MapReduce with batch = 8 — leaves of 8 headers (links, heights, data hashes constrained: ~46 SHA-256 compressions per header), nodes that
    verify their children in-circuit and check adjacency, and the outer circuit that verifies the chain's root proof and lays down the
    light-client skip rules (two validator sets of 100, 90 shared; > 2/3 and > 1/3 power rules; block numbers).  Rank r proves and folds the
    r-th contiguous part of the chain (skip/8/N leaves per rank), ONE all-gather of node proofs, rank 0 folds the root and proves the outer
    circuit.  Whole-job seconds: first run (records the circuits with the Python builder) and steady state; every rank must call it."""
    import importlib
    import torch
    import torch.distributed as dist
    cs = importlib.import_module(graft.PKG_NAME + ".combined_skip_mr")
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    provers = [pkg.Prover(_gpu_index(local_rank)) for _ in range(3)]
    for p in provers:
        p.set_poseidon_constants(*consts)
    dev = torch.device("cuda", local_rank) if (world > 1 and not _rehearsal()) else None
    chain = dm.HeaderChainMapReduce(provers[0], consts, leaf_headers=8, fan_in=8, map_provers=provers[1:])
    _maybe_fault("combined_skip", rank)
    idx = list(range(shared)) + [None] * (n_validators - shared)
    res = {"batch": 8, "fan_in": 8, "ranks": world, "map_provers_per_gpu": 3, "validators_per_set": n_validators, "shared_validators": shared,
           "queries": 28, "pow_bits": 16}
    for skip in skips:
        leaves = skip // 8
        if leaves % world or ((leaves // world) & (leaves // world - 1)):
            if rank == 0:
                res[f"skip_{skip}"] = {"skipped": f"{leaves} leaves do not split into a power-of-two number per rank over {world} ranks"}
            continue
        mr = cs.CombinedSkipMapReduce(provers[0], consts, skip=skip, chain=chain, max_skip=4096)
        entry = {"headers": skip, "leaves": leaves, "leaves_per_rank": leaves // world}
        for run in ("first_run_records_circuits", "steady_state"):
            case = mr.synthetic_case(n_validators, n_validators, idx, trusted_height=4_000_000 + (run == "steady_state"), seed=skip + (run == "steady_state"))
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
            out = mr.prove_skip_distributed(*case, device=dev)
            dt = time.perf_counter() - t0
            if world > 1:
                tt = torch.tensor([dt, out["map_seconds"]], dtype=torch.float64, device=_coll_device())
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                dt, map_s = float(tt[0].item()), float(tt[1].item())
            else:
                map_s = out["map_seconds"]
            if rank == 0:
                import hashlib
                tf, _, hdrs, (vk, _vp), signed, _, h0 = case
                lvl = [hashlib.sha256(b"\x00" + int(h0 + 1 + k).to_bytes(32, "big") + hdrs[k][6][2:]).digest() for k in range(skip)]
                while len(lvl) > 1:
                    lvl = [hashlib.sha256(b"\x01" + lvl[i] + lvl[i + 1]).digest() for i in range(0, len(lvl), 2)]
                gd = importlib.import_module(graft.PKG_NAME + ".gadgets")
                t1 = time.perf_counter()
                ok = (out["commitment"] == lvl[0] and out["trusted_hash"] == dm.HeaderChainMapReduce.header_hash(tf)
                      and out["target_hash"] == dm.HeaderChainMapReduce.header_hash(hdrs[-1])
                      and mr.verify(out["root_proof"], out["key"], out["trusted_hash"], out["target_hash"], gd.signer_digest_host(consts, vk, signed),
                                    h0, h0 + skip, lvl[0]))
                entry[run] = {"seconds": round(dt, 4), "map_seconds_max_over_ranks": round(map_s, 4),
                              "chain_seconds_rank0": out["chain_seconds"], "outer_seconds": out["outer_seconds"],
                              "reduce_seconds_rank0": round(out["chain_seconds"] - out["map_seconds"], 4), "levels_on_rank0": out["levels"],
                              "verified_and_hashes_commitment_match_hashlib": bool(ok), "verify_seconds": round(time.perf_counter() - t1, 4),
                              "headers_per_second": round(skip / dt, 1), "root_proof_bytes": len(out["root_proof"]), "outer_rows": out["outer_rows"]}
                entry["record_seconds_rank0"] = out["record_seconds"]
        if rank == 0:
            res[f"skip_{skip}"] = entry
        mr.free()
    # ---- the COMPLETE statement: the same skip with the target validators' Ed25519 signatures proved in-circuit (signature_mr.py: one 2^17-row
    # leaf per validator slot, 100 validators padded to 128 slots, folded to a root that the outer circuit verifies beside the chain's root)
    sig_skip = max(skips)
    sig_leaves = sig_skip // 8
    if os.environ.get("GLP_BENCH_SIGNATURES", "1") != "0" and sig_leaves % world == 0 and 128 % world == 0 and 128 // world >= 2:
        sm = importlib.import_module(graft.PKG_NAME + ".signature_mr")
        # the signature MapReduce gets three provers (ctxs) of its own: at N = 1 the chain and the signatures are then proved side by side
        sig_provers = [pkg.Prover(_gpu_index(local_rank)) for _ in range(3)]
        for p in sig_provers:
            p.set_poseidon_constants(*consts)
        sigs = sm.SignatureSetMapReduce(sig_provers[0], consts, msg_len=112, hash_offset=16, fan_in=8, map_provers=sig_provers[1:])
        mr = cs.CombinedSkipMapReduce(provers[0], consts, skip=sig_skip, chain=chain, max_skip=4096, signatures=sigs)
        entry = {"headers": sig_skip, "chain_leaves": sig_leaves, "validators": n_validators, "signer_digest_slots": 128, "vote_bytes": 112}
        for run in ("first_run_records_circuits", "steady_state"):
            t_gen = time.perf_counter()
            *case, seeds = mr.synthetic_case(n_validators, n_validators, idx, trusted_height=4_100_000 + (run == "steady_state"),
                                             seed=7000 + (run == "steady_state"), real_keys=True)
            case[4] = [bool(i % 9) for i in range(n_validators)]                # 89 of 100 sign (comparable powers: > 2/3 and > 1/3 hold)
            votes = mr.synthetic_votes(case, seeds)
            t_gen = time.perf_counter() - t_gen
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
            out = mr.prove_skip_distributed(*case, device=dev, votes=votes)
            dt = time.perf_counter() - t0
            if world > 1:
                tt = torch.tensor([dt, out["map_seconds"], out["signature_map_seconds"]], dtype=torch.float64, device=_coll_device())
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                dt, map_s, smap_s = (float(v) for v in tt.tolist())
            else:
                map_s, smap_s = out["map_seconds"], out["signature_map_seconds"]
            if rank == 0:
                gd = importlib.import_module(graft.PKG_NAME + ".gadgets")
                tf, _, hdrs, (vk, _vp), signed, _, h0 = case
                t1 = time.perf_counter()
                ok = (out["signatures_in_circuit"] and out["target_hash"] == dm.HeaderChainMapReduce.header_hash(hdrs[-1])
                      and mr.verify(out["root_proof"], out["key"], out["trusted_hash"], out["target_hash"],
                                    gd.signer_digest_host(consts, vk, signed, pad_to=128), h0, h0 + sig_skip, out["commitment"]))
                entry[run] = {"seconds": round(dt, 4), "chain_map_seconds_max_over_ranks": round(map_s, 4),
                              "signature_map_seconds_max_over_ranks": round(smap_s, 4), "signature_seconds_rank0": out["signature_seconds"],
                              "chain_seconds_rank0": out["chain_seconds"], "outer_seconds": out["outer_seconds"], "outer_rows": out["outer_rows"],
                              "signature_levels_on_rank0": out["signature_levels"], "signers": int(sum(signed)),
                              "signature_leaves_proved": out["signature_slots"],
                              "verified_with_the_host_signer_digest": bool(ok), "verify_seconds": round(time.perf_counter() - t1, 4),
                              "signatures_per_second": round(int(sum(signed)) / max(out["signature_seconds"], 1e-9), 1),
                              "root_proof_bytes": len(out["root_proof"]), "synthetic_keys_and_votes_python_seconds": round(t_gen, 2)}
                entry["record_seconds_rank0"] = dict(out["record_seconds"], **{"sig_" + k: v for k, v in out["signature_record_seconds"].items()})
        # BASELINE configs[1] with the real statement: CombinedStep = ONE header after the trusted one (a one-header chain leaf, no chain nodes), the same
        # validator set behind both headers, every signature in-circuit.  One rank only (a single chain leaf does not shard); reuses the signature recordings.
        if world == 1:
            chain1 = dm.HeaderChainMapReduce(provers[0], consts, leaf_headers=1, fan_in=8, map_provers=provers[1:])
            st = cs.CombinedSkipMapReduce(provers[0], consts, skip=1, batch=1, chain=chain1, max_skip=4096, signatures=sigs)
            ident = list(range(n_validators))
            step = {"headers": 1, "validators": n_validators, "signer_digest_slots": 128}
            for run in ("first_run_records_circuits", "steady_state"):
                *case, seeds = st.synthetic_case(n_validators, n_validators, ident, trusted_height=4_200_000 + (run == "steady_state"),
                                                 seed=9000 + (run == "steady_state"), real_keys=True)
                case[4] = [bool(i % 9) for i in range(n_validators)]
                votes = st.synthetic_votes(case, seeds)
                t0 = time.perf_counter()
                out = st.prove_skip(*case, votes=votes)
                dt = time.perf_counter() - t0
                gd = importlib.import_module(graft.PKG_NAME + ".gadgets")
                tf, _, hdrs, (vk, _vp), signed, _, h0 = case
                ok = (out["signatures_in_circuit"] and out["target_hash"] == dm.HeaderChainMapReduce.header_hash(hdrs[-1])
                      and st.verify(out["root_proof"], out["key"], out["trusted_hash"], out["target_hash"],
                                    gd.signer_digest_host(consts, vk, signed, pad_to=128), h0, h0 + 1, out["commitment"]))
                step[run] = {"seconds": round(dt, 4), "chain_seconds": out["chain_seconds"], "signature_seconds": out["signature_seconds"],
                             "outer_seconds": out["outer_seconds"], "outer_rows": out["outer_rows"], "verified_with_the_host_signer_digest": bool(ok),
                             "signature_leaves_proved": out["signature_slots"],
                             "constrained_rows_total": out["signature_slots"] * sigs.leaf_stats["rows"] + chain1.leaf_program.stats["rows"] + out["outer_rows"]}
            step["note"] = ("CombinedStep's shape with the real statement: the target header is the trusted header's successor (block numbers, last_block_id "
                            "link, data commitment of the one block), ONE validator set behind both headers (every target validator is the trusted "
                            "validator at its position), > 2/3 flagged, every flagged signature verified in-circuit; build-defined, NOT upstream's circuit")
            res["step_with_signatures"] = step
            st.free()
            chain1.free()
        if rank == 0:
            entry["signature_leaf"] = {k: v for k, v in sigs.leaf_stats.items() if k in ("rows", "rows_used", "arith_gates", "sha_rows", "field_products")}
            entry["note"] = ("the COMPLETE statement: header chain + skip rules + every flagged target validator's Ed25519 signature over vote bytes naming "
                             "the target header, all in-circuit (non-native field arithmetic on arithmetic gates + range-check rows; SHA-512 by bit "
                             "decomposition); vote bytes are a build-defined fixed-length stand-in for the canonical vote encoding")
            res[f"skip_{sig_skip}_with_signatures"] = entry
        mr.free()
        sigs.free()
        for p in sig_provers:
            p.close()
    if rank == 0:
        res["leaf"] = {k: v for k, v in chain.leaf_program.stats.items() if k in ("rows", "rows_used", "sha_rows")}
        res["note"] = ("build-defined statement (NOT upstream's circuit): public inputs of the final proof = trusted header hash, target header hash, "
                       "signer digest, trusted block, target block, data commitment; skip_<n>: WITHOUT the Ed25519 half (signer digest exposed for a native check); "
                       "skip_<n>_with_signatures: the complete statement; seconds = Map + Reduce + outer circuit, whole job, max over ranks")
    chain.free()
    for p in provers:
        p.close()
    return res


def data_commitment_range_leg(pkg, rank, local_rank, world, blocks=4096, leaf_blocks=64, fan_in=8):
    """BASELINE configs[4] shape with a statement that MEANS something: the data commitment of a 4096-block range proved as a MapReduce of
    proofs (data_commitment_mr.py) — 64 leaves of 64 blocks on the SHA row gates (rank r proves the r-th contiguous part), each rank folds its
    leaves into a node proof that verifies them in-circuit, ONE all-gather of the node proofs, rank 0 folds the root.  First run records the
    circuits (host builder); the second is the steady state.  Every rank must call it."""
    import hashlib
    import importlib
    import torch
    import torch.distributed as dist
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    pc = importlib.import_module(graft.PKG_NAME + ".poseidon_constants")
    consts = tuple(np.array(a, dtype=np.uint64) for a in pc.default_constants())
    pr = pkg.Prover(_gpu_index(local_rank))
    pr.set_poseidon_constants(*consts)
    dev = torch.device("cuda", local_rank) if (world > 1 and not _rehearsal()) else None
    extra = [pkg.Prover(_gpu_index(local_rank)) for _ in range(2)]        # 3 concurrent provers per GPU for the Map step (as in mapreduce_leg)
    for p in extra:
        p.set_poseidon_constants(*consts)
    mr = dm.DataCommitmentMapReduce(pr, consts, leaf_blocks=leaf_blocks, fan_in=fan_in, map_provers=extra)
    _maybe_fault("data_commitment_range", rank)
    res = {"blocks": blocks, "leaf_blocks": leaf_blocks, "fan_in": fan_in, "ranks": world, "map_provers_per_gpu": 3,
           "sha256_compressions": (2 * blocks - 1) * 2}
    rng = np.random.default_rng(12)                                  # the same range on every rank
    for run in ("first_run_records_circuits", "steady_state"):
        hs = [3_000_000 + i for i in range(blocks)]
        rs = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in hs]
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        out = mr.prove_range_distributed(hs, rs, device=dev)
        dt = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([dt, out["map_seconds"]], dtype=torch.float64, device=_coll_device())
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt, map_s = float(tt[0].item()), float(tt[1].item())
        else:
            map_s = out["map_seconds"]
        if rank == 0:
            lvl = [hashlib.sha256(b"\x00" + int(h).to_bytes(32, "big") + r).digest() for h, r in zip(hs, rs)]
            while len(lvl) > 1:
                lvl = [hashlib.sha256(b"\x01" + lvl[i] + lvl[i + 1]).digest() for i in range(0, len(lvl), 2)]
            t1 = time.perf_counter()
            ok = out["commitment"] == lvl[0] and mr.verify(out["root_proof"], out["key"], hs, rs, out["commitment"])
            res[run] = {"seconds": round(dt, 4), "map_seconds_max_over_ranks": round(map_s, 4), "levels_on_rank0": out["levels"],
                        "commitment_matches_hashlib_and_verifies": bool(ok), "verify_seconds": round(time.perf_counter() - t1, 4),
                        "root_proof_bytes": len(out["root_proof"]), "blocks_per_second": round(blocks / dt, 1)}
    if rank == 0:
        res["record_seconds_rank0"] = dict(mr.record_seconds)
        res["leaf"] = {"rows": mr.leaf_program.stats["rows"], "wires": mr.leaf_circuit.n_wires}
        res["nodes"] = {f"level{k[0]}_fan{k[1]}": {s: v for s, v in rp.stats.items() if s in ("rows", "rows_used", "poseidon_rows", "sha_rows", "arith_gates")}
                        for k, rp in mr.nodes.items()}
        res["note"] = ("build-defined statement (NOT upstream's circuit): public inputs of the root proof = the 8 words of the RFC 6962 SHA-256 root over "
                       "abi.encode(height, dataRoot) of the whole range + a Poseidon digest tree of the tuples; every compression constrained (SHA row gates), "
                       "every child proof verified in-circuit; seconds = Map + Reduce, whole job")
    mr.free()
    for p in extra:
        p.close()
    pr.close()
    return res


def mapreduce_bench(leaves_per_rank=16, log_n=16, W=80):
    """BASELINE configs[2]/[3] shape (skip / batch leaves): Map = one leaf proof per leaf, leaf i on
    rank i % world; exchange = one all-gather of padded proofs (RCCL when launched under
    torch.distributed.run, a no-op on one rank).  Leaf circuit = the build-defined circuit; `seconds` is map + gather, the Reduce
    forms (native verification, aggregation tree, recursive verification) are reported beside it under `aggregation`."""
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(_gpu_index(local_rank))
    if world > 1:
        _init_dist(local_rank)
    res = mapreduce_leg(graft.load_package(), rank, local_rank, world, leaves_per_rank, log_n, W)
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--full", action="store_true", help="also the single-launch median, the roofline, the other sizes, the CPU baseline and the "
                                                        "optional prove / MapReduce legs (a plain run times the headline transform only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write a fixed sample of the last timed step's output to DIR/*.npy (rank 0)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--no-sizes", action="store_true", help="with --full: skip the 2^20/2^22/2^24 sweep")
    ap.add_argument("--no-prove", action="store_true", help="with --full: skip the end-to-end prove leg")
    ap.add_argument("--sweep", action="store_true", help="tuning aid: time alternative pass plans and exit")
    ap.add_argument("--hash-bench", action="store_true", help="tuning aid: Poseidon / LDE / Merkle stage times and exit")
    ap.add_argument("--prove-bench", action="store_true", help="end-to-end prove time of the build-defined circuit and exit")
    ap.add_argument("--mapreduce", action="store_true", help="map (leaf proofs sharded over ranks) + all-gather timing and exit")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.sweep:
        return sweep()
    if args.hash_bench:
        return hash_bench()
    if args.prove_bench:
        return prove_bench([(14, 16), (16, 80), (20, 80)])
    if args.mapreduce:
        return mapreduce_bench()
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    torch.cuda.set_device(_gpu_index(local_rank))
    if world > 1:
        _init_dist(local_rank)

    pkg = graft.load_package()
    pr = pkg.Prover(_gpu_index(local_rank))
    log_n, batch = args.log_n, args.batch
    n = 1 << log_n

    host = splitmix_fill(n * batch, 0x9E3779B97F4A7C15 + rank).reshape(batch, n)
    d = pr.to_device(host)
    del host

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        pr.sync()

    for _ in range(args.warmup):
        pr.ntt_(d, log_n, batch)
    barrier()
    t0 = time.perf_counter()
    pr.timer_start()
    for _ in range(args.steps):
        pr.ntt_(d, log_n, batch)
    ev_ms = pr.timer_stop()
    barrier()
    wall = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([wall], dtype=torch.float64, device=_coll_device())
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        wall = float(tt.item())
    ms_per_step = wall * 1e3 / args.steps
    alg_bytes = 16.0 * n * batch
    value = alg_bytes * world / (ms_per_step * 1e-3) / 1e9
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, d, batch, n)

    out = None
    if rank == 0:
        plan = pr.describe_plan(log_n, batch)
        out = {
            "metric": "Goldilocks NTT GB/s @ 2^20\u20132^24", "value": round(value, 2), "unit": "GB/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "config": {"workload": f"forward NTT, n=2^{log_n}, batch={batch} per GPU, in place, natural order "
                                   f"(BASELINE configs[1] wires shape)", "log_n": log_n, "batch_per_gpu": batch,
                       "plan": plan, "algorithmic_bytes_per_step": alg_bytes,
                       "plan_is_the_bit_exact_tested_plan": plan == EXPECTED_HEADLINE_PLAN if (log_n, batch) == (20, 128) else None,
                       "event_ms_per_step": round(ev_ms / args.steps, 4), "timing": TIMING_PROTOCOL},
        }
    if not args.full:
        d.free()
        pr.close()
        if rank == 0:
            print(json.dumps(out), flush=True)
        _finish(world)
        return

    if rank == 0:
        # SURVEY.md 8(d)'s protocol beside the contract's mean: 50 individually HIP-event-timed transforms after the warm-up, median
        singles = []
        for _ in range(50):
            pr.timer_start()
            pr.ntt_(d, log_n, batch)
            singles.append(pr.timer_stop())
        median50 = float(np.median(singles))
        # per-pass kernel times of ONE transform, HIP events on the ctx stream
        pr.set_profiling(True)
        acc = None
        reps = max(3, min(args.steps, 10))
        for _ in range(reps):
            pr.ntt_(d, log_n, batch)
            ms = pr.last_pass_ms()
            acc = ms if acc is None else [a + b for a, b in zip(acc, ms)]
        pr.set_profiling(False)
        pass_ms = [a / reps for a in acc]
        # roofline.achieved: the pass kernels of one transform, timed by HIP events on the ctx stream around the SAME --steps back-to-back
        # transforms `value` is taken over (no event between the passes: the kernels run exactly as in the timed region; the stream holds nothing
        # else, so event time / steps = the summed average launch durations of the pass kernels + their launch gaps).  pass_ms is the split
        # from the profiling mode, which brackets every pass with its own events and runs ~2 % slower: it apportions, it does not define.
        kern_ms = ev_ms / args.steps
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
        out["config"].update({"median_ms_of_50_single_launch_timings": round(median50, 4),
                              "median_of_50_gbps": round(alg_bytes / (median50 * 1e-3) / 1e9, 1)})
        out["roofline"] = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                           "frac": round(achieved / HBM_PEAK_GBPS, 4),
                           "traffic": pmc_traffic_bytes(plan, float(n) * batch),
                           "kernel": "glp_ntt_pass_kernel (all passes of one transform)",
                           "kernel_ms_per_transform": round(kern_ms, 4),
                           "pass_ms_profiling_mode": [round(m, 4) for m in pass_ms],
                           "pass_gbps_profiling_mode": [round(alg_bytes / (m * 1e-3) / 1e9, 1) for m in pass_ms]}
    d.free()

    if rank == 0 and not args.no_sizes:
        sizes = {}
        for ln, b in ((20, 1), (22, 1), (24, 1), (22, 32), (24, 8)):
            x = splitmix_fill((1 << ln) * b, 5).reshape(b, 1 << ln)
            dd = pr.to_device(x)
            ms = time_ntt(pr, dd, ln, b, steps=10, warmup=3)
            dd.free()
            sizes[f"2^{ln}xb{b}"] = {"ms": round(ms, 4), "gbps": round(16.0 * (1 << ln) * b / (ms * 1e-3) / 1e9, 1),
                                     "plan": pr.describe_plan(ln, b)}
        out["sizes"] = sizes
    if rank == 0 and world == 1 and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(log_n)
    pr.close()
    # ---- the contract line goes out NOW: metric, roofline, cpu_baseline.  Everything after this point is extra; whatever happens there — an
    # exception, a peer lost inside a collective on a fabric this build never ran on, a leg that takes too long — cannot cost the record.
    # The enriched line (same contract fields + the optional legs) is printed again at the end.
    if rank == 0:
        print(json.dumps(dict(out, optional_legs="pending: the enriched line follows")), flush=True)
    if args.no_prove:
        _finish(world)
        return
    legs = LegRunner(rank, world, out)
    legs.start_watchdog()

    def prove_leg():
        # first half of the BASELINE metric, as far as it can be honoured: end-to-end prove time of the build's own 2^20-row circuits
        # (configs[1] size); the upstream circuits are not in the mount
        r = prove_bench([(20, 80)], quiet=True)[0]
        return {"seconds": r["prove_s_best"], "verified": r["verified"], "verify_seconds": r["verify_s"], "circuit": r["circuit"], "log_n": 20,
                "wires": 80, "proof_bytes": r["proof_bytes"], "queries": 28, "pow_bits": 16, "stage_ms": r["stage_ms"],
                "stage_detail": prove_stage_detail(r["stage_ms"], 20, 80), "cpu_baseline": prove_cpu_baseline(pkg),
                "note": "commit wires, Z/partial products, quotient, FRI openings; inputs resident in HBM"}
    if world == 1:
        legs.run("prove", prove_leg, estimate_s=30)
        legs.run("prove_constrained", lambda: prove_constrained_leg(pkg), estimate_s=15)
    # the metric's first half: CombinedSkip(128) and CombinedSkip(1024) with the real statement (configs[2]/[3]), then configs[4]'s 4096-block
    # data commitment — MapReduces of proofs, on every rank (powers of two up to 64 ranks).  GLP_BENCH_RANGE=0 skips them.
    if os.environ.get("GLP_BENCH_RANGE", "1") != "0" and world <= 64 and world & (world - 1) == 0:
        legs.run("combined_skip", lambda: combined_skip_leg(pkg, rank, local_rank, world), collective=True, estimate_s=100)
        legs.run("data_commitment_range", lambda: data_commitment_range_leg(pkg, rank, local_rank, world), collective=True, estimate_s=25)
        if os.environ.get("GLP_BENCH_HEADER_CHAIN", "0") == "1":      # superseded by combined_skip (same leaves, 4-header form); opt-in
            legs.run("header_chain_range", lambda: header_chain_leg(pkg, rank, local_rank, world), collective=True, estimate_s=25)
    # the MapReduce shape with the build's arithmetic leaf: 16 leaf proofs per GPU + one all-gather + the Reduce forms, every rank
    legs.run("mapreduce", lambda: mapreduce_leg(pkg, rank, local_rank, world), collective=True, estimate_s=40)
    if world == 1:
        legs.run("data_commitment_circuit", lambda: data_commitment_leg(pkg), estimate_s=10)
        legs.run("validator_set_circuit", lambda: validator_set_leg(pkg), estimate_s=5)
        legs.run("skip_circuit", lambda: skip_leg(pkg), estimate_s=5)
    legs.finish()
    if rank == 0:
        print(json.dumps(out), flush=True)
    _finish(world)


def _finish(world):
    if world > 1:
        import torch.distributed as dist
        try:                                             # the line is out: a peer that left early must not turn it into a failure
            dist.barrier()
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001
            pass


_FAULT = os.environ.get("GLP_BENCH_INJECT_FAULT", "")      # "<leg>:<rank>[:hang]": rehearsal aid (tests the leg runner, never set by the driver)


def _maybe_fault(leg, rank):
    """called from inside the collective legs: raises (or sleeps forever with ':hang') on the named rank"""
    parts = _FAULT.split(":")
    if len(parts) >= 2 and parts[0] == leg and int(parts[1]) == rank:
        if len(parts) > 2 and parts[2] == "hang":
            time.sleep(10 ** 6)
        raise RuntimeError(f"injected fault in {leg} on rank {rank}")


class LegRunner:
    """Runs the optional legs so that none of them can cost the bench record.
      * every leg is try/except'ed: its object is the result or {"error": ...};
      * at N > 1 the ranks meet after every collective leg at a STORE barrier (torch.distributed's rendezvous store: host-side, no GPU
        collective).  A rank whose leg raised still arrives there; if every rank arrives, all are at a clean point and go on with the next leg.
        If some rank does not arrive within GLP_BENCH_LEG_GRACE seconds of the first failure (it is stuck inside a collective its failed peer
        never entered), the job is aborted: the 'abort' key is set, every rank's watchdog thread sees it, rank 0 prints the line it has with
        `optional_legs_aborted`, and every rank leaves with exit code 0 (the contract line is already out);
      * a total budget (GLP_BENCH_OPTIONAL_BUDGET, default 270 s — the driver allows 600 s for the whole run) and a per-leg limit
        (GLP_BENCH_LEG_TIMEOUT, default 150 s): a leg is skipped when its estimate does not fit what is left, and a leg still running at its
        limit is treated as hung (same exit path as an abort, marked `optional_legs_timed_out`).
    The watchdog only ever prints and exits (os._exit): it never re-execs and starts nothing on the GPU."""

    def __init__(self, rank, world, out):
        self.rank, self.world, self.out = rank, world, out
        self.budget = float(os.environ.get("GLP_BENCH_OPTIONAL_BUDGET", "270"))
        self.leg_limit = float(os.environ.get("GLP_BENCH_LEG_TIMEOUT", "150"))
        self.grace = float(os.environ.get("GLP_BENCH_LEG_GRACE", "20"))
        self.t0 = time.monotonic()
        self.leg_started, self.leg_name, self.seq = None, None, 0
        self.store = None
        if world > 1:
            try:
                import torch.distributed as dist
                self.store = dist.distributed_c10d._get_default_store()
            except Exception:  # noqa: BLE001 — without the store only the time limits protect the line
                self.store = None
        import threading
        self.done = threading.Event()
        self.lock = threading.Lock()

    def left(self):
        return self.budget - (time.monotonic() - self.t0)

    # ---- watchdog thread --------------------------------------------------------------------------------------------------------
    def start_watchdog(self):
        import threading
        threading.Thread(target=self._watch, daemon=True).start()

    def _leave(self, why):
        if self.rank == 0:
            with self.lock:
                snap = dict(self.out)
            snap[why[0]] = why[1]
            try:
                line = json.dumps(snap)
            except Exception:  # noqa: BLE001
                line = json.dumps({k: v for k, v in snap.items() if k in CONTRACT_KEYS} | {why[0]: why[1]})
            print(line, flush=True)
        sys.stdout.flush()
        os._exit(0)

    def _watch(self):
        while not self.done.wait(0.5):
            name, started = self.leg_name, self.leg_started
            if started is not None and time.monotonic() - started > self.leg_limit:
                self._set_abort(f"leg {name} exceeded {self.leg_limit:.0f} s on rank {self.rank}")
                self._leave(("optional_legs_timed_out", f"{name}: still running after {self.leg_limit:.0f} s"))
            if self.left() < -5:
                self._leave(("optional_legs_timed_out", f"budget of {self.budget:.0f} s spent (in {name})"))
            why = self._aborted()
            if why:
                self._leave(("optional_legs_aborted", why))

    def _set_abort(self, why):
        if self.store is not None:
            try:
                self.store.set("glp_bench_abort", why)
            except Exception:  # noqa: BLE001
                pass

    def _aborted(self):
        if self.store is None:
            return None
        try:
            if self.store.check(["glp_bench_abort"]):
                return self.store.get("glp_bench_abort").decode(errors="replace")
        except Exception:  # noqa: BLE001
            return None
        return None

    # ---- legs -------------------------------------------------------------------------------------------------------------------
    def run(self, name, fn, collective=False, estimate_s=10):
        if self.left() < estimate_s:
            if self.rank == 0:
                with self.lock:
                    self.out[name] = {"skipped": f"{self.left():.0f} s of the optional budget left, the leg needs about {estimate_s} s"}
            return
        self.leg_name, self.leg_started = name, time.monotonic()
        failed = None
        try:
            res = fn()
        except Exception as e:  # noqa: BLE001
            failed = f"{type(e).__name__}: {e}"[:300]
            res = {"error": failed}
        self.leg_started = None
        if self.rank == 0:
            with self.lock:
                self.out[name] = res
        if collective and self.world > 1:
            self._meet(name, failed)

    def _meet(self, name, failed):
        """store barrier after a collective leg; aborts the job when a peer does not arrive after some rank has failed"""
        if self.store is None:
            return
        self.seq += 1
        key = f"glp_bench_leg{self.seq}"
        try:
            if failed:
                self.store.set(f"{key}_failed", f"rank {self.rank}: {failed}")
            self.store.add(f"{key}_count", 1)
            first_failure = None
            while True:
                if int(self.store.add(f"{key}_count", 0)) >= self.world:
                    break
                if first_failure is None and self.store.check([f"{key}_failed"]):
                    first_failure = time.monotonic()
                if first_failure is not None and time.monotonic() - first_failure > self.grace:
                    why = self.store.get(f"{key}_failed").decode(errors="replace")
                    self._set_abort(f"{name}: {why}; a peer never left the leg")
                    time.sleep(3600)                     # the watchdog thread ends the process
                time.sleep(0.05)
            if self.rank == 0 and self.store.check([f"{key}_failed"]):
                with self.lock:
                    if isinstance(self.out.get(name), dict):
                        self.out[name].setdefault("failed_on", self.store.get(f"{key}_failed").decode(errors="replace"))
        except Exception as e:  # noqa: BLE001 — a store error: fall back to the time limits
            if self.rank == 0:
                with self.lock:
                    self.out.setdefault("leg_runner_warnings", []).append(f"{name}: store barrier failed: {e}"[:200])

    def finish(self):
        self.done.set()


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                 "data", "config", "roofline", "cpu_baseline")


if __name__ == "__main__":
    main()
