"""The witness checker without a GPU.  First the reference alone (tests/check_ref.py): every witness pref.build_circuit makes is satisfied and
every mutation case gives a violation.  Then the kernels of glp_plonk_check_witness[_batch] on the CPU (tests/emu_check: the four check kernels
and the two decode kernels of csrc/check_kernels.cuh with the driver's grids) against that reference word for word — counts, first key, list,
values and peers — and the host decode function of csrc/check_plan.h on every cell of a 2^3 and a 2^13 circuit, with its refusals.  The same
source as a stand-alone program under AddressSanitizer + UBSan is built and run directly."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_ref as cref  # noqa: E402
import fri_verifier as fv  # noqa: E402
import plonk_ref as pref  # noqa: E402
from conftest import P, ROOT, poseidon_consts, ptr, u64p  # noqa: E402

D = os.path.join(ROOT, "tests", "emu_check")
SENTINEL = 0x5E5E5E5E
u32p = ctypes.POINTER(ctypes.c_uint32)
BAD = 0xFFFFFFFF
KEY_NONE = (1 << 64) - 1


class Violation(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("row", ctypes.c_uint32), ("index", ctypes.c_uint32), ("n_in_row", ctypes.c_uint32),
                ("peer_wire", ctypes.c_uint32), ("peer_row", ctypes.c_uint32), ("value", ctypes.c_uint64), ("peer_value", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def ech():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_check.so"))
    c32, c64 = ctypes.c_uint32, ctypes.c_uint64
    lib.emu_sigma_decode_host.argtypes = [u64p, c64, c32, c32, u32p]
    lib.emu_sigma_decode.argtypes = [u64p, c32, c32, u32p, u64p]
    lib.emu_check.argtypes = [u64p, u32p, u64p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), u64p, c32, c32, c32, c32, c32, c32, c32, u64p,
                              ctypes.c_void_p]
    return lib


def circuits():
    """name -> (circuit, Poseidon constants kind): small shapes with every row kind"""
    out = {}
    out["3-8-8"] = (pref.build_circuit(np.random.default_rng(1), 3, 8), None)
    out["9-16-8-pub"] = (pref.build_circuit(np.random.default_rng(2), 9, 16, n_routed=8, n_public=2), None)
    for kind in ("small", "big"):
        consts = poseidon_consts(kind)
        rng = np.random.default_rng(3)
        out["6-144-24-all-" + kind] = (pref.build_circuit(rng, 6, 144, n_routed=24, n_public=2, poseidon_rows=range(10, 16), consts=consts,
                                                          sha_rows=range(20, 44), ext_rows=range(50, 56)), kind)
    return out


@pytest.fixture(scope="module")
def cases():
    return circuits()


def mutations(circ):
    """(label, wires) — one per constraint family of the circuit, each expected to fail"""
    n, R, W = 1 << circ["log_n"], circ["R"], circ["W"]
    w = circ["wires"]
    q = circ["consts"][0]
    arith = next(i for i in range(circ["n_public"], n) if int(q[i]))
    out = [("arith", cref.mutate(w, arith, 3)), ("arith-last-chunk", cref.mutate(w, arith, R - 1))]
    if circ["n_public"]:
        out.append(("public", cref.mutate(w, 0, 0)))
    if circ["flags"] & pref.FLAG_POSEIDON:
        row = next(i for i in range(n) if int(circ["consts"][5][i]))
        for k in (0, 3, 40, 70, 100, 122):
            wire, val = cref.poseidon_target(k)
            out.append((f"poseidon-{k}", cref.mutate(w, row, wire, val)))
    if circ["flags"] & pref.FLAG_SHA:
        kinds = cref.sha_kinds(circ)
        for k in (0, 45, 77, 131, 132, 133, 134, 135, 136, 137, 138, 139):
            row, wire, val = cref.sha_target(k, kinds)
            out.append((f"sha-{k}", cref.mutate(w, row, wire, val)))
    if circ["flags"] & pref.FLAG_EXT:
        row = next(i for i in range(n) if int(circ["consts"][-1][i]))
        out += [("ext-0", cref.mutate(w, row, 6)), ("ext-1", cref.mutate(w, row, R - 1))]
    return out


def test_reference_alone(cases):
    """before anything is compared with it: built witnesses pass, every mutation case fails, and the targeted constraint is the one reported"""
    for name, (circ, _) in cases.items():
        rc = cref.RefChecker(circ)
        summary, lst = rc.check(circ["wires"], circ["public"])
        assert lst == [] and not any(summary.values()), name
        M = circ["R"] // 8
        for label, w in mutations(circ):
            summary, lst = rc.check(w, circ["public"])
            assert lst and summary["n_gate_bad"] + summary["n_copy_bad"] > 0, (name, label)
            gate = [v for v in lst if v["kind"] == cref.GATE]
            if label.startswith("poseidon-"):
                assert gate[0]["index"] == 2 + 3 * M + int(label.split("-")[1]), (name, label)
            if label.startswith("sha-"):
                assert gate[0]["index"] == rc.first_sha + int(label.split("-")[1]), (name, label)
            if label == "public":
                assert gate[0]["index"] == 1 and gate[0]["row"] == 0


def emu_run(ech, circ, kind, wires_list, publics, max_list):
    n, R, W = 1 << circ["log_n"], circ["R"], circ["W"]
    B = len(wires_list)
    cells = cref.decode_sigma(circ["sigmas"], circ["log_n"])
    sidx = np.array([[jj * n + ii for (jj, ii) in row] for row in cells], dtype=np.uint32)
    consts = np.ascontiguousarray(circ["consts"], dtype=np.uint64)
    pc = np.concatenate(poseidon_consts(kind or "small")).astype(np.uint64)
    mats = [np.ascontiguousarray(w, dtype=np.uint64) for w in wires_list]
    ptrs = (ctypes.c_void_p * B)(*[m.ctypes.data for m in mats])
    pubs = np.ascontiguousarray(publics, dtype=np.uint64).reshape(B, circ["n_public"]) if circ["n_public"] else np.zeros(1, dtype=np.uint64)
    acc = np.zeros((B, 5), dtype=np.uint64)
    lists = (Violation * (B * max_list + 1))()
    lists[B * max_list].kind = SENTINEL
    ech.emu_check(ptr(consts), sidx.ctypes.data_as(u32p), ptr(pc), 1 if kind != "big" else 0, ptrs, ptr(pubs), B, circ["log_n"], W, R, circ["n_public"],
                  circ["flags"], max_list, ptr(acc), ctypes.addressof(lists))
    assert lists[B * max_list].kind == SENTINEL
    out = []
    for b in range(B):
        a = [int(v) for v in acc[b]]
        summary = {"n_gate_bad": a[0], "n_copy_bad": a[1], "n_gate_rows": a[3] & 0xFFFFFFFF, "n_copy_rows": a[3] >> 32}
        summary["n_listed"] = min(summary["n_gate_rows"] + summary["n_copy_rows"], max_list)
        lst = [{k: int(getattr(lists[b * max_list + i], k)) for k, _ in Violation._fields_} for i in range(summary["n_listed"])]
        out.append((summary, lst, a[2]))
    return out


@pytest.mark.parametrize("name", ["3-8-8", "9-16-8-pub", "6-144-24-all-small", "6-144-24-all-big"])
def test_kernels_equal_reference(ech, cases, name):
    """one batched run per circuit: the good witness first and last, every mutation between them (a wrong instance offset cannot pass), a list
    shorter than the violations of some instances; every summary, list entry, value and peer as the reference gives them"""
    circ, kind = cases[name]
    rc = cref.RefChecker(circ)
    muts = mutations(circ)
    wires_list = [circ["wires"]] + [w for _, w in muts] + [circ["wires"]]
    publics = [circ["public"]] * len(wires_list)
    max_list = 3
    got = emu_run(ech, circ, kind, wires_list, publics, max_list)
    for b, w in enumerate(wires_list):
        summary, lst = rc.check(w, circ["public"], max_list)
        assert got[b][0] == summary, (name, b)
        assert got[b][1] == lst, (name, b)
        if lst:
            assert got[b][2] == (lst[0]["row"] << 20) | (lst[0]["kind"] << 19) | lst[0]["index"]
        else:
            assert got[b][2] == KEY_NONE
    assert not got[0][1] and not got[-1][1]


def test_wrong_public_input_is_a_gate_violation(ech, cases):
    circ, kind = cases["9-16-8-pub"]
    other = list(circ["public"])
    other[1] = (other[1] + 1) % P
    (summary, lst, _), = emu_run(ech, circ, kind, [circ["wires"]], [other], 4)
    assert (summary, lst) == cref.RefChecker(circ).check(circ["wires"], other, 4)
    assert lst[0]["row"] == 1 and lst[0]["index"] == 1 and lst[0]["kind"] == cref.GATE


@pytest.mark.parametrize("log_n,W,R", [(3, 8, 8), (13, 16, 8)])
def test_decode_every_cell(ech, log_n, W, R):
    """the host decode function and the decode kernels on every routed cell: 2^3 (fewer rows than a wavefront) and 2^13 (indices beyond the
    4096-entry first-level root table); then the refusals"""
    circ = pref.build_circuit(np.random.default_rng(log_n), log_n, W, n_routed=R)
    n = 1 << log_n
    sig = np.ascontiguousarray(circ["sigmas"], dtype=np.uint64)
    want = np.array([[jj * n + ii for (jj, ii) in row] for row in cref.decode_sigma(circ["sigmas"], log_n)], dtype=np.uint32)
    assert (want != np.arange(R * n, dtype=np.uint32).reshape(R, n)).any()
    got = np.zeros((R, n), dtype=np.uint32)
    ech.emu_sigma_decode_host(ptr(sig), R * n, log_n, R, got.ctypes.data_as(u32p))
    assert np.array_equal(got, want)
    idx = np.zeros((R, n), dtype=np.uint32)
    status = np.zeros(2, dtype=np.uint64)
    ech.emu_sigma_decode(ptr(sig), log_n, R, idx.ctypes.data_as(u32p), ptr(status))
    assert np.array_equal(idx, want) and [int(v) for v in status] == [KEY_NONE, KEY_NONE]
    # not on the domain: zero, a value off every coset of the subgroup (x + 1 for a domain point x need not be one: checked by the reference
    # dictionary), and a coset j' >= R
    dom = cref.domain(log_n, R)
    off = next(v for v in ((int(sig[1, 2]) + d) % P for d in range(1, 50)) if v not in dom)
    beyond = pow(7, R, P) * pow(fv.root(log_n), 5, P) % P
    vals = np.array([0, off, beyond, int(sig[0, 0])], dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint32)
    ech.emu_sigma_decode_host(ptr(vals), 4, log_n, R, out.ctypes.data_as(u32p))
    assert [int(v) for v in out[:3]] == [BAD, BAD, BAD] and int(out[3]) == int(want[0, 0])
    for cell, v in (((1, 3), off), ((0, 5), beyond)):
        bad = sig.copy()
        bad[cell] = v
        ech.emu_sigma_decode(ptr(bad), log_n, R, idx.ctypes.data_as(u32p), ptr(status))
        assert int(status[0]) == cell[0] * n + cell[1] and int(idx.max()) < R * n
        with pytest.raises(cref.SigmaError, match=f"no domain point: wire {cell[0]}, row {cell[1]}"):
            cref.decode_sigma(bad, log_n)
    # a map that is no bijection: two cells sent to one target
    bad = sig.copy()
    bad[1, 1] = sig[0, 4] if sig[1, 1] != sig[0, 4] else sig[0, 5]
    ech.emu_sigma_decode(ptr(bad), log_n, R, idx.ctypes.data_as(u32p), ptr(status))
    assert int(status[0]) == KEY_NONE and int(status[1]) != KEY_NONE
    with pytest.raises(cref.SigmaError, match="not a bijection") as ei:
        cref.decode_sigma(bad, log_n)
    j, i = divmod(int(status[1]), n)
    assert f"wire {j}, row {i}" in str(ei.value)


def test_sanitized_program():
    """the same kernels as a stand-alone program under AddressSanitizer + UBSan, run directly"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_check_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "emu_check_san ok" in r.stdout, r.stdout[-3000:]
