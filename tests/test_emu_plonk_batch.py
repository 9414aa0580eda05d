"""The kernels of glp_plonk_prove_batch on the CPU (tests/emu_plonk_batch): every batched body of csrc/plonk_batch_kernels.cuh, launched with
the grids the driver uses (256 lanes, B * blocks_per_instance workgroups), against the single-instance body of csrc/plonk_kernels.cuh it
replaces, word for word, on random canonical arrays (K7 needs no satisfiable witness for this).  Every instance holds independent data, so a
wrong instance offset cannot pass; sentinel words between the instances' outputs must be left alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, poseidon_consts, ptr, rand_field, u64p

D = os.path.join(ROOT, "tests", "emu_plonk_batch")
SENTINEL = np.uint64(0x5E5E5E5E5E5E5E5E)
GAP = 3
ptrs_t = ctypes.POINTER(ctypes.c_void_p)
POS, SHA, EXT = 1, 2, 4


@pytest.fixture(scope="module")
def epb():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_plonk_batch.so"))
    c32, c64, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    lib.emu_gather_wires_batch.argtypes = [ptrs_t, c64, c32, c32, u64p]
    lib.emu_perm_quotients_batch.argtypes = [ptrs_t, u64p, c32, c32, c32, u64p, u64p, u64p, c64, u64p, c64]
    lib.emu_perm_quotients_single.argtypes = [u64p, u64p, c32, c32, u64p, u64p, u64p, u64p]
    lib.emu_scan.argtypes = [u64p, u64p, c32, c32, c32, u64p]
    lib.emu_quotient_batch.argtypes = [u64p, u64p, ptrs_t, ptrs_t, ptrs_t, c32, c32, c32, c32, c32, ci, u64p, u64p, u64p, u64p, c32, u64p, c64]
    lib.emu_quotient_single.argtypes = [u64p, u64p, u64p, u64p, u64p, c32, c32, c32, c32, c32, ci, u64p, u64p, u64p, u64p, u64p]
    return lib


def host_ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def row(a, i):
    return ptr(np.ascontiguousarray(a[i]))


def test_gather_wires(epb):
    """B matrices side by side; a length that is no multiple of 256 and fewer blocks per instance than one pass needs"""
    rng = np.random.default_rng(1)
    B, words = 3, 1000
    src = [rand_field(rng, words) for _ in range(B)]
    dst = np.full(B * words + GAP, SENTINEL, dtype=np.uint64)
    epb.emu_gather_wires_batch(host_ptrs(src), words, B, 2, ptr(dst))
    assert np.array_equal(dst[:B * words].reshape(B, words), np.stack(src))
    assert np.all(dst[B * words:] == SENTINEL)


# (log_n, routed): the small domain, M = 17 and M = 1 chunks, the upper root table (n > 4096), two scan blocks (2^11)
@pytest.mark.parametrize("log_n,R", [(3, 8), (3, 136), (10, 8), (11, 16), (13, 8)])
@pytest.mark.parametrize("B", [1, 3])
def test_perm_products(epb, log_n, R, B):
    """K6a batched against K6a single per instance; then the three UNCHANGED scan kernels launched with B * NCHAL challenges over the dense
    [B * NCHAL]-major buffers against NCHAL challenges per instance"""
    n, M = 1 << log_n, R // 8
    rng = np.random.default_rng(1000 * log_n + 10 * R + B)
    wires = [rand_field(rng, (R, n)) for _ in range(B)]
    sig, betas, gammas = rand_field(rng, (R, n)), rand_field(rng, (B, 2)), rand_field(rng, (B, 2))
    qvw, rrw = 2 * M * n, 2 * n
    qv = np.full((B, qvw + GAP), SENTINEL, dtype=np.uint64)
    rr = np.full((B, rrw + GAP), SENTINEL, dtype=np.uint64)
    epb.emu_perm_quotients_batch(host_ptrs(wires), ptr(sig), log_n, R, B, ptr(betas), ptr(gammas), ptr(qv), qvw + GAP, ptr(rr), rrw + GAP)
    qd, rd = np.zeros((B, qvw), dtype=np.uint64), np.zeros((B, rrw), dtype=np.uint64)
    for i in range(B):
        q1, r1 = np.zeros(qvw, dtype=np.uint64), np.zeros(rrw, dtype=np.uint64)
        epb.emu_perm_quotients_single(ptr(wires[i]), ptr(sig), log_n, R, row(betas, i), row(gammas, i), ptr(q1), ptr(r1))
        assert np.array_equal(qv[i, :qvw], q1) and np.array_equal(rr[i, :rrw], r1), i
        assert np.all(qv[i, qvw:] == SENTINEL) and np.all(rr[i, rrw:] == SENTINEL), i
        qd[i], rd[i] = q1, r1
    if log_n > 11:
        return                                                          # the scan's shapes are covered at 2^11 (two blocks) and below
    zs = np.zeros((B, qvw), dtype=np.uint64)
    epb.emu_scan(ptr(rd), ptr(qd), log_n, M, 2 * B, ptr(zs))
    for i in range(B):
        z1 = np.zeros(qvw, dtype=np.uint64)
        epb.emu_scan(row(rd, i), row(qd, i), log_n, M, 2, ptr(z1))
        assert np.array_equal(zs[i], z1), i
    assert len({zs[i].tobytes() for i in range(B)}) == B


# (log_n, W, R, flags): every flag combination the driver selects between, at N = 2^6 (no upper root table); M = 17 and M = 1
SHAPES = [(3, 8, 8, 0), (3, 160, 136, 0), (3, 136, 80, POS), (3, 160, 136, POS), (3, 160, 16, SHA), (3, 144, 80, SHA | POS), (3, 144, 80, EXT | POS | SHA),
          (3, 16, 16, EXT)]


def quotient_case(epb, log_n, W, R, flags, kind, with_pi, B, seed):
    rb = 3
    N, M = 1 << (log_n + rb), R // 8
    n_const = 6 + (4 if flags & SHA else 0) + (1 if flags & EXT else 0)
    rng = np.random.default_rng(seed)
    consts, sig = rand_field(rng, (n_const, N)), rand_field(rng, (R, N))
    wires, zs, pi = ([rand_field(rng, s) for _ in range(B)] for s in ((W, N), (2 * M, N), (N,)))
    betas, gammas, alphas = (rand_field(rng, (B, 2)) for _ in range(3))
    pos = np.concatenate(poseidon_consts(kind)).astype(np.uint64)
    small = 1 if kind == "small" else 0
    ow = 2 * N
    out = np.full((B, ow + GAP), SENTINEL, dtype=np.uint64)
    epb.emu_quotient_batch(ptr(consts), ptr(sig), host_ptrs(wires), host_ptrs(zs), host_ptrs(pi) if with_pi else None, log_n, rb, W, R, flags, small,
                           ptr(pos), ptr(betas), ptr(gammas), ptr(alphas), B, ptr(out), ow + GAP)
    ref = []
    for i in range(B):
        o1 = np.zeros(ow, dtype=np.uint64)
        epb.emu_quotient_single(ptr(consts), ptr(sig), ptr(wires[i]), ptr(zs[i]), ptr(pi[i]) if with_pi else None, log_n, rb, W, R, flags, small, ptr(pos),
                                row(betas, i), row(gammas, i), row(alphas, i), ptr(o1))
        assert np.array_equal(out[i, :ow], o1), i
        assert np.all(out[i, ow:] == SENTINEL), i
        ref.append(o1.tobytes())
    assert len(set(ref)) == B


# both MDS kinds where the circuit has Poseidon rows (without them the kind selects nothing), public inputs present and absent, B = 1 and 3
CASES = [s + (kind, with_pi, B) for s in SHAPES for kind in (("small", "big") if s[3] & POS else ("small",)) for with_pi in (False, True) for B in (1, 3)]


@pytest.mark.parametrize("log_n,W,R,flags,kind,with_pi,B", CASES)
def test_quotient(epb, log_n, W, R, flags, kind, with_pi, B):
    """K7 (and K7s with SHA rows) batched against single, per instance: <false>, <true, true> (small MDS) and the generic <true, false>"""
    quotient_case(epb, log_n, W, R, flags, kind, with_pi, B, 7 * log_n + W + R + 13 * flags + (kind == "big") + 2 * with_pi + 4 * B)


@pytest.mark.parametrize("W,R,flags,kind,with_pi", [(16, 16, 0, "small", True), (136, 24, POS, "small", False)])
def test_quotient_with_upper_root_table(epb, W, R, flags, kind, with_pi):
    """log_n = 10: N = 2^13, the upper root table in use, 32 workgroups per instance"""
    quotient_case(epb, 10, W, R, flags, kind, with_pi, 3, 99 + W)


def test_sanitized_standalone_program():
    """the same source as an ordinary executable under AddressSanitizer + UBSan: every batched body against the single one, word for word"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_plonk_batch_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
