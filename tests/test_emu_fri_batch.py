"""The kernels of glp_fri_prove_batch on the CPU (tests/emu_fri_batch): every batched body of csrc/fri_batch_kernels.cuh, launched with the
grids of the product's own plan (csrc/fri_batch_plan.h), against the single-instance body it replaces, word for word.  Every instance holds
independent random data, so a wrong instance offset cannot pass.  The plan's counts come from the product library, which loads without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, poseidon_consts, ptr, rand_field, u64p

D = os.path.join(ROOT, "tests", "emu_fri_batch")
SENTINEL = np.uint64(0x5E5E5E5E5E5E5E5E)
u32p = ctypes.POINTER(ctypes.c_uint32)
ullp = ctypes.POINTER(ctypes.c_ulonglong)
ptrs_t = ctypes.POINTER(ctypes.c_void_p)


@pytest.fixture(scope="module")
def efb():
    subprocess.run(["make", "-s"], cwd=D, check=True)
    lib = ctypes.CDLL(os.path.join(D, "libglp_emu_fri_batch.so"))
    c32, c64 = ctypes.c_uint32, ctypes.c_uint64
    lib.emu_powers_eval_batch.restype = ctypes.c_long
    lib.emu_powers_eval_batch.argtypes = [ptrs_t, c32, u32p, u32p, c32, c32, c32, u64p, u64p, u64p]
    lib.emu_powers_eval_single.argtypes = [u64p, c32, c32, u64p, u64p, u64p]
    lib.emu_combine_batch.argtypes = [ptrs_t, c32, c32, u32p, u32p, c32, c32, c32, u64p, c64, ctypes.c_int, u64p, c64]
    lib.emu_combine_single.argtypes = [ptrs_t, c32, u32p, u32p, c32, c32, u64p, c64, u64p]
    lib.emu_fold_layer_batch.argtypes = [u64p, c64, u64p, c64, c32, c32, c64, u64p, c32]
    lib.emu_fold2_chain.argtypes = [u64p, u64p, c32, c32, c64, u64p]
    lib.emu_pow_batch.argtypes = [u64p, u32p, c32, c64, c64, c32, ullp, u64p, ctypes.c_int]
    lib.emu_pow_single.argtypes = [u64p, c64, c64, c32, ullp, u64p, ctypes.c_int]
    lib.emu_gather_multi.argtypes = [ptrs_t, u64p, c64, u64p]
    lib.emu_gather_single.argtypes = [u64p, u64p, c64, u64p]
    return lib


def p32(a):
    return a.ctypes.data_as(u32p)


def host_ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


@pytest.mark.parametrize("log_n", [3, 8, 13])
def test_powers_and_openings(efb, log_n):
    """two batches (2 and 1 polynomials; masks 1 and 3), two points, B = 2: a partial chunk (2^3, 2^8), then more than one chunk (2^13)"""
    B, NP = 2, 2
    n_polys, masks = np.array([2, 1], dtype=np.uint32), np.array([1, 3], dtype=np.uint32)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    coeffs = [rand_field(rng, (int(n_polys[b]), n)) for _ in range(B) for b in range(2)]
    z = rand_field(rng, (B, NP, 2))
    n_chunks = (n + 4095) // 4096
    total = 2 + 1 + 1
    zp = np.zeros((B, NP, n, 2), dtype=np.uint64)
    part = np.zeros((B, total * n_chunks, 2), dtype=np.uint64)
    assert efb.emu_powers_eval_batch(host_ptrs(coeffs), log_n, p32(n_polys), p32(masks), 2, NP, B, ptr(z), ptr(zp), ptr(part)) == total * n_chunks
    for i in range(B):
        k = 0
        for p in range(NP):
            for b in range(2):
                if not (int(masks[b]) >> p) & 1:
                    continue
                zp1 = np.zeros((n, 2), dtype=np.uint64)
                part1 = np.zeros((int(n_polys[b]) * n_chunks, 2), dtype=np.uint64)
                efb.emu_powers_eval_single(ptr(coeffs[i * 2 + b]), log_n, int(n_polys[b]), ptr(np.ascontiguousarray(z[i, p])), ptr(zp1), ptr(part1))
                assert np.array_equal(zp[i, p], zp1), (i, p)
                assert np.array_equal(part[i, k:k + len(part1)], part1), (i, p, b)
                k += len(part1)
        assert k == total * n_chunks


@pytest.mark.parametrize("log_N", [6, 13])
def test_combine(efb, log_N):
    """2 points, 3 batches, masks 1, 3, 1, against the existing sequence of glp_fri_combine_kernel launches plus the addition; both load
    widths; the gap between the instances' codewords is left alone"""
    B, NP, rb = 2, 2, 1
    n_polys, masks = np.array([3, 2, 1], dtype=np.uint32), np.array([1, 3, 1], dtype=np.uint32)
    total = 3 + 2 + 1 + 2
    N = 1 << log_N
    rng = np.random.default_rng(40 + log_N)
    ldes = [rand_field(rng, (int(n_polys[b]), N)) for _ in range(B) for b in range(3)]
    cmb = rand_field(rng, (B, 4 * NP + 2 * total))                   # Y, z, alpha powers: any canonical words
    stride = 2 * N + 6
    ref = np.zeros((B, N, 2), dtype=np.uint64)
    for i in range(B):
        assert efb.emu_combine_single(host_ptrs(ldes[3 * i:3 * i + 3]), log_N, p32(n_polys), p32(masks), 3, NP, ptr(np.ascontiguousarray(cmb[i])), 7,
                                      ptr(ref[i])) == 0
    for v16 in (1, 0):
        out = np.full((B, stride), SENTINEL, dtype=np.uint64)
        assert efb.emu_combine_batch(host_ptrs(ldes), log_N - rb, rb, p32(n_polys), p32(masks), 3, NP, B, ptr(cmb), 7, v16, ptr(out), stride) == 0
        for i in range(B):
            assert np.array_equal(out[i, :2 * N].reshape(N, 2), ref[i]), (v16, i)
            assert np.all(out[i, 2 * N:] == SENTINEL), (v16, i)


@pytest.mark.parametrize("log_len,a", [(1, 1), (4, 4), (5, 5), (7, 3), (12, 4), (13, 4), (14, 2)])
@pytest.mark.parametrize("B", [1, 3])
def test_fold_layer(efb, log_len, a, B):
    """one launch against arity_bits successive glp_fri_fold2_kernel launches; strides larger than dense, the gaps left alone"""
    rng = np.random.default_rng(100 * log_len + 10 * a + B)
    in_words, out_words = 2 << log_len, (2 << log_len) >> a
    in_stride, out_stride = in_words + 6, out_words + 4
    src = rand_field(rng, (B, in_stride))
    betas = rand_field(rng, (B, 2))
    out = np.full((B, out_stride), SENTINEL, dtype=np.uint64)
    assert efb.emu_fold_layer_batch(ptr(src), in_stride, ptr(out), out_stride, log_len, a, 7, ptr(betas), B) == 0
    for b in range(B):
        want = np.zeros(out_words, dtype=np.uint64)
        efb.emu_fold2_chain(ptr(np.ascontiguousarray(src[b, :in_words])), ptr(want), log_len, a, 7, ptr(np.ascontiguousarray(betas[b])))
        assert np.array_equal(out[b, :out_words], want), b
        assert np.all(out[b, out_words:] == SENTINEL), b
    # the product's argument rule (glp_fri_fold_layer_batch_check) is the emulation's too
    assert efb.emu_fold_layer_batch(ptr(src), in_words - 2, ptr(out), out_stride, log_len, a, 7, ptr(betas), B) == -1
    assert efb.emu_fold_layer_batch(ptr(src), in_stride, ptr(out), out_words + 1, log_len, a, 7, ptr(betas), B) == -1


@pytest.mark.parametrize("small", [2, 0])
def test_pow_windows(efb, small):
    """two seeds at 6 bits, a window of 512 nonces cut into two halves: both instances search the first half; the second half is searched
    by instance 1 alone, and instance 0's word must stay as the first half left it"""
    rc, circ, diag = poseidon_consts("small" if small else "big")
    c384 = np.concatenate([rc, circ, diag]).astype(np.uint64)
    seeds = rand_field(np.random.default_rng(6), (2, 4))
    found = np.full(2, 2**64 - 1, dtype=np.uint64)
    both, one = np.array([0, 1], dtype=np.uint32), np.array([1], dtype=np.uint32)
    efb.emu_pow_batch(ptr(seeds), p32(both), 2, 0, 256, 6, found.ctypes.data_as(ullp), ptr(c384), small)
    ref = []
    for i in range(2):
        r = ctypes.c_ulonglong(2**64 - 1)
        efb.emu_pow_single(ptr(np.ascontiguousarray(seeds[i])), 0, 256, 6, ctypes.byref(r), ptr(c384), small)
        ref.append(r.value)
    assert [int(v) for v in found] == ref
    assert any(v < 256 for v in ref)                                  # at 6 bits a half of 256 nonces finds one for at least one seed
    keep0 = int(found[0])
    found[1] = np.uint64(2**64 - 1)                                   # instance 1 is made to search on, instance 0 is not listed
    efb.emu_pow_batch(ptr(seeds), p32(one), 1, 256, 200, 6, found.ctypes.data_as(ullp), ptr(c384), small)
    r = ctypes.c_ulonglong(2**64 - 1)
    efb.emu_pow_single(ptr(np.ascontiguousarray(seeds[1])), 256, 200, 6, ctypes.byref(r), ptr(c384), small)
    assert int(found[1]) == r.value and (256 <= r.value < 456 or r.value == 2**64 - 1)
    assert int(found[0]) == keep0


def test_gather_multi(efb):
    rng = np.random.default_rng(3)
    srcs = [rand_field(rng, k) for k in (100, 37, 1000)]
    n = 700
    pairs = np.zeros((n, 2), dtype=np.uint64)
    pairs[:, 0] = rng.integers(0, 3, n)
    pairs[:, 1] = [rng.integers(0, len(srcs[int(s)])) for s in pairs[:, 0]]
    out = np.zeros(n, dtype=np.uint64)
    efb.emu_gather_multi(host_ptrs(srcs), ptr(pairs), n, ptr(out))
    assert np.array_equal(out, np.array([srcs[int(s)][int(o)] for s, o in pairs], dtype=np.uint64))
    # one source: the existing glp_gather_kernel
    sel = np.ascontiguousarray(pairs[pairs[:, 0] == 2][:, 1])
    one = np.zeros(len(sel), dtype=np.uint64)
    efb.emu_gather_single(ptr(srcs[2]), ptr(sel), len(sel), ptr(one))
    assert np.array_equal(one, out[pairs[:, 0] == 2])


def hand_plan(log_n, fb, a, rb, cap, pow_bits, merkle_plan):
    """(launches, synchronises) from the header comment of glp_fri_prove_batch alone"""
    L = (log_n - fb) // a if log_n > fb else 0
    launches, syncs = 3 + (1 if pow_bits else 0) + 1, 1 + L + 1 + (1 if pow_bits else 0) + 1
    log_len = log_n + rb
    for _ in range(L):
        log_leaves = log_len - a
        launches += merkle_plan(log_leaves, min(cap, log_leaves))[0] + 1
        log_len -= a
    return launches, syncs


# (log_n, rate, cap, arity, final, pow): (launches, synchronises), written down by hand.  Tree launches (glp_merkle_batch, default fusion)
# are 1 leaf launch + 1 fused launch for a tree with at most 9 levels above its leaves, one more fused launch beyond that.
PLANS = {
    (10, 3, 4, 4, 5, 8): (3 + (2 + 1) + 1 + 1, 1 + 1 + 1 + 1 + 1),                  # one layer: 2^9 leaves
    (12, 3, 4, 4, 5, 10): (3 + (2 + 1) + 1 + 1, 5),                                 # one layer: 2^11 leaves
    (9, 1, 2, 2, 3, 4): (3 + 3 * (2 + 1) + 1 + 1, 1 + 3 + 1 + 1 + 1),               # three layers: 2^8, 2^6, 2^4 leaves
    (6, 2, 0, 1, 2, 0): (3 + 4 * (2 + 1) + 0 + 1, 1 + 4 + 1 + 0 + 1),               # four layers of arity 2, no PoW
    (5, 3, 8, 4, 5, 6): (3 + 0 + 1 + 1, 1 + 0 + 1 + 1 + 1),                         # no layer
    (14, 3, 4, 4, 5, 16): (3 + 2 * (2 + 1) + 1 + 1, 1 + 2 + 1 + 1 + 1),             # two layers: 2^13 and 2^9 leaves
    (16, 3, 4, 4, 5, 16): (3 + (3 + 1) + (2 + 1) + 1 + 1, 6),                       # the signature leaf: 2^15 leaves (11 levels: 9 + 2 fused) and 2^11
}


def test_plan_counts(pkg):
    lib = pkg.load_library()
    for (log_n, rb, cap, a, fb, pw), want in PLANS.items():
        for masks, mults in (([1], (1,)), ([1, 1, 3, 1], (1, 5))):     # the counts do not depend on the batches or the points
            got = pkg.Prover.fri_prove_batch_plan(log_n, rb, cap, masks, arity_bits=a, final_poly_bits=fb, pow_bits=pw, point_mults=mults)
            assert got == want, (log_n, masks)
        assert hand_plan(log_n, fb, a, rb, cap, pw, pkg.Prover.merkle_batch_plan) == want
    cfg = pkg.Prover._fri_config(12, 3, 4, 4, 5, 28, 16, pkg.COSET_SHIFT, (1,))
    m = np.array([1], dtype=np.uint32)
    n = ctypes.c_uint32()
    assert lib.glp_fri_prove_batch_plan(ctypes.byref(cfg), m.ctypes.data, 1, ctypes.byref(n), None) == 0
    for bad in ([2], [0], [3]):                                        # a point that does not exist / no point / both
        mm = np.array(bad, dtype=np.uint32)
        assert lib.glp_fri_prove_batch_plan(ctypes.byref(cfg), mm.ctypes.data, 1, ctypes.byref(n), None) == -1
    assert lib.glp_fri_prove_batch_plan(ctypes.byref(cfg), m.ctypes.data, 0, ctypes.byref(n), None) == -1
    assert lib.glp_fri_prove_batch_plan(ctypes.byref(pkg.Prover._fri_config(12, 3, 4, 6, 5, 28, 16, 7, (1,))), m.ctypes.data, 1, None, None) == -1
    assert lib.glp_fri_prove_batch_plan(ctypes.byref(pkg.Prover._fri_config(20, 3, 4, 4, 19, 28, 16, 7, (1,))), m.ctypes.data, 1, None, None) == -5


def test_sanitized_standalone_program():
    """the same source as an ordinary executable under AddressSanitizer + UBSan: every batched body against the single one, word for word"""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    r = subprocess.run([os.path.join(D, "emu_fri_batch_san")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
