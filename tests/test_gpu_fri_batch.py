"""glp_fri_prove_batch on the GPU: B opening proofs of one shape in one call are, byte for byte, the B proofs glp_fri_prove writes one at a
time (the unchanged single-proof path is the reference), both verifiers accept them, the launch / synchronise counts are the planned ones
whatever B is, and a faulty instance fails the whole call by name.  Every instance holds independent random data, so a wrong instance
offset cannot pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_verifier as fv  # noqa: E402
from conftest import P, poseidon_consts, ptr, rand_field, root_of_unity  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0x5E5E5E5E5E5E5E5E)


@pytest.fixture()
def setup(prover, oracle):
    rc, circ, diag = poseidon_consts("small")
    prover.set_poseidon_constants(rc, circ, diag)
    oracle.orc_poseidon_set_constants(ptr(rc), ptr(circ), ptr(diag))
    return prover, oracle


# log_n, n_polys per batch, open_masks, second point (None or "w_n"), rate, cap, arity, final, queries, pow, B, how each batch is committed:
# "shared" = ONE from_values object used by every instance, "views" = from_values_batch views, "own" = one from_values object per instance
ROWS = [
    (10, [5], [1], None, 3, 4, 4, 5, 10, 8, 3, ["views"]),                                         # plain case, one layer
    (12, [7, 2, 3, 4], [1, 1, 3, 1], "w_n", 3, 4, 4, 5, 12, 10, 4, ["shared", "views", "views", "own"]),   # the PLONK driver's shape
    (9, [1], [1], None, 1, 2, 2, 3, 8, 4, 2, ["views"]),                                           # arity 2, three layers, rate 1/2
    (6, [3], [1], None, 2, 0, 1, 2, 6, 0, 5, ["own"]),                                             # arity 1, cap 0, no PoW
    (5, [2], [1], None, 3, 8, 4, 5, 5, 6, 2, ["views"]),                                           # no fold layer, cap clamped to the tree
    (14, [20, 4, 8], [1, 1, 1], None, 3, 4, 4, 5, 28, 16, 2, ["views", "own", "views"]),           # log_N = 17: the root table's upper half
    (10, [5], [1], None, 3, 4, 4, 5, 10, 8, 1, ["own"]),                                           # B = 1
]


def make_instances(pkg, prover, rng, log_n, polys, rb, cap_h, B, kinds):
    """-> (instances [B][n_batches], everything to free)"""
    cols, owned = [], []
    for k, kind in zip(polys, kinds):
        if kind == "shared":
            pb = pkg.PolynomialBatch.from_values(prover, rand_field(rng, (k, 1 << log_n)), rb, cap_h)
            owned.append(pb)
            cols.append([pb] * B)
        elif kind == "views":
            views = pkg.PolynomialBatch.from_values_batch(prover, rand_field(rng, (B, k, 1 << log_n)), rb, cap_h)
            owned.append(views[0].slabs)
            cols.append(views)
        else:
            pbs = [pkg.PolynomialBatch.from_values(prover, rand_field(rng, (k, 1 << log_n)), rb, cap_h) for _ in range(B)]
            owned += pbs
            cols.append(pbs)
    return [[col[i] for col in cols] for i in range(B)], owned


def row_kwargs(row):
    log_n, polys, masks, pt, rb, cap_h, a, fb, nq, pw, B, kinds = row
    mults = (1,) if pt is None else (1, root_of_unity(log_n))
    return dict(arity_bits=a, final_poly_bits=fb, num_queries=nq, pow_bits=pw, point_mults=mults, open_masks=masks)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"2p{r[0]}x{'+'.join(map(str, r[1]))}_B{r[10]}")
def test_batch_equals_sequential(setup, pkg, oracle, row):
    prover, _ = setup
    log_n, polys, masks, pt, rb, cap_h, a, fb, nq, pw, B, kinds = row
    rng = np.random.default_rng(1000 * log_n + 10 * len(polys) + B)
    instances, owned = make_instances(pkg, prover, rng, log_n, polys, rb, cap_h, B, kinds)
    kw = row_kwargs(row)
    ref = [prover.fri_prove(inst, rb, cap_h, **kw) for inst in instances]         # the unchanged single-proof path
    assert len(set(ref)) == B                                                      # independent data: B different proofs
    got = prover.fri_prove_batch(instances, rb, cap_h, **kw)
    assert len(got) == B
    for i in range(B):
        assert got[i] == ref[i], f"instance {i} differs from glp_fri_prove"
        info = fv.parse_and_verify(got[i], oracle)
        assert info["n_polys"] == polys and len(info["queries"]) == nq
        assert prover.fri_verify(got[i], min_queries=nq, min_pow_bits=pw, min_rate_bits=rb), prover.last_reject
    assert prover.fri_prove_batch(instances, rb, cap_h, **kw) == got              # a second call: the same bytes
    for o in owned:
        o.free()


def test_pow_grind_batch_across_windows(setup):
    """three seeds at 22 bits (one window = 2^22 nonces): with the package's default constants the single-seed search finds 5778092,
    5371340 and 3494516 (brute force on the CPU), i.e. windows 1, 1, 0 — the instance that finishes in window 0 must sit window 1 out
    and the others must keep the smallest nonce of window 1.  (The issue quotes other nonces, which the default constants do not accept; the
    property it asks for — at least two windows — holds and is asserted on the reference values alone.)
    The window count is checked through the direct entry point only: the seeds of a proof call come out of its transcript and cannot be
    chosen, so a proof with exactly these seeds cannot be arranged."""
    prover, _ = setup
    seeds = rand_field(np.random.default_rng(2026), (3, 4))
    ref = [prover.pow_grind(seeds[i], 22) for i in range(3)]
    assert len({n >> 22 for n in ref}) >= 2, ref
    assert prover.pow_grind_batch(seeds, 22) == ref
    assert prover.pow_grind_batch(seeds[:1], 22) == ref[:1]
    assert prover.pow_grind_batch(seeds, 0) == [0, 0, 0]
    assert prover.pow_grind_batch(np.zeros((0, 4), dtype=np.uint64), 22) == []


def test_generic_mds_and_unaligned_lde(prover, pkg, oracle):
    """the two instantiations the small-constant cases never launch: glp_pow_batch_kernel<false> (an MDS the fast path does not admit) and
    glp_fri_combine_batch_kernel<false> (an LDE that is only 8-byte aligned: 8-byte row loads)"""
    rc, circ, diag = poseidon_consts("big")
    prover.set_poseidon_constants(rc, circ, diag)
    seeds = rand_field(np.random.default_rng(9), (3, 4))
    assert prover.pow_grind_batch(seeds, 10) == [prover.pow_grind(s, 10) for s in seeds]
    log_n, rb, cap_h = 7, 2, 1
    rng = np.random.default_rng(10)
    pbs = [pkg.PolynomialBatch.from_values(prover, rand_field(rng, (3, 1 << log_n)), rb, cap_h) for _ in range(2)]
    kw = dict(arity_bits=2, final_poly_bits=3, num_queries=5, pow_bits=3)
    ref = [prover.fri_prove([pb], rb, cap_h, **kw) for pb in pbs]
    assert prover.fri_prove_batch([[pb] for pb in pbs], rb, cap_h, **kw) == ref
    # instance 1's LDE moved one word off its 16-byte alignment
    lde = pbs[1].lde.download((3, 1 << (log_n + rb)))
    moved = prover.to_device(np.concatenate([np.zeros(1, dtype=np.uint64), lde.reshape(-1)]))
    odd = pkg.PolynomialBatch(prover, 3, log_n, rb, cap_h)
    odd.coeffs, odd.lde, odd.digests, odd.cap = pbs[1].coeffs, moved.ptr + 8, pbs[1].digests, pbs[1].cap
    assert prover.fri_prove_batch([[pbs[0]], [odd]], rb, cap_h, **kw) == ref
    moved.free()
    odd.coeffs = odd.digests = None
    for pb in pbs:
        pb.free()
    rc, circ, diag = poseidon_consts("small")
    prover.set_poseidon_constants(rc, circ, diag)


def fold_chain(prover, evals, a, shift, beta):
    """arity_bits successive glp_fri_fold2 calls with beta, beta^2, .. and shift, shift^2, .. (the sequential prover's loop)"""
    cur, b = evals, (int(beta[0]), int(beta[1]))
    for _ in range(a):
        cur = prover.fri_fold2(cur, shift, np.array(b, dtype=np.uint64))
        b = fv.emul(b, b)
        shift = shift * shift % P
    return cur


# (17, 4) is added to the issue's shapes: the layer kernel reads the inverse table at w^-rev(j), j < 2^(log_len - arity), so ITS first read
# of the table's upper half is at log_len - arity = 13
FOLD_SHAPES = [(1, 1), (4, 4), (5, 5), (7, 3), (12, 4), (13, 4), (14, 2)]


@pytest.mark.parametrize("log_len,a,B", [(ll, a, B) for ll, a in FOLD_SHAPES for B in (1, 3)] + [(17, 4, 1)])
def test_fold_layer_batch(setup, pkg, log_len, a, B):
    prover, _ = setup
    rng = np.random.default_rng(100 * log_len + 10 * a + B)
    n = 1 << log_len
    in_words, out_words = 2 * n, 2 * n >> a
    in_stride, out_stride = in_words + 6, out_words + 4          # larger than dense, even
    src = rand_field(rng, (B, in_stride))
    betas = rand_field(rng, (B, 2))
    d_in = prover.to_device(src)
    d_out = prover.to_device(np.full((B, out_stride), SENTINEL, dtype=np.uint64))
    prover.fri_fold_layer_batch_(d_in, in_stride, d_out, out_stride, log_len, a, pkg.COSET_SHIFT, betas, B)
    got = d_out.download((B, out_stride))
    for b in range(B):
        want = fold_chain(prover, src[b, :in_words].reshape(n, 2), a, pkg.COSET_SHIFT, betas[b])
        assert np.array_equal(got[b, :out_words].reshape(-1, 2), want), b
        assert np.all(got[b, out_words:] == SENTINEL), b
    # the numpy helper (dense strides) gives the same words
    dense = prover.fri_fold_layer_batch(src[:, :in_words].reshape(B, n, 2), a, pkg.COSET_SHIFT, betas)
    assert np.array_equal(dense.reshape(B, -1), got[:, :out_words])
    d_in.free()
    d_out.free()


def test_fold_layer_batch_refusals(setup, pkg):
    prover, _ = setup
    d = prover.to_device(np.zeros(4096, dtype=np.uint64))
    o = prover.alloc(4096 * 8)
    beta = np.array([[1, 2]], dtype=np.uint64)
    prover.fri_fold_layer_batch_(d, 64, o, 8, 5, 3, 7, beta, 0)                  # B = 0: nothing to do
    for args in [(63, 8, 5, 3), (64, 7, 5, 3), (66, 9, 5, 3), (64, 8, 5, 6), (64, 8, 2, 3), (64, 8, 5, 0)]:
        with pytest.raises(pkg.GlpError, match="GLP_E_INVALID"):
            prover.fri_fold_layer_batch_(d, args[0], o, args[1], args[2], args[3], 7, beta, 1)
    with pytest.raises(pkg.GlpError, match="GLP_E_INVALID"):
        prover.fri_fold_layer_batch_(d.ptr + 8, 64, o, 8, 5, 3, 7, beta, 1)          # not 16-byte aligned
    with pytest.raises(pkg.GlpError, match="GLP_E_INVALID"):
        prover.fri_fold_layer_batch_(d, 64, o, 8, 5, 3, 7, np.array([[P, 0]], dtype=np.uint64), 1)
    d.free()
    o.free()


def test_counts_equal_the_plan_whatever_B(setup, pkg):
    """the PLONK driver's shape (second table row) at B = 1 and B = 4: what the driver counted is the plan plus one launch and one
    synchronise per PoW window after the first, and the same for both B"""
    prover, _ = setup
    row = ROWS[1]
    log_n, polys, masks, pt, rb, cap_h, a, fb, nq, pw, _, kinds = row
    kw = row_kwargs(row)
    plan = pkg.Prover.fri_prove_batch_plan(log_n, rb, cap_h, masks, arity_bits=a, final_poly_bits=fb, num_queries=nq, pow_bits=pw,
                                           point_mults=kw["point_mults"])
    # by hand from the header comment of glp_fri_prove_batch: L = (12 - 5) / 4 = 1 layer, whose tree has 2^(15 - 4) = 2^11 leaves and cap 4:
    # one leaf launch + one fused launch of the 7 levels above them (glp_merkle_batch at the default fusion) = 2
    hand_launches = 3 + (2 + 1) + 1 + 1
    hand_syncs = 1 + 1 + 1 + 1 + 1
    assert pkg.Prover.merkle_batch_plan(11, 4)[0] == 2
    assert plan == (hand_launches, hand_syncs)
    seen = []
    for B in (1, 4):
        rng = np.random.default_rng(77 + B)
        instances, owned = make_instances(pkg, prover, rng, log_n, polys, rb, cap_h, B, kinds)
        prover.fri_prove_batch(instances, rb, cap_h, **kw)
        launches, syncs, windows = prover.fri_last_batch_counts()
        assert windows >= 1
        assert (launches, syncs) == (plan[0] + windows - 1, plan[1] + windows - 1), B
        seen.append((launches - windows, syncs - windows))
        for o in owned:
            o.free()
    assert seen[0] == seen[1]
    # no PoW, no layer: the three opening launches and the gather
    assert pkg.Prover.fri_prove_batch_plan(5, 3, 8, [1], pow_bits=0) == (4, 3)
    with pytest.raises(pkg.GlpError):
        pkg.Prover.fri_prove_batch_plan(12, 3, 4, [1, 2], point_mults=(1,))          # a mask naming a point that does not exist


def test_refusals_are_all_or_nothing(setup, pkg, oracle):
    prover, _ = setup
    log_n, rb, cap_h = 8, 3, 2
    kw = dict(num_queries=8, pow_bits=4)
    rng = np.random.default_rng(5)
    mk = lambda k: pkg.PolynomialBatch.from_values(prover, rand_field(rng, (k, 1 << log_n)), rb, cap_h)  # noqa: E731
    a0, a1, a2, odd = mk(2), mk(2), mk(2), mk(3)
    assert prover.fri_prove_batch([], rb, cap_h, **kw) == []                     # B = 0
    with pytest.raises(pkg.GlpError, match="GLP_E_INVALID.*instance 1"):               # n_polys differs between instances
        prover.fri_prove_batch([[a0], [odd]], rb, cap_h, **kw)
    # open_mask differing between instances cannot be said through the Python wrapper (one mask list per call): straight through the ABI
    import ctypes
    cfg = pkg.Prover._fri_config(log_n, rb, cap_h, 4, 5, 8, 4, pkg.COSET_SHIFT, (1, root_of_unity(log_n)))
    arr = (pkg.FriBatch * 2)()
    for i, (b, m) in enumerate(((a0, 3), (a1, 1))):
        arr[i] = pkg.FriBatch(b.coeffs.ptr, b.lde.ptr, b.digests.ptr, b.cap.ctypes.data, b.n_polys, m)
    proofs, lens = (ctypes.c_void_p * 2)(), (ctypes.c_size_t * 2)()
    assert prover.lib.glp_fri_prove_batch(prover.ctx, ctypes.byref(cfg), arr, 1, 2, proofs, lens) == -1      # GLP_E_INVALID
    assert proofs[0] is None and proofs[1] is None
    assert b"instance 1" in prover.lib.glp_last_error(prover.ctx)
    # one instance whose LDE does not belong to its coefficients, made from two honest commitments
    chimera = pkg.PolynomialBatch(prover, 2, log_n, rb, cap_h)
    chimera.coeffs, chimera.lde, chimera.digests, chimera.cap = a1.coeffs, a2.lde, a2.digests, a2.cap
    for i, b in enumerate((a0, chimera)):
        arr[i] = pkg.FriBatch(b.coeffs.ptr, b.lde.ptr, b.digests.ptr, b.cap.ctypes.data, b.n_polys, 1)
    cfg1 = pkg.Prover._fri_config(log_n, rb, cap_h, 4, 5, 8, 4, pkg.COSET_SHIFT, (1,))
    proofs[0] = proofs[1] = 1                                                    # must be reset to NULL by the call
    assert prover.lib.glp_fri_prove_batch(prover.ctx, ctypes.byref(cfg1), arr, 1, 2, proofs, lens) != 0
    assert proofs[0] is None and proofs[1] is None                               # no proof is returned
    assert b"instance 1" in prover.lib.glp_last_error(prover.ctx)
    with pytest.raises(pkg.GlpError, match="instance 2"):
        prover.fri_prove_batch([[a0], [a1], [chimera], [a2]], rb, cap_h, **kw)
    # the next valid call on the same prover succeeds with the right bytes
    good = [[a0], [a1], [a2]]
    assert prover.fri_prove_batch(good, rb, cap_h, **kw) == [prover.fri_prove(g, rb, cap_h, **kw) for g in good]
    chimera.coeffs = chimera.lde = chimera.digests = None
    for b in (a0, a1, a2, odd):
        b.free()
