"""glp_merkle_batch / glp_commit_values_batch on the GPU: B trees per call against B calls of the existing single-tree path (itself
oracle-tested in test_gpu_hash.py), every digest word and every cap; PolynomialBatch.from_values_batch against from_values; the batched
views through fri_prove."""
import numpy as np
import pytest

from conftest import oracle_merkle, poseidon_consts, ptr, rand_field

pytestmark = pytest.mark.gpu


def use_consts(prover, oracle, kind):
    rc, circ, diag = poseidon_consts(kind)
    prover.set_poseidon_constants(rc, circ, diag)
    oracle.orc_poseidon_set_constants(ptr(rc), ptr(circ), ptr(diag))


_REF = {}


def reference(prover, B, leaf_len, log_leaves, cap_h, kind="small"):
    """(leaves, [(digests, cap) of merkle_tree per tree]), computed once per shape and constant kind and left unchanged"""
    key = (B, leaf_len, log_leaves, cap_h, kind)
    if key not in _REF:
        rng = np.random.default_rng(B * 1000 + leaf_len * 100 + log_leaves)
        leaves = rand_field(rng, (B, 1 << log_leaves, leaf_len))
        _REF[key] = (leaves, [prover.merkle_tree(leaves[b], cap_h) for b in range(B)])
    return _REF[key]


def check(prover, B, leaf_len, log_leaves, cap_h, fuse, kind="small"):
    leaves, refs = reference(prover, B, leaf_len, log_leaves, cap_h, kind)
    dig, caps = prover.merkle_trees(leaves, cap_h, fuse_max_log=fuse)
    assert dig.shape[0] == B and caps.shape == (B, 1 << cap_h, 4)
    for b in range(B):
        assert np.array_equal(dig[b], refs[b][0]), (fuse, b)
        assert np.array_equal(caps[b], refs[b][1]), (fuse, b)
        assert np.array_equal(dig[b][-(1 << cap_h):], caps[b]), (fuse, b)
    return leaves, dig, caps


SHAPES = [(3, 135, 12, 4), (5, 3, 8, 0), (2, 4, 5, 5), (2, 20, 16, 4)]


@pytest.mark.parametrize("B,leaf_len,log_leaves,cap_h", SHAPES)
def test_merkle_trees_match_single_trees(prover, oracle, pkg, B, leaf_len, log_leaves, cap_h):
    use_consts(prover, oracle, "small")
    leaves, dig, caps = check(prover, B, leaf_len, log_leaves, cap_h, None)
    # polynomial-major leaves give the same trees
    dig2, caps2 = prover.merkle_trees(np.ascontiguousarray(leaves.transpose(0, 2, 1)), cap_h, poly_major=True)
    assert np.array_equal(dig2, dig) and np.array_equal(caps2, caps)
    if (B, leaf_len, log_leaves, cap_h) == SHAPES[0]:
        for b in range(B):
            dig_ref, cap_ref = oracle_merkle(oracle, leaves[b], cap_h)
            assert np.array_equal(dig[b], dig_ref) and np.array_equal(caps[b], cap_ref), b
    if log_leaves > cap_h:
        assert pkg.Prover.merkle_batch_plan(log_leaves, cap_h)[1] >= 1          # the fused kernel really ran


@pytest.mark.parametrize("B,leaf_len,log_leaves,cap_h", [SHAPES[0], SHAPES[3]])
@pytest.mark.parametrize("fuse", ["never", "everything", "from_2p13"])
def test_merkle_trees_fusion_settings(prover, oracle, pkg, B, leaf_len, log_leaves, cap_h, fuse):
    use_consts(prover, oracle, "small")
    f = {"never": 0, "everything": log_leaves, "from_2p13": 13}[fuse]
    if (log_leaves, fuse) == (16, "from_2p13"):
        # unfused levels and two fused launches in one call: 2^15 and 2^14 nodes one launch each, then 9 levels, then the last one
        assert pkg.Prover.merkle_batch_plan(log_leaves, cap_h, f) == (5, 2)
    check(prover, B, leaf_len, log_leaves, cap_h, f)


@pytest.mark.parametrize("kind", ["medium", "big"])
def test_merkle_trees_other_constants(prover, oracle, kind):
    use_consts(prover, oracle, kind)
    try:
        check(prover, *SHAPES[0], None, kind=kind)
    finally:
        use_consts(prover, oracle, "small")


def test_strides_gaps_and_stream_ordered_caps(prover, oracle, pkg):
    """tree strides larger than a tree: the digest gap keeps its sentinel; h_caps = NULL leaves the call stream-ordered, and the caps read
    back after sync() equal the synchronous ones"""
    use_consts(prover, oracle, "small")
    B, leaf_len, log_leaves, cap_h = 3, 135, 12, 4
    leaves, refs = reference(prover, B, leaf_len, log_leaves, cap_h)
    n = 1 << log_leaves
    nd = pkg.Prover.merkle_digest_len(log_leaves, cap_h)
    sstride, dstride = n * leaf_len + 13, nd + 9
    src = np.zeros((B, sstride), dtype=np.uint64)
    src[:, :n * leaf_len] = leaves.reshape(B, -1)
    src[:, n * leaf_len:] = 12345
    sentinel = np.uint64(0x5E5E5E5E5E5E5E5E)
    d_src = prover.to_device(src)
    d_dig = prover.to_device(np.full((B, dstride), sentinel, dtype=np.uint64))
    caps = prover.merkle_batch_(d_src, sstride, leaf_len, log_leaves, cap_h, B, d_dig, digest_tree_stride=dstride)
    got = d_dig.download((B, dstride))
    for b in range(B):
        assert np.array_equal(got[b, :nd].reshape(-1, 4), refs[b][0]) and np.array_equal(caps[b], refs[b][1]), b
        assert np.all(got[b, nd:] == sentinel), b
    d_dig.upload(np.full((B, dstride), sentinel, dtype=np.uint64))
    assert prover.merkle_batch_(d_src, sstride, leaf_len, log_leaves, cap_h, B, d_dig, digest_tree_stride=dstride, want_caps=False) is None
    prover.sync()
    again = d_dig.download((B, dstride))
    assert np.array_equal(again, got)
    assert np.array_equal(again[:, nd - (4 << cap_h):nd].reshape(B, 1 << cap_h, 4), caps)
    d_src.free()
    d_dig.free()


def test_argument_refusals(prover, oracle, pkg):
    use_consts(prover, oracle, "small")
    lib = prover.lib
    log_leaves, cap_h, leaf_len, B = 3, 0, 5, 2
    nd = pkg.Prover.merkle_digest_len(log_leaves, cap_h)
    d_src = prover.to_device(np.zeros(4096, dtype=np.uint64))
    d_dig = prover.to_device(np.full(4096, 7, dtype=np.uint64))

    def call(src_stride, pm, pstride, ll, lg, ch, dstride, b=B, src=d_src.ptr, dig=d_dig.ptr):
        return lib.glp_merkle_batch(prover.ctx, src, src_stride, pm, pstride, ll, lg, ch, b, 0, dig, dstride, None)

    assert call(8 * 5, 0, 0, leaf_len, log_leaves, cap_h, nd) == 0
    assert call(8 * 5, 0, 0, leaf_len, log_leaves, cap_h, nd - 1) == -1          # digest_tree_stride short
    assert b"digest_tree_stride" in lib.glp_last_error(prover.ctx)
    assert call(8 * 5 - 1, 0, 0, leaf_len, log_leaves, cap_h, nd) == -1          # src_tree_stride short
    assert call(4 * 9 + 8, 1, 9, leaf_len, log_leaves, cap_h, nd) == 0           # the last polynomial row needs only its first 8 words
    assert call(4 * 9 + 7, 1, 9, leaf_len, log_leaves, cap_h, nd) == -1
    assert call(64, 1, 7, leaf_len, log_leaves, cap_h, nd) == -1                 # poly_stride < leaves
    assert call(64, 0, 0, leaf_len, log_leaves, 4, nd) == -1                     # cap_h > log_leaves
    assert call(64, 0, 0, 0, log_leaves, cap_h, nd) == -1                        # leaf_len == 0
    assert call(64, 0, 0, leaf_len, log_leaves, cap_h, nd, src=None) == -1
    assert call(2**64 - 1, 1, 1 << 63, leaf_len, log_leaves, cap_h, nd) == -1    # 4 rows of 2^63 words: the footprint does not fit 64 bits
    assert call(1 << 40, 0, 0, leaf_len, 31, 0, 1 << 40, b=1 << 31) == -5            # 2^23 leaf workgroups per tree x 2^31 trees: grid too large
    assert b"workgroups" in lib.glp_last_error(prover.ctx)
    prover.sync()
    before = d_dig.download((4096,))
    assert call(0, 0, 0, 0, 99, 0, 0, b=0, src=None, dig=None) == 0              # B == 0 does nothing at all
    prover.sync()
    assert np.array_equal(d_dig.download((4096,)), before)
    # without constants: GLP_E_STATE
    pr = pkg.Prover(0)
    d = pr.alloc(8 * 4096)
    assert pr.lib.glp_merkle_batch(pr.ctx, d.ptr, 40, 0, 0, leaf_len, log_leaves, cap_h, B, 0, d.ptr, nd, None) == -6
    pr.close()
    d_src.free()
    d_dig.free()


def test_from_values_batch_matches_from_values(prover, oracle, pkg):
    use_consts(prover, oracle, "small")
    B, n_polys, log_n, rate_bits, cap_h = 3, 5, 6, 3, 2
    vals = rand_field(np.random.default_rng(9), (B, n_polys, 1 << log_n))
    views = pkg.PolynomialBatch.from_values_batch(prover, vals, rate_bits, cap_h)
    assert len(views) == B
    N = 1 << (log_n + rate_bits)
    nd = pkg.Prover.merkle_digest_len(log_n + rate_bits, cap_h)
    slabs = views[0].slabs
    coeffs = slabs.coeffs.download((B, n_polys, 1 << log_n))
    lde = slabs.lde.download((B, n_polys, N))
    dig = slabs.digests.download((B, nd))
    for b in range(B):
        pb = pkg.PolynomialBatch.from_values(prover, vals[b], rate_bits, cap_h)
        assert views[b].coeffs == slabs.coeffs.ptr + b * n_polys * (8 << log_n) and views[b].slabs is slabs
        assert np.array_equal(coeffs[b], pb.coeffs.download((n_polys, 1 << log_n))), b
        assert np.array_equal(lde[b], pb.lde.download((n_polys, N))), b
        assert np.array_equal(dig[b], pb.digests.download((nd,))), b
        assert np.array_equal(views[b].cap, pb.cap), b
        pb.free()
    views[1].free()                                                     # a view owns nothing: the slabs stay
    assert np.array_equal(slabs.lde.download((B, n_polys, N)), lde)
    slabs.free()
    assert slabs.lde is None


def test_fri_prove_over_batched_views(prover, oracle, pkg):
    use_consts(prover, oracle, "small")
    n_polys, log_n, rate_bits, cap_h = 4, 8, 3, 2
    vals = rand_field(np.random.default_rng(10), (2, n_polys, 1 << log_n))
    views = pkg.PolynomialBatch.from_values_batch(prover, vals, rate_bits, cap_h)
    singles = [pkg.PolynomialBatch.from_values(prover, vals[b], rate_bits, cap_h) for b in range(2)]
    kw = dict(arity_bits=2, final_poly_bits=3, num_queries=8, pow_bits=6)
    proof = prover.fri_prove(views, rate_bits, cap_h, **kw)
    assert proof == prover.fri_prove(singles, rate_bits, cap_h, **kw)
    assert prover.fri_verify(proof, 8, 6), prover.last_reject
    for pb in singles:
        pb.free()
    views[0].slabs.free()
