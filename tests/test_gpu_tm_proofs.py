"""glp_tm_forest_create / glp_tm_forest_proofs / glp_tm_verify_inclusion_batch on the device, through the C ABI, at the cases of
tests/tm_proof_cases.py (the ones tests/test_emu_tm_proofs.py runs on the CPU) against the RECURSIVE hashlib reference: roots, aunts, counts and
leaf hashes; the launch and synchronise counts at 8, 512, 1025 and 4096 leaves; refused calls that write nothing and make no handle; the
negative matrix of the verifier; 4096 DataRootTuples through blobstream.data_root_inclusion_proofs; one small prove_range(..., inclusion=True);
header_field_proofs of the data hash of 8 headers."""
import ctypes
import importlib
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_inputs_cases as cic  # noqa: E402
import tm_proof_cases as cases  # noqa: E402
from conftest import poseidon_consts  # noqa: E402
import __graft_entry__ as graft  # noqa: E402


@pytest.mark.gpu
def test_forests_and_paths_on_the_device(prover):
    for c in cases.proof_cases():
        forest = prover.tm_forest(c.trees)
        try:
            biggest = max((len(t) for t in c.trees), default=0)
            want_launches = (1 if c.call.total else 0) + (max(0, (biggest - 1).bit_length() - 9) if biggest > 1 else 0) + 1
            assert forest.create_counts == (want_launches if c.trees else 0, 0), c.name
            assert forest.roots() == c.roots, c.name
            assert forest.info()[:3] == (c.call.B, c.call.total, (biggest - 1).bit_length() if biggest > 1 else 0), c.name
            stride = c.max_aunts + 2                           # two slots more than any row needs: they come back zero
            aunts, na, lh = forest.proofs_arrays(c.queries, aunt_stride=stride)
            assert forest.proofs_counts == ((1, 0) if c.queries else (0, 0)), c.name
            assert na.tolist() == [len(a) for a in c.aunts], c.name
            assert np.array_equal(aunts, c.aunts_array(stride)), c.name
            assert [lh[q].tobytes() for q in range(len(c.queries))] == c.leaf_hashes, c.name
            if c.name in ("B1-n5", "B65", "B4-wide"):          # every leaf in numbering order: both query arrays NULL
                flat = [(t, i) for t, leaves in enumerate(c.trees) for i in range(len(leaves))]
                proofs = forest.proofs()
                assert len(proofs) == len(flat)
                for q, (t, i) in enumerate(flat):
                    assert proofs[q] == (len(c.trees[t]), i, cases.leaf_hash(c.trees[t][i]), c.refs[t].path(i)), (c.name, q)
        finally:
            forest.free()


@pytest.mark.gpu
def test_counts_at_the_stated_sizes(prover):
    for name, launches in (("B1-n8", 2), ("B1-n512", 2), ("big-n1025", 4), ("big-n4096", 5)):
        c = cases.case(name)
        forest = prover.tm_forest(c.trees)
        assert forest.create_counts == (launches, 0), name
        forest.free()
        forest = prover.tm_forest(c.trees, roots=True)         # host roots: one copy, one synchronise
        assert forest.create_counts == (launches, 1) and forest.roots() == c.roots, name
        forest.free()
    c = cases.case("big-n4096")
    forest = prover.tm_forest(c.trees)
    try:
        proofs = forest.proofs([(0, 77)])
        assert forest.proofs_counts == (1, 0) and proofs[0][3] == c.refs[0].path(77)
        every = forest.proofs()
        assert forest.proofs_counts == (1, 0) and len(every) == 4096
        leaves = c.trees[0]
        for n in (1, 4096):
            status = prover.tm_verify_inclusion_batch(forest.roots(), every[:n], leaves[:n])
            assert prover.tm_forest_last_counts() == (1, 1) and not status.any(), n
        for i in (0, 1, 2047, 2048, 4095):
            assert list(every[i][3]) == c.refs[0].path(i) and cases.hash_from_aunts(i, 4096, every[i][2], every[i][3]) == c.roots[0]
    finally:
        forest.free()


@pytest.mark.gpu
def test_refused_calls_write_nothing_and_make_no_handle(prover):
    lib = prover.lib
    data = prover.to_device(np.ones(16, dtype=np.uint8))
    for name, data_len, offs, first, total, B, want in cic.refused_tree_calls():
        h = ctypes.c_void_p()
        h_roots = np.full((B, 32), cases.SENTINEL, dtype=np.uint8)
        rc = lib.glp_tm_forest_create(prover.ctx, data.ptr, data_len, offs.ctypes.data, first.ctypes.data, total, B, h_roots.ctypes.data, ctypes.byref(h))
        if name == "a tree over the maximum":                  # 513 leaves of no bytes: refused by the 512-leaf call, built here
            assert rc == 0 and h.value and h_roots[0].tobytes() == cic.tm_root([b""] * total)
            assert prover.tm_forest_last_counts() == (3, 1)
            lib.glp_tm_forest_destroy(h)
        else:
            assert rc == want == -1 and not h.value and np.all(h_roots == cases.SENTINEL), name
            assert prover.tm_forest_last_counts() == (0, 0), name
    data.free()
    # queries: a leaf equal to the tree's count, a tree equal to n_trees, a stride too small — nothing is launched, nothing written
    forest = prover.tm_forest([[b"a"], [b"b", b"c"]])
    d_aunts, d_na = prover.to_device(np.full(4 * 4 * 32, cases.SENTINEL, dtype=np.uint8)), prover.to_device(np.full(4, 0xEEEEEEEE, dtype=np.uint32))
    u = lambda *v: np.array(v, dtype=np.uint64)
    for what, qt, ql, nq, stride in (("leaf == count", u(0, 1), u(0, 2), 2, 4), ("tree == n_trees", u(1, 2), u(0, 0), 2, 4),
                                     ("stride too small", u(0, 1), u(0, 1), 2, 0), ("not total_leaves queries", None, None, 2, 4)):
        rc = lib.glp_tm_forest_proofs(prover.ctx, forest.handle, None if qt is None else qt.ctypes.data, None if ql is None else ql.ctypes.data, nq,
                                      d_aunts.ptr, stride, d_na.ptr, None)
        assert rc == -1 and prover.tm_forest_last_counts() == (0, 0), what
    assert np.all(d_aunts.download(4 * 4 * 32, dtype=np.uint8) == cases.SENTINEL) and np.all(d_na.download(4, dtype=np.uint32) == 0xEEEEEEEE)
    forest.free()
    d_aunts.free()
    d_na.free()
    empty = prover.tm_forest([])                               # n_trees == 0: GLP_OK, no launch, no query admitted
    assert empty.create_counts == (0, 0) and empty.roots() == [] and empty.proofs() == []
    empty.free()
    assert prover.tm_verify_inclusion_batch([], [], []).size == 0


@pytest.mark.gpu
def test_verifier_statuses_on_the_device(pkg, prover):
    m = cases.negative_matrix()
    status = prover.tm_verify_inclusion_arrays(m.roots, m.leaves, m.index, m.total, m.aunts, m.n_aunts, m.root_of)
    assert prover.tm_forest_last_counts() == (1, 1)
    bad = [(p, m.kind[p], int(status[p]), m.want[p]) for p in range(m.n) if status[p] != m.want[p]]
    assert not bad, bad[:8]
    # unsound host arrays: refused before the launch
    with pytest.raises(pkg.GlpError, match="names no root"):
        prover.tm_verify_inclusion_arrays(m.roots, m.leaves[:2], m.index[:2], m.total[:2], m.aunts[:2], m.n_aunts[:2], [0, len(m.roots)])
    assert prover.tm_forest_last_counts() == (0, 0)


@pytest.mark.gpu
def test_data_root_inclusion_proofs_of_4096_tuples(prover):
    bs = cic.bs
    rng = random.Random(4096)
    heights = [3_000_000 + k for k in range(4096)]
    data_roots = [rng.randbytes(32) for _ in heights]
    commitment, proofs = bs.data_root_inclusion_proofs(prover, heights, data_roots)
    assert commitment == bs.data_commitment(prover, heights, data_roots) and len(proofs) == 4096
    assert not bs.verify_data_root_inclusions(prover, commitment, heights, data_roots, proofs).any()
    for k, p in enumerate(proofs):
        leaf = bs.encode_data_root_tuple(heights[k], data_roots[k])
        assert (p.total, p.index, p.leaf_hash, len(p.aunts)) == (4096, k, cases.leaf_hash(leaf), 12)
        assert cases.hash_from_aunts(p.index, p.total, p.leaf_hash, list(p.aunts)) == commitment, k
    _, some = bs.data_root_inclusion_proofs(prover, heights, data_roots, indices=[5, 4095])
    assert some == [proofs[5], proofs[4095]]
    assert bs.verify_data_root_inclusion(prover, commitment, heights[5], data_roots[5], some[0])
    assert not bs.verify_data_root_inclusion(prover, commitment, heights[5] + 1, data_roots[5], some[0])
    # validator-set membership: leaves of differing lengths (the power's varint), against the set's hash
    keys, powers = [rng.randbytes(32) for _ in range(101)], [0, 1, 127, 128, 1 << 40] * 20 + [7]
    vhash, vproofs = bs.validator_inclusion_proofs(prover, keys, powers, indices=[0, 64, 100])
    assert vhash == bs.validator_set_hash(prover, keys, powers)
    for i, p in zip((0, 64, 100), vproofs):
        assert cases.hash_from_aunts(i, 101, cases.leaf_hash(bs.encode_validator(keys[i], powers[i])), list(p.aunts)) == vhash
    assert not prover.tm_verify_inclusion_batch([vhash], vproofs, [bs.encode_validator(keys[i], powers[i]) for i in (0, 64, 100)]).any()


@pytest.mark.gpu
def test_header_field_proofs_against_header_hash(prover):
    bs, dcm = cic.bs, cic.dcm
    rng = random.Random(8)
    headers = cic.make_chain(rng, cic.FIELD_LENGTHS, 8, 1 << 21, rng.randbytes(32))
    hashes, proofs = bs.header_field_proofs(prover, headers, 6)
    assert hashes == [dcm.HeaderChainMapReduce.header_hash(h) for h in headers]
    for b, p in enumerate(proofs):
        assert (p.total, p.index, p.leaf_hash) == (14, 6, cases.leaf_hash(headers[b][6]))
        assert cases.hash_from_aunts(6, 14, p.leaf_hash, list(p.aunts)) == hashes[b]
    status = prover.tm_verify_inclusion_batch(hashes, proofs, [h[6] for h in headers], root_of=list(range(8)))
    assert not status.any()
    status = prover.tm_verify_inclusion_batch(hashes, proofs, [h[6] for h in headers], root_of=[(b + 1) % 8 for b in range(8)])
    assert status.tolist() == [cases.BAD_ROOT] * 8


@pytest.mark.gpu
def test_prove_range_with_inclusion_proofs(prover):
    """8 tuples in 2 leaves of 4: the root proof and key equal the run without inclusion proofs, every inclusion proof verifies against the
    proven commitment, a tuple with a changed byte is refused"""
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    bs = cic.bs
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    rng = random.Random(4101)
    heights = [7_100_000 + k for k in range(8)]
    roots = [rng.randbytes(32) for _ in heights]
    mr = dm.DataCommitmentMapReduce(prover, consts, leaf_blocks=4, fan_in=2, num_queries=6, pow_bits=4)
    try:
        plain = mr.prove_range(heights, roots)
        out = mr.prove_range(heights, roots, inclusion=True)
        assert "inclusion" not in plain and set(out) == set(plain) | {"inclusion"}
        assert out["root_proof"] == plain["root_proof"] and np.array_equal(out["key"], plain["key"]) and out["commitment"] == plain["commitment"]
        assert len(out["inclusion"]) == 8
        assert not bs.verify_data_root_inclusions(prover, out["commitment"], heights, roots, out["inclusion"]).any()
        for k, p in enumerate(out["inclusion"]):
            assert cases.hash_from_aunts(p.index, p.total, cases.leaf_hash(bs.encode_data_root_tuple(heights[k], roots[k])), list(p.aunts)) == out["commitment"]
        changed = bytearray(roots[3])
        changed[9] ^= 0x20
        assert not bs.verify_data_root_inclusion(prover, out["commitment"], heights[3], bytes(changed), out["inclusion"][3])
        assert bs.verify_data_root_inclusion(prover, out["commitment"], heights[3], roots[3], out["inclusion"][3])
    finally:
        mr.free()
