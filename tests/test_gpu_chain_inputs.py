"""glp_tm_merkle_root_batch and glp_header_chain_leaf_inputs on the device, through the C ABI, at the shapes of tests/chain_inputs_cases.py (the
ones tests/test_emu_chain_inputs.py runs on the CPU): roots against the recursive hashlib tree, rows / statuses / hashes against
_chain_leaf_inputs, _map_chain's tests and header_hash; the launch and synchronise counts for 8 and 1024 headers; one small chain proved with
device_inputs off and on (same root proof bytes, same key, accepted by the native verifier); tampered headers refused with the existing texts."""
import ctypes
import hashlib
import importlib
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_inputs_cases as cases  # noqa: E402
from conftest import poseidon_consts  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

NQ, PW = 6, 4


@pytest.mark.gpu
def test_batched_trees_on_the_device(prover):
    for call in cases.tree_calls():
        assert prover.tm_merkle_root_batch(call.trees) == call.roots, call.name
        assert prover.tm_merkle_root_batch_last_counts() == (2 if call.total else 1, 1), call.name
    assert prover.tm_merkle_root_batch([]) == []
    assert prover.tm_merkle_root_batch_last_counts() == (0, 0)
    # roots left on the device: no synchronise in the call
    call = next(c for c in cases.tree_calls() if c.name == "B65")
    d_roots = prover.tm_merkle_root_batch(call.trees, download=False)
    assert prover.tm_merkle_root_batch_last_counts() == (2, 0)
    got = d_roots.download((call.B, 32), dtype=np.uint8)
    d_roots.free()
    assert [got[t].tobytes() for t in range(call.B)] == call.roots
    # tree by tree against glp_tm_merkle_root_var
    for t, leaves in enumerate(call.trees[:12]):
        assert prover.tm_merkle_root_var(leaves) == call.roots[t], t


@pytest.mark.gpu
def test_refused_tree_calls_write_nothing_on_the_device(prover):
    data = prover.to_device(np.ones(16, dtype=np.uint8))
    for name, data_len, offs, first, total, B, want in cases.refused_tree_calls():
        d_roots = prover.to_device(np.full((B, 32), 0xEE, dtype=np.uint8))
        h_roots = np.full((B, 32), 0xEE, dtype=np.uint8)
        rc = prover.lib.glp_tm_merkle_root_batch(prover.ctx, data.ptr, data_len, offs.ctypes.data, first.ctypes.data, total, B, d_roots.ptr,
                                                 h_roots.ctypes.data)
        assert rc == want, name
        assert np.all(h_roots == 0xEE) and np.all(d_roots.download((B, 32), dtype=np.uint8) == 0xEE), name
        assert prover.tm_merkle_root_batch_last_counts() == (0, 0), name
        d_roots.free()
    data.free()


def run_chain(pkg, prover, c, pad=3):
    layout = pkg.HeaderChainLayout.of(c.field_lengths, c.B, c.g)
    width = layout.n_words()
    stride = width + pad
    d_hdr = prover.to_device(c.blob)
    d_out = prover.to_device(np.full((c.n // c.B, stride), cases.SENTINEL, dtype=np.uint64))
    d_hashes = prover.alloc(32 * (c.n + 1))
    status = np.full(c.n, -1, dtype=np.int32)
    start = np.frombuffer(c.start, dtype=np.uint8).copy()
    prover._chk(prover.lib.glp_header_chain_leaf_inputs(prover.ctx, ctypes.byref(layout), d_hdr.ptr, start.ctypes.data, c.first, c.n, d_out.ptr, stride,
                                                        d_hashes.ptr, status.ctypes.data), "glp_header_chain_leaf_inputs")
    out = d_out.download((c.n // c.B, stride))
    hashes = d_hashes.download((c.n + 1, 32), dtype=np.uint8)
    for b in (d_hdr, d_out, d_hashes):
        b.free()
    assert np.all(out[:, width:] == cases.SENTINEL), "a row wrote past its width"
    return out[:, :width], status, [hashes[k].tobytes() for k in range(c.n + 1)]


def assert_chain(c, rows, status, hashes):
    assert hashes == c.hashes, c.name
    assert status.tolist() == c.status.tolist(), c.name
    want = c.rows_array(rows.shape[1])
    for l in range(rows.shape[0]):
        assert np.array_equal(rows[l], want[l]), (c.name, l, np.nonzero(rows[l] != want[l])[0][:8].tolist())
        if c.rows[l] is None:
            assert not rows[l].any(), (c.name, l)


@pytest.mark.gpu
def test_chain_rows_statuses_and_hashes_on_the_device(pkg, prover):
    for c in cases.good_chains() + cases.tampered_chains() + cases.truncated_chains() + [cases.nonminimal_chain()]:
        assert_chain(c, *run_chain(pkg, prover, c))
        launches, syncs = prover.header_chain_last_input_counts()
        assert launches <= 4 and syncs == 1, c.name


@pytest.mark.gpu
def test_counts_do_not_grow_with_the_chain(pkg, prover):
    """8 and 1024 headers: at most 4 launches and one synchronise alike; the hashes of the long chain equal header_hash, its rows
    _chain_leaf_inputs, at a few leaves spread over it"""
    rng = random.Random(5)
    counts = {}
    for n in (8, 1024):
        start = rng.randbytes(32)
        first = (1 << 21) + 77
        headers = cases.make_chain(rng, cases.FIELD_LENGTHS, n, first, start)
        layout = pkg.HeaderChainLayout.of(cases.FIELD_LENGTHS, 8, 4)
        blob = np.frombuffer(b"".join(x for h in headers for x in h), dtype=np.uint8)
        d_hdr = prover.to_device(blob)
        d_in, status, d_hashes = prover.header_chain_leaf_inputs(layout, d_hdr, start, first, n)
        counts[n] = prover.header_chain_last_input_counts()
        assert not status.any()
        width = layout.n_words()
        rows = d_in.download((n // 8, width))
        hashes = d_hashes.download((n + 1, 32), dtype=np.uint8)
        for b in (d_hdr, d_in, d_hashes):
            b.free()
        for l in sorted({0, n // 16, n // 8 - 1}):
            prev = start if l == 0 else cases.dcm.HeaderChainMapReduce.header_hash(headers[8 * l - 1])
            assert hashes[8 * l].tobytes() == prev
            assert rows[l].tolist() == cases.dcm._chain_leaf_inputs(prev, first + 8 * l, headers[8 * l:8 * l + 8], 4), l
        assert hashes[n].tobytes() == cases.dcm.HeaderChainMapReduce.header_hash(headers[-1])
    assert counts[8] == counts[1024] and counts[8][0] <= 4 and counts[8][1] == 1


@pytest.mark.gpu
def test_invalid_calls_and_the_empty_chain(pkg, prover):
    layout = pkg.HeaderChainLayout.of(cases.FIELD_LENGTHS, 2, 4)
    width = layout.n_words()
    d = prover.alloc(4 * layout.header_bytes())
    d_out = prover.alloc(2 * width * 8)
    status = np.zeros(4, dtype=np.int32)
    start = np.zeros(32, dtype=np.uint8)
    call = lambda hdr, st, n, out, stride, h_status: prover.lib.glp_header_chain_leaf_inputs(
        prover.ctx, ctypes.byref(layout), hdr, st, 1 << 21, n, out, stride, None, h_status)
    assert call(d.ptr, start.ctypes.data, 0, d_out.ptr, width, status.ctypes.data) == 0
    assert prover.header_chain_last_input_counts() == (0, 0)
    assert call(d.ptr, start.ctypes.data, 3, d_out.ptr, width, status.ctypes.data) == -1            # not a whole number of leaves
    assert call(None, start.ctypes.data, 4, d_out.ptr, width, status.ctypes.data) == -1
    assert call(d.ptr, None, 4, d_out.ptr, width, status.ctypes.data) == -1
    assert call(d.ptr, start.ctypes.data, 4, None, width, status.ctypes.data) == -1
    assert call(d.ptr, start.ctypes.data, 4, d_out.ptr, width, None) == -1
    assert call(d.ptr, start.ctypes.data, 4, d_out.ptr, width - 1, status.ctypes.data) == -1        # a stride below the row
    d.free()
    d_out.free()


@pytest.mark.gpu
def test_chain_proved_with_device_inputs_equals_the_python_path(pkg, prover):
    """4 headers in 2 leaves of 2, one node: device_inputs off and on (device_witness in both) give the same root proof bytes, public inputs, key
    and end hash; the native verifier accepts the root; a share in the middle of the chain (_map_chain, what a rank of prove_chain_distributed
    runs) gives the same leaf proof; tampered headers are refused with the texts of the Python path and the same header index.  One object: its
    recordings are shared, device_inputs is the attribute the keyword sets."""
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    rng = random.Random(4200)
    start, first = hashlib.sha256(b"trusted header").digest(), 2_500_000
    headers = cases.make_chain(rng, cases.FIELD_LENGTHS, 4, first, start)
    end = dm.HeaderChainMapReduce.header_hash(headers[-1])
    mr = dm.HeaderChainMapReduce(prover, consts, leaf_headers=2, fan_in=2, num_queries=NQ, pow_bits=PW, device_witness=True, device_inputs=True)
    try:
        assert mr.device_inputs
        on = mr.prove_chain(start, first, headers)
        hashes = [start] + [dm.HeaderChainMapReduce.header_hash(h) for h in headers]
        share_on = mr._map_chain(hashes, first, headers, 2, 4)
        mr.device_inputs = False
        off = mr.prove_chain(start, first, headers)
        share_off = mr._map_chain(hashes, first, headers, 2, 4)
        mr.device_inputs = True
        assert on["root_proof"] == off["root_proof"] and on["public"] == off["public"] and np.array_equal(on["key"], off["key"])
        assert on["end_hash"] == off["end_hash"] == end and on["commitment"] == off["commitment"] and on["leaves"] == 2
        assert share_on == share_off and len(share_on) == 1
        assert mr.verify_chain(on["root_proof"], on["key"], start, end, on["commitment"], first), prover.last_reject
        dist = mr.prove_chain_distributed(start, first, headers)                 # one rank: its share is the whole chain, one hash kept on the host
        assert dist["ranks"] == 1 and dist["public"] == on["public"] and np.array_equal(dist["key"], on["key"]) and dist["end_hash"] == end
        assert mr.verify_chain(dist["root_proof"], dist["key"], start, end, dist["commitment"], first), prover.last_reject
        assert not mr.verify_chain(on["root_proof"], on["key"], start, end, on["commitment"], first + 1)
        for kind, at, text in (("link-bit", 0, "header 0 does not name its predecessor's hash"), ("link-prefix", 3, "header 3 does not name"),
                               ("height+1", 2, f"header 2: the height field is not the encoding of {first + 2}"),
                               ("varint-overlong", 1, f"header 1: the height field is not the encoding of {first + 1}"),
                               ("data-prefix", 3, f"header 3: the height field is not the encoding of {first + 3}, or the data-hash field is malformed")):
            bad = [list(h) for h in headers]
            cases.tamper(bad, start, first, at, kind, 4)
            for flag in (True, False):
                mr.device_inputs = flag
                with pytest.raises(ValueError, match=text):
                    mr.prove_chain(start, first, bad)
        mr.device_inputs = True
        with pytest.raises(ValueError, match="recorded lengths"):
            mr.prove_chain(start, first, [h[:13] + [h[13] + b"x"] for h in headers])
    finally:
        mr.free()
