"""Device-side witness evaluation (glp_witness_eval_device: csrc/witness_kernels.cuh) against the host evaluator glp_witness_eval on the
MI355X: byte-identical variables for accepted instances, the host's verdict and copy-constraint index for refused ones, the other instances
of a batch unaffected; the Map steps with the device_witness keyword on give the proofs they give with it off."""
import ctypes
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import P, poseidon_consts, ptr, rand_field  # noqa: E402
import __graft_entry__ as graft  # noqa: E402
from test_emu_witness import synthetic_cases, synthetic_program  # noqa: E402
from test_emu_witness_segments import segmented_cases, segmented_synthetic_program  # noqa: E402

NONE = (1 << 64) - 1


def _mod(name):
    graft.load_package()
    return importlib.import_module(graft.PKG_NAME + name)


def host_eval(lib, prog, n_values, eq, consts, inputs):
    inp = np.ascontiguousarray(inputs, dtype=np.uint64)
    vals = np.zeros(n_values, dtype=np.uint64)
    bad = ctypes.c_size_t(0)
    rc = lib.glp_witness_eval(*(a.ctypes.data for a in consts), prog.ctypes.data, prog.size, inp.ctypes.data if inp.size else None, inp.size,
                              vals.ctypes.data, vals.size, eq.ctypes.data if eq.size else None, eq.size // 2, ctypes.byref(bad))
    return rc, (NONE if bad.value == ctypes.c_size_t(-1).value else bad.value), vals


def raw_device_eval(prover, prog, n_inputs, n_values, eq, batch, pad=5, seg=None):
    """the C ABI directly: plan (segmented when seg holds the segment bounds), upload, evaluate, download everything"""
    lib = prover.lib
    prog, eq = np.ascontiguousarray(prog, dtype=np.uint64), np.ascontiguousarray(eq, dtype=np.uint64)
    h = ctypes.c_void_p()
    if seg is None:
        assert lib.glp_witness_plan_create(prog.ctypes.data, prog.size, n_inputs, n_values, eq.ctypes.data if eq.size else None, eq.size // 2, ctypes.byref(h)) == 0
    else:
        seg = np.ascontiguousarray(seg, dtype=np.uint64)
        assert lib.glp_witness_plan_create_ex(prog.ctypes.data, prog.size, n_inputs, n_values, eq.ctypes.data if eq.size else None, eq.size // 2,
                                              seg.ctypes.data, seg.size - 1, ctypes.byref(h)) == 0
    inp = np.ascontiguousarray(batch, dtype=np.uint64).reshape(len(batch), n_inputs)
    B, stride = inp.shape[0], n_values + pad
    d_in = prover.to_device(inp)
    d_vals = prover.to_device(np.full((B, stride), 0xABCD, dtype=np.uint64))
    status, bad = np.full(B, 99, dtype=np.int32), np.zeros(B, dtype=np.uint64)
    try:
        for _ in range(2):                                                 # the second call finds the plan resident
            prover._chk(lib.glp_witness_eval_device(prover.ctx, h, d_in.ptr, d_vals.ptr, stride, B, status.ctypes.data, bad.ctypes.data), "glp_witness_eval_device")
        vals = d_vals.download((B, stride))
    finally:
        d_in.free()
        d_vals.free()
        lib.glp_witness_plan_destroy(h)
    assert np.all(vals[:, n_values:] == 0xABCD)
    return status, bad, vals[:, :n_values]


def check_batch(prover, prog, consts, batch, want):
    """glp_witness_eval_device against glp_witness_eval, instance by instance"""
    status, bad, vals = raw_device_eval(prover, prog.prog, prog.n_inputs, prog.n_values, prog.eq_pairs, batch)
    for b, inputs in enumerate(batch):
        rc_h, bad_h, vals_h = host_eval(prover.lib, prog.prog, prog.n_values, prog.eq_pairs, consts, inputs)
        print(f"instance {b}: host ({rc_h}, {bad_h})  device ({int(status[b])}, {int(bad[b])})")
        assert (int(status[b]), int(bad[b])) == (rc_h, bad_h), f"instance {b}"
        assert rc_h == want[b]
        if rc_h == 0 or bad_h != NONE:
            assert vals[b].tobytes() == vals_h.tobytes(), f"instance {b}"


@pytest.mark.gpu
def test_eight_signatures_one_forged(prover):
    ec = _mod(".ed25519_circuit")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    msgs = [f"vote: block 4000000 round 0, validator {i}".encode().ljust(112, b".") for i in range(8)]
    keys = [ec.keypair_and_sign(hashlib.sha256(b"validator %d" % i).digest(), m) for i, m in enumerate(msgs)]
    b, _ = ec.ed25519_circuit(object(), keys[0][0], keys[0][1], msgs[0])
    prog = b.program()
    sigs = [k[1] for k in keys]
    forged = bytearray(sigs[5])
    forged[40] ^= 1
    sigs[5] = bytes(forged)
    batch = [ec.witness_inputs(keys[i][0], sigs[i], msgs[i]) for i in range(8)]
    check_batch(prover, prog, consts, batch, [0, 0, 0, 0, 0, -7, 0, 0])
    # the Python face: the same slab, the refusal names the instance, a batch without the forgery yields public values without a download of the slab
    with pytest.raises(ValueError, match="instance 5: the inputs do not satisfy the circuit"):
        prog.evaluate_device(prover, batch)
    slab = prog.evaluate_device(prover, batch[:5])
    for i in (0, 4):
        want = prog.evaluate(consts, batch[i], threads=1)
        assert np.array_equal(slab.download(i), want)
        assert [int(v) for v in slab.gather_vars(i, prog.public_vars)] == ec.public_inputs(keys[i][0], msgs[i])
    slab.free()


@pytest.mark.gpu
def test_data_commitment_header_chain_and_recursion_node_programs(prover):
    dm = _mod(".data_commitment_mr")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    rng = np.random.default_rng(41)
    # DataCommitment leaves (SHA rows + Poseidon): four leaves of two tuples, one with a word that is not 32 bits
    mr = dm.DataCommitmentMapReduce(prover, consts, leaf_blocks=2, fan_in=2, num_queries=6, pow_bits=4)
    heights = [7_000_000 + k for k in range(8)]
    roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
    mr._record_leaf()
    batch = [[w for h, r in zip(heights[k:k + 2], roots[k:k + 2]) for w in dm.tuple_words(h, r)] for k in range(0, 8, 2)]
    bad = list(batch[2])
    bad[3] = 1 << 32
    check_batch(prover, mr.leaf_program, consts, batch + [bad], [0, 0, 0, 0, -7])
    # a recursion node over two of its leaf proofs (Poseidon, POSEIDON_SWAP, EINV): B = 1 and B = 2, and a tampered child
    leaves = mr.prove_leaves(heights, roots)
    mr.reduce(leaves)
    node = next(v for k, v in mr.nodes.items() if k[0] == 1)
    kinds = set()
    pc, words = 0, node.program.prog
    oplen = [8, 3, 4, 3, 5, 2, 25, 10, 6, 6, 4, 5, 26, 9, 24]
    while pc < words.size:
        kinds.add(int(words[pc]))
        pc += oplen[int(words[pc])]
    assert {6, 12, 4} <= kinds
    in01, _ = node.program.inputs_from_words(leaves[0:2])
    in23, _ = node.program.inputs_from_words(leaves[2:4])
    check_batch(prover, node.program, consts, [in01], [0])
    check_batch(prover, node.program, consts, [in01, in23], [0, 0])
    w = np.frombuffer(leaves[1], dtype="<u8").copy()
    w[int(node.program.input_tags[len(node.program.input_tags) // 2, 1])] ^= np.uint64(1)
    in_bad, _ = node.program.inputs_from_words([leaves[0], w.tobytes()])
    check_batch(prover, node.program, consts, [in23, in_bad, in01], [0, -7, 0])
    mr.free()
    # header-chain leaves
    ch = dm.HeaderChainMapReduce(prover, consts, leaf_headers=2, fan_in=2, num_queries=6, pow_bits=4)
    headers, _ = ch.synthetic_chain(8)
    first = 1 << (7 * (ch.n_groups - 1))
    ch._record_leaf()
    hashes = [bytes(32)] + [ch.header_hash(h) for h in headers]
    batch = [dm._chain_leaf_inputs(hashes[k], first + k, headers[k:k + 2], ch.n_groups) for k in range(0, 8, 2)]
    check_batch(prover, ch.leaf_program, consts, batch, [0, 0, 0, 0])
    ch.free()


@pytest.mark.gpu
def test_more_instances_than_workgroups(prover):
    """300 instances of a small program: the grid is one workgroup per compute unit, the rest is the grid-stride loop"""
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    prog, nv = [], 4
    for i in range(4):
        prog += [1, i, i]
    prev = 0
    for k in range(30):
        prog += [0, nv, prev, (k + 1) % 4, (k + 2) % 4, 3 + k, 5, 7]
        prev = nv
        nv += 1
    prog += [6] + list(range(nv, nv + 12)) + [prev, 0, 1, 2, 3, prev, 0, 1, 2, 3, prev, 0]
    nv += 12
    eq = np.array([0, 1], dtype=np.uint64)                                 # inputs 0 and 1 must be equal
    prog = np.array(prog, dtype=np.uint64)
    rng = np.random.default_rng(300)
    batch = rand_field(rng, (300, 4))
    batch[:, 1] = batch[:, 0]
    broken = [7, 255, 256, 299]
    batch[broken, 1] ^= np.uint64(1)
    status, bad, vals = raw_device_eval(prover, prog, 4, nv, eq, batch)
    for b in range(300):
        rc_h, bad_h, vals_h = host_eval(prover.lib, prog, nv, eq, consts, batch[b])
        assert (int(status[b]), int(bad[b])) == (rc_h, bad_h) == ((-7, 0) if b in broken else (0, NONE))
        assert vals[b].tobytes() == vals_h.tobytes()


def check_raw_batch(prover, prog, n_inputs, n_values, eq, consts, batch, want, seg=None):
    """check_batch for a program given as arrays: verdict, first failing pair, values — instance by instance against glp_witness_eval"""
    status, bad, vals = raw_device_eval(prover, prog, n_inputs, n_values, eq, batch, seg=seg)
    for b, inputs in enumerate(batch):
        rc_h, bad_h, vals_h = host_eval(prover.lib, prog, n_values, eq, consts, inputs)
        print(f"instance {b}: host ({rc_h}, {bad_h})  device ({int(status[b])}, {int(bad[b])})")
        assert (int(status[b]), int(bad[b])) == (rc_h, bad_h), f"instance {b}"
        assert rc_h == want[b], f"instance {b}"
        if rc_h == 0 or bad_h != NONE:
            assert vals[b].tobytes() == vals_h.tobytes(), f"instance {b}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "big"])
def test_every_op_kind_on_both_constant_kinds(prover, kind):
    """the synthetic program of tests/test_emu_witness.py (every op kind, a 150-wide level, a 40-deep chain) with its thirteen accept / refuse
    cases through glp_witness_eval_kernel<true> (small-integer MDS) and <false> (generic MDS: any other injected constants)"""
    consts = poseidon_consts(kind)
    prog, n_values, eq = synthetic_program()
    batch, want = synthetic_cases(np.random.default_rng(14))
    assert len(batch) == 14 and sorted(set(want)) == [-7, -1, 0]
    prover.set_poseidon_constants(*consts)
    try:
        check_raw_batch(prover, prog, 62, n_values, eq, consts, batch, want)
    finally:
        prover.set_poseidon_constants(*poseidon_consts("small"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "big"])
def test_segmented_every_op_kind_on_both_constant_kinds(prover, kind):
    """the segmented synthetic program of tests/test_emu_witness_segments.py (prefix | two segments | tail, a refusal in each launch) through
    glp_witness_eval_part_kernel<true> and <false>"""
    consts = poseidon_consts(kind)
    prog, n_values, eq, seg = segmented_synthetic_program()
    batch, want = segmented_cases(np.random.default_rng(15))
    assert len(batch) == 7 and sorted(set(want)) == [-7, -1, 0]
    prover.set_poseidon_constants(*consts)
    try:
        check_raw_batch(prover, prog, 62, n_values, eq, consts, batch, want, seg=seg)
    finally:
        prover.set_poseidon_constants(*poseidon_consts("small"))


@pytest.mark.gpu
def test_map_steps_with_device_witness_give_the_same_proofs(prover, pkg):
    dm, sm, ec = _mod(".data_commitment_mr"), _mod(".signature_mr"), _mod(".ed25519_circuit")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    extra = pkg.Prover(0)
    extra.set_poseidon_constants(*consts)
    rng = np.random.default_rng(4100)
    heights = [7_000_000 + k for k in range(8)]
    roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
    res = {}
    for on in (False, True):
        mr = dm.DataCommitmentMapReduce(prover, consts, leaf_blocks=2, fan_in=2, num_queries=6, pow_bits=4, map_provers=[extra], device_witness=on,
                                        device_witness_chunk=3)
        leaves = mr.prove_leaves(heights, roots)
        out = mr.prove_range(heights, roots)
        res[on] = (leaves, out["root_proof"], np.array(out["key"]))
        if not on:
            vkey = mr.expected_key(8)
        else:
            assert mr.verify(out["root_proof"], vkey, heights, roots, out["commitment"]), prover.last_reject
            with pytest.raises(ValueError, match="instance 3"):
                mr._map_inputs([[w for h, r in zip(heights[k:k + 2], roots[k:k + 2]) for w in dm.tuple_words(h, r)] if k != 6 else [1 << 32] * 32
                                for k in range(0, 8, 2)])
        mr.free()
    assert res[False][0] == res[True][0] and res[False][1] == res[True][1] and np.array_equal(res[False][2], res[True][2])
    # the signature Map: 5 validators (one unsigned) padded to 8 slots, as tests/test_gpu_combined_skip.py runs it
    block = hashlib.sha256(b"a block").digest()
    res = {}
    for on in (False, True):
        sigs = sm.SignatureSetMapReduce(prover, consts, msg_len=48, hash_offset=8, fan_in=2, num_queries=6, pow_bits=4, map_provers=[extra],
                                        device_witness=on, device_witness_chunk=4)
        msgs = [sigs.vote_bytes(block, i) for i in range(5)]
        seeds = [hashlib.sha256(b"seed %d" % i).digest() for i in range(5)]
        pubs = [ec.keypair_and_sign(s, m)[0] for s, m in zip(seeds, msgs)]
        sg = [ec.keypair_and_sign(s, m)[1] for s, m in zip(seeds, msgs)]
        flags = [True, True, True, True, False]
        sg[4] = None
        so = sigs.prove_set(pubs, sg, msgs, flags)
        slots = sigs._slots(pubs, sg, msgs, flags)
        leaves = sigs._map(slots, 0, 4)
        res[on] = (leaves, so["root_proof"], np.array(so["key"]))
        if not on:
            vkey = sigs.expected_key(5)
        else:
            assert np.array_equal(vkey, so["key"]) and sigs.verify_set(so["root_proof"], vkey, so["block_hash"], so["signer_digest"]), prover.last_reject
        sigs.free()
    assert res[False][0] == res[True][0] and res[False][1] == res[True][1] and np.array_equal(res[False][2], res[True][2])
    extra.close()
