"""The Reduce step with its witnesses made on the device, on the MI355X: the segmented plan (glp_witness_plan_create_ex — a workgroup per
(node, child) in three stream-ordered launches) against the host evaluator and against the single-workgroup device path; the word checks
(glp_witness_check_words) against WitnessProgram.check_words through RecursionProgram.prove; and the MapReduces — DataCommitment, signature
set with its padded root, an outer node over children of different circuits — giving with device_witness on the proofs they give with it off.
Shapes: the smallest the suite uses (num_queries=6, pow_bits=4)."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import poseidon_consts  # noqa: E402
from test_gpu_witness_device import NONE, _mod, host_eval  # noqa: E402

NQ, PW = 6, 4


@pytest.fixture(scope="module")
def env(prover, pkg):
    """(constants, a second prover on the same GPU, {fan-in: (DataCommitment MapReduce over 4 * fan-in heights, heights, roots, leaf proofs)}):
    recorded once, shared by the tests below — which switch the objects' device_witness attribute, the value the keyword sets, instead of
    recording every circuit a second time"""
    dm = _mod(".data_commitment_mr")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    extra = pkg.Prover(0)
    extra.set_poseidon_constants(*consts)
    rng = np.random.default_rng(4200)
    shapes = {}
    for fan in (2, 4):
        mr = dm.DataCommitmentMapReduce(prover, consts, leaf_blocks=2, fan_in=fan, num_queries=NQ, pow_bits=PW, map_provers=[extra], device_witness_chunk=3)
        heights = [7_000_000 + k for k in range(4 * fan)]
        roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
        shapes[fan] = (mr, heights, roots, mr.prove_leaves(heights, roots))
    yield consts, extra, shapes
    for mr, _, _, _ in shapes.values():
        mr.free()
    extra.close()


def level1_node(mr, leaves):
    """the recorded level-1 node program of the MapReduce (recorded by the first reduce)"""
    if not any(k[0] == 1 for k in mr.nodes):
        mr.reduce(leaves, max_levels=1)
    return next(v for k, v in mr.nodes.items() if k[0] == 1)


def raw_device_eval(prover, prog, plan, batch, pad=5):
    """glp_witness_eval_device on a plan handle: (status, first_bad, values) of every instance"""
    inp = np.ascontiguousarray(batch, dtype=np.uint64).reshape(len(batch), prog.n_inputs)
    B, stride = inp.shape[0], prog.n_values + pad
    d_in = prover.to_device(inp)
    d_vals = prover.to_device(np.full((B, stride), 0xABCD, dtype=np.uint64))
    status, bad = np.full(B, 99, dtype=np.int32), np.zeros(B, dtype=np.uint64)
    try:
        for _ in range(2):                                                 # the second call finds the plan resident
            prover._chk(prover.lib.glp_witness_eval_device(prover.ctx, plan, d_in.ptr, d_vals.ptr, stride, B, status.ctypes.data, bad.ctypes.data),
                        "glp_witness_eval_device")
        vals = d_vals.download((B, stride))
    finally:
        d_in.free()
        d_vals.free()
    assert np.all(vals[:, prog.n_values:] == 0xABCD)
    return status.tolist(), [int(x) for x in bad], vals[:, :prog.n_values]


def flip_word(proofs, child, pos):
    words = [np.frombuffer(p, dtype="<u8").copy() for p in proofs]
    words[child][pos] ^= np.uint64(1)
    return [w.tobytes() for w in words]


@pytest.mark.gpu
def test_segmented_evaluation_of_two_nodes_and_a_tampered_one(prover, env):
    consts, _, shapes = env
    mr, _, _, leaves = shapes[4]
    prog = level1_node(mr, leaves).program
    parts = prog.plan_parts()
    print(f"level-1 node, fan-in 4: {prog.n_values} variables, parts (ops, depth, steps) {[tuple(p.values()) for p in parts]}, "
          f"single workgroup {prog.plan_stats()}")
    assert len(parts) == 4 + 2 and len(prog.plan_parts(segments=False)) == 1
    tags = prog.input_tags[prog.input_tags[:, 0] == 2]
    bad_group = flip_word(leaves[0:4], 2, int(tags[len(tags) // 2, 1]))
    batch = [prog.inputs_from_words(g)[0] for g in (leaves[0:4], leaves[4:8], bad_group)]
    st_seg, bad_seg, vals_seg = raw_device_eval(prover, prog, prog.plan(segments=True), batch)
    st_one, bad_one, vals_one = raw_device_eval(prover, prog, prog.plan(), batch)
    print(f"segmented {st_seg} {bad_seg}; single workgroup {st_one} {bad_one}")
    assert st_seg == st_one == [0, 0, -7] and bad_seg == bad_one and bad_seg[:2] == [NONE, NONE] and bad_seg[2] != NONE
    assert vals_seg.tobytes() == vals_one.tobytes()
    for b in range(3):
        rc_h, bad_h, vals_h = host_eval(prover.lib, prog.prog, prog.n_values, prog.eq_pairs, consts, batch[b])
        assert (st_seg[b], bad_seg[b]) == (rc_h, bad_h)
        assert vals_seg[b].tobytes() == vals_h.tobytes(), f"instance {b}"
    # the Python face: evaluate's values, evaluate's refusal
    slab = prog.evaluate_device(prover, batch[:2], segments=True)
    for b in range(2):
        assert np.array_equal(slab.download(b), prog.evaluate(consts, batch[b]))
    with pytest.raises(ValueError, match=f"instance 2: the inputs do not satisfy the circuit \\(copy constraint {bad_seg[2]} fails\\)"):
        prog.evaluate_device(prover, batch, slab=slab, segments=True)
    slab.free()


@pytest.mark.gpu
def test_word_checks_refuse_with_the_host_message(prover, env):
    _, _, shapes = env
    mr, _, _, leaves = shapes[4]
    rp = level1_node(mr, leaves)
    prog, group = rp.program, leaves[0:4]
    assert prog.wc_var.shape[0] and prog.wc_bits.shape[0]
    good_host, good_dev = rp.prove(group, NQ, PW), rp.prove(group, NQ, PW, device_witness=True)
    assert good_host == good_dev
    for table in (prog.wc_var, prog.wc_bits):
        k, pos = (int(v) for v in table[table.shape[0] // 2, :2])
        bad = flip_word(group, k, pos)
        with pytest.raises(ValueError) as host:
            rp.prove(bad, NQ, PW)
        with pytest.raises(ValueError) as dev:
            rp.prove(bad, NQ, PW, device_witness=True)
        print(f"host: {host.value}\ndevice: {dev.value}")
        assert str(host.value) == str(dev.value) == f"input {k}: word {pos} differs from the " + (
            "value the circuit derives" if table is prog.wc_var else "index the transcript derives")
    # a tampered INPUT word: the evaluator's refusal, the same text on both paths
    tags = prog.input_tags[prog.input_tags[:, 0] == 1]
    bad = flip_word(group, 1, int(tags[len(tags) // 3, 1]))
    with pytest.raises(ValueError) as host:
        rp.prove(bad, NQ, PW)
    with pytest.raises(ValueError) as dev:
        rp.prove(bad, NQ, PW, device_witness=True)
    assert str(host.value) == str(dev.value) and "copy constraint" in str(host.value)
    # two nodes at once: the refusal names the instance
    slab = rp.witness_batch([group, leaves[4:8]])
    assert slab.B == 2
    k, pos = (int(v) for v in prog.wc_var[0, :2])
    with pytest.raises(ValueError, match=f"instance 1: input {k}: word {pos} differs from the value the circuit derives"):
        rp.witness_batch([group, flip_word(leaves[4:8], k, pos)])


@pytest.mark.gpu
@pytest.mark.parametrize("fan", [2, 4])
def test_reduce_gives_the_same_proofs(prover, env, fan):
    """fan-in 2 over 8 heights: 4 leaves, two nodes, a root of 2; fan-in 4 over 16 heights: 8 leaves, two nodes of 4, a root of 2 — two groups per
    level-1 level, so the second prover proves from the main prover's slab"""
    _, _, shapes = env
    mr, heights, roots, leaves = shapes[fan]
    res = {}
    try:
        for on in (False, True):
            mr.device_witness = on
            out = mr.prove_range(heights, roots)
            nodes, _, node_key, _ = mr.reduce(leaves, max_levels=1)
            assert len(nodes) == 2 and [lv["nodes"] for lv in out["levels"]] == [2, 1]
            res[on] = (nodes, np.array(node_key), out["root_proof"], np.array(out["key"]), out["commitment"])
        for a, b in zip(res[False], res[True]):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        mr.device_witness = False
        vkey = mr.expected_key(len(heights))
        assert np.array_equal(vkey, res[True][3])
        assert mr.verify(res[True][2], vkey, heights, roots, res[True][4]), prover.last_reject
    finally:
        mr.device_witness = False


@pytest.mark.gpu
def test_signature_set_padded_root(prover, env):
    """5 validators in 8 slots, fan-in 2: four leaves fold to two nodes, and the root is the trimmed _padded_root"""
    sm, ec = _mod(".signature_mr"), _mod(".ed25519_circuit")
    consts, extra, _ = env
    block = hashlib.sha256(b"a block").digest()
    sigs = sm.SignatureSetMapReduce(prover, consts, msg_len=48, hash_offset=8, fan_in=2, num_queries=NQ, pow_bits=PW, map_provers=[extra],
                                    device_witness_chunk=4)
    msgs = [sigs.vote_bytes(block, i) for i in range(5)]
    seeds = [hashlib.sha256(b"seed %d" % i).digest() for i in range(5)]
    pubs = [ec.keypair_and_sign(s, m)[0] for s, m in zip(seeds, msgs)]
    sg = [ec.keypair_and_sign(s, m)[1] for s, m in zip(seeds, msgs)][:4] + [None]
    flags = [True, True, True, True, False]
    res = {}
    for on in (False, True):
        sigs.device_witness = on
        so = res[on] = sigs.prove_set(pubs, sg, msgs, flags)
    assert any(k[0] == "padded_root" for k in sigs.nodes)
    assert res[False]["root_proof"] == res[True]["root_proof"] and np.array_equal(res[False]["key"], res[True]["key"])
    assert sigs.verify_set(so["root_proof"], res[False]["key"], so["block_hash"], so["signer_digest"]), prover.last_reject
    sigs.free()


@pytest.mark.gpu
def test_children_of_different_circuits(prover, pkg, env):
    """one node over a DataCommitment root and a header-chain root: two segments of different lengths"""
    dm, vc = _mod(".data_commitment_mr"), _mod(".verifier_circuit")
    consts, _, shapes = env
    mr, heights, roots, _ = shapes[2]
    dc = mr.prove_range(heights, roots)
    ch = dm.HeaderChainMapReduce(prover, consts, leaf_headers=2, fan_in=2, num_queries=NQ, pow_bits=PW)
    headers, _ = ch.synthetic_chain(8)
    chain = ch.prove_chain(bytes(32), 1 << (7 * (ch.n_groups - 1)), headers)
    specs = [dict(leaf_key=dc["key"], n_public=mr.N_PUBLIC, child_is_recursion=True, child_sha=True),
             dict(leaf_key=chain["key"], n_public=ch.N_PUBLIC, child_is_recursion=True, child_sha=True)]
    proofs = [dc["root_proof"], chain["root_proof"]]
    rp = vc.RecursionProgram(prover, proofs, dc["key"], NQ, PW, pkg.SHA_GATE_WIRES, consts, n_routed=80, n_public=mr.N_PUBLIC, cap_height=1,
                             child_is_recursion=True, child_sha=True, builder_wires=pkg.SHA_GATE_WIRES, specs=specs)
    parts = rp.program.plan_parts()
    print(f"parts (ops, depth, steps) {[tuple(p.values()) for p in parts]}")
    assert len(parts) == 2 + 2 and parts[1] != parts[2]
    host, dev = rp.prove(proofs, NQ, PW), rp.prove(proofs, NQ, PW, device_witness=True)
    assert host == dev
    assert prover.plonk_verify(dev[0], rp.key(), NQ, PW, public=dev[1]), prover.last_reject
    rp.free()
    ch.free()
