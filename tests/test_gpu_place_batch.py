"""Batched witness placement (glp_witness_place_batch) and batched proving of Reduce levels, on the MI355X.  Placement of several slab rows in
one call against DeviceWitnessBatch.device_witness per row, byte for byte, with its launch and synchronise counts; RecursionProgram.prove_batch
against prove per group; a whole Reduce with prove_batch on against prove_batch off (the parent's code path), with host and device witnesses; a
tampered child in the second run of a level; and the C ABI sequence from a compiled host (tests/cpp/host_place.cpp).
Shapes: those of test_gpu_reduce_device.py (leaf_blocks=2, num_queries=6, pow_bits=4, one extra prover on the same GPU)."""
import hashlib
import importlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_ref as pref  # noqa: E402
from conftest import ROOT, poseidon_consts, ptr  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

NQ, PW = 6, 4
SENTINEL = 0x5E5E5E5E5E5E5E5E
GAP = 5


def _mod(name):
    graft.load_package()
    return importlib.import_module(graft.PKG_NAME + name)


def leaf_inputs(dm, heights, roots, lo, count):
    return [[w for h, r in zip(heights[2 * k:2 * k + 2], roots[2 * k:2 * k + 2]) for w in dm.tuple_words(h, r)] for k in range(lo, lo + count)]


@pytest.fixture(scope="module")
def env(prover, pkg, oracle):
    """(constants, a second prover on the same GPU, {fan-in: (DataCommitment MapReduce, heights, roots, leaf proofs)}): fan-in 2 over 8 leaves
    (4 -> 2 -> 1 nodes) and fan-in 4 over 12 leaves (three level-1 nodes), recorded once and shared by the tests below — which switch the objects'
    prove_batch / device_witness attributes, the values the keywords set, instead of recording every circuit again"""
    dm = _mod(".data_commitment_mr")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    oracle.orc_poseidon_set_constants(*(ptr(a) for a in consts))
    extra = pkg.Prover(0)
    extra.set_poseidon_constants(*consts)
    rng = np.random.default_rng(4300)
    shapes = {}
    for fan, n_leaves in ((2, 8), (4, 12)):
        mr = dm.DataCommitmentMapReduce(prover, consts, leaf_blocks=2, fan_in=fan, num_queries=NQ, pow_bits=PW, map_provers=[extra], device_witness_chunk=32)
        heights = [7_100_000 + k for k in range(2 * n_leaves)]
        roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
        shapes[fan] = (mr, heights, roots, mr.prove_leaves(heights, roots))
    yield consts, extra, shapes
    for mr, _, _, _ in shapes.values():
        mr.free()
    extra.close()


def level1_node(mr, leaves):
    if not any(k[0] == 1 for k in mr.nodes):
        mr.reduce(leaves, max_levels=1)
    return next(v for k, v in mr.nodes.items() if k[0] == 1)


def flip_word(proofs, child, pos):
    words = [np.frombuffer(p, dtype="<u8").copy() for p in proofs]
    words[child][pos] ^= np.uint64(1)
    return [w.tobytes() for w in words]


def check_placement(pkg, main, other, slab, ids):
    """device_witness_batch(ids) against device_witness per id: the matrices byte for byte, the public values, the sentinels in the gap behind
    every matrix, the counts; on the slab's own prover and from another ctx of the same device"""
    prog = slab.program
    words = prog.W << prog.log_n
    ref = {}
    for i in sorted(set(ids)):
        dw, public = slab.device_witness(main, i, reuse=False)
        ref[i] = (dw.download(words).tobytes(), public)
        dw.free()
    assert len({m for m, _ in ref.values()}) == len(ref) and len({tuple(p) for _, p in ref.values()}) == len(ref)     # the instances differ
    counts = {}
    for pr in (main, other):
        for B in (1, len(ids)):
            use = ids[:B]
            # the Python face: a [B][W][n] buffer
            out = pkg.DeviceBuffer(pr, B * words * 8)
            publics = slab.device_witness_batch(pr, use, out)
            counts[(pr is main, B)] = pr.witness_last_place_counts()
            got = out.download((B, words))
            out.free()
            for j, i in enumerate(use):
                assert got[j].tobytes() == ref[i][0], f"matrix {j} (slab row {i})"
                assert publics[j] == ref[i][1], f"public values {j} (slab row {i})"
            # the C face with a wire stride above W * n and no public values: sentinels survive, nothing is synchronised by the call
            gapped = pr.to_device(np.full((B, words + GAP), SENTINEL, dtype=np.uint64))
            assert pr.witness_place_batch(prog.layout(), slab.buf, slab.stride, use, gapped, words + GAP, want_public=False) is None
            assert pr.witness_last_place_counts() == (counts[(pr is main, B)][0] - (1 if prog.public_vars.size else 0), 0)
            pr.sync()
            got = gapped.download((B, words + GAP))
            gapped.free()
            for j, i in enumerate(use):
                assert got[j, :words].tobytes() == ref[i][0], f"gapped matrix {j} (slab row {i})"
            assert np.all(got[:, words:] == SENTINEL)
    print(f"{prog.W} x 2^{prog.log_n}, Poseidon rows {prog.pos_row_ids.size}, SHA rows {prog.sha_row_ids.size}: (launches, synchronises) {counts}")
    want = (1 + bool(prog.pos_row_ids.size) + bool(prog.sha_row_ids.size) + bool(prog.public_vars.size), 1 if prog.public_vars.size else 0)
    assert set(counts.values()) == {want} and want[0] <= 4 and want[1] <= 1             # the same at B = 1 and B = 3, on both ctxs
    # B = 0: nothing
    assert main.witness_place_batch(prog.layout(), slab.buf, slab.stride, [], slab.buf, words).shape ==(0, prog.public_vars.size)
    assert main.witness_last_place_counts() == (0, 0)


@pytest.mark.gpu
def test_placement_of_node_witnesses(pkg, prover, env):
    """the fan-in-4 level-1 node program (Poseidon rows): three nodes evaluated on the device, placed as ids [2, 0, 1]"""
    _, extra, shapes = env
    mr, _, _, leaves = shapes[4]
    rp = level1_node(mr, leaves)
    assert rp.program.pos_row_ids.size and rp.program.public_vars.size
    slab = rp.witness_batch([leaves[0:4], leaves[4:8], leaves[8:12]])
    assert slab.B == 3
    check_placement(pkg, prover, extra, slab, [2, 0, 1])


@pytest.mark.gpu
def test_placement_of_leaf_witnesses(pkg, prover, env):
    """the leaf program (SHA rows): three leaves evaluated on the device, placed as ids [2, 0, 1]"""
    dm = _mod(".data_commitment_mr")
    _, extra, shapes = env
    mr, heights, roots, _ = shapes[2]
    prog = mr.leaf_program
    assert prog.sha_row_ids.size and len(set(prog.sha_kinds.tolist())) == 4
    slab = prog.evaluate_device(prover, leaf_inputs(dm, heights, roots, 1, 3))
    try:
        check_placement(pkg, prover, extra, slab, [2, 0, 1])
        with pytest.raises(IndexError):
            slab.device_witness_batch(prover, [0, 3], slab.buf)
    finally:
        slab.free()


@pytest.mark.gpu
@pytest.mark.parametrize("device_witness", [False, True])
def test_prove_batch_equals_prove(prover, oracle, env, device_witness):
    """the four fan-in-2 groups of 8 leaves through ONE RecursionProgram.prove_batch call against four prove calls, byte for byte; each proof is
    accepted by the library's verifier and by the independent restatement (tests/plonk_ref.py)"""
    consts, _, shapes = env
    mr, _, _, leaves = shapes[2]
    rp = level1_node(mr, leaves)
    groups = [leaves[k:k + 2] for k in range(0, 8, 2)]
    ref = [rp.prove(g, NQ, PW, device_witness=device_witness) for g in groups]
    assert len({p for p, _ in ref}) == 4
    got = rp.prove_batch(groups, NQ, PW, device_witness=device_witness)
    assert len(got) == 4
    for i in range(4):
        assert got[i][0] == ref[i][0], f"proof {i} differs from prove()"
        assert got[i][1] == ref[i][1], f"public values {i} differ from prove()"
        assert rp.circuit.verify(got[i][0], NQ, PW, public=got[i][1]), (i, prover.last_reject)
        pref.verify_plonk(got[i][0], oracle, pos_consts=consts, public=got[i][1])
    # the buffer is reused: a smaller and a reordered call
    assert rp.prove_batch([groups[3], groups[1]], NQ, PW, device_witness=device_witness) == [ref[3], ref[1]]
    assert rp.prove_batch([groups[2]], NQ, PW, device_witness=device_witness) == [ref[2]]
    assert rp.prove_batch([], NQ, PW, device_witness=device_witness) == []


@pytest.mark.gpu
@pytest.mark.parametrize("device_witness", [False, True])
def test_reduce_with_batched_levels(prover, env, monkeypatch, device_witness):
    """fan-in 2 over 8 leaves: 4 -> 2 -> 1 nodes.  With prove_batch = 3 level 1 is cut into runs of 3 + 1 nodes, one on the main prover and one on
    the extra prover, level 2 is one run of 2 and the root goes through prove; with prove_batch = 0 (the code path before this feature) every
    node is its own prover call.  Same node proofs, same root proof, same key; the commitment is hashlib's."""
    vc = _mod(".verifier_circuit")
    _, extra, shapes = env
    mr, heights, roots, leaves = shapes[2]
    calls = []
    orig_batch, orig_placed = vc.RecursionProgram.prove_batch, vc.RecursionProgram.prove_placed

    def prove_batch(self, groups, *a, **kw):
        groups = list(groups)
        calls.append(("prove_batch", self.prover, len(groups)))
        return orig_batch(self, groups, *a, **kw)

    def prove_placed(self, slab, ids, *a, **kw):
        ids = list(ids)
        calls.append(("prove_placed", self.prover, len(ids)))
        return orig_placed(self, slab, ids, *a, **kw)
    monkeypatch.setattr(vc.RecursionProgram, "prove_batch", prove_batch)
    monkeypatch.setattr(vc.RecursionProgram, "prove_placed", prove_placed)
    res = {}
    try:
        mr.device_witness = device_witness
        for k in (0, 3):
            mr.prove_batch = k
            del calls[:]
            levels = []
            nodes, _, node_key, _ = mr.reduce(leaves, max_levels=1)
            root, public, key, _ = mr.reduce(leaves, levels)
            assert [lv["nodes"] for lv in levels] == [4, 2, 1]
            res[k] = (nodes, np.array(node_key), root, np.array(key), public)
            if k == 0:
                assert not calls
            else:
                outer = [c for c in calls if c[0] == ("prove_placed" if device_witness else "prove_batch")]
                # twice level 1 (the max_levels=1 call, then the whole fold): runs of 3 and 1 on two provers; once level 2: one run of 2
                assert sorted(c[2] for c in outer) == [1, 1, 2, 3, 3], calls
                assert {c[1] for c in outer if c[2] == 3} == {prover} and {c[1] for c in outer if c[2] == 1} == {extra}
        for a, b in zip(res[0], res[3]):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    finally:
        mr.prove_batch, mr.device_witness = 0, False
    lvl = [hashlib.sha256(b"\x00" + int(h).to_bytes(32, "big") + rr).digest() for h, rr in zip(heights, roots)]
    while len(lvl) > 1:
        lvl = [hashlib.sha256(b"\x01" + lvl[i] + lvl[i + 1]).digest() for i in range(0, len(lvl), 2)]
    root, key, public = res[3][2], res[3][3], res[3][4]
    assert b"".join(struct.pack(">I", v) for v in public[:8]) == lvl[0]
    assert mr.verify(root, key, heights, roots, lvl[0]), prover.last_reject


@pytest.mark.gpu
@pytest.mark.parametrize("device_witness", [False, True])
def test_tampered_child_in_the_second_run(prover, env, device_witness):
    """level 1 of 4 nodes with prove_batch = 3: node 3 is the second run (on the extra prover).  A child of it whose redundant word was flipped is
    refused with prove's own text and the node's position; nothing comes back; the same objects then fold the good leaves to the same root"""
    _, _, shapes = env
    mr, _, _, leaves = shapes[2]
    rp = level1_node(mr, leaves)
    prog = rp.program
    k, pos = (int(v) for v in prog.wc_var[prog.wc_var.shape[0] // 2, :2])
    bad_pair = flip_word(leaves[6:8], k, pos)
    with pytest.raises(ValueError) as host:
        rp.prove(bad_pair, NQ, PW)
    text = str(host.value)
    assert text == f"input {k}: word {pos} differs from the value the circuit derives"
    try:
        mr.prove_batch, mr.device_witness = 0, False
        want = mr.reduce(leaves)
        mr.prove_batch, mr.device_witness = 3, device_witness
        got = None
        with pytest.raises(ValueError) as e:
            got = mr.reduce(leaves[:6] + bad_pair)
        assert got is None and str(e.value) == f"instance 3: {text}"
        # RecursionProgram.prove_batch itself: the instance within the call
        with pytest.raises(ValueError) as e:
            got = rp.prove_batch([leaves[0:2], bad_pair, leaves[2:4]], NQ, PW, device_witness=device_witness)
        assert got is None and str(e.value) == f"instance 1: {text}"
        with pytest.raises(ValueError) as e:
            got = rp.prove_batch([bad_pair], NQ, PW, device_witness=device_witness)
        assert got is None and str(e.value) == text
        again = mr.reduce(leaves)
        assert again[0] == want[0] and again[1] == want[1] and np.array_equal(again[2], want[2])
    finally:
        mr.prove_batch, mr.device_witness = 0, False


@pytest.mark.gpu
def test_map_places_each_group_with_one_call(prover, env):
    """the Map step with device witnesses and prove_batch = 3: each group through device_witness_batch; the leaf proofs of the unbatched Map"""
    _, _, shapes = env
    mr, heights, roots, leaves = shapes[2]
    prog = mr.leaf_program
    try:
        mr.prove_batch, mr.device_witness = 3, True
        assert mr.prove_leaves(heights, roots) == leaves
        # the main prover's last group: placement, Poseidon rows (the tuples' digest), SHA rows, public values; one synchronise
        assert prover.witness_last_place_counts() == (2 + bool(prog.pos_row_ids.size) + bool(prog.sha_row_ids.size), 1)
    finally:
        mr.prove_batch, mr.device_witness = 0, False


@pytest.mark.gpu
def test_cpp_host_places_and_proves_two_instances(pkg, prover, env, tmp_path):
    """tests/cpp/host_place.cpp (g++, C ABI only) on the exported leaf recording: layout create -> glp_witness_eval_device -> glp_witness_place_batch
    (slab rows {1, 0}) -> glp_plonk_prove_batch; both proofs accepted by glp_plonk_verify_ex there, and here they are the Map step's proofs of
    those two leaves byte for byte"""
    dm = _mod(".data_commitment_mr")
    consts, _, shapes = env
    mr, heights, roots, leaves = shapes[2]
    mr.leaf_program.export_raw(str(tmp_path / "leaf"))
    np.array(leaf_inputs(dm, heights, roots, 4, 2), dtype="<u8").tofile(str(tmp_path / "inputs.bin"))
    np.concatenate([np.asarray(a, dtype=np.uint64) for a in consts]).astype("<u8").tofile(str(tmp_path / "pc.bin"))
    exe = tmp_path / "host_place"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_place.cpp"),
                    "-o", str(exe), "-L", libdir, "-lglprover", "-pthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe), str(tmp_path / "pc.bin"), str(NQ), str(PW), str(tmp_path / "leaf"), str(tmp_path / "inputs.bin"), str(tmp_path / "proof")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout
    prog = mr.leaf_program
    n_launches = 2 + bool(prog.pos_row_ids.size) + bool(prog.sha_row_ids.size)     # placement, Poseidon rows (the digest), SHA rows, public values
    assert f"place launches {n_launches} syncs 1" in r.stdout and n_launches <= 4, r.stdout
    lines = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines() if " " in ln)
    assert int(lines["key0"]) == int(mr.leaf_circuit.cap()[0])
    for i, leaf in enumerate((5, 4)):                                             # instance i is slab row 1 - i
        proof = (tmp_path / f"proof{i}.bin").read_bytes()
        assert proof == leaves[leaf], f"instance {i} is not the Map step's proof of leaf {leaf}"
        public = [int(v) for v in lines[f"public{i}"].split()]
        assert public == [int(v) for v in pkg.proof_public_inputs(proof)]
        assert mr.leaf_circuit.verify(proof, NQ, PW, public=public), prover.last_reject
