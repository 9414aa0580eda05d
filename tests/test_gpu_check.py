"""glp_plonk_check_witness / glp_plonk_check_witness_batch on the GPU against the reference (tests/check_ref.py) word for word: status,
summary, list, values and peers.  Shapes are the smallest at which each part can go wrong; which test launches which kernel:
tests/GPU_COVERAGE_CHECK.md.  A satisfied witness must also PROVE (from the same device buffer) and verify; a witness the checker refuses must
not — the checker's verdict is the verifier's."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_ref as cref  # noqa: E402
import fri_verifier as fv  # noqa: E402
import plonk_ref as pref  # noqa: E402
from conftest import P, poseidon_consts, ptr, root_of_unity  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def use_consts(prover, kind):
    rc, circ, diag = consts = poseidon_consts(kind)
    prover.set_poseidon_constants(rc, circ, diag)
    return consts


def make_key(pkg, prover, circ, sigmas=None):
    return pkg.PlonkCircuit(prover, circ["consts"], circ["sigmas"] if sigmas is None else sigmas, n_wires=circ["W"], n_public=circ["n_public"],
                            poseidon=bool(circ["flags"] & pref.FLAG_POSEIDON), sha=bool(circ["flags"] & pref.FLAG_SHA),
                            ext=bool(circ["flags"] & pref.FLAG_EXT))


def all_kinds_circuit(consts, seed=3):
    """6/144/24 with Poseidon, SHA (all four kinds), extension and arithmetic rows and two public inputs"""
    circ = pref.build_circuit(np.random.default_rng(seed), 6, 144, n_routed=24, n_public=2, poseidon_rows=range(10, 16), consts=consts,
                              sha_rows=range(20, 44), ext_rows=range(50, 56))
    assert sorted(set(cref.sha_kinds(circ).values())) == [0, 1, 2, 3]
    return circ


def as_ref(res):
    return res.summary, res.violations


# ---- satisfied circuits -------------------------------------------------------------------------------------------------------------------------
def satisfied_case(name, consts):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "3-8-8":                      # one chunk, fewer rows than a wavefront
        return pref.build_circuit(rng, 3, 8)
    if name == "13-16-8-pub2":               # advice wires, indices beyond the 4096-entry first-level root table
        return pref.build_circuit(rng, 13, 16, n_routed=8, n_public=2)
    if name == "6-136-24-poseidon-small":
        return pref.build_circuit(rng, 6, 136, n_routed=24, poseidon_rows=range(5, 25), consts=consts)
    if name == "6-160-136-poseidon-big":
        return pref.build_circuit(rng, 6, 160, n_routed=136, n_public=2, poseidon_rows=range(5, 14), consts=consts)
    if name == "6-144-16-sha":
        circ = pref.build_circuit(rng, 6, 144, n_routed=16, sha_rows=range(8, 40))
        assert sorted(set(cref.sha_kinds(circ).values())) == [0, 1, 2, 3]
        return circ
    if name == "6-144-24-all":
        return all_kinds_circuit(consts)
    if name == "5-8-8-pub-n":                # n_public = n
        return pref.build_circuit(rng, 5, 8, n_public=32)
    raise KeyError(name)


@pytest.mark.parametrize("name,kind", [("3-8-8", "small"), ("13-16-8-pub2", "small"), ("6-136-24-poseidon-small", "small"),
                                       ("6-160-136-poseidon-big", "big"), ("6-144-16-sha", "small"), ("6-144-24-all", "small"),
                                       ("5-8-8-pub-n", "small")])
def test_satisfied_circuit_passes_and_proves(pkg, prover, name, kind):
    try:
        consts = use_consts(prover, kind)
        circ = satisfied_case(name, consts)
        assert cref.check(circ)[1] == []
        ck = make_key(pkg, prover, circ)
        dw = prover.to_device(circ["wires"])
        res = ck.check_(dw, circ["public"])
        assert res.ok and res.violations == [] and not any(res.summary.values()), res
        first = prover.plonk_last_check_counts()
        again = ck.check_(dw, circ["public"])
        assert again.ok
        later = prover.plonk_last_check_counts()
        n_kernels = 2 + bool(circ["flags"] & pref.FLAG_POSEIDON) + bool(circ["flags"] & pref.FLAG_SHA)
        assert first == (2 + 1 + n_kernels, 1) and later == (1 + n_kernels, 1)     # the decode happens once per key
        proof = ck.prove_(dw, 28, 16, public=circ["public"])
        assert ck.verify(proof, public=circ["public"] if circ["n_public"] else None), prover.last_reject
        dw.free()
        ck.free()
    finally:
        use_consts(prover, "small")


# ---- one mutation per constraint, batched ---------------------------------------------------------------------------------------------------------
def run_batch(pkg, prover, circ, wires_list, publics=None, max_list=8):
    """every instance of ONE check_batch_ call against the reference; returns the product's results"""
    ck = make_key(pkg, prover, circ)
    bufs = [prover.to_device(w) for w in wires_list]
    publics = [circ["public"]] * len(bufs) if publics is None else publics
    try:
        got = ck.check_batch_(bufs, publics if circ["n_public"] else None, max_list=max_list)
    finally:
        for b in bufs:
            b.free()
        ck.free()
    rc = cref.RefChecker(circ)
    for b, w in enumerate(wires_list):
        summary, lst = rc.check(w, publics[b], max_list)
        assert as_ref(got[b]) == (summary, lst), (b, got[b], summary, lst[:2])
        assert got[b].ok == (not lst)
    return got


@pytest.mark.parametrize("kind", ["small", "big"])
def test_poseidon_constraints_one_mutation_each(pkg, prover, kind):
    """6/160/136: B = 123, instance k alters the wire Poseidon constraint k pins; one call; every first index reported, every list the reference's.
    On both MDS kinds: "small" runs glp_check_poseidon_kernel<true>, "big" (random 64-bit entries) the generic glp_check_poseidon_kernel<false>"""
    try:
        consts = use_consts(prover, kind)
        circ = pref.build_circuit(np.random.default_rng(61), 6, 160, n_routed=136, n_public=2, poseidon_rows=range(5, 14), consts=consts)
        M = circ["R"] // 8
        wires = []
        for k in range(pref.POS_CONSTRAINTS):
            wire, val = cref.poseidon_target(k)
            wires.append(cref.mutate(circ["wires"], 5 + k % 9, wire, val))
        got = run_batch(pkg, prover, circ, wires)
        firsts = [next(v["index"] for v in r.violations if v["kind"] == cref.GATE) for r in got]
        assert firsts == [2 + 3 * M + k for k in range(pref.POS_CONSTRAINTS)]
    finally:
        use_consts(prover, "small")


def test_sha_constraints_one_mutation_each(pkg, prover):
    """6/144/16: B = 140, per kind the bit or carry wire of each boolean slot, and a routed word of each packed-word slot"""
    use_consts(prover, "small")
    circ = satisfied_case("6-144-16-sha", None)
    kinds = cref.sha_kinds(circ)
    wires = [cref.mutate(circ["wires"], *cref.sha_target(k, kinds)) for k in range(pref.SHA_CONSTRAINTS)]
    got = run_batch(pkg, prover, circ, wires)
    firsts = [next(v["index"] for v in r.violations if v["kind"] == cref.GATE) for r in got]
    assert firsts == [2 + 3 * (circ["R"] // 8) + k for k in range(pref.SHA_CONSTRAINTS)]


def test_arithmetic_extension_and_public_slots(pkg, prover):
    """6/144/24 with every row kind: both slots of every chunk on an arithmetic row and on an extension row, and the public-input row"""
    consts = use_consts(prover, "small")
    circ = all_kinds_circuit(consts)
    n, M = 1 << circ["log_n"], circ["R"] // 8
    arith = next(i for i in range(circ["n_public"], n) if int(circ["consts"][0][i]))
    ext = next(i for i in range(n) if int(circ["consts"][-1][i]))
    wires, want = [], []
    for c in range(M):
        for row, w0, w1 in ((arith, 8 * c + 3, 8 * c + 7), (ext, 8 * c + 6, 8 * c + 7)):
            wires += [cref.mutate(circ["wires"], row, w0), cref.mutate(circ["wires"], row, w1)]
            want += [(row, 3 + 3 * c), (row, 4 + 3 * c)]
    wires.append(cref.mutate(circ["wires"], 1, 0))
    want.append((1, 1))
    got = run_batch(pkg, prover, circ, wires)
    assert [next((v["row"], v["index"]) for v in r.violations if v["kind"] == cref.GATE) for r in got] == want
    # the statement, not the witness, off by one word: the same constraint
    other = list(circ["public"])
    other[0] = (other[0] + 5) % P
    got = run_batch(pkg, prover, circ, [circ["wires"]], publics=[other])
    assert got[0].violations[0]["row"] == 0 and got[0].violations[0]["index"] == 1


# ---- copy constraints ------------------------------------------------------------------------------------------------------------------------------
def test_copy_constraints_name_the_cycle_edges(pkg, prover):
    use_consts(prover, "small")
    circ = pref.build_circuit(np.random.default_rng(13), 13, 16, n_routed=8, n_public=2)
    n, R = 1 << 13, 8
    rc = cref.RefChecker(circ)
    cells = rc.cells
    q = [int(v) for v in circ["consts"][0]]
    # a member of a copy class of three or more cells whose cycle neighbours sit in other rows, on a row whose gates do not read it (q = 0)
    pred = {cells[j][i]: (j, i) for j in range(R) for i in range(n)}
    cell = next((j, i) for i in range(2, n) for j in range(R) if not q[i] and cells[j][i] != (j, i) and cells[cells[j][i][0]][cells[j][i][1]] != (j, i)
                and cells[j][i][1] != i and pred[(j, i)][1] != i)
    j, i = cell
    bad = cref.mutate(circ["wires"], i, j)
    summary, lst = rc.check(bad, circ["public"])
    assert summary["n_copy_bad"] == 2 and summary["n_gate_bad"] == 0 and sorted(v["row"] for v in lst) == sorted([i, pred[cell][1]])
    # harmless: an advice cell, and an arithmetic cell on a q = 0 row that belongs to no class
    lone = next((jj, ii) for ii in range(2, n) for jj in range(R) if not q[ii] and cells[jj][ii] == (jj, ii) and pred[(jj, ii)] == (jj, ii))
    ok1 = cref.mutate(circ["wires"], 77, R + 3)
    ok2 = cref.mutate(circ["wires"], lone[1], lone[0])
    assert rc.check(ok1, circ["public"])[1] == [] and rc.check(ok2, circ["public"])[1] == []
    got = run_batch(pkg, prover, circ, [bad, ok1, ok2], max_list=4)
    assert [r.ok for r in got] == [False, True, True]
    e = {v["row"]: v for v in got[0].violations}
    assert e[i]["index"] == j and (e[i]["peer_wire"], e[i]["peer_row"]) == cells[j][i] and e[i]["value"] == int(bad[j, i])
    pj, pi = pred[cell]
    assert e[pi]["index"] == pj and (e[pi]["peer_wire"], e[pi]["peer_row"]) == cell and e[pi]["peer_value"] == int(bad[j, i])
    ck = make_key(pkg, prover, circ)
    for w in (ok1, ok2):
        proof = ck.prove(w, 28, 16, public=circ["public"])
        assert ck.verify(proof, public=circ["public"]), prover.last_reject
    ck.free()


# ---- the checker's verdict is the verifier's ------------------------------------------------------------------------------------------------------
def seeded_mutations(circ, count=40, seed=2026):
    rng = np.random.default_rng(seed)
    n, W, R = 1 << circ["log_n"], circ["W"], circ["R"]
    out = []
    for _ in range(count):
        j = int(rng.integers(0, R)) if rng.random() < 0.6 else int(rng.integers(R, W))     # routed cells mostly bind, advice cells mostly do not
        out.append(cref.mutate(circ["wires"], int(rng.integers(0, n)), j))
    return out


def test_verdict_equals_verifier(pkg, prover):
    """40 seeded single-cell mutations of a 6/144/24 circuit with all row kinds: check says OK exactly when the reference does, and the proof
    made from that witness verifies exactly in those cases"""
    consts = use_consts(prover, "small")
    circ = all_kinds_circuit(consts)
    rc = cref.RefChecker(circ)
    muts = seeded_mutations(circ)
    want = [rc.check(w, circ["public"], 4) for w in muts]
    harmless = sum(1 for _, lst in want if not lst)
    assert harmless >= 5 and len(muts) - harmless >= 25, harmless
    ck = make_key(pkg, prover, circ)
    for w, (summary, lst) in zip(muts, want):
        dw = prover.to_device(w)
        res = ck.check_(dw, circ["public"], max_list=4)
        assert as_ref(res) == (summary, lst) and res.ok == (not lst)
        proof = ck.prove_(dw, 28, 16, public=circ["public"])
        assert bool(ck.verify(proof, public=circ["public"])) == res.ok, (res, prover.last_reject)
        dw.free()
    ck.free()


# ---- batch plumbing -----------------------------------------------------------------------------------------------------------------------------------
SENT32, SENT64 = 0x5E5E5E5E, 0x5E5E5E5E5E5E5E5E


def raw_batch(pkg, prover, ck, bufs, publics, max_list):
    """glp_plonk_check_witness_batch through ctypes with a sentinel behind every output array"""
    B = len(bufs)
    status = (ctypes.c_int32 * (B + 1))()
    sums = (pkg.CheckSummary * (B + 1))()
    lists = (pkg.CheckViolation * (B * max_list + 1))()
    status[B] = 0x5E5E5E5
    sums[B].n_gate_bad, sums[B].n_listed = SENT64, SENT32
    lists[B * max_list].kind, lists[B * max_list].value = SENT32, SENT64
    pub = np.ascontiguousarray(publics, dtype=np.uint64) if ck.n_public else None
    ptrs = (ctypes.c_void_p * B)(*[b.ptr for b in bufs])
    rc = prover.lib.glp_plonk_check_witness_batch(prover.ctx, ck.h, ptrs, pub.ctypes.data if pub is not None else None, B, status, sums, lists, max_list)
    assert rc == 0, prover.lib.glp_last_error(prover.ctx)
    assert status[B] == 0x5E5E5E5 and sums[B].n_gate_bad == SENT64 and sums[B].n_listed == SENT32
    assert lists[B * max_list].kind == SENT32 and lists[B * max_list].value == SENT64
    return [(status[b], sums[b].as_dict(), [lists[b * max_list + k].as_dict() for k in range(sums[b].n_listed)]) for b in range(B)]


def test_batch_plumbing(pkg, prover):
    consts = use_consts(prover, "small")
    circ = all_kinds_circuit(consts)
    n = 1 << circ["log_n"]
    rc = cref.RefChecker(circ)
    arith = [i for i in range(circ["n_public"], n) if int(circ["consts"][0][i])]
    good = circ["wires"]
    bads = [cref.mutate(good, arith[0], 3), cref.mutate(good, arith[1], 7), cref.mutate(good, 12, 30)]       # distinct rows and constraints
    ck = make_key(pkg, prover, circ)
    bufs = {id(w): prover.to_device(w) for w in [good] + bads}
    assert ck.check_(bufs[id(good)], circ["public"]).ok           # the key's first check decodes sigma: two more launches, once
    counts = {}
    for label, insts in (("mixed", [good, bads[0], good]), ("all-bad", bads)):
        for B in (1, 2, 3):
            ws = insts[:B]
            got = raw_batch(pkg, prover, ck, [bufs[id(w)] for w in ws], [circ["public"]] * B, 5)
            counts[(label, B)] = prover.plonk_last_check_counts()
            for b, w in enumerate(ws):
                summary, lst = rc.check(w, circ["public"], 5)
                assert got[b] == (-7 if lst else 0, summary, lst), (label, B, b)
    assert counts[("mixed", 1)] == counts[("mixed", 3)] == counts[("all-bad", 1)] == counts[("all-bad", 3)] == (5, 1), counts
    # two pointers to the same matrix, and the single form on the same buffers
    got = raw_batch(pkg, prover, ck, [bufs[id(bads[1])], bufs[id(bads[1])]], [circ["public"]] * 2, 5)
    assert got[0] == got[1] and got[0][0] == -7
    res = ck.check_(bufs[id(bads[2])], circ["public"])
    assert not res.ok and as_ref(res) == rc.check(bads[2], circ["public"], 16)
    msg = prover.lib.glp_last_error(prover.ctx).decode()
    assert f"row {res.violations[0]['row']}" in msg and f"constraint {res.violations[0]['index']}" in msg, msg
    assert ck.check_batch_([]) == []
    with pytest.raises(pkg.GlpError, match="instance 1"):
        ck.check_batch_([bufs[id(good)], 0], [circ["public"]] * 2)
    for b in bufs.values():
        b.free()
    ck.free()


# ---- keys whose sigma is no permutation of the routed cells -------------------------------------------------------------------------------------------
def bad_key_circuit(w=None):
    """6/16/8; w: store sigma on that root of unity (a build with another two-adic generator) instead of the generator-7 one"""
    circ = pref.build_circuit(np.random.default_rng(5), 6, 16, n_routed=8)
    if w is not None:
        circ = dict(circ, sigmas=np.array(cref.encode_sigma(cref.decode_sigma(circ["sigmas"], 6), 6, w), dtype=np.uint64))
    return circ


def refuse_bad_keys(pkg, prover, circ, w=None):
    """one sigma value replaced by a point off the domain, by a point of a coset that is not routed, and two cells sent to one target: each
    GLP_E_INVALID with the cell the reference names; then the untouched key passes, and a mutated witness gives the reference's list"""
    dom = cref.domain(6, 8, w)
    off = next(v for v in ((int(circ["sigmas"][2, 9]) + d) % P for d in range(1, 50)) if v not in dom)
    for cell, value, what in (((2, 9), off, "no routed cell"), ((1, 4), pow(7, 8, P), "no routed cell"), ((3, 7), None, "no permutation")):
        sig = circ["sigmas"].copy()
        sig[cell] = sig[0, 20] if value is None else value
        if value is None:
            assert sig[cell] != circ["sigmas"][cell]
        with pytest.raises(cref.SigmaError) as ref_err:
            cref.decode_sigma(sig, 6, w)
        ck = make_key(pkg, prover, circ, sigmas=sig)
        for _ in range(2):                       # a key that does not decode keeps no table: the second call says the same
            with pytest.raises(pkg.GlpError, match="GLP_E_INVALID") as err:
                ck.check(circ["wires"])
            assert what in str(err.value)
            named = str(err.value).split("(wire ")[1].split(")")[0].replace(" row ", " ")
            j, i = (int(x) for x in named.split(","))
            assert f"wire {j}, row {i}" in str(ref_err.value), (str(err.value), str(ref_err.value))
        ck.free()
    ck = make_key(pkg, prover, circ)
    assert ck.check(circ["wires"]).ok
    row = next(i for i in range(64) if int(circ["consts"][0][i]))
    bad_w = cref.mutate(circ["wires"], row, 3)
    bad = ck.check(bad_w)
    assert not bad.ok and as_ref(bad) == cref.RefChecker(circ, w=w).check(bad_w, [], 16)
    ck.free()


def test_bad_keys_are_refused_with_the_cell_named(pkg, prover):
    use_consts(prover, "small")
    refuse_bad_keys(pkg, prover, bad_key_circuit())


# ---- the opt-in keyword of the MapReduce classes ----------------------------------------------------------------------------------------------------------
def test_check_witness_keyword_of_the_data_commitment_mapreduce(pkg, prover):
    """the smallest range (two one-block leaves, one node of two): with check_witness the proofs are byte for byte those of the unchecked path;
    one corrupted cell of one placed leaf raises ValueError naming that leaf and row — on the single and on the batched Map path"""
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    consts = use_consts(prover, "small")
    rng = np.random.default_rng(77)
    heights = [5_000_000, 5_000_001]
    roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
    kw = dict(leaf_blocks=1, fan_in=2, num_queries=6, pow_bits=4)
    off = dm.DataCommitmentMapReduce(prover, consts, **kw)
    want = off.prove_range(heights, roots)
    want_leaves = off.prove_leaves(heights, roots)
    off.free()
    for batch in (0, 2):
        on = dm.DataCommitmentMapReduce(prover, consts, check_witness=True, prove_batch=batch, **kw)
        seen = []
        on._placed_hook = lambda p, addr, leaf: seen.append(leaf)
        got = on.prove_range(heights, roots)
        assert got["root_proof"] == want["root_proof"] and on.prove_leaves(heights, roots) == want_leaves
        assert seen == [0, 1, 0, 1]
        assert prover.plonk_last_check_counts()[1] == 1
        # cell (wire 0, row 0) of leaf 1, as placed, off by one: row 0 exposes wire 0 as the first public input
        assert on.leaf_circuit.n_public > 0

        def corrupt(p, addr, leaf):
            if leaf == 1:
                word = np.zeros(1, dtype=np.uint64)
                p._chk(p.lib.glp_d2h(p.ctx, word.ctypes.data, addr, 8), "glp_d2h")
                word[0] = (int(word[0]) + 1) % P
                p._chk(p.lib.glp_h2d(p.ctx, addr, word.ctypes.data, 8), "glp_h2d")
        on._placed_hook = corrupt
        with pytest.raises(ValueError, match=r"check_witness: leaf 1: witness not satisfied: row 0, kind gate, index 1 "):
            on.prove_leaves(heights, roots)
        on._placed_hook = None
        assert on.prove_leaves(heights, roots) == want_leaves
        on.free()


def test_check_witness_names_a_failing_node(pkg, prover, monkeypatch):
    """four one-block leaves, fan-in 2, prove_batch = 1: level 1 has two nodes, each a run of its own, so the second run starts at node 1.  One
    cell of that node's PLACED witness is corrupted (the node program's placement wrapped): ValueError names level 1, node 1, the row, the kind
    and the index, and nothing of the level is returned; unwrapped, the object folds the same leaves to the same root as before"""
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    consts = use_consts(prover, "small")
    rng = np.random.default_rng(78)
    heights = [6_000_000 + k for k in range(4)]
    roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
    kw = dict(leaf_blocks=1, fan_in=2, num_queries=6, pow_bits=4, prove_batch=1)
    on = dm.DataCommitmentMapReduce(prover, consts, check_witness=True, **kw)
    leaves = on.prove_leaves(heights, roots)
    want_root = on.reduce(leaves)[0]                 # every node witness checked and satisfied (records the node circuits)
    rp = next(v for k, v in on.nodes.items() if k[0] == 1)
    place, calls = rp.program.device_witness, []

    def corrupting(p, vals, **kwargs):
        out = place(p, vals, **kwargs)
        calls.append(kwargs.get("out"))
        if len(calls) == 2:                          # the second node of level 1: cell (wire 0, row 0), its first public input
            addr = kwargs["out"]
            word = np.zeros(1, dtype=np.uint64)
            p._chk(p.lib.glp_d2h(p.ctx, word.ctypes.data, addr, 8), "glp_d2h")
            word[0] = (int(word[0]) + 1) % P
            p._chk(p.lib.glp_h2d(p.ctx, addr, word.ctypes.data, 8), "glp_h2d")
        return out
    monkeypatch.setattr(rp.program, "device_witness", corrupting)
    with pytest.raises(ValueError, match=r"^check_witness: level 1 node 1: witness not satisfied: row 0, kind gate, index 1 "):
        on.reduce(leaves)
    assert len(calls) == 2 and all(isinstance(a, int) for a in calls)
    monkeypatch.undo()
    assert on.reduce(leaves)[0] == want_root
    on.free()


# ---- the library built on the alternative two-adic generator decodes its own circuits ------------------------------------------------------------------
def altgen_child():
    """runs in a child process with GLP_LIB = lib/libglprover_altgen.so: the same routing, sigma stored on that build's roots of unity"""
    pkg = graft.load_package()
    assert pkg.field_params()[0] != pow(7, (P - 1) >> 32, P)
    prover = pkg.Prover(0)
    rc_, circ_, diag_ = poseidon_consts("small")
    prover.set_poseidon_constants(rc_, circ_, diag_)
    circ = pref.build_circuit(np.random.default_rng(9), 13, 16, n_routed=8, n_public=2)
    w = root_of_unity(13)
    assert w != fv.root(13)
    cells = cref.decode_sigma(circ["sigmas"], 13)
    alt = dict(circ, sigmas=np.array(cref.encode_sigma(cells, 13, w), dtype=np.uint64))
    ref = cref.RefChecker(alt, w=w)
    ck = make_key(pkg, prover, alt)
    good = ck.check(alt["wires"], alt["public"])
    assert good.ok, good
    q = [int(v) for v in alt["consts"][0]]
    row = next(i for i in range(5000, 1 << 13) if q[i])
    bad_w = cref.mutate(alt["wires"], row, 2)
    bad = ck.check(bad_w, alt["public"])
    assert not bad.ok and (bad.summary, bad.violations) == ref.check(bad_w, alt["public"], 16)
    proof = ck.prove(alt["wires"], 28, 16, public=alt["public"])
    assert ck.verify(proof, public=alt["public"]), prover.last_reject
    ck.free()
    # the circuit of the bad-key test, on this build's roots: the same refusals, the same cells named
    w6 = root_of_unity(6)
    assert w6 != fv.root(6)
    refuse_bad_keys(pkg, prover, bad_key_circuit(w6), w6)
    prover.close()
    print("altgen child ok")


def test_altgen_library_decodes_its_own_circuits():
    alt = os.path.join(os.path.dirname(HERE), graft.PKG_NAME, "lib", "libglprover_altgen.so")
    assert not os.environ.get("GLP_LIB"), "this test selects the library itself"
    assert os.path.exists(alt), "lib/libglprover_altgen.so is not built (__graft_entry__.build() does it)"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "altgen-child"], env=dict(os.environ, GLP_LIB=alt), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, cwd=os.path.dirname(HERE), timeout=300)
    assert r.returncode == 0 and "altgen child ok" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__" and sys.argv[1:] == ["altgen-child"]:
    altgen_child()
