"""glp_plonk_verify_batch / glp_fri_verify_batch on the GPU: B proofs per call, their query phases as device work items
(csrc/verify_batch_kernels.cuh).  The expected value of every comparison is the SINGLE verifier on the same bytes
(glp_plonk_verify_host_ex / glp_fri_verify_host_ex: status and reason text; the failing query from the single verifier's code as
tests/emu_verify_batch exposes it), never the code under test."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_ref as pref  # noqa: E402
import verify_batch_cases as vbc  # noqa: E402
from conftest import poseidon_consts, rand_field  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = vbc.NAMES
LAUNCH_BUDGET, SYNC_BUDGET = 2, 1            # include/glprover.h: per chunk, and one chunk holds 2^30 Merkle items


@pytest.fixture(scope="module")
def consts():
    return tuple(np.ascontiguousarray(a, dtype=np.uint64) for a in poseidon_consts("small"))


@pytest.fixture(scope="module")
def pr(prover, consts):
    prover.set_poseidon_constants(*consts)
    return prover


def single(pkg, consts, proof, cap, mq, mp, public=None):
    """(ok, reason text) of the single host verifier for a circuit proof"""
    ok, why = pkg.plonk_verify_host(consts, proof, cap, mq, mp, public=pkg.UNBOUND if public is None else public)
    return ok, None if ok else why[len("proof rejected: "):]


def fri_single(pkg, consts, proof, mq, mp, mr=1):
    ok, why = pkg.fri_verify_host(consts, proof, mq, mp, mr)
    return ok, None if ok else why[len("proof rejected: "):]


def tamper_last_leaf(proof, plonk=True):
    w = np.frombuffer(proof, dtype="<u8").copy()
    w[vbc.layout(w, plonk)["last_leaf"]] ^= np.uint64(1)
    return w.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_golden_corpus_in_one_call(pkg, pr, consts, name):
    """every case of a golden proof's corpus in ONE batched call, word for word against the single verifier"""
    lib = pkg.load_library()
    cases, prm = vbc.corpus(name)
    expected = vbc.single_expected(lib, consts, cases, prm)
    b = vbc.Batch(cases)
    if prm["plonk"]:
        code = lib.glp_plonk_verify_batch(pr.ctx, b.ptrs, b.lens, b.n, prm["cap"].ctypes.data, prm["cap"].size, None, 0, prm["min_queries"],
                                          prm["min_pow_bits"], b.verdicts, b.digests.ctypes.data)
    else:
        code = lib.glp_fri_verify_batch(pr.ctx, b.ptrs, b.lens, b.n, prm["min_queries"], prm["min_pow_bits"], prm["min_rate_bits"], b.verdicts, None)
    assert code == 0, pr.lib.glp_last_error(pr.ctx)
    counts = pr.verify_last_batch_counts()
    print(name, len(cases), "cases", counts)
    assert counts["launches"] == LAUNCH_BUDGET and counts["host_syncs"] == SYNC_BUDGET
    bad = []
    for k, (label, w, hdr) in enumerate(cases):
        v = b.verdicts[k]
        got = (int(v.status), None if v.status == 0 else lib.glp_verify_reason_text(v.reason).decode())
        if got != expected[k]:
            bad.append((label, got, expected[k]))
    assert not bad, f"{len(bad)} of {len(cases)} verdicts differ from the single verifier's, first: {bad[:5]}"
    assert b.verdicts[0].status == 0 and b.verdicts[0].on_device == 1
    # the failing query: the single verifier's own numbers (its code as tests/emu_verify_batch exposes it: the C ABI carries no query)
    queries = vbc.single_queries(vbc.load_single_verifier(), consts, cases, prm)
    for k in range(b.n):
        assert (queries[k][0], lib.glp_verify_reason_text(queries[k][1]).decode() or None) == expected[k], cases[k][0]
        assert b.verdicts[k].query == queries[k][2], (cases[k][0], b.verdicts[k].query, queries[k][2])
    if prm["plonk"]:
        for k in range(0, b.n, 97):
            try:
                want = pkg.proof_digest_host(consts, cases[k][1].tobytes())
            except Exception:  # noqa: BLE001 — the header does not parse: the batched call leaves zeros
                want = [0, 0, 0, 0]
            assert [int(x) for x in b.digests[k]] == [int(x) for x in want], cases[k][0]
    # no fallback for the untampered proof and for every tamper outside the header words: the same corpus without its header cases, once more
    body = [c for c in cases if not c[2]]
    bb = vbc.Batch(body)
    if prm["plonk"]:
        assert lib.glp_plonk_verify_batch(pr.ctx, bb.ptrs, bb.lens, bb.n, prm["cap"].ctypes.data, prm["cap"].size, None, 0, prm["min_queries"],
                                          prm["min_pow_bits"], bb.verdicts, None) == 0
    else:
        assert lib.glp_fri_verify_batch(pr.ctx, bb.ptrs, bb.lens, bb.n, prm["min_queries"], prm["min_pow_bits"], prm["min_rate_bits"], bb.verdicts, None) == 0
    c2 = pr.verify_last_batch_counts()
    assert c2["fallback"] == 0 and c2["on_device"] == sum(1 for k in range(bb.n) if bb.verdicts[k].on_device) > len(body) // 2
    assert (c2["launches"], c2["host_syncs"]) == (LAUNCH_BUDGET, SYNC_BUDGET)


def circuit_proofs(pkg, pr, consts):
    """fresh proofs from the GPU prover: [(name, proof, cap, public, queries, pow_bits)]"""
    out = []
    for log_n in (3, 9, 13):
        c = pref.build_circuit(np.random.default_rng(100 + log_n), log_n, 8)
        ck = pkg.PlonkCircuit(pr, c["consts"], c["sigmas"])
        out.append((f"w8-{log_n}", ck.prove(c["wires"], 5, 2), ck.cap(), [], 5, 2))
        ck.free()
    g = pref.build_circuit(np.random.default_rng(7), 9, 136, n_routed=24, n_public=2, poseidon_rows=[3, 17, 18, 300], consts=consts)
    gk = pkg.PlonkCircuit(pr, g["consts"], g["sigmas"], n_wires=136, n_public=2, poseidon=True)
    out.append(("poseidon-9", gk.prove(g["wires"], 4, 2, public=g["public"]), gk.cap(), [int(v) for v in g["public"]], 4, 2))
    gk.free()
    h = pref.build_circuit(np.random.default_rng(8), 9, 144, n_routed=24, n_public=1, poseidon_rows=[2], consts=consts,
                           sha_rows=[3, 4, 5, 6, 9, 10, 11, 12, 20, 21, 22, 30, 400])
    hk = pkg.PlonkCircuit(pr, h["consts"], h["sigmas"], n_wires=144, n_public=1, poseidon=True, sha=True)
    out.append(("sha-9", hk.prove(h["wires"], 4, 2, public=h["public"]), hk.cap(), [int(v) for v in h["public"]], 4, 2))
    hk.free()
    return out


@pytest.fixture(scope="module")
def fresh(pkg, pr, consts):
    return circuit_proofs(pkg, pr, consts)


def test_fresh_circuit_proofs_and_last_leaf_tamper(pkg, pr, consts, fresh):
    """W = 8 at log_n 3 (no layer), 9 (one), 13 (two layers at 16-to-1), a Poseidon-row and a SHA-row circuit: accepted; with the LAST
    query's last leaf tampered: the single verifier's reason and query"""
    for name, proof, cap, pub, q, pw in fresh:
        bad = tamper_last_leaf(proof)
        res = pr.plonk_verify_batch([proof, bad, proof], cap, q, pw, publics=[pub, pub, pub])
        want = single(pkg, consts, bad, cap, q, pw, public=pub)
        assert single(pkg, consts, proof, cap, q, pw, public=pub) == (True, None), name
        assert res[0] == (True, None, None) and res[2] == (True, None, None), (name, res)
        assert not want[0] and res[1] == (False, want[1], q - 1), (name, res, want)
        assert pr.verify_last_batch_counts() == {"launches": LAUNCH_BUDGET, "host_syncs": SYNC_BUDGET, "on_device": 3, "fallback": 0}
    L = {name: (np.frombuffer(p, dtype="<u8")) for name, p, *_ in fresh}
    assert len(L["w8-13"]) > len(L["w8-9"]) > len(L["w8-3"])


def fri_proofs(pkg, pr):
    """stand-alone FRI proofs: [(name, proof, queries, pow_bits)]"""
    out = []
    rng = np.random.default_rng(31)

    def mk(name, log_n, polys, cap_h, arity, fpb, mults=(1,), masks=None, q=5):
        batches = [pkg.PolynomialBatch.from_values(pr, rand_field(rng, (k, 1 << log_n)), 3, cap_h) for k in polys]
        out.append((name, pr.fri_prove(batches, 3, cap_h, arity_bits=arity, final_poly_bits=fpb, num_queries=q, pow_bits=2, point_mults=mults,
                                       open_masks=masks), q, 2))
        for b in batches:
            b.free()

    mk("arity1", 7, [3, 9], 2, 1, 3)
    mk("arity2-two-points", 8, [3, 2], 2, 2, 3, mults=(1, 5), masks=[3, 1])
    mk("arity4", 10, [5], 3, 4, 2)
    mk("all-cap-layer", 6, [2, 6], 6, 1, 2)              # log_n 6, final_poly_bits 2, cap_height 6: the layer trees are all cap (path length 0)
    mk("arity5-fallback", 10, [4], 2, 5, 3)
    return out


def test_fri_shapes_and_fallback(pkg, pr, consts):
    proofs = fri_proofs(pkg, pr)
    batch, want = [], []
    for name, proof, q, pw in proofs:
        bad = tamper_last_leaf(proof, plonk=False)
        batch += [proof, bad]
        want += [fri_single(pkg, consts, proof, q, pw, 3), fri_single(pkg, consts, bad, q, pw, 3)]
        assert want[-2] == (True, None) and not want[-1][0], (name, want[-2:])
    res, sts = pr.fri_verify_batch(batch, 5, 2, 3, want_statements=True)
    assert [(r[0], r[1]) for r in res] == want, (res, want)
    assert all(r[2] == 4 for r in res[1::2]), res
    c = pr.verify_last_batch_counts()
    assert c == {"launches": LAUNCH_BUDGET, "host_syncs": SYNC_BUDGET, "on_device": 8, "fallback": 2}, c
    for k, (name, proof, q, pw) in enumerate(proofs):
        assert pr.fri_verify(proof, q, pw, 3)
        assert sts[2 * k] == pr.last_statement and sts[2 * k + 1] is None, name


def test_generic_mds_constants(pkg):
    """random 64-bit MDS entries: the generic permutation body in the Merkle items (glp_verify_merkle_kernel<false>)"""
    big = tuple(np.ascontiguousarray(a, dtype=np.uint64) for a in poseidon_consts("big"))
    p2 = pkg.Prover(0)
    try:
        p2.set_poseidon_constants(*big)
        rng = np.random.default_rng(77)
        batches = [pkg.PolynomialBatch.from_values(p2, rand_field(rng, (k, 1 << 8)), 3, 2) for k in (3, 9)]
        proof = p2.fri_prove(batches, 3, 2, arity_bits=2, final_poly_bits=3, num_queries=5, pow_bits=2)
        for b in batches:
            b.free()
        bad = tamper_last_leaf(proof, plonk=False)
        want = [fri_single(pkg, big, proof, 5, 2, 3), fri_single(pkg, big, bad, 5, 2, 3)]
        assert want[0] == (True, None) and not want[1][0]
        res = p2.fri_verify_batch([proof, bad], 5, 2, 3)
        assert [(r[0], r[1]) for r in res] == want and res[1][2] == 4, (res, want)
        assert p2.verify_last_batch_counts() == {"launches": LAUNCH_BUDGET, "host_syncs": SYNC_BUDGET, "on_device": 2, "fallback": 0}
    finally:
        p2.close()


def test_mixed_shapes_unbound_and_bound(pkg, pr, consts, fresh):
    proofs = [p for _, p, *_ in fresh]
    caps = [c for _, _, c, *_ in fresh]
    res = pr.plonk_verify_batch(proofs, pkg.UNBOUND, 4, 2)
    assert res == [(True, None, None)] * len(proofs)
    res = pr.plonk_verify_batch(proofs, caps[1], 4, 2)
    for k, r in enumerate(res):
        assert r == ((True, None, None) if k == 1 else (False, "preprocessed commitment differs from the circuit's", None)), (k, r)
    assert pr.verify_last_batch_counts()["on_device"] == 1
    # wrong public inputs: the host verifier's text
    name, proof, cap, pub, q, pw = fresh[3]
    wrong = [pub[0], (pub[1] + 1) % vbc.P]
    res = pr.plonk_verify_batch([proof, proof], cap, q, pw, publics=[wrong, pub])
    assert res == [(False, single(pkg, consts, proof, cap, q, pw, public=wrong)[1], None), (True, None, None)]
    assert res[0][1] == "public inputs differ from the expected statement"
    # the digests of the same call
    res, dg = pr.plonk_verify_batch(proofs, pkg.UNBOUND, 4, 2, want_digests=True)
    assert dg == [pr.proof_digest(p) for p in proofs]


def test_batch_sizes_and_counts(pkg, pr, consts, fresh):
    """B = 1, 2, 65 and 130, accepted and refused proofs interleaved, one pointer repeated; launches and synchronises do not depend on B"""
    lib = pkg.load_library()
    name, proof, cap, pub, q, pw = fresh[1]
    good = np.frombuffer(proof, dtype="<u8").copy()
    bad = np.frombuffer(tamper_last_leaf(proof), dtype="<u8").copy()
    want_bad = single(pkg, consts, bad.tobytes(), cap, q, pw)
    seen = {}
    for B in (1, 2, 65, 130):
        arrs = [good if k % 3 != 1 else bad for k in range(B)]              # the same two arrays again and again: repeated pointers
        ptrs = (ctypes.c_void_p * B)(*[a.ctypes.data for a in arrs])
        lens = (ctypes.c_size_t * B)(*[a.nbytes for a in arrs])
        verdicts = (vbc.Verdict * B)()
        assert lib.glp_plonk_verify_batch(pr.ctx, ptrs, lens, B, cap.ctypes.data, cap.size, None, 0, q, pw, verdicts, None) == 0
        for k in range(B):
            v = verdicts[k]
            if k % 3 != 1:
                assert v.status == 0 and v.on_device == 1
            else:
                assert (v.status, lib.glp_verify_reason_text(v.reason).decode(), v.query) == (-7, want_bad[1], q - 1)
        seen[B] = pr.verify_last_batch_counts()
        assert seen[B]["on_device"] == B and seen[B]["fallback"] == 0
        msg = lib.glp_last_error(pr.ctx).decode()
        if B > 1:
            assert "proof 1 rejected: " + want_bad[1] in msg, msg
    assert (seen[1]["launches"], seen[1]["host_syncs"]) == (seen[130]["launches"], seen[130]["host_syncs"])
    assert seen[130]["launches"] <= LAUNCH_BUDGET and seen[130]["host_syncs"] <= SYNC_BUDGET
    # B = 0 does nothing; a null table and a misaligned proof are refused
    assert lib.glp_plonk_verify_batch(pr.ctx, None, None, 0, None, 0, None, 0, q, pw, None, None) == 0
    assert lib.glp_plonk_verify_batch(pr.ctx, None, None, 1, None, 0, None, 0, q, pw, None, None) == -1
    one = (ctypes.c_void_p * 1)(good.ctypes.data + 4)
    ln = (ctypes.c_size_t * 1)(good.nbytes - 8)
    assert lib.glp_plonk_verify_batch(pr.ctx, one, ln, 1, None, 0, None, 0, q, pw, (vbc.Verdict * 1)(), None) == -1
    # without Poseidon constants: GLP_E_STATE
    p2 = pkg.Prover(0)
    try:
        one = (ctypes.c_void_p * 1)(good.ctypes.data)
        ln = (ctypes.c_size_t * 1)(good.nbytes)
        assert lib.glp_plonk_verify_batch(p2.ctx, one, ln, 1, None, 0, None, 0, q, pw, (vbc.Verdict * 1)(), None) == -6
    finally:
        p2.close()


def test_reduce_with_and_without_verify_batch(pkg, pr, consts, fresh):
    mr = importlib.import_module(pkg.__name__ + ".mapreduce")
    c = pref.build_circuit(np.random.default_rng(55), 6, 8)
    ck = pkg.PlonkCircuit(pr, c["consts"], c["sigmas"])
    proofs = [ck.prove(c["wires"], 28, 16) for _ in range(4)]
    leaf = lambda p: ck.verify(p, 28, 16)  # noqa: E731
    batch = lambda ps: [r[0] for r in ck.verify_batch(ps, 28, 16)]  # noqa: E731

    def batch_dg(ps):
        res, dg = ck.verify_batch(ps, 28, 16, want_digests=True)
        return [r[0] for r in res], dg

    assert mr.reduce_verify(leaf, proofs) is True and mr.reduce_verify(None, proofs, verify_batch=batch) is True
    a = mr.reduce_aggregate(pr, leaf, proofs)
    b = mr.reduce_aggregate(pr, None, proofs, verify_batch=batch_dg)
    b2 = mr.reduce_aggregate(pr, None, proofs, verify_batch=batch)
    assert a["ok"] and b["ok"] and b2["ok"]
    assert a["digests"] == b["digests"] == b2["digests"] and a["root"] == b["root"] == b2["root"]
    assert mr.verify_aggregate(pr, b["root_proof"], b["key"], b["digests"], b["root"])
    bad = list(proofs)
    bad[2] = tamper_last_leaf(bad[2])
    assert mr.reduce_verify(leaf, bad) is False and mr.reduce_verify(None, bad, verify_batch=batch) is False
    ra, rb = mr.reduce_aggregate(pr, leaf, bad), mr.reduce_aggregate(pr, None, bad, verify_batch=batch_dg)
    assert ra["ok"] is False and rb["ok"] is False and "root_proof" not in rb
    # the callable may be ck.verify_batch itself: its (ok, reason, query) rows are read as verdicts, never as truthy tuples
    rows = lambda ps: ck.verify_batch(ps, 28, 16)  # noqa: E731
    rows_dg = lambda ps: ck.verify_batch(ps, 28, 16, want_digests=True)  # noqa: E731
    assert mr.reduce_verify(None, proofs, verify_batch=rows) is True and mr.reduce_verify(None, bad, verify_batch=rows) is False
    assert mr.reduce_aggregate(pr, None, bad, verify_batch=rows_dg)["ok"] is False
    assert mr.reduce_aggregate(pr, None, proofs, verify_batch=rows_dg)["digests"] == a["digests"]
    # a leaf whose header does not parse (zeroed bytes) and one that is no whole number of words: no digest comes back for them (None), and the
    # Reduce says False both ways instead of raising
    for broken in (bytes(len(proofs[1])), proofs[1][:-3]):
        mal = [proofs[0], broken, proofs[2], proofs[3]]
        assert mr.reduce_verify(leaf, mal) is False
        for vb in (batch, batch_dg, rows, rows_dg):
            assert mr.reduce_verify(None, mal, verify_batch=vb) is False
            r = mr.reduce_aggregate(pr, None, mal, verify_batch=vb)
            assert r["ok"] is False and "root_proof" not in r
        assert mr.reduce_aggregate(pr, leaf, mal)["ok"] is False
    ck.free()
