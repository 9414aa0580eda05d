"""glp_plonk_prove_batch on the GPU: B witnesses of ONE circuit through one prover call, against the unchanged single path
(glp_plonk_prove_ex, once per instance) byte for byte.  Every instance holds independent data and, where the circuit has public inputs,
different public inputs, so a wrong instance offset cannot pass.

Where B satisfiable witnesses of one circuit come from: pref.build_circuit draws circuit and witness together, so fresh_witness re-walks the
built circuit's cells in build_circuit's order with fresh values (a copy class's first cell fresh or derived, later members copied; gate
outputs recomputed with pref.poseidon_row / pref.sha_row).  Each instance is first proved by the single path and accepted by
pref.verify_plonk and ck.verify: the helper is validated through the reference alone.

Which test launches which new instantiation (rows of CASES below):
  glp_plonk_gather_wires_batch_kernel, glp_perm_quotients_batch_kernel   every row
  glp_quotient_batch_kernel<false>                                       plain-6, plain-11-public, sha, mirror-19
  glp_quotient_batch_kernel<true, true>                                  poseidon-small, sha+poseidon, ext+poseidon+sha
  glp_quotient_batch_kernel<true, false>                                 poseidon-big
  glp_quotient_sha_batch_kernel                                          sha, sha+poseidon, ext+poseidon+sha"""
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_verifier as fv  # noqa: E402
import plonk_ref as pref  # noqa: E402
from conftest import poseidon_consts, ptr, rand_field  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

pytestmark = pytest.mark.gpu
P = fv.P


def _mod(name):
    graft.load_package()
    return importlib.import_module(graft.PKG_NAME + name)


def use_consts(prover, oracle, kind):
    rc, circ, diag = consts = poseidon_consts(kind)
    prover.set_poseidon_constants(rc, circ, diag)
    oracle.orc_poseidon_set_constants(ptr(rc), ptr(circ), ptr(diag))
    return consts


# ---- B witnesses of one built circuit ------------------------------------------------------------------------------------------------
def copy_classes(circ):
    """class id of every routed cell, from the cycles of sigma: sigma_j(row i) = k_j' * w^i' names the next cell (j', i') of the cycle"""
    n, R = 1 << circ["log_n"], circ["R"]
    ks, w = pref.ks_of(R), fv.root(circ["log_n"])
    cell_of, x = {}, 1
    for i in range(n):
        for j in range(R):
            cell_of[ks[j] * x % P] = (j, i)
        x = x * w % P
    sig = [[int(v) for v in r] for r in circ["sigmas"]]
    cls = [[-1] * n for _ in range(R)]
    k = 0
    for j0 in range(R):
        for i0 in range(n):
            j, i = j0, i0
            while cls[j][i] < 0:
                cls[j][i] = k
                j, i = cell_of[sig[j][i]]
            k += (j, i) == (j0, i0)
    return cls


def fresh_witness(circ, rng, cls):
    """another satisfying witness of circ: build_circuit's walk over the cells, in its order, with fresh values"""
    n, W, R, flags = 1 << circ["log_n"], circ["W"], circ["R"], circ["flags"]
    C = [[int(v) for v in r] for r in circ["consts"]]
    q, c0, c1, c2, q_pos = C[0], C[1], C[2], C[3], C[5]
    q_sha = C[6:10] if flags & pref.FLAG_SHA else [[0] * n] * 4
    q_ext = C[-1] if flags & pref.FLAG_EXT else [0] * n
    old = circ["wires"]
    w = [[0] * n for _ in range(W)]
    val = {}
    rnd = lambda: int(rng.integers(0, 1 << 62)) * 4 % P
    r32 = lambda: int(rng.integers(0, 1 << 32))

    def free(j, i):                                   # a free cell: its class's value when an earlier member set one, else fresh
        k = cls[j][i]
        if k not in val:
            val[k] = rnd()
        w[j][i] = val[k]

    def derived(j, i, v):                             # a gate output or an unconstrained cell: never a copy of an earlier cell
        w[j][i] = v
        if j < R:
            assert cls[j][i] not in val
            val[cls[j][i]] = v

    for i in range(n):
        if q_ext[i]:
            for c in range(R // 8):
                for k in range(6):
                    free(8 * c + k, i)
                x0, x1, y0, y1, z0, z1 = (w[8 * c + k][i] for k in range(6))
                derived(8 * c + 6, i, (x0 * y0 + 7 * x1 * y1 + z0) % P)
                derived(8 * c + 7, i, (x0 * y1 + x1 * y0 + z1) % P)
            for j in range(R, W):
                w[j][i] = rnd()
        elif any(qs[i] for qs in q_sha):
            kind = [qs[i] for qs in q_sha].index(1)
            words = {pref.SHA_E: lambda: [r32() for _ in range(6)], pref.SHA_A: lambda: [r32(), r32(), r32(), int(rng.integers(0, 5 << 32))],
                     pref.SHA_W: lambda: [r32() for _ in range(4)], pref.SHA_ADD: lambda: [r32() for _ in range(2 * int(rng.integers(0, 5)))]}[kind]()
            row = pref.sha_row(kind, words, c2[i])
            for j in range(W):
                derived(j, i, row[j] if j < pref.SHA_WIRES else rnd())
        elif q_pos[i]:
            for j in range(12):
                free(j, i)
            row = pref.poseidon_row([w[j][i] for j in range(12)], circ["pos_consts"], swap=int(old[pref.POS_SWAP][i]))
            for j in range(12, W):
                derived(j, i, row[j] if j < pref.POS_WIRES else rnd())
        else:
            for g in range(R // 4):
                for k in range(3):
                    free(4 * g + k, i)
                x, y, z = w[4 * g][i], w[4 * g + 1][i], w[4 * g + 2][i]
                derived(4 * g + 3, i, (c0[i] * x * y + c1[i] * z + c2[i]) % P if q[i] else rnd())
            for j in range(R, W):
                w[j][i] = rnd()
    return np.array(w, dtype=np.uint64)


def instances_of(circ, rng, B):
    """B witnesses (the built one first) with their public inputs"""
    cls = copy_classes(circ)
    wires = [circ["wires"]] + [fresh_witness(circ, rng, cls) for _ in range(B - 1)]
    return wires, [[int(v) for v in w[0, :circ["n_public"]]] for w in wires]


def mirror_circuit(log_n, W, rng, B):
    """no active gate; identity sigma except sigma[0][i] = k_0 * w^(i + n/2) (= -w^i), wire 0 equal on rows i and i + n/2, every other cell random:
    any such witness is valid, and because the copies cross the halves every block product of the scan differs from 1"""
    n = 1 << log_n
    w, ks = fv.root(log_n), pref.ks_of(W)
    wp, x = [0] * n, 1
    for i in range(n):
        wp[i] = x
        x = x * w % P
    sig = np.array([[k * v % P for v in wp] if j else [(P - v) % P for v in wp] for j, k in enumerate(ks)], dtype=np.uint64)
    wires = []
    for _ in range(B):
        m = rand_field(rng, (W, n))
        m[0, n // 2:] = m[0, :n // 2]
        wires.append(m)
    circ = {"log_n": log_n, "W": W, "R": W, "n_public": 0, "flags": 0, "consts": np.zeros((pref.NCONST, n), dtype=np.uint64), "sigmas": sig,
            "wires": wires[0], "public": [], "pos_consts": None}
    return circ, wires, [[] for _ in range(B)]


def build_case(name, rng, consts):
    """(circuit dict, PlonkCircuit keyword arguments, B witnesses, B public-input lists, num_queries, pow_bits)"""
    pick = lambda n, lo, k: sorted(int(v) for v in rng.choice(np.arange(lo, n), size=k, replace=False))
    if name.startswith("plain-6"):
        circ, B = pref.build_circuit(rng, 6, 8), int(name.split("B")[1])
    elif name == "plain-11-public":
        circ, B = pref.build_circuit(rng, 11, 16, n_public=3), 2
    elif name in ("poseidon-small", "poseidon-big"):
        log_n, W, R, npub, npos = (8, 136, 80, 4, 40) if name == "poseidon-small" else (6, 160, 136, 2, 9)
        circ, B = pref.build_circuit(rng, log_n, W, n_routed=R, n_public=npub, poseidon_rows=pick(1 << log_n, npub, npos), consts=consts), (3 if name == "poseidon-small" else 2)
    elif name == "sha":
        circ, B = pref.build_circuit(rng, 6, 160, n_routed=16, sha_rows=pick(64, 0, 20)), 2
    elif name == "sha+poseidon":
        rows = pick(256, 2, 70)
        circ, B = pref.build_circuit(rng, 8, 144, n_routed=80, n_public=2, sha_rows=rows[:60], poseidon_rows=rows[60:], consts=consts), 2
    elif name == "ext+poseidon+sha":
        rows = [int(v) for v in rng.choice(np.arange(2, 256), size=30 + 12 + 20, replace=False)]
        circ, B = pref.build_circuit(rng, 8, 144, n_routed=80, n_public=2, ext_rows=sorted(rows[:30]), poseidon_rows=sorted(rows[30:42]), consts=consts,
                                     sha_rows=sorted(rows[42:])), 2
    else:
        assert name == "mirror-19"
        circ, wires, publics = mirror_circuit(19, 8, rng, 2)
        return circ, wires, publics, 6, 4
    wires, publics = instances_of(circ, rng, B)
    return circ, wires, publics, 8, 4


def plonk_circuit(pkg, prover, circ):
    f = circ["flags"]
    return pkg.PlonkCircuit(prover, circ["consts"], circ["sigmas"], n_wires=circ["W"], n_public=circ["n_public"], poseidon=bool(f & pref.FLAG_POSEIDON),
                            sha=bool(f & pref.FLAG_SHA), ext=bool(f & pref.FLAG_EXT))


CASES = ["plain-6-B1", "plain-6-B3", "plain-6-B5", "plain-11-public", "poseidon-small", "poseidon-big", "sha", "sha+poseidon", "ext+poseidon+sha", "mirror-19"]


@pytest.mark.parametrize("name", CASES)
def test_batch_equals_sequential(prover, oracle, pkg, name):
    """the batch call's proofs equal the B single-path proofs byte for byte, both verifiers accept each, a second batch call gives the same bytes"""
    kind = "big" if name == "poseidon-big" else "small"
    try:
        consts = use_consts(prover, oracle, kind)
        rng = np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))
        circ, wires, publics, nq, pw = build_case(name, rng, consts)
        B = len(wires)
        ck = plonk_circuit(pkg, prover, circ)
        dws = [prover.to_device(w) for w in wires]
        pubs = publics if circ["n_public"] else None
        ref = [ck.prove_(dws[i], nq, pw, public=publics[i] if circ["n_public"] else None) for i in range(B)]
        assert len(set(ref)) == B
        if circ["n_public"]:
            assert len({tuple(p) for p in publics}) == B
        pc = consts if circ["flags"] & pref.FLAG_POSEIDON else None
        for i in range(B):
            assert ck.verify(ref[i], nq, pw, public=publics[i] if circ["n_public"] else None), (i, prover.last_reject)
            pref.verify_plonk(ref[i], oracle, pos_consts=pc, public=publics[i])
        got = ck.prove_batch_(dws, pubs, nq, pw)
        assert len(got) == B
        for i in range(B):
            assert got[i] == ref[i], f"instance {i} differs from the single path"
        assert ck.prove_batch_(dws, pubs, nq, pw) == ref
        if name == "plain-6-B3":                                   # the host-array form, and two instances on one wire matrix
            assert ck.prove_batch(wires, pubs, nq, pw) == ref
            assert ck.prove_batch_([dws[1], dws[0], dws[1]], None, nq, pw) == [ref[1], ref[0], ref[1]]
        for d in dws:
            d.free()
        ck.free()
    finally:
        use_consts(prover, oracle, "small")


def test_counts_do_not_depend_on_B(prover, oracle, pkg):
    """the PLONK driver's own launches and synchronises, and the opening proof's, for B = 1, 2, 5 of the 2^11 x 16 circuit with public inputs,
    against the formulas of the header comments written out by hand"""
    use_consts(prover, oracle, "small")
    rng = np.random.default_rng(11)
    circ = pref.build_circuit(rng, 11, 16, n_public=3)
    wires, publics = instances_of(circ, rng, 5)
    ck = plonk_circuit(pkg, prover, circ)
    dws = [prover.to_device(w) for w in wires]
    # glp_plonk_prove_batch: 1 (wire gather) + 4 (K6) + 1 (K7) + 0 (no SHA rows) + 1 (un-bit-reversal) + 1 (unshift); no synchronise of its own
    want_plonk = (1 + 4 + 1 + 0 + 1 + 1, 0)
    # glp_fri_prove_batch at log_n 11, final 5, arity 4: L = 1 layer, a tree of 2^10 leaves (cap 4: one leaf launch + one fused launch), PoW on
    want_fri = (3 + ((1 + 1) + 1) + 1 + 1, 1 + 1 + 1 + 1 + 1, 1)
    seen = {}
    for B in (1, 2, 5):
        proofs = ck.prove_batch_(dws[:B], publics[:B], 8, 4)
        assert len(proofs) == B
        seen[B] = (prover.plonk_last_batch_counts(), prover.fri_last_batch_counts())
    assert seen[1] == seen[2] == seen[5] == (want_plonk, want_fri)
    for d in dws:
        d.free()
    ck.free()


def test_faulty_instance_fails_the_call(prover, oracle, pkg):
    use_consts(prover, oracle, "small")
    rng = np.random.default_rng(12)
    circ = pref.build_circuit(rng, 6, 16, n_public=3)
    wires, publics = instances_of(circ, rng, 3)
    ck = plonk_circuit(pkg, prover, circ)
    dws = [prover.to_device(w) for w in wires]
    good = ck.prove_batch_(dws, publics, 8, 4)
    assert good == [ck.prove_(dws[i], 8, 4, public=publics[i]) for i in range(3)] and len(set(good)) == 3
    assert ck.prove_batch_([], [], 8, 4) == []
    # a public input >= p in instance 1 of 3
    bad_pub = [list(p) for p in publics]
    bad_pub[1][2] = P
    with pytest.raises(pkg.GlpError, match="instance 1"):
        ck.prove_batch_(dws, bad_pub, 8, 4)
    assert ck.prove_batch_(dws, publics, 8, 4) == good
    # a NULL wire pointer
    with pytest.raises(pkg.GlpError, match="instance 1"):
        ck.prove_batch_([dws[0], 0, dws[2]], publics, 8, 4)
    assert ck.prove_batch_(dws, publics, 8, 4) == good
    # a gate violation in instance 1 of 3: whatever the single path does with that witness, the batch does
    row = next(i for i in range(3, 64) if int(circ["consts"][0][i]) == 1)
    broken = wires[1].copy()
    broken[3, row] ^= np.uint64(1)
    db = prover.to_device(broken)
    try:
        single = ck.prove_(db, 8, 4, public=publics[1])
    except pkg.GlpError:
        single = None
    if single is None:
        with pytest.raises(pkg.GlpError, match="instance 1"):
            ck.prove_batch_([dws[0], db, dws[2]], publics, 8, 4)
    else:
        assert not ck.verify(single, 8, 4, public=publics[1])
        assert ck.prove_batch_([dws[0], db, dws[2]], publics, 8, 4) == [good[0], single, good[2]]
    assert ck.prove_batch_(dws, publics, 8, 4) == good
    for d in dws + [db]:
        d.free()
    ck.free()


def _root(heights, roots):
    lvl = [hashlib.sha256(b"\x00" + int(h).to_bytes(32, "big") + r).digest() for h, r in zip(heights, roots)]
    while len(lvl) > 1:
        lvl = [hashlib.sha256(b"\x01" + lvl[i] + lvl[i + 1]).digest() for i in range(0, len(lvl), 2)]
    return lvl[0]


def test_map_step_with_prove_batch(prover, pkg):
    """the Map step with prove_batch = 3 over 5 leaves on two provers (groups of 3 and 2), with the witnesses from the host evaluators and from the
    device: the same leaf proofs as prove_batch = 0.  A range needs 2^k leaves to have a root, so the root (verifier-derived key, hashlib's
    commitment) is that of the first 4 leaves, proved by the same batched object.  Then the signature Map with prove_batch = 2 over 3 validators."""
    dm, sm, ec = _mod(".data_commitment_mr"), _mod(".signature_mr"), _mod(".ed25519_circuit")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    extra = pkg.Prover(0)
    extra.set_poseidon_constants(*consts)
    rng = np.random.default_rng(4200)
    heights = [7_100_000 + k for k in range(10)]
    roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in heights]
    base = dm.DataCommitmentMapReduce(prover, consts, leaf_blocks=2, fan_in=2, num_queries=6, pow_bits=4, map_provers=[extra], prove_batch=0)
    want = base.prove_leaves(heights, roots)
    vkey = base.expected_key(8)
    base.free()
    assert len(want) == 5 and len(set(want)) == 5
    for on in (False, True):
        mr = dm.DataCommitmentMapReduce(prover, consts, leaf_blocks=2, fan_in=2, num_queries=6, pow_bits=4, map_provers=[extra], prove_batch=3,
                                        device_witness=on)
        assert mr.prove_leaves(heights, roots) == want, on
        out = mr.prove_range(heights[:8], roots[:8])
        assert np.array_equal(out["key"], vkey) and mr.verify(out["root_proof"], vkey, heights[:8], roots[:8], out["commitment"]), prover.last_reject
        assert out["commitment"] == _root(heights[:8], roots[:8])
        with pytest.raises(ValueError):
            mr._map_inputs([[w for h, r in zip(heights[k:k + 2], roots[k:k + 2]) for w in dm.tuple_words(h, r)] if k != 6 else [1 << 32] * 32
                            for k in range(0, 10, 2)])
        mr.free()
    block = hashlib.sha256(b"a block").digest()
    sigs = sm.SignatureSetMapReduce(prover, consts, msg_len=48, hash_offset=8, fan_in=2, num_queries=6, pow_bits=4, prove_batch=2)
    sigs._record_leaf()                                            # once: the 2^16-row leaf's recording is host work, the same for both runs
    msgs = [sigs.vote_bytes(block, i) for i in range(3)]
    seeds = [hashlib.sha256(b"seed %d" % i).digest() for i in range(3)]
    pubs = [ec.keypair_and_sign(s, m)[0] for s, m in zip(seeds, msgs)]
    sg = [ec.keypair_and_sign(s, m)[1] for s, m in zip(seeds, msgs)]
    slots = sigs._slots(pubs, sg, msgs, [True, True, True])
    batched = sigs._map(slots, 0, 3)                               # groups of 2 and 1
    sigs.prove_batch = 0
    assert sigs._map(slots, 0, 3) == batched and len(set(batched)) == 3
    sigs.free()
    extra.close()
