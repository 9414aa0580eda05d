"""The batched verifier without a GPU.  The whole corpus of tests/verify_batch_cases.py — every golden proof with every word tampered three
ways, truncated, with a trailing word and with two tampers in different queries — goes through (a) the kernels of csrc/verify_batch_kernels.cuh
on the CPU with the driver's grids (tests/emu_verify_batch) and (b) glp_plonk_verify_batch_host / glp_fri_verify_batch_host, the same item
bodies run serially.  The expected value of every comparison is the SINGLE verifier on the same bytes: status and reason text from
glp_plonk_verify_host_ex / glp_fri_verify_host_ex, the failing query from the single verifier's code as the emulation library exposes it
(the C ABI of the single verifier carries no query number).  The digests must equal glp_plonk_proof_digest_host.  The same source as a
stand-alone program under AddressSanitizer + UBSan is built and run directly over the corpus."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_batch_cases as vbc  # noqa: E402
from conftest import ROOT, poseidon_consts  # noqa: E402

D = os.path.join(ROOT, "tests", "emu_verify_batch")
NOQ = 0xFFFFFFFF
NAMES = vbc.NAMES


@pytest.fixture(scope="module")
def vemu():
    return vbc.load_single_verifier()


@pytest.fixture(scope="module")
def consts():
    return tuple(np.ascontiguousarray(a, dtype=np.uint64) for a in poseidon_consts("small"))


def cap_args(prm):
    cap = prm["cap"]
    return (cap.ctypes.data, cap.size) if cap is not None else (None, 0)


def run_emu(vemu, consts, cases, prm):
    b = vbc.Batch(cases)
    counts = (ctypes.c_uint32 * 4)()
    rc, circ, diag = consts
    cp, cn = cap_args(prm)
    assert vemu.emu_verify_batch(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, int(prm["plonk"]), b.ptrs, b.lens, b.n, cp, cn, None, 0,
                                prm["min_queries"], prm["min_pow_bits"], prm["min_rate_bits"], b.verdicts, b.digests.ctypes.data, counts) == 0
    return b, [int(c) for c in counts]


def run_host(pkg, consts, cases, prm):
    lib = pkg.load_library()
    b = vbc.Batch(cases)
    rc, circ, diag = consts
    nd, nf = ctypes.c_uint32(0), ctypes.c_uint32(0)
    if prm["plonk"]:
        cp, cn = cap_args(prm)
        code = lib.glp_plonk_verify_batch_host(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, b.ptrs, b.lens, b.n, cp, cn, None, 0,
                                               prm["min_queries"], prm["min_pow_bits"], b.verdicts, b.digests.ctypes.data, ctypes.byref(nd),
                                               ctypes.byref(nf))
    else:
        code = lib.glp_fri_verify_batch_host(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, b.ptrs, b.lens, b.n, prm["min_queries"],
                                             prm["min_pow_bits"], prm["min_rate_bits"], b.verdicts, None, ctypes.byref(nd), ctypes.byref(nf))
    assert code == 0
    return b, (int(nd.value), int(nf.value))


single_queries = vbc.single_queries


def compare(pkg, cases, expected, queries, b, who):
    lib = pkg.load_library()
    bad = []
    for k, (label, _, _) in enumerate(cases):
        v = b.verdicts[k]
        got = (int(v.status), None if v.status == 0 else lib.glp_verify_reason_text(v.reason).decode(), int(v.query))
        want = (expected[k][0], expected[k][1], queries[k][2])
        if got != want:
            bad.append((label, got, want))
    assert not bad, f"{who}: {len(bad)} of {len(cases)} verdicts differ from the single verifier's, first: {bad[:5]}"


@pytest.mark.parametrize("name", NAMES)
def test_corpus_matches_single_verifier(pkg, vemu, consts, name):
    lib = pkg.load_library()
    cases, prm = vbc.corpus(name)
    expected = vbc.single_expected(lib, consts, cases, prm)
    queries = single_queries(vemu, consts, cases, prm)
    # the two faces of the single verifier agree with each other (the query numbers are taken from the second)
    for k in range(len(cases)):
        assert expected[k][0] == queries[k][0]
        assert expected[k][1] == (None if queries[k][0] == 0 else lib.glp_verify_reason_text(queries[k][1]).decode())
    assert expected[0] == (0, None), "the untampered proof is accepted"
    reasons = {e[1] for e in expected}
    for must in ("truncated", "trailing data in proof", "Merkle path does not lead to the cap", "non-canonical leaf",
                 "query index does not match the transcript") + (("a layer value does not continue the fold",
                                                                  "layer Merkle path does not lead to the cap") if name in ("fri", "l2") else ()):
        assert must in reasons, f"the corpus of {name} never meets '{must}'"
    # two calls per path: the corpus without its header cases (where n_fallback == 0 is a condition, not a measurement), then the header cases
    body_idx = [k for k, c in enumerate(cases) if not c[2]]
    hdr_idx = [k for k, c in enumerate(cases) if c[2]]
    assert body_idx[0] == 0 and len(body_idx) > len(cases) // 2 and hdr_idx
    before = {"truncated", "bad tag", "non-canonical cap", "non-canonical opening", "non-canonical layer cap", "non-canonical final polynomial",
              "proof of work failed", "non-canonical public input", "preprocessed commitment differs from the circuit's", "bad plonk header"}
    seen = {}
    for who, run in (("emulated kernels", lambda cs: run_emu(vemu, consts, cs, prm)), ("host form", lambda cs: run_host(pkg, consts, cs, prm))):
        for idx in (body_idx, hdr_idx):
            sub = [cases[k] for k in idx]
            b, counts = run(sub)
            compare(pkg, sub, [expected[k] for k in idx], [queries[k] for k in idx], b, who)
            if prm["plonk"]:
                for j, (label, w, _) in enumerate(sub):
                    try:
                        want = pkg.proof_digest_host(consts, w.tobytes())
                    except Exception:  # noqa: BLE001 — the header does not parse: the batched call leaves zeros
                        want = [0, 0, 0, 0]
                    assert [int(x) for x in b.digests[j]] == [int(x) for x in want], (who, label)
            if idx is body_idx:
                # the untampered proof and every tamper outside the header words: no fallback, and whatever reaches the query loop is on the device
                n_dev, n_fb = (counts[2], counts[3]) if who == "emulated kernels" else counts
                assert n_fb == 0, who
                if who == "emulated kernels":
                    assert counts[0] == 2 and counts[1] == 1, "two launches and one synchronise, whatever the batch holds"
                seen[who] = n_dev
                assert n_dev == sum(1 for j in range(len(sub)) if b.verdicts[j].on_device)
                assert b.verdicts[0].on_device == 1 and b.verdicts[0].status == 0
                for j, (label, _, _) in enumerate(sub):
                    v = b.verdicts[j]
                    text = lib.glp_verify_reason_text(v.reason).decode()
                    if v.status != 0 and v.query != NOQ:
                        assert v.on_device == 1, label
                    if v.on_device == 0:                  # refused before the query loop
                        assert v.status != 0 and text in before, (label, text)
    assert seen["emulated kernels"] == seen["host form"]
    # the lowest key wins: a tamper in a later query never hides one in an earlier query
    byl = {c[0]: k for k, c in enumerate(cases)}
    if "double-late-early" in byl:
        assert queries[byl["double-late-early"]][2] == 1 and queries[byl["double-early-late"]][2] == 0 and queries[byl["double-noncanon-late"]][2] == 0
        assert expected[byl["double-noncanon-late"]][1] == "non-canonical leaf"


def test_arity5_header_falls_back_with_the_single_verdict(pkg, vemu, consts):
    lib = pkg.load_library()
    words, prm = vbc.golden("fri")
    prm = dict(prm, min_pow_bits=0)
    cases = [("arity5", vbc.fri_header_arity5(), True), ("intact", words, False), ("arity5-again", vbc.fri_header_arity5(), True)]
    expected = vbc.single_expected(lib, consts, cases, prm)
    queries = single_queries(vemu, consts, cases, prm)
    assert expected[0][0] == -7 and queries[0][2] != NOQ, "the hand-made proof must reach the query loop, or it tests no fallback"
    b, counts = run_emu(vemu, consts, cases, prm)
    compare(pkg, cases, expected, queries, b, "emulated kernels")
    assert counts[2:] == [1, 2] and [b.verdicts[k].on_device for k in range(3)] == [0, 1, 0]
    hb, (n_dev, n_fb) = run_host(pkg, consts, cases, prm)
    compare(pkg, cases, expected, queries, hb, "host form")
    assert (n_dev, n_fb) == (1, 2)


def test_python_host_wrappers(pkg, consts):
    """plonk_verify_batch_host / fri_verify_batch_host: list of (ok, reason, query), digests, counts, the wrappers' own verdict for bytes that
    are no whole words, B = 0"""
    words, prm = vbc.golden("gates")
    good = words.tobytes()
    bad = words.copy()
    bad[-1] ^= np.uint64(1)
    res, digests, counts = pkg.plonk_verify_batch_host(consts, [good, bad.tobytes(), good[:-3], good], prm["cap"], prm["min_queries"], prm["min_pow_bits"],
                                                       publics=pkg.UNBOUND, want_digests=True, want_counts=True)
    assert res[0] == (True, None, None) and res[3] == (True, None, None)
    assert res[1][0] is False and res[1][1] == pkg.plonk_verify_host(consts, bad.tobytes(), prm["cap"], prm["min_queries"], prm["min_pow_bits"],
                                                                     public=pkg.UNBOUND)[1][len("proof rejected: "):]
    assert res[1][2] == vbc.layout(words, True)["nq"] - 1
    assert res[2] == (False, pkg.NOT_WORDS, None) and digests[2] is None
    assert digests[0] == [int(v) for v in pkg.proof_digest_host(consts, good)] and digests[0] == digests[3]
    assert counts == (3, 0)
    assert pkg.plonk_verify_batch_host(consts, [], prm["cap"]) == []
    ok, why, q = pkg.plonk_verify_batch_host(consts, [good], prm["cap"])[0]                       # the defaults demand 28 queries / 16 bits
    assert not ok and "fewer queries" in why and q is None
    with pytest.raises(pkg.GlpError):
        pkg.plonk_verify_batch_host(consts, [good], None)
    fw, fprm = vbc.golden("fri")
    fres = pkg.fri_verify_batch_host(consts, [fw.tobytes(), fw.tobytes() + bytes(8)], fprm["min_queries"], fprm["min_pow_bits"], fprm["min_rate_bits"])
    assert fres == [(True, None, None), (False, "trailing data in proof", None)]
    # expected public inputs, one row per proof: the gates proof is about ITS statement
    import json
    with open(os.path.join(vbc.HERE, "golden", "proofs.json")) as f:
        pub = json.load(f)["gates"]["public"]
    res = pkg.plonk_verify_batch_host(consts, [good, good], prm["cap"], prm["min_queries"], prm["min_pow_bits"], publics=[pub, [pub[1], pub[0]]])
    assert res == [(True, None, None), (False, "public inputs differ from the expected statement", None)]


def test_sanitized_program_over_the_corpus(consts, tmp_path):
    """the emulation as a stand-alone program under AddressSanitizer + UBSan, run directly: every case in a heap block of exactly its length.
    The corpus here is thinned in ONE respect, for the run time under the sanitizers (the full one takes minutes): of the words that are field
    data — everything outside the header words — every 16th position is tampered.  No address, length or trip count in the verifiers depends on
    such a word (the plan is computed from the header words and the proof's length alone), so they can move no access.  What can is all there:
    every header word tampered three ways, every truncation of the full corpus, the trailing word, the double tampers."""
    subprocess.run(["make", "-s", "sanitized"], cwd=D, check=True)
    rc, circ, diag = consts
    blob = [rc, circ, diag]
    groups = []
    for name in NAMES:
        cases, prm = vbc.corpus(name, step=16, all_header=True)
        cap = prm["cap"] if prm["cap"] is not None else np.zeros(0, dtype=np.uint64)
        g = [np.array([int(prm["plonk"]), prm["min_queries"], prm["min_pow_bits"], prm["min_rate_bits"], cap.size], dtype=np.uint64), cap,
             np.array([len(cases)], dtype=np.uint64)]
        for _, w, _ in cases:
            g += [np.array([w.nbytes], dtype=np.uint64), w]
        groups.append(g)
    blob.append(np.array([len(groups)], dtype=np.uint64))
    for g in groups:
        blob += g
    path = tmp_path / "corpus.bin"
    np.concatenate([np.ascontiguousarray(a, dtype=np.uint64).ravel() for a in blob]).tofile(path)
    r = subprocess.run([os.path.join(D, "emu_verify_batch_san"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "emu_verify_batch_san ok" in r.stdout, r.stdout[-3000:]


def test_declarations_are_plain_c(pkg, tmp_path):
    """tests/cpp/abi_c99_verify_batch.c as strict C99 against the library: it links the device calls and runs the ctx-less ones"""
    pkg.load_library()
    exe = tmp_path / "abi_c99_verify_batch"
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "abi_c99_verify_batch.c"), "-o", str(exe), "-L", libdir, "-lglprover",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip() == "verdict -7 truncated size 16 ok 1 linked 1"
