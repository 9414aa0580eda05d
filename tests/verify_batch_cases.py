"""The corpus of the batched verifier's tests (tests/test_emu_verify_batch.py, tests/test_gpu_verify_batch.py), generated deterministically from
the committed golden proofs (tests/golden/proofs.json, tests/golden/verify_batch_l2.json).  Per proof:
  - the proof itself;
  - every `step`-th word position tampered three ways: low bit flipped, set to p, set to 0 (step 1 for the four goldens);
  - truncation after every word of the first and of the last query, and at every 64th word elsewhere;
  - one trailing word appended;
  - two simultaneous tampers in different queries (the lowest key must win), in both orders of severity.
The layout (where the FRI part, its header and the queries start) is recomputed here from the header words, independently of the library."""
import ctypes
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P = 0xFFFFFFFF00000001
NAMES = ("plonk", "gates", "sha", "fri", "l2")           # l2: tests/golden/verify_batch_l2.json (committed; its absence is an error)


class Verdict(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reason", ctypes.c_uint32), ("query", ctypes.c_uint32), ("on_device", ctypes.c_uint32)]


def fri_layout(w, f0):
    """(first word after the FRI header block, first query word, words per query, queries, offset inside a query of its last leaf — the last
    layer's, or the last batch's when there is no layer) of the FRI part that starts at word f0"""
    log_n, rb, cap0, a, fb, nq = (int(w[f0 + k]) for k in range(1, 7))
    nb, n_pts = int(w[f0 + 9]), int(w[f0 + 10])
    pm = [int(v) for v in w[f0 + 11 + n_pts: f0 + 11 + n_pts + 2 * nb]]
    n_polys, masks = pm[0::2], pm[1::2]
    log_N = log_n + rb
    pos = f0 + 11 + n_pts + 2 * nb
    header_end = pos
    pos += nb * (4 << cap0)
    total = sum(n_polys[b] for p in range(n_pts) for b in range(nb) if (masks[b] >> p) & 1)
    pos += 2 * total
    L = (log_n - fb) // a if log_n > fb else 0
    qwords = 1 + sum(n_polys[b] + 4 * (log_N - cap0) for b in range(nb))
    last_leaf = qwords - 4 * (log_N - cap0) - n_polys[-1]           # the last batch's leaf, until a layer follows
    log_len = log_N
    for _ in range(L):
        log_leaves = log_len - a
        chh = min(cap0, log_leaves)
        pos += 4 << chh
        last_leaf = qwords
        qwords += (2 << a) + 4 * (log_leaves - chh)
        log_len -= a
    pos += (2 << (log_n - a * L)) + 1
    return header_end, pos, qwords, nq, last_leaf


def layout(words, plonk):
    """dict: header (the set of header word positions), q0, qwords, nq, last_leaf (first word of the LAST query's last leaf)"""
    w = words
    hdr = set()
    f0 = 0
    if plonk:
        log_N = int(w[1]) + int(w[4])
        capw = 4 << min(int(w[5]), log_N)
        f0 = 8 + int(w[6]) + 4 * capw
        hdr |= set(range(8))
    header_end, q0, qwords, nq, last_leaf = fri_layout(w, f0)
    hdr |= set(range(f0, header_end))
    assert q0 + qwords * nq == len(w), "the layout computed here must end where the proof ends"
    return {"header": hdr, "q0": q0, "qwords": qwords, "nq": nq, "last_leaf": q0 + (nq - 1) * qwords + last_leaf}


def golden(name):
    """(words, params) of one golden proof: params = plonk, min_queries, min_pow_bits, min_rate_bits, cap (np array or None)"""
    fn = "verify_batch_l2.json" if name == "l2" else "proofs.json"
    with open(os.path.join(HERE, "golden", fn)) as f:
        g = json.load(f)
    g = g if name == "l2" else g[name]
    words = np.frombuffer(bytes.fromhex(g["proof"]), dtype="<u8").copy()
    plonk = name != "fri"
    return words, {"plonk": plonk, "min_queries": g["queries"], "min_pow_bits": g["pow_bits"], "min_rate_bits": g.get("rate_bits", 1),
                   "cap": np.array(g["circuit_cap"], dtype=np.uint64) if plonk else None}


def corpus(name, step=None, all_header=False):
    """[(label, np.uint64 words, in_header)]: the cases of one golden proof, always in the same order.  step: tamper every step-th word
    (default: every word, every 7th of l2); all_header: and every header word whatever the step"""
    words, prm = golden(name)
    lay = layout(words, prm["plonk"])
    step = step or (7 if name == "l2" else 1)
    n = len(words)
    out = [("intact", words, False)]
    for t in sorted(set(range(0, n, step)) | (lay["header"] if all_header else set())):
        for kind, val in (("flip", int(words[t]) ^ 1), ("p", P), ("zero", 0)):
            if val == int(words[t]):
                continue
            bad = words.copy()
            bad[t] = np.uint64(val)
            out.append((f"{kind}@{t}", bad, t in lay["header"]))
    q0, qw, nq = lay["q0"], lay["qwords"], lay["nq"]
    cuts = set(range(64, n, 64)) | set(range(q0, q0 + qw + 1)) | set(range(n - qw, n))
    for cut in sorted(c for c in cuts if 0 < c < n):
        out.append((f"cut@{cut}", words[:cut].copy(), cut <= max(lay["header"])))
    out.append(("trailing", np.concatenate([words, np.zeros(1, dtype=np.uint64)]), False))
    if nq >= 2:
        # a leaf word of query 1 and of the last query, then the last word of query 0's last path and the first leaf word of the last query
        for label, ta, tb in (("late-early", q0 + (nq - 1) * qw + 1, q0 + qw + 1), ("early-late", q0 + qw - 1, q0 + (nq - 1) * qw + 2),
                              ("noncanon-late", q0 + (nq - 1) * qw + 1, q0 + 2)):
            bad = words.copy()
            bad[ta] ^= np.uint64(1)
            bad[tb] = np.uint64(P) if label == "noncanon-late" else bad[tb] ^ np.uint64(2)
            out.append((f"double-{label}", bad, False))
    return out, prm


class Batch:
    """cases as the C entry points take them: keeps the arrays alive; .ptrs, .lens, .n"""

    def __init__(self, cases):
        self.arrs = [np.ascontiguousarray(c[1], dtype=np.uint64) for c in cases]
        self.n = len(self.arrs)
        self.ptrs = (ctypes.c_void_p * max(1, self.n))(*[a.ctypes.data for a in self.arrs])
        self.lens = (ctypes.c_size_t * max(1, self.n))(*[a.nbytes for a in self.arrs])
        self.verdicts = (Verdict * max(1, self.n))()
        self.digests = np.zeros((max(1, self.n), 4), dtype=np.uint64)


def single_expected(lib, consts, cases, prm):
    """[(status, text after 'proof rejected: ' or None)] from glp_plonk_verify_host_ex / glp_fri_verify_host_ex, case by case"""
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in consts)
    err = ctypes.create_string_buffer(256)
    cap = prm["cap"]
    out = []
    for _, w, _ in cases:
        w = np.ascontiguousarray(w, dtype=np.uint64)
        if prm["plonk"]:
            code = lib.glp_plonk_verify_host_ex(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, w.ctypes.data, w.nbytes, cap.ctypes.data, cap.size,
                                                None, 0, prm["min_queries"], prm["min_pow_bits"], err, 256)
        else:
            code = lib.glp_fri_verify_host_ex(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, w.ctypes.data, w.nbytes, prm["min_queries"],
                                              prm["min_pow_bits"], prm["min_rate_bits"], None, err, 256)
        text = err.value.decode()
        assert code in (0, -7), code
        assert code == 0 or text.startswith("proof rejected: ")
        out.append((code, None if code == 0 else text[len("proof rejected: "):]))
    return out


def load_single_verifier():
    """the emulation library (tests/emu_verify_batch), for its emu_verify_single: the SINGLE verifier's code with the failing query exposed,
    which the C ABI of the single verifier does not carry"""
    import subprocess
    d = os.path.join(HERE, "emu_verify_batch")
    subprocess.run(["make", "-s"], cwd=d, check=True)
    lib = ctypes.CDLL(os.path.join(d, "libglp_emu_verify_batch.so"))
    vp, c32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    lib.emu_verify_batch.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, c32, vp, sz, vp, sz, c32, c32, c32, vp, vp, vp]
    lib.emu_verify_single.argtypes = [vp, vp, vp, ctypes.c_int, vp, sz, vp, sz, vp, sz, c32, c32, c32, vp]
    return lib


def single_queries(emu, consts, cases, prm):
    """[(status, reason, failing query)] of the single verifier's code, case by case"""
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in consts)
    cap = prm["cap"]
    cp, cn = (cap.ctypes.data, cap.size) if cap is not None else (None, 0)
    out = []
    v = Verdict()
    for _, w, _ in cases:
        w = np.ascontiguousarray(w, dtype=np.uint64)
        assert emu.emu_verify_single(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, int(prm["plonk"]), w.ctypes.data, w.nbytes, cp, cn, None, 0,
                                     prm["min_queries"], prm["min_pow_bits"], prm["min_rate_bits"], ctypes.byref(v)) == 0
        out.append((int(v.status), int(v.reason), int(v.query)))
    return out


def fri_header_arity5():
    """a hand-made stand-alone FRI proof whose header says arity_bits = 5: the shape the items do not take.  The words after the header
    are the golden proof's (canonical, long enough for the caps and the final polynomial of that reading) and it declares no proof of
    work, so the host phase reaches the query loop — which then runs in place, by the single verifier's code (fallback), and refuses."""
    from_golden, _ = golden("fri")
    w = from_golden.copy()
    w[4] = np.uint64(5)
    w[7] = np.uint64(0)
    return w
