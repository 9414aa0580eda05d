"""Host-side binding of libglprover.so (include/glprover.h) for the prover hot path.

The reference's host language is Rust and its prover is plonky2 (neither is in
/root/reference, which holds only `.gitignore:1` and `changelog.md:1-2`, nor in this image),
so this module mirrors the *names* of the upstream operator surface for the path — recalled,
unverified: ``fft`` / ``ifft`` / ``coset_fft`` / ``lde`` of
``plonky2_field::fft`` and ``PolynomialBatch::from_values`` / ``from_coeffs`` of
``plonky2::fri::oracle`` — on top of the C ABI.  It is test/bench plumbing: ctypes for the
calls, numpy (or torch tensors via ``data_ptr()``) for buffers.

There is no CPU fallback.  Importing works anywhere (so the ABI can be inspected without a
GPU), but ``Prover()`` raises ``GlpError`` unless a gfx950 device is usable and the library
was built (``python -c "import __graft_entry__ as g; g.build()"``).
"""
import ctypes
import os

import numpy as np

P = 2**64 - 2**32 + 1
COSET_SHIFT = 7  # multiplicative generator, the coset shift used for LDEs
NTT_INVERSE = 1
NTT_BITREV = 2

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLP_LIB") or os.path.join(_HERE, "lib", "libglprover.so")   # GLP_LIB: A/B builds (tuning)

_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p


class GlpError(RuntimeError):
    pass


_ERR = {-1: "GLP_E_INVALID", -2: "GLP_E_NODEVICE", -3: "GLP_E_HIP", -4: "GLP_E_NOMEM",
        -5: "GLP_E_UNSUPPORTED", -6: "GLP_E_STATE", -7: "GLP_E_REJECT"}

_lib = None


class FriConfig(ctypes.Structure):
    _fields_ = [("log_n", ctypes.c_uint32), ("rate_bits", ctypes.c_uint32), ("cap_height", ctypes.c_uint32),
                ("arity_bits", ctypes.c_uint32), ("final_poly_bits", ctypes.c_uint32), ("num_queries", ctypes.c_uint32),
                ("pow_bits", ctypes.c_uint32), ("shift", ctypes.c_uint64), ("n_points", ctypes.c_uint32),
                ("point_mult", ctypes.c_uint64 * 4)]


class FriBatch(ctypes.Structure):
    _fields_ = [("d_coeffs", ctypes.c_void_p), ("d_lde", ctypes.c_void_p), ("d_digests", ctypes.c_void_p),
                ("h_cap", ctypes.c_void_p), ("n_polys", ctypes.c_uint32), ("open_mask", ctypes.c_uint32)]


class CircuitShape(ctypes.Structure):
    """glp_circuit_shape"""
    _fields_ = [("log_n", ctypes.c_uint32), ("n_wires", ctypes.c_uint32), ("n_routed", ctypes.c_uint32), ("n_public", ctypes.c_uint32),
                ("rate_bits", ctypes.c_uint32), ("cap_height", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class CheckViolation(ctypes.Structure):
    """glp_check_violation"""
    _fields_ = [("kind", ctypes.c_uint32), ("row", ctypes.c_uint32), ("index", ctypes.c_uint32), ("n_in_row", ctypes.c_uint32),
                ("peer_wire", ctypes.c_uint32), ("peer_row", ctypes.c_uint32), ("value", ctypes.c_uint64), ("peer_value", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CheckSummary(ctypes.Structure):
    """glp_check_summary"""
    _fields_ = [("n_gate_bad", ctypes.c_uint64), ("n_copy_bad", ctypes.c_uint64), ("n_gate_rows", ctypes.c_uint32),
                ("n_copy_rows", ctypes.c_uint32), ("n_listed", ctypes.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Ed25519InputLayout(ctypes.Structure):
    """glp_ed25519_input_layout: which form of ed25519_circuit.witness_inputs a row has (ED25519_FORM_*), the window of message lengths
    (min = max in the plain and the flagged form) and whether the half-size scalar hints follow"""
    _fields_ = [("form", ctypes.c_uint32), ("msg_len_min", ctypes.c_uint32), ("msg_len_max", ctypes.c_uint32), ("split_scalars", ctypes.c_uint32)]

    def n_words(self):
        n = ctypes.c_uint64()
        if load_library().glp_ed25519_leaf_input_words(ctypes.byref(self), ctypes.byref(n)) != 0:
            raise GlpError("no statement has this input layout")
        return int(n.value)


ED25519_FORM_PLAIN, ED25519_FORM_FLAGGED, ED25519_FORM_VOTE = 0, 1, 2
ED25519_IN_OK, ED25519_IN_REJECT, ED25519_IN_NO_PAIR, ED25519_IN_INVALID = 0, 1, 2, 3


class HeaderChainLayout(ctypes.Structure):
    """glp_header_chain_layout: what a header-chain leaf recording fixes — the byte lengths of the 14 field encodings, the headers per leaf and
    the varint bytes of a height"""
    _fields_ = [("field_len", ctypes.c_uint32 * 14), ("leaf_headers", ctypes.c_uint32), ("n_groups", ctypes.c_uint32)]

    @classmethod
    def of(cls, field_lengths, leaf_headers, n_groups):
        if len(field_lengths) != 14:
            raise GlpError("a header has 14 field encodings")
        return cls((ctypes.c_uint32 * 14)(*[int(x) for x in field_lengths]), int(leaf_headers), int(n_groups))

    def header_bytes(self):
        return sum(self.field_len)

    def n_words(self):
        n = ctypes.c_uint64()
        if load_library().glp_header_chain_leaf_input_words(ctypes.byref(self), ctypes.byref(n)) != 0:
            raise GlpError("no leaf statement has this header layout")
        return int(n.value)


HEADER_CHAIN_OK, HEADER_CHAIN_BAD_LINK, HEADER_CHAIN_BAD_HEIGHT, HEADER_CHAIN_BAD_DATA_FIELD = 0, 1, 2, 3
TM_BATCH_MAX_LEAVES = 512
TM_FOREST_MAX_LEAVES = 1 << 24
TM_INCLUSION_OK, TM_INCLUSION_BAD_SHAPE, TM_INCLUSION_BAD_ROOT = 0, 1, 2


class DeviceRows:
    """rows [lo, hi) of a resident [n][stride] u64 buffer, for WitnessProgram.evaluate_device(d_inputs=): a view — free() releases nothing"""

    def __init__(self, buf, stride_words, lo, hi):
        self.buf, self.ptr, self.nbytes = buf, buf.ptr + lo * stride_words * 8, (hi - lo) * stride_words * 8

    def __int__(self):
        return self.ptr

    def free(self):
        self.ptr = None


CHECK_GATE, CHECK_COPY = 0, 1
CHECK_KIND_NAMES = {CHECK_GATE: "gate", CHECK_COPY: "copy"}


class CheckResult:
    """what PlonkCircuit.check* found for one witness: ok, summary (dict of the glp_check_summary counts) and violations (list of dicts, one per
    failing row and kind with that row's lowest failing index, ascending by (row, kind), at most max_list of them)"""

    def __init__(self, ok, summary, violations):
        self.ok, self.summary, self.violations = bool(ok), summary, violations

    def __bool__(self):
        return self.ok

    def first(self):
        return self.violations[0] if self.violations else None

    def describe(self):
        if self.ok:
            return "satisfied"
        s = self.summary
        head = f"{s['n_gate_bad']} failing gate constraints in {s['n_gate_rows']} rows, {s['n_copy_bad']} copy mismatches in {s['n_copy_rows']} rows"
        v = self.first()
        if v is None:
            return head
        return f"row {v['row']}, kind {CHECK_KIND_NAMES[v['kind']]}, index {v['index']} ({head})"

    def __repr__(self):
        return f"CheckResult({self.describe()})"


PLONK_NCONST = 6                 # constant columns: q_arith, c0, c1, c2, q_pi, q_pos
PLONK_NCONST_SHA = 10            # ... + q_she, q_sha, q_shw, q_add for circuits with SHA-256 rows
CIRCUIT_SHA_GATES = 2
CIRCUIT_EXT_GATE = 4                # one more constant column, q_ext (last): rows whose 8-wire chunks are extension multiply-adds
SHA_GATE_WIRES = 144
SHA_ROW_E, SHA_ROW_A, SHA_ROW_W, SHA_ROW_ADD = 0, 1, 2, 3
CIRCUIT_POSEIDON_GATE = 1
POS_GATE_WIRES = 135


class FriStatement(ctypes.Structure):
    """what a stand-alone FRI proof proves (glp_fri_statement): the caller compares it with the statement it expects"""
    _fields_ = [("log_n", ctypes.c_uint32), ("rate_bits", ctypes.c_uint32), ("cap_height", ctypes.c_uint32), ("n_batches", ctypes.c_uint32),
                ("n_points", ctypes.c_uint32), ("num_queries", ctypes.c_uint32), ("pow_bits", ctypes.c_uint32), ("total_polys", ctypes.c_uint32),
                ("shift", ctypes.c_uint64), ("zeta", ctypes.c_uint64 * 2), ("point_mult", ctypes.c_uint64 * 4),
                ("caps_word_off", ctypes.c_size_t), ("cap_words", ctypes.c_size_t), ("openings_word_off", ctypes.c_size_t),
                ("n_openings", ctypes.c_size_t), ("n_polys", ctypes.c_uint32 * 64), ("open_mask", ctypes.c_uint32 * 64)]

    def as_dict(self, proof):
        """decoded against the proof bytes: caps [n_batches][cap_words] and openings [(a, b)] in (point, batch, poly) order"""
        w = np.frombuffer(bytes(proof), dtype="<u8")
        caps = [[int(v) for v in w[self.caps_word_off + b * self.cap_words: self.caps_word_off + (b + 1) * self.cap_words]]
                for b in range(self.n_batches)]
        op = w[self.openings_word_off: self.openings_word_off + 2 * self.n_openings]
        return {"log_n": self.log_n, "rate_bits": self.rate_bits, "cap_height": self.cap_height, "n_batches": self.n_batches,
                "n_points": self.n_points, "num_queries": self.num_queries, "pow_bits": self.pow_bits, "shift": self.shift,
                "zeta": (self.zeta[0], self.zeta[1]), "point_mult": [self.point_mult[i] for i in range(self.n_points)],
                "n_polys": [self.n_polys[b] for b in range(self.n_batches)], "open_mask": [self.open_mask[b] for b in range(self.n_batches)],
                "caps": caps, "openings": [(int(op[2 * k]), int(op[2 * k + 1])) for k in range(self.n_openings)]}


class VerifyVerdict(ctypes.Structure):
    """one proof's verdict of a batched verification (glp_verify_verdict)"""
    _fields_ = [("status", ctypes.c_int32), ("reason", ctypes.c_uint32), ("query", ctypes.c_uint32), ("on_device", ctypes.c_uint32)]


NOT_WORDS = "proof length is not a whole number of u64 words"


class _ProofBatch:
    """B proofs as the batched verifiers take them: one 8-byte aligned copy each, a pointer table and a length table.  A proof that is not a
    whole number of words is never handed over: its verdict is the wrappers' own (as Prover._verify gives it)."""

    def __init__(self, proofs):
        self.raw = [bytes(p) for p in proofs]
        self.sent = [i for i, r in enumerate(self.raw) if r and len(r) % 8 == 0]
        self.words = [np.frombuffer(self.raw[i], dtype="<u8").copy() for i in self.sent]
        self.ptrs = (ctypes.c_void_p * max(1, len(self.sent)))(*[w.ctypes.data for w in self.words])
        self.lens = (ctypes.c_size_t * max(1, len(self.sent)))(*[w.nbytes for w in self.words])
        self.verdicts = (VerifyVerdict * max(1, len(self.sent)))()

    def results(self, lib):
        """[(ok, reason text or None, failing query or None)] in the callers' order"""
        out = [(False, NOT_WORDS, None)] * len(self.raw)
        for k, i in enumerate(self.sent):
            v = self.verdicts[k]
            if v.status == 0:
                out[i] = (True, None, None)
            else:
                out[i] = (False, lib.glp_verify_reason_text(v.reason).decode(), None if v.query == 0xFFFFFFFF else int(v.query))
        return out

    def spread(self, rows, fill):
        """per-sent-proof rows back into the callers' order"""
        out = [fill] * len(self.raw)
        for k, i in enumerate(self.sent):
            out[i] = rows[k]
        return out


def _publics_arg(publics, batch):
    """(pointer-or-None, n_public, keepalive) for [B][n_public] expected public inputs; None / UNBOUND = do not bind"""
    if publics is None or (isinstance(publics, str) and publics == UNBOUND):
        return None, 0, None
    rows = [[int(v) for v in publics[i]] for i in batch.sent]
    n_pub = len(rows[0]) if rows else 0
    if any(len(r) != n_pub for r in rows):
        raise GlpError("verify_batch: every proof of a batch takes the same number of expected public inputs")
    a = np.ascontiguousarray(rows, dtype=np.uint64).reshape(len(rows), n_pub)
    keep = a if a.size else np.zeros(1, dtype=np.uint64)
    return keep.ctypes.data, n_pub, keep


def _cap_arg(circuit_cap, who):
    if circuit_cap is None:
        raise GlpError(f"{who}: circuit_cap is required (pass UNBOUND to skip the binding explicitly)")
    return None if isinstance(circuit_cap, str) and circuit_cap == UNBOUND else np.ascontiguousarray(circuit_cap, dtype=np.uint64)


def plonk_verify_batch_host(constants, proofs, circuit_cap, min_queries=None, min_pow_bits=None, publics=None, want_digests=False,
                            want_counts=False):
    """B circuit proofs through the batched verifier WITHOUT a GPU (glp_plonk_verify_batch_host): the same host phase and the same item
    bodies as Prover.plonk_verify_batch, run one after the other.  Returns [(ok, reason, query)]; with want_digests / want_counts a tuple
    that also carries the [B] digests (None where the header does not parse) / (n_on_device, n_fallback)."""
    lib = load_library()
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in constants)
    if rc.size != 360 or circ.size != 12 or diag.size != 12:
        raise GlpError("Poseidon constants: 360 round constants, 12 + 12 MDS entries")
    b = _ProofBatch(proofs)
    cap = _cap_arg(circuit_cap, "plonk_verify_batch_host")
    pp, pn, keep = _publics_arg(publics, b)
    dg = np.zeros((max(1, len(b.sent)), 4), dtype=np.uint64)
    nd, nf = ctypes.c_uint32(0), ctypes.c_uint32(0)
    code = lib.glp_plonk_verify_batch_host(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, b.ptrs, b.lens, len(b.sent),
                                           cap.ctypes.data if cap is not None else None, cap.size if cap is not None else 0, pp, pn,
                                           DEFAULT_MIN_QUERIES if min_queries is None else min_queries,
                                           DEFAULT_MIN_POW_BITS if min_pow_bits is None else min_pow_bits, b.verdicts, dg.ctypes.data,
                                           ctypes.byref(nd), ctypes.byref(nf))
    if code != 0:
        raise GlpError(f"glp_plonk_verify_batch_host: {_ERR.get(code, code)}")
    out = (b.results(lib),)
    if want_digests:
        out += (b.spread([[int(v) for v in row] if row.any() else None for row in dg[:len(b.sent)]], None),)
    if want_counts:
        out += ((int(nd.value), int(nf.value)),)
    return out[0] if len(out) == 1 else out


def fri_verify_batch_host(constants, proofs, min_queries=None, min_pow_bits=None, min_rate_bits=None, want_counts=False):
    """B stand-alone FRI proofs through the batched verifier without a GPU (glp_fri_verify_batch_host): [(ok, reason, query)]"""
    lib = load_library()
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in constants)
    if rc.size != 360 or circ.size != 12 or diag.size != 12:
        raise GlpError("Poseidon constants: 360 round constants, 12 + 12 MDS entries")
    b = _ProofBatch(proofs)
    nd, nf = ctypes.c_uint32(0), ctypes.c_uint32(0)
    code = lib.glp_fri_verify_batch_host(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, b.ptrs, b.lens, len(b.sent),
                                         DEFAULT_MIN_QUERIES if min_queries is None else min_queries,
                                         DEFAULT_MIN_POW_BITS if min_pow_bits is None else min_pow_bits,
                                         DEFAULT_MIN_RATE_BITS if min_rate_bits is None else min_rate_bits, b.verdicts, None,
                                         ctypes.byref(nd), ctypes.byref(nf))
    if code != 0:
        raise GlpError(f"glp_fri_verify_batch_host: {_ERR.get(code, code)}")
    return (b.results(lib), (int(nd.value), int(nf.value))) if want_counts else b.results(lib)


# security parameters every verify wrapper requires unless the caller says otherwise: 28 queries at rate 1/8 + 16 bits of
# proof of work (the prover's defaults).  A proof made with weaker parameters is REJECTED by default.
DEFAULT_MIN_QUERIES = 28
DEFAULT_MIN_POW_BITS = 16
DEFAULT_MIN_RATE_BITS = 3
MERKLE_FUSE_DEFAULT = 0xFFFFFFFF      # glp_merkle_batch: the library's measured fusion threshold (include/glprover.h)
UNBOUND = "unbound"      # explicit opt-out for plonk_verify*: do not bind the proof to a circuit's verifying key


def load_library():
    """dlopen libglprover.so; raises GlpError (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GlpError(f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    # One HIP / HSA runtime per process.  PyTorch bundles its own copies (and its own RCCL, which binds to the HSA runtime by dlopen): if
    # this library initialises the system runtime FIRST and torch arrives later (mapreduce.py imports it), RCCL ends up on a second,
    # uninitialised HSA instance — ncclCommInitRank then fails with "no ROCm-capable device is detected" (found on the GPU box by running two
    # test files alone; the full suite imports torch at collection time, which is why it never showed there).  A Python process that can
    # import torch therefore does so BEFORE this library is loaded.  Hosts without Python (tests/cpp) have one runtime to begin with.
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001 — no torch: nothing to order
        pass
    lib = ctypes.CDLL(LIB_PATH)
    sig = {
        "glp_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int]),
        "glp_destroy": (None, [_vp]),
        "glp_last_error": (ctypes.c_char_p, [_vp]),
        "glp_version": (ctypes.c_char_p, []),
        "glp_alloc": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_size_t]),
        "glp_free": (ctypes.c_int, [_vp, _vp]),
        "glp_h2d": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
        "glp_d2h": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
        "glp_sync": (ctypes.c_int, [_vp]),
        "glp_trim_pool": (ctypes.c_int, [_vp]),
        "glp_bind_thread": (ctypes.c_int, [_vp]),
        "glp_set_stream": (ctypes.c_int, [_vp, _vp]),
        "glp_timer_start": (ctypes.c_int, [_vp]),
        "glp_timer_stop": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
        "glp_field_op": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_uint64]),
        "glp_fri_verify": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]),
        "glp_plonk_verify": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]),
        "glp_plonk_circuit_cap": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_size_t)]),
        "glp_tm_merkle_root_var": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp]),
        "glp_fri_verify_ex": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp]),
        "glp_fri_verify_host_ex": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                  _vp, ctypes.c_char_p, ctypes.c_size_t]),
        "glp_fri_verify_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p,
                                               ctypes.c_size_t]),
        "glp_plonk_verify_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_uint32,
                                                 ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]),
        "glp_ntt": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]),
        "glp_ntt_ex": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                      ctypes.c_uint64, ctypes.c_uint32]),
        "glp_lde_coset": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_uint64, ctypes.c_uint32]),
        "glp_transpose": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64]),
        "glp_ntt_set_plan": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_char_p]),
        "glp_ntt_describe_plan": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p,
                                                 ctypes.c_size_t]),
        "glp_set_profiling": (ctypes.c_int, [_vp, ctypes.c_int]),
        "glp_last_pass_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]),
        "glp_last_stage_ms": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_float),
                                             ctypes.POINTER(ctypes.c_int)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # optional entry points (bound when the library exports them)
    opt = {
        "glp_set_poseidon_constants": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, _vp]),
        "glp_poseidon_permute": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64]),
        "glp_merkle": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp]),
        "glp_merkle_from_polys": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_uint32, _vp, _vp]),
        "glp_merkle_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp]),
        "glp_merkle_batch_plan": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                                 ctypes.POINTER(ctypes.c_uint32)]),
        "glp_commit_values_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                   _vp, _vp, ctypes.c_uint64, _vp]),
        "glp_fri_fold2": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint64, _vp]),
        "glp_sha256_trace": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
        "glp_sha512_trace": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
        "glp_ed25519_witness": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp]),
        "glp_ed25519_leaf_input_words": (ctypes.c_int, [ctypes.POINTER(Ed25519InputLayout), ctypes.POINTER(ctypes.c_uint64)]),
        "glp_ed25519_leaf_inputs": (ctypes.c_int, [_vp, ctypes.POINTER(Ed25519InputLayout), _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp,
                                                   ctypes.c_uint64, _vp, ctypes.c_size_t, _vp]),
        "glp_ed25519_last_input_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 2),
        "glp_ed25519_half_scalars": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp]),
        "glp_tm_merkle_root": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint64, _vp]),
        "glp_tm_merkle_root_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp]),
        "glp_tm_merkle_root_batch_last_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 2),
        "glp_tm_merkle_root_batch_host": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp]),
        "glp_tm_forest_create": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp, ctypes.POINTER(_vp)]),
        "glp_tm_forest_info": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_uint64)]),
        "glp_tm_forest_roots": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
        "glp_tm_forest_destroy": (ctypes.c_int, [_vp]),
        "glp_tm_forest_proofs": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp]),
        "glp_tm_verify_inclusion_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp,
                                                         ctypes.c_uint64, _vp]),
        "glp_tm_forest_last_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 2),
        "glp_tm_forest_proofs_host": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, _vp, _vp,
                                                     ctypes.c_uint32, _vp, _vp]),
        "glp_tm_verify_inclusion_batch_host": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp,
                                                              ctypes.c_uint64, _vp]),
        "glp_header_chain_leaf_input_words": (ctypes.c_int, [ctypes.POINTER(HeaderChainLayout), ctypes.POINTER(ctypes.c_uint64)]),
        "glp_header_chain_leaf_inputs": (ctypes.c_int, [_vp, ctypes.POINTER(HeaderChainLayout), _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp,
                                                        ctypes.c_size_t, _vp, _vp]),
        "glp_header_chain_last_input_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 2),
        "glp_header_chain_leaf_inputs_host": (ctypes.c_int, [ctypes.POINTER(HeaderChainLayout), _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp,
                                                             ctypes.c_size_t, _vp, _vp]),
        "glp_challenger_new": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
        "glp_challenger_free": (None, [_vp]),
        "glp_challenger_observe": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
        "glp_challenger_challenges": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
        "glp_eval_at_ext": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp]),
        "glp_pow_grind": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp]),
        "glp_fri_prove": (ctypes.c_int, [_vp, ctypes.POINTER(FriConfig), ctypes.POINTER(FriBatch), ctypes.c_uint32,
                                         ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_size_t)]),
        "glp_free_host": (None, [_vp]),
        "glp_fri_prove_batch": (ctypes.c_int, [_vp, ctypes.POINTER(FriConfig), ctypes.POINTER(FriBatch), ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_size_t)]),
        "glp_fri_prove_batch_plan": (ctypes.c_int, [ctypes.POINTER(FriConfig), _vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                                    ctypes.POINTER(ctypes.c_uint32)]),
        "glp_fri_last_batch_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 3),
        "glp_pow_grind_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]),
        "glp_fri_fold_layer_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_uint64, _vp, ctypes.c_uint32]),
        "glp_plonk_setup": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.POINTER(_vp)]),
        "glp_plonk_free": (None, [_vp]),
        "glp_plonk_prove": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp),
                                           ctypes.POINTER(ctypes.c_size_t)]),
        "glp_plonk_debug_stage": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
        "glp_plonk_setup_ex": (ctypes.c_int, [_vp, ctypes.POINTER(CircuitShape), _vp, _vp, ctypes.POINTER(_vp)]),
        "glp_plonk_prove_ex": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp),
                                              ctypes.POINTER(ctypes.c_size_t)]),
        "glp_plonk_prove_batch": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_size_t)]),
        "glp_plonk_last_batch_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 2),
        "glp_plonk_check_witness": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32]),
        "glp_plonk_check_witness_batch": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), _vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32]),
        "glp_plonk_last_check_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 2),
        "glp_plonk_verify_ex": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_uint32,
                                               ctypes.c_uint32]),
        "glp_plonk_verify_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_uint32,
                                                  ctypes.c_uint32, _vp, _vp]),
        "glp_fri_verify_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp]),
        "glp_verify_reason_text": (ctypes.c_char_p, [ctypes.c_uint32]),
        "glp_verify_last_batch_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 4),
        "glp_plonk_verify_batch_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                                       ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.POINTER(ctypes.c_uint32),
                                                       ctypes.POINTER(ctypes.c_uint32)]),
        "glp_fri_verify_batch_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                     _vp, _vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
        "glp_plonk_verify_host_ex": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                                    ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]),
        "glp_plonk_proof_public_inputs": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, ctypes.POINTER(ctypes.c_size_t)]),
        "glp_poseidon_gate_fill_rows": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_uint32]),
        "glp_plonk_proof_digest": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
        "glp_plonk_proof_digest_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
        "glp_sha_gate_fill_rows": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32]),
        "glp_witness_eval": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_size_t)]),
        "glp_witness_eval_mt": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.c_size_t), _vp, ctypes.c_size_t, ctypes.c_uint32]),
        "glp_poseidon_permute_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t]),
        "glp_witness_plan_create": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
        "glp_witness_plan_destroy": (None, [_vp]),
        "glp_witness_plan_stats": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint64)] * 4),
        "glp_witness_plan_run_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        "glp_witness_eval_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_uint32, _vp, _vp]),
        "glp_witness_plan_create_ex": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                                      ctypes.POINTER(_vp)]),
        "glp_witness_plan_parts": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32), _vp, _vp, _vp]),
        "glp_witness_check_words": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32,
                                                   _vp, _vp]),
        "glp_witness_check_words_host": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32,
                                                        _vp, _vp]),
        "glp_gather_u64": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t]),
        "glp_witness_layout_create": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_size_t, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32,
                                                     _vp, ctypes.c_uint32, ctypes.POINTER(_vp), ctypes.c_char_p, ctypes.c_size_t]),
        "glp_witness_layout_destroy": (None, [_vp]),
        "glp_witness_layout_info": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]
                                    + [ctypes.POINTER(ctypes.c_uint32)] * 3),
        "glp_witness_place_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_uint32, _vp, ctypes.c_size_t, _vp]),
        "glp_witness_last_place_counts": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_uint32)] * 2),
        "glp_field_params": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]),
        "glp_comm_unique_id": (ctypes.c_int, [_vp]),
        "glp_comm_init": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
        "glp_comm_rank": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
        "glp_comm_destroy": (ctypes.c_int, [_vp]),
        "glp_comm_reserve": (ctypes.c_int, [_vp, ctypes.c_size_t]),
        "glp_allgather_proofs": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
        "glp_allreduce_min_u64": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
    }
    for name, (res, args) in opt.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def field_params():
    """(two-adic generator, log2 of w_64) of the loaded build (glp_field_params)"""
    lib = load_library()
    g, e = ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = lib.glp_field_params(ctypes.byref(g), ctypes.byref(e))
    if rc != 0:
        raise GlpError("glp_field_params: the build's two-adic generator pair is inconsistent")
    return int(g.value), int(e.value)


def _host_verify(fn_name, constants, proof, extra, min_queries, min_pow_bits):
    """(accepted, reason) from the ctx-less verifiers: works on a host without a GPU"""
    lib = load_library()
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in constants)
    if rc.size != 360 or circ.size != 12 or diag.size != 12:
        raise GlpError("Poseidon constants: 360 round constants, 12 + 12 MDS entries")
    raw = bytes(proof)
    if len(raw) % 8 or not raw:
        return False, "proof length is not a whole number of u64 words"
    words = np.frombuffer(raw, dtype="<u8").copy()
    err = ctypes.create_string_buffer(256)
    rcode = getattr(lib, fn_name)(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, words.ctypes.data, words.nbytes, *extra,
                                  min_queries, min_pow_bits, err, 256)
    if rcode == 0:
        return True, None
    if rcode == -7:
        return False, err.value.decode()
    raise GlpError(f"{fn_name}: {_ERR.get(rcode, rcode)}")


def fri_verify_host(constants, proof, min_queries=DEFAULT_MIN_QUERIES, min_pow_bits=DEFAULT_MIN_POW_BITS,
                    min_rate_bits=DEFAULT_MIN_RATE_BITS, want_statement=False):
    """verify a FRI opening proof without a GPU or a ctx; constants = (rc[360], mds_circ[12], mds_diag[12]).
    Returns (accepted, reason) — or (accepted, reason, statement dict) with want_statement: OK alone does not say WHICH
    statement was proven (log_n, caps, points, openings all come from the proof), compare the statement with yours."""
    lib = load_library()
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in constants)
    if rc.size != 360 or circ.size != 12 or diag.size != 12:
        raise GlpError("Poseidon constants: 360 round constants, 12 + 12 MDS entries")
    raw = bytes(proof)
    if len(raw) % 8 or not raw:
        return (False, "proof length is not a whole number of u64 words") + ((None,) if want_statement else ())
    words = np.frombuffer(raw, dtype="<u8").copy()
    err = ctypes.create_string_buffer(256)
    st = FriStatement()
    rcode = lib.glp_fri_verify_host_ex(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, words.ctypes.data, words.nbytes, min_queries,
                                       min_pow_bits, min_rate_bits, ctypes.addressof(st), err, 256)
    if rcode not in (0, -7):
        raise GlpError(f"glp_fri_verify_host_ex: {_ERR.get(rcode, rcode)}")
    res = (True, None) if rcode == 0 else (False, err.value.decode())
    return res + ((st.as_dict(raw) if rcode == 0 else None,) if want_statement else ())


def _public_arg(public):
    """(pointer-or-None, count, keepalive) for the h_public / n_public pair: None = the statement has NO public inputs (a proof
    carrying some is rejected), UNBOUND = do not bind, else the expected words"""
    if isinstance(public, str) and public == UNBOUND:
        return None, 0, None
    a = np.ascontiguousarray([] if public is None else [int(v) for v in public], dtype=np.uint64)
    keep = a if a.size else np.zeros(1, dtype=np.uint64)
    return keep.ctypes.data, a.size, keep


def plonk_verify_host(constants, proof, circuit_cap, min_queries=DEFAULT_MIN_QUERIES, min_pow_bits=DEFAULT_MIN_POW_BITS, public=None):
    """verify a circuit proof without a GPU or a ctx.  A proof is about (circuit, public inputs): circuit_cap
    (PlonkCircuit.cap()) binds the circuit — required; public = the expected public inputs (None: the statement has none).
    Pass UNBOUND for either to skip that binding explicitly (tests, diagnostics)."""
    if circuit_cap is None:
        raise GlpError("plonk_verify_host: circuit_cap is required (pass UNBOUND to skip the binding explicitly)")
    cap = None if isinstance(circuit_cap, str) and circuit_cap == UNBOUND else np.ascontiguousarray(circuit_cap, dtype=np.uint64)
    pp, pn, keep = _public_arg(public)
    extra = (cap.ctypes.data if cap is not None else None, cap.size if cap is not None else 0, pp, pn)
    return _host_verify("glp_plonk_verify_host_ex", constants, proof, extra, min_queries, min_pow_bits)


def poseidon_permute_host(consts, states):
    """Poseidon permutation of [n][12] states on the host (glp_poseidon_permute_host); consts = (rc[360], mds_circ[12], mds_diag[12])"""
    lib = load_library()
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in consts)
    s = np.array(states, dtype=np.uint64).reshape(-1, 12)
    code = lib.glp_poseidon_permute_host(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, s.ctypes.data, s.shape[0])
    if code != 0:
        raise GlpError(f"glp_poseidon_permute_host -> {code}")
    return s


def proof_digest_host(constants, proof):
    """Prover.proof_digest without a GPU or a ctx"""
    lib = load_library()
    rc, circ, diag = (np.ascontiguousarray(a, dtype=np.uint64) for a in constants)
    words = np.frombuffer(bytes(proof), dtype="<u8").copy()
    out = np.zeros(4, dtype=np.uint64)
    if lib.glp_plonk_proof_digest_host(rc.ctypes.data, circ.ctypes.data, diag.ctypes.data, words.ctypes.data, words.nbytes, out.ctypes.data) != 0:
        raise GlpError("not a circuit proof of this format")
    return [int(v) for v in out]


def proof_public_inputs(proof):
    """the public inputs a circuit proof carries (no verification)"""
    lib = load_library()
    words = np.frombuffer(bytes(proof), dtype="<u8").copy()
    n = ctypes.c_size_t(0)
    if lib.glp_plonk_proof_public_inputs(words.ctypes.data, words.nbytes, None, ctypes.byref(n)) != 0:
        raise GlpError("not a circuit proof of this format")
    out = np.zeros(max(1, n.value), dtype=np.uint64)
    n2 = ctypes.c_size_t(n.value)
    lib.glp_plonk_proof_public_inputs(words.ctypes.data, words.nbytes, out.ctypes.data, ctypes.byref(n2))
    return [int(v) for v in out[:n.value]]


class DeviceBuffer:
    """A hipMalloc'd block owned by a Prover (freed with it or by .free())."""

    def __init__(self, prover, nbytes):
        self.prover = prover
        self.nbytes = int(nbytes)
        p = _vp()
        prover._chk(prover.lib.glp_alloc(prover.ctx, ctypes.byref(p), self.nbytes), "glp_alloc")
        self.ptr = p.value
        prover._bufs.add(self)

    def free(self):
        if self.ptr:
            self.prover._chk(self.prover.lib.glp_free(self.prover.ctx, self.ptr), "glp_free")
            self.ptr = None
            self.prover._bufs.discard(self)

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        self.prover._chk(self.prover.lib.glp_h2d(self.prover.ctx, self.ptr, a.ctypes.data, a.nbytes), "glp_h2d")
        return self

    def download(self, shape, dtype=np.uint64, offset_bytes=0):
        out = np.empty(shape, dtype=dtype)
        assert offset_bytes + out.nbytes <= self.nbytes
        self.prover._chk(self.prover.lib.glp_d2h(self.prover.ctx, out.ctypes.data, self.ptr + offset_bytes, out.nbytes),
                         "glp_d2h")
        return out


def _ptr(x):
    """device pointer of a DeviceBuffer / torch tensor / int"""
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


class Prover:
    """One glp_ctx: one GPU, one stream.  Device-level calls take device pointers
    (DeviceBuffer, torch tensor or int); the numpy helpers below them copy in and out."""

    def __init__(self, device=0):
        self.lib = load_library()
        self._bufs = set()
        self._circuits = []
        ctx = _vp()
        rc = self.lib.glp_create(ctypes.byref(ctx), int(device))
        if rc != 0:
            raise GlpError(f"glp_create(device={device}) failed: {_ERR.get(rc, rc)} — no CPU fallback exists")
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            for ck in list(self._circuits):      # circuits hold pool blocks of this ctx: free them first
                ck.free()
            for b in list(self._bufs):
                b.free()
            self.lib.glp_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.glp_last_error(self.ctx)
            raise GlpError(f"{what}: {_ERR.get(rc, rc)}: {msg.decode() if msg else ''}")

    # ---- memory / stream -------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        a = np.ascontiguousarray(arr)
        return DeviceBuffer(self, max(a.nbytes, 8)).upload(a)

    def bind_thread(self):
        """call once from a worker thread before driving this prover from it (HIP's current device is per thread)"""
        self._chk(self.lib.glp_bind_thread(self.ctx), "glp_bind_thread")

    def sync(self):
        self._chk(self.lib.glp_sync(self.ctx), "glp_sync")

    def trim_pool(self):
        """return the prover drivers' cached temporaries to the driver (glp_trim_pool)"""
        self._chk(self.lib.glp_trim_pool(self.ctx), "glp_trim_pool")

    def set_stream(self, hip_stream):
        self._chk(self.lib.glp_set_stream(self.ctx, hip_stream), "glp_set_stream")

    def timer_start(self):
        self._chk(self.lib.glp_timer_start(self.ctx), "glp_timer_start")

    def timer_stop(self):
        ms = ctypes.c_float()
        self._chk(self.lib.glp_timer_stop(self.ctx, ctypes.byref(ms)), "glp_timer_stop")
        return ms.value

    # ---- MapReduce exchange behind the C ABI (RCCL communicator owned by the ctx) ------------------------
    COMM_ID_BYTES = 128

    @staticmethod
    def comm_unique_id():
        """rank 0 makes the id; hand its bytes to the other ranks out of band, then every rank calls comm_init"""
        lib = load_library()
        buf = ctypes.create_string_buffer(Prover.COMM_ID_BYTES)
        rc = lib.glp_comm_unique_id(buf)
        if rc != 0:
            raise GlpError(f"glp_comm_unique_id: {_ERR.get(rc, rc)}")
        return buf.raw

    def comm_init(self, comm_id, rank, nranks):
        assert len(comm_id) == self.COMM_ID_BYTES
        self._chk(self.lib.glp_comm_init(self.ctx, ctypes.create_string_buffer(bytes(comm_id), self.COMM_ID_BYTES), rank, nranks),
                  "glp_comm_init")
        self.comm_rank, self.comm_size = rank, nranks

    def comm_destroy(self):
        self._chk(self.lib.glp_comm_destroy(self.ctx), "glp_comm_destroy")
        self.comm_rank = self.comm_size = None

    def comm_reserve(self, block_bytes):
        """staging for exchanges of blocks this large (no collective inside: agree on the outcome before the exchange)"""
        self._chk(self.lib.glp_comm_reserve(self.ctx, int(block_bytes)), "glp_comm_reserve")

    def allgather_bytes(self, block):
        """every rank passes a block of the SAME length; returns the nranks blocks concatenated in rank order.  A GlpError from here means
        the ranks may be out of step: abort the job on every rank."""
        a = np.frombuffer(bytes(block), dtype=np.uint8)
        out = np.empty(a.size * self.comm_size, dtype=np.uint8)
        self._chk(self.lib.glp_allgather_proofs(self.ctx, a.ctypes.data, a.size, out.ctypes.data), "glp_allgather_proofs")
        return out

    def allreduce_min(self, values):
        v = np.ascontiguousarray(values, dtype=np.uint64).copy()
        self._chk(self.lib.glp_allreduce_min_u64(self.ctx, v.ctypes.data, v.size), "glp_allreduce_min_u64")
        return v

    FIELD_OPS = {"add": 0, "sub": 1, "mul": 2, "mul_pow2": 3, "inv": 4, "reduce128": 5, "reduce128_lazy": 6, "mul_any": 7,
                 "fold_small": 8, "mad_eps_lazy": 9, "mad_eps": 10}

    def field_op(self, op, a, b=None):
        """element-wise Goldilocks arithmetic on the GPU (the kernels' own device functions)"""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        da = self.to_device(a)
        db = self.to_device(np.ascontiguousarray(b, dtype=np.uint64)) if b is not None else None
        do = self.alloc(max(8, a.nbytes))
        self._chk(self.lib.glp_field_op(self.ctx, self.FIELD_OPS[op], da.ptr, db.ptr if db else None, do.ptr, a.size), "glp_field_op")
        out = do.download(a.shape)
        for x in (da, db, do):
            if x:
                x.free()
        return out

    # ---- device-level transforms -------------------------------------------------------
    def ntt_(self, d_io, log_n, batch=1, inverse=False):
        self._chk(self.lib.glp_ntt(self.ctx, _ptr(d_io), log_n, batch, 1 if inverse else 0), "glp_ntt")

    def ntt_ex(self, d_src, d_dst, log_n, batch=1, src_stride=None, dst_stride=None, flags=0):
        n = 1 << log_n
        self._chk(self.lib.glp_ntt_ex(self.ctx, _ptr(d_src), _ptr(d_dst), log_n, batch, src_stride or n,
                                      dst_stride or n, flags), "glp_ntt_ex")

    def lde_coset_(self, d_coeffs, d_out, log_n, rate_bits, batch=1, shift=COSET_SHIFT, flags=0):
        self._chk(self.lib.glp_lde_coset(self.ctx, _ptr(d_coeffs), _ptr(d_out), log_n, rate_bits, batch, shift, flags),
                  "glp_lde_coset")

    def transpose_(self, d_in, d_out, rows, cols):
        self._chk(self.lib.glp_transpose(self.ctx, _ptr(d_in), _ptr(d_out), rows, cols), "glp_transpose")

    def set_plan(self, log_n, plan):
        self._chk(self.lib.glp_ntt_set_plan(self.ctx, log_n, plan.encode() if plan else None), "glp_ntt_set_plan")

    def describe_plan(self, log_n, batch=1, flags=0):
        buf = ctypes.create_string_buffer(256)
        self._chk(self.lib.glp_ntt_describe_plan(self.ctx, log_n, batch, flags, buf, 256), "glp_ntt_describe_plan")
        return buf.value.decode()

    def set_profiling(self, on):
        self._chk(self.lib.glp_set_profiling(self.ctx, 1 if on else 0), "glp_set_profiling")

    def last_pass_ms(self):
        ms = (ctypes.c_float * 8)()
        n = ctypes.c_int()
        self._chk(self.lib.glp_last_pass_ms(self.ctx, ms, ctypes.byref(n)), "glp_last_pass_ms")
        return [ms[i] for i in range(n.value)]

    def last_stage_ms(self):
        """[(stage name, ms)] of the last prove while profiling was on"""
        names = ctypes.create_string_buffer(2048)
        ms = (ctypes.c_float * 32)()
        n = ctypes.c_int(32)
        self._chk(self.lib.glp_last_stage_ms(self.ctx, names, 2048, ms, ctypes.byref(n)), "glp_last_stage_ms")
        ns = names.value.decode().split(";") if n.value else []
        return [(ns[i], round(ms[i], 3)) for i in range(n.value)]

    # ---- numpy in / numpy out (upstream names, recalled: plonky2_field::fft) -----------
    def _xform(self, x, flags):
        x = np.ascontiguousarray(x, dtype=np.uint64)
        one = x.ndim == 1
        a = x.reshape(1, -1) if one else x
        batch, n = a.shape
        log_n = n.bit_length() - 1
        assert 1 << log_n == n, "length must be a power of two"
        d = self.to_device(a)
        self.ntt_ex(d, d, log_n, batch, flags=flags)
        out = d.download(a.shape)
        d.free()
        return out[0] if one else out

    def fft(self, coeffs):
        """coefficients -> evaluations on <w_n>, natural order"""
        return self._xform(coeffs, 0)

    def ifft(self, values):
        """evaluations -> coefficients (inverse transform, scaled by 1/n)"""
        return self._xform(values, NTT_INVERSE)

    def fft_bitrev(self, coeffs):
        return self._xform(coeffs, NTT_BITREV)

    def lde(self, coeffs, rate_bits, shift=COSET_SHIFT, bitrev=False):
        """coset low-degree extension: [batch][n] coefficients -> [batch][n << rate_bits] values"""
        x = np.ascontiguousarray(coeffs, dtype=np.uint64)
        one = x.ndim == 1
        a = x.reshape(1, -1) if one else x
        batch, n = a.shape
        log_n = n.bit_length() - 1
        assert 1 << log_n == n
        d_in = self.to_device(a)
        d_out = self.alloc(a.nbytes << rate_bits)
        self.lde_coset_(d_in, d_out, log_n, rate_bits, batch, shift, NTT_BITREV if bitrev else 0)
        out = d_out.download((batch, n << rate_bits))
        d_in.free()
        d_out.free()
        return out[0] if one else out

    def coset_fft(self, coeffs, shift=COSET_SHIFT):
        return self.lde(coeffs, 0, shift)

    # ---- Poseidon / Merkle / FRI / SHA-2 (rows a4, a8, a9) -------------------------------
    def set_poseidon_constants(self, rc, circ, diag):
        rc = np.ascontiguousarray(rc, dtype=np.uint64)
        circ = np.ascontiguousarray(circ, dtype=np.uint64)
        diag = np.ascontiguousarray(diag, dtype=np.uint64)
        self._chk(self.lib.glp_set_poseidon_constants(self.ctx, rc.ctypes.data, rc.size, circ.ctypes.data, diag.ctypes.data),
                  "glp_set_poseidon_constants")
        self._pos_consts = (rc.copy(), circ.copy(), diag.copy())

    def poseidon_permute_host(self, states):
        """the same permutation by the library's host arithmetic (no device round trip: what the circuit builder hashes single states with)"""
        if getattr(self, "_pos_consts", None) is None:
            raise GlpError("poseidon_permute_host: set_poseidon_constants first")
        return poseidon_permute_host(self._pos_consts, states)

    def poseidon_permute_(self, d_states, n):
        self._chk(self.lib.glp_poseidon_permute(self.ctx, _ptr(d_states), n), "glp_poseidon_permute")

    def poseidon_permute(self, states):
        s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 12)
        d = self.to_device(s)
        self.poseidon_permute_(d, s.shape[0])
        out = d.download(s.shape)
        d.free()
        return out

    @staticmethod
    def merkle_digest_len(log_leaves, cap_h):
        return 4 * ((2 << log_leaves) - (1 << cap_h))

    def merkle_(self, d_src, leaf_len, log_leaves, cap_h, d_digests, poly_major=False, poly_stride=None, want_cap=True):
        cap = np.zeros((1 << cap_h, 4), dtype=np.uint64) if want_cap else None
        capp = cap.ctypes.data if want_cap else None
        if poly_major:
            self._chk(self.lib.glp_merkle_from_polys(self.ctx, _ptr(d_src), poly_stride or (1 << log_leaves), leaf_len, log_leaves,
                                                     cap_h, _ptr(d_digests), capp), "glp_merkle_from_polys")
        else:
            self._chk(self.lib.glp_merkle(self.ctx, _ptr(d_src), leaf_len, log_leaves, cap_h, _ptr(d_digests), capp), "glp_merkle")
        return cap

    def merkle_tree(self, leaves, cap_h, poly_major=False):
        """leaves [n_leaves][leaf_len] (or, poly_major, [leaf_len][n_leaves]) -> (digests, cap)"""
        a = np.ascontiguousarray(leaves, dtype=np.uint64)
        n_leaves, leaf_len = (a.shape[1], a.shape[0]) if poly_major else a.shape
        log_leaves = n_leaves.bit_length() - 1
        assert 1 << log_leaves == n_leaves
        d = self.to_device(a)
        nd = self.merkle_digest_len(log_leaves, cap_h)
        dd = self.alloc(nd * 8)
        cap = self.merkle_(d, leaf_len, log_leaves, cap_h, dd, poly_major=poly_major)
        dig = dd.download((nd // 4, 4))
        d.free()
        dd.free()
        return dig, cap

    @staticmethod
    def merkle_batch_plan(log_leaves, cap_h, fuse_max_log=None):
        """(launches, fused launches) glp_merkle_batch issues for one shape, leaf hashing included (host only)"""
        n, f = ctypes.c_uint32(), ctypes.c_uint32()
        rc = load_library().glp_merkle_batch_plan(log_leaves, cap_h, MERKLE_FUSE_DEFAULT if fuse_max_log is None else fuse_max_log,
                                                  ctypes.byref(n), ctypes.byref(f))
        if rc != 0:
            raise GlpError(f"glp_merkle_batch_plan: {_ERR.get(rc, rc)}")
        return n.value, f.value

    def merkle_batch_(self, d_src, src_tree_stride, leaf_len, log_leaves, cap_h, B, d_digests, digest_tree_stride=None, poly_major=False,
                      poly_stride=None, fuse_max_log=None, want_caps=True):
        """B trees of one shape in one call (glp_merkle_batch): strides in u64 words; returns caps [B][2^cap_h][4], or None (and no
        synchronisation) with want_caps=False"""
        caps = np.zeros((B, 1 << cap_h, 4), dtype=np.uint64) if want_caps else None
        self._chk(self.lib.glp_merkle_batch(self.ctx, _ptr(d_src), src_tree_stride, 1 if poly_major else 0,
                                            (poly_stride or (1 << log_leaves)) if poly_major else 0, leaf_len, log_leaves, cap_h, B,
                                            MERKLE_FUSE_DEFAULT if fuse_max_log is None else fuse_max_log, _ptr(d_digests),
                                            self.merkle_digest_len(log_leaves, cap_h) if digest_tree_stride is None else digest_tree_stride,
                                            caps.ctypes.data if want_caps and B else None), "glp_merkle_batch")
        return caps

    def merkle_trees(self, leaves, cap_h, poly_major=False, fuse_max_log=None):
        """the batched twin of merkle_tree: leaves [B][n_leaves][leaf_len] (or, poly_major, [B][leaf_len][n_leaves]) ->
        (digests [B][*][4], caps [B][2^cap_h][4])"""
        a = np.ascontiguousarray(leaves, dtype=np.uint64)
        assert a.ndim == 3
        B = a.shape[0]
        n_leaves, leaf_len = (a.shape[2], a.shape[1]) if poly_major else a.shape[1:]
        log_leaves = n_leaves.bit_length() - 1
        assert 1 << log_leaves == n_leaves
        nd = self.merkle_digest_len(log_leaves, cap_h)
        d = self.to_device(a)
        dd = self.alloc(max(8, B * nd * 8))
        caps = self.merkle_batch_(d, n_leaves * leaf_len, leaf_len, log_leaves, cap_h, B, dd, poly_major=poly_major, fuse_max_log=fuse_max_log)
        dig = dd.download((B, nd // 4, 4))
        d.free()
        dd.free()
        return dig, caps

    def fri_fold2(self, evals, shift, beta):
        """evals [n][2] in bit-reversed order over shift*<w_n> -> [n/2][2]"""
        e = np.ascontiguousarray(evals, dtype=np.uint64)
        n = e.shape[0]
        log_n = n.bit_length() - 1
        b = np.ascontiguousarray(beta, dtype=np.uint64)
        d = self.to_device(e)
        o = self.alloc(max(8, e.nbytes // 2))
        self._chk(self.lib.glp_fri_fold2(self.ctx, d.ptr, o.ptr, log_n, shift, b.ctypes.data), "glp_fri_fold2")
        out = o.download((n // 2, 2))
        d.free()
        o.free()
        return out

    def sha256_trace(self, padded, blocks_per_msg, want_trace=True):
        """padded: [n_msgs][blocks_per_msg*64] uint8 -> (digests [n][8] u32, trace [n][blocks][576] u32)"""
        m = np.ascontiguousarray(padded, dtype=np.uint8)
        n = m.shape[0]
        d = self.to_device(m)
        dd = self.alloc(max(8, n * 32))
        dt = self.alloc(n * blocks_per_msg * 576 * 4) if want_trace and n else None
        self._chk(self.lib.glp_sha256_trace(self.ctx, d.ptr, n, blocks_per_msg, dd.ptr, dt.ptr if dt else None), "glp_sha256_trace")
        dig = dd.download((n, 8), np.uint32)
        tr = dt.download((n, blocks_per_msg, 576), np.uint32) if dt else None
        for b in (d, dd, dt):
            if b:
                b.free()
        return dig, tr

    def sha512_trace(self, padded, blocks_per_msg, want_trace=True):
        m = np.ascontiguousarray(padded, dtype=np.uint8)
        n = m.shape[0]
        d = self.to_device(m)
        dd = self.alloc(max(8, n * 64))
        dt = self.alloc(n * blocks_per_msg * 720 * 8) if want_trace and n else None
        self._chk(self.lib.glp_sha512_trace(self.ctx, d.ptr, n, blocks_per_msg, dd.ptr, dt.ptr if dt else None), "glp_sha512_trace")
        dig = dd.download((n, 8), np.uint64)
        tr = dt.download((n, blocks_per_msg, 720), np.uint64) if dt else None
        for b in (d, dd, dt):
            if b:
                b.free()
        return dig, tr

    # ---- transcript + FRI opening proof (rows a5, a8, a12; build-defined protocol) ---------
    def challenger(self):
        return Challenger(self)

    def eval_at_ext(self, d_coeffs, log_n, n_polys, z, stride=None):
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros((n_polys, 2), dtype=np.uint64)
        self._chk(self.lib.glp_eval_at_ext(self.ctx, _ptr(d_coeffs), stride or (1 << log_n), log_n, n_polys, zz.ctypes.data,
                                           out.ctypes.data), "glp_eval_at_ext")
        return out

    def pow_grind(self, seed4, pow_bits):
        sd = np.ascontiguousarray(seed4, dtype=np.uint64)
        nonce = ctypes.c_uint64()
        self._chk(self.lib.glp_pow_grind(self.ctx, sd.ctypes.data, pow_bits, ctypes.byref(nonce)), "glp_pow_grind")
        return nonce.value

    def fri_prove(self, batches, rate_bits, cap_height, arity_bits=4, final_poly_bits=5, num_queries=28, pow_bits=16,
                  shift=COSET_SHIFT, point_mults=(1,), open_masks=None):
        """batches: PolynomialBatch objects of equal log_n committed with (rate_bits, cap_height).
        point_mults: opening points zeta*m; open_masks[i]: bitmask of points batch i is opened at
        (default: every batch at every point).  Returns the proof bytes (little-endian u64 words)."""
        log_n = batches[0].log_n
        pm = (ctypes.c_uint64 * 4)(*(list(point_mults) + [0] * (4 - len(point_mults))))
        cfg = FriConfig(log_n, rate_bits, cap_height, arity_bits, final_poly_bits, num_queries, pow_bits, shift, len(point_mults), pm)
        if open_masks is None:
            open_masks = [(1 << len(point_mults)) - 1] * len(batches)
        arr = (FriBatch * len(batches))()
        keep = []
        for i, b in enumerate(batches):
            assert b.log_n == log_n and b.rate_bits == rate_bits
            cap = np.ascontiguousarray(b.cap, dtype=np.uint64)
            keep.append(cap)
            arr[i] = FriBatch(_ptr(b.coeffs), _ptr(b.lde), _ptr(b.digests), cap.ctypes.data, b.n_polys, open_masks[i])
        proof = _vp()
        ln = ctypes.c_size_t()
        self._chk(self.lib.glp_fri_prove(self.ctx, ctypes.byref(cfg), arr, len(batches), ctypes.byref(proof), ctypes.byref(ln)),
                  "glp_fri_prove")
        data = ctypes.string_at(proof.value, ln.value)
        self.lib.glp_free_host(proof)
        return data

    @staticmethod
    def _fri_config(log_n, rate_bits, cap_height, arity_bits, final_poly_bits, num_queries, pow_bits, shift, point_mults):
        pm = (ctypes.c_uint64 * 4)(*(list(point_mults) + [0] * (4 - len(point_mults))))
        return FriConfig(log_n, rate_bits, cap_height, arity_bits, final_poly_bits, num_queries, pow_bits, shift, len(point_mults), pm)

    def fri_prove_batch(self, instances, rate_bits, cap_height, arity_bits=4, final_poly_bits=5, num_queries=28, pow_bits=16,
                        shift=COSET_SHIFT, point_mults=(1,), open_masks=None):
        """B opening proofs of one shape in one call (glp_fri_prove_batch).  instances: a list of lists of PolynomialBatch, one inner
        list per proof (views of from_values_batch and objects of from_values may be mixed, and an object may appear in several
        instances).  Returns the B proofs, each byte for byte what fri_prove returns for that instance alone."""
        B = len(instances)
        if B == 0:
            return []
        nb = len(instances[0])
        log_n = instances[0][0].log_n
        cfg = self._fri_config(log_n, rate_bits, cap_height, arity_bits, final_poly_bits, num_queries, pow_bits, shift, point_mults)
        if open_masks is None:
            open_masks = [(1 << len(point_mults)) - 1] * nb
        arr = (FriBatch * (B * nb))()
        keep = []
        for i, inst in enumerate(instances):
            assert len(inst) == nb
            for j, b in enumerate(inst):
                assert b.log_n == log_n and b.rate_bits == rate_bits
                cap = np.ascontiguousarray(b.cap, dtype=np.uint64)
                keep.append(cap)
                arr[i * nb + j] = FriBatch(_ptr(b.coeffs), _ptr(b.lde), _ptr(b.digests), cap.ctypes.data, b.n_polys, open_masks[j])
        proofs = (_vp * B)()
        lens = (ctypes.c_size_t * B)()
        self._chk(self.lib.glp_fri_prove_batch(self.ctx, ctypes.byref(cfg), arr, nb, B, proofs, lens), "glp_fri_prove_batch")
        out = []
        for i in range(B):
            out.append(ctypes.string_at(proofs[i], lens[i]))
            self.lib.glp_free_host(proofs[i])
        return out

    @staticmethod
    def fri_prove_batch_plan(log_n, rate_bits, cap_height, open_masks, arity_bits=4, final_poly_bits=5, num_queries=28, pow_bits=16,
                             shift=COSET_SHIFT, point_mults=(1,)):
        """(launches, stream synchronises) one fri_prove_batch call issues for that shape when every PoW search ends in its first
        window, whatever B is (host only)"""
        cfg = Prover._fri_config(log_n, rate_bits, cap_height, arity_bits, final_poly_bits, num_queries, pow_bits, shift, point_mults)
        masks = np.ascontiguousarray(open_masks, dtype=np.uint32)
        nl, ns = ctypes.c_uint32(), ctypes.c_uint32()
        rc = load_library().glp_fri_prove_batch_plan(ctypes.byref(cfg), masks.ctypes.data, masks.size, ctypes.byref(nl), ctypes.byref(ns))
        if rc != 0:
            raise GlpError(f"glp_fri_prove_batch_plan: {_ERR.get(rc, rc)}")
        return nl.value, ns.value

    def fri_last_batch_counts(self):
        """(launches, stream synchronises, PoW windows) of the last fri_prove_batch on this prover"""
        v = [ctypes.c_uint32() for _ in range(3)]
        self._chk(self.lib.glp_fri_last_batch_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_fri_last_batch_counts")
        return tuple(x.value for x in v)

    def plonk_last_batch_counts(self):
        """(launches, stream synchronises) the PLONK driver's own code issued in the last PlonkCircuit.prove_batch_ on this prover; the opening
        proof's are fri_last_batch_counts()"""
        v = [ctypes.c_uint32() for _ in range(2)]
        self._chk(self.lib.glp_plonk_last_batch_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_plonk_last_batch_counts")
        return tuple(x.value for x in v)

    def plonk_last_check_counts(self):
        """(kernel launches, stream synchronises) of the last PlonkCircuit.check* on this prover (glp_plonk_last_check_counts)"""
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._chk(self.lib.glp_plonk_last_check_counts(self.ctx, ctypes.byref(a), ctypes.byref(b)), "glp_plonk_last_check_counts")
        return a.value, b.value

    def pow_grind_batch(self, seeds, pow_bits):
        """seeds [B][4] -> B nonces, each what pow_grind returns for that seed"""
        sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(sd.shape[0], dtype=np.uint64)
        self._chk(self.lib.glp_pow_grind_batch(self.ctx, sd.ctypes.data, sd.shape[0], pow_bits, out.ctypes.data), "glp_pow_grind_batch")
        return [int(v) for v in out]

    def fri_fold_layer_batch_(self, d_in, in_stride, d_out, out_stride, log_len, arity_bits, shift, betas, B):
        """one committed fold layer of B codewords on the device (glp_fri_fold_layer_batch); strides in u64 words"""
        b = np.ascontiguousarray(betas, dtype=np.uint64)
        self._chk(self.lib.glp_fri_fold_layer_batch(self.ctx, _ptr(d_in), in_stride, _ptr(d_out), out_stride, log_len, arity_bits, shift,
                                                    b.ctypes.data, B), "glp_fri_fold_layer_batch")

    def fri_fold_layer_batch(self, evals, arity_bits, shift, betas):
        """evals [B][2^log_len][2] (bit-reversed order over shift*<w>), betas [B][2] -> [B][2^(log_len - arity_bits)][2]: what arity_bits
        successive fri_fold2 calls give per codeword"""
        e = np.ascontiguousarray(evals, dtype=np.uint64)
        B, n = e.shape[0], e.shape[1]
        log_len = n.bit_length() - 1
        d = self.to_device(e)
        o = self.alloc(max(16, B * (16 * n >> arity_bits)))
        self.fri_fold_layer_batch_(d, 2 * n, o, 2 * n >> arity_bits, log_len, arity_bits, shift, betas, B)
        out = o.download((B, n >> arity_bits, 2))
        d.free()
        o.free()
        return out

    def _verify(self, what, call, proof):
        """True = accepted, False = rejected (reason in self.last_reject); bad arguments raise"""
        buf = np.frombuffer(bytes(proof) + b"", dtype=np.uint8)
        if buf.size % 8 or buf.size == 0:
            self.last_reject = "proof length is not a whole number of u64 words"
            return False
        words = np.frombuffer(buf.tobytes(), dtype="<u8").copy()          # 8-byte aligned copy
        rc = call(words.ctypes.data, words.nbytes)
        if rc == 0:
            self.last_reject = None
            return True
        if rc == -7:
            msg = self.lib.glp_last_error(self.ctx)
            self.last_reject = msg.decode() if msg else "rejected"
            return False
        self._chk(rc, what)

    def fri_verify(self, proof, min_queries=DEFAULT_MIN_QUERIES, min_pow_bits=DEFAULT_MIN_POW_BITS, min_rate_bits=DEFAULT_MIN_RATE_BITS):
        """native verifier of a stand-alone FRI opening proof (glp_fri_verify_ex).  On acceptance self.last_statement holds WHAT
        was proven (log_n, caps, points, openings): the caller must compare it with the statement it expects."""
        st = FriStatement()
        ok = self._verify("glp_fri_verify_ex", lambda p, n: self.lib.glp_fri_verify_ex(self.ctx, p, n, min_queries, min_pow_bits,
                                                                                     min_rate_bits, ctypes.addressof(st)), proof)
        self.last_statement = st.as_dict(proof) if ok else None
        return ok

    def plonk_verify(self, proof, circuit_cap, min_queries=DEFAULT_MIN_QUERIES, min_pow_bits=DEFAULT_MIN_POW_BITS, public=None):
        """native verifier of a PlonkCircuit proof.  A proof is about (circuit, public inputs): circuit_cap (PlonkCircuit.cap())
        binds the circuit — required; public = the expected public inputs (None: the statement has none).  UNBOUND for either
        skips that binding explicitly."""
        if circuit_cap is None:
            raise GlpError("plonk_verify: circuit_cap is required (pass UNBOUND to skip the binding explicitly)")
        cap = None if isinstance(circuit_cap, str) and circuit_cap == UNBOUND else np.ascontiguousarray(circuit_cap, dtype=np.uint64)
        pp, pn, keep = _public_arg(public)
        return self._verify("glp_plonk_verify_ex",
                            lambda p, n: self.lib.glp_plonk_verify_ex(self.ctx, p, n, cap.ctypes.data if cap is not None else None,
                                                                      cap.size if cap is not None else 0, pp, pn, min_queries, min_pow_bits),
                            proof)

    def plonk_verify_batch(self, proofs, circuit_cap, min_queries=DEFAULT_MIN_QUERIES, min_pow_bits=DEFAULT_MIN_POW_BITS, publics=None,
                           want_digests=False):
        """B circuit proofs in one call, their query phases on the device (glp_plonk_verify_batch; opt-in).  circuit_cap as for plonk_verify
        (required, UNBOUND skips the binding); publics: None / UNBOUND = do not bind, else one row of expected public inputs per proof.
        Returns [(ok, reason text, failing query)] — what plonk_verify and last_reject give proof by proof; with want_digests also the
        proofs' digests (proof_digest), None where the header does not parse."""
        b = _ProofBatch(proofs)
        cap = _cap_arg(circuit_cap, "plonk_verify_batch")
        pp, pn, keep = _publics_arg(publics, b)
        dg = np.zeros((max(1, len(b.sent)), 4), dtype=np.uint64)
        self._chk(self.lib.glp_plonk_verify_batch(self.ctx, b.ptrs, b.lens, len(b.sent), cap.ctypes.data if cap is not None else None,
                                                  cap.size if cap is not None else 0, pp, pn, min_queries, min_pow_bits, b.verdicts,
                                                  dg.ctypes.data), "glp_plonk_verify_batch")
        res = b.results(self.lib)
        if want_digests:
            return res, b.spread([[int(v) for v in row] if row.any() else None for row in dg[:len(b.sent)]], None)
        return res

    def fri_verify_batch(self, proofs, min_queries=DEFAULT_MIN_QUERIES, min_pow_bits=DEFAULT_MIN_POW_BITS, min_rate_bits=DEFAULT_MIN_RATE_BITS,
                         want_statements=False):
        """B stand-alone FRI proofs in one call (glp_fri_verify_batch): [(ok, reason text, failing query)]; with want_statements also what
        each accepted proof proves (as fri_verify leaves it in last_statement), None for a refused one"""
        b = _ProofBatch(proofs)
        sts = (FriStatement * max(1, len(b.sent)))()
        self._chk(self.lib.glp_fri_verify_batch(self.ctx, b.ptrs, b.lens, len(b.sent), min_queries, min_pow_bits, min_rate_bits, b.verdicts,
                                                sts), "glp_fri_verify_batch")
        res = b.results(self.lib)
        if want_statements:
            rows = [sts[k].as_dict(b.raw[i]) if b.verdicts[k].status == 0 else None for k, i in enumerate(b.sent)]
            return res, b.spread(rows, None)
        return res

    def verify_last_batch_counts(self):
        """what the last *_verify_batch on this ctx issued: dict launches, host_syncs, on_device, fallback"""
        v = [ctypes.c_uint32(0) for _ in range(4)]
        self._chk(self.lib.glp_verify_last_batch_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_verify_last_batch_counts")
        return dict(zip(("launches", "host_syncs", "on_device", "fallback"), (int(x.value) for x in v)))

    def proof_digest(self, proof):
        """4-word digest of a circuit proof's statement and commitments (glp_plonk_proof_digest): the aggregation tree's leaf"""
        words = np.frombuffer(bytes(proof), dtype="<u8").copy()
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.glp_plonk_proof_digest(self.ctx, words.ctypes.data, words.nbytes, out.ctypes.data), "glp_plonk_proof_digest")
        return [int(v) for v in out]

    def poseidon_gate_fill_rows(self, d_wires, log_n, n_wires, rows):
        """witness generation for Poseidon rows: wires 12..129 of every listed row from its wires 0..11, in place on the device"""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        if r.size == 0:
            return
        dr = self.to_device(r)
        try:
            self._chk(self.lib.glp_poseidon_gate_fill_rows(self.ctx, _ptr(d_wires), log_n, n_wires, dr.ptr, r.size), "glp_poseidon_gate_fill_rows")
            self.sync()
        finally:
            dr.free()

    def sha_gate_fill_rows(self, d_wires, log_n, n_wires, rows, kinds):
        """witness generation for SHA rows: the bit wires 12..143 of row rows[k] (kind kinds[k]) from its routed words, in place on the device"""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        k = np.ascontiguousarray(kinds, dtype=np.uint32)
        assert r.size == k.size
        if r.size == 0:
            return
        dr, dk = self.to_device(r), self.to_device(k)
        try:
            self._chk(self.lib.glp_sha_gate_fill_rows(self.ctx, _ptr(d_wires), log_n, n_wires, dr.ptr, dk.ptr, r.size), "glp_sha_gate_fill_rows")
            self.sync()
        finally:
            dr.free()
            dk.free()

    def gather(self, d_dst, d_src, n_src, d_index, n):
        """d_dst[i] = d_src[d_index[i]] (0xFFFFFFFF -> 0), all on the device: witness placement (glp_gather_u64)"""
        self._chk(self.lib.glp_gather_u64(self.ctx, _ptr(d_dst), _ptr(d_src), n_src, _ptr(d_index), n), "glp_gather_u64")

    def witness_place_batch(self, layout, d_values, value_stride, rows, d_wires, wire_stride_words, want_public=True):
        """B wire matrices side by side from slab rows `rows` of d_values (glp_witness_place_batch: at most 4 launches and 1 synchronise whatever
        B is).  layout: a glp_witness_layout handle (WitnessProgram.layout()).  Returns the [B][n_public] public values, or None with
        want_public=False (then the call only enqueues work on this prover's stream)."""
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        B = r.size
        n_pub = ctypes.c_uint32(0)
        self._chk(self.lib.glp_witness_layout_info(layout, None, None, None, None, None, ctypes.byref(n_pub)), "glp_witness_layout_info")
        pub = np.zeros((B, n_pub.value), dtype=np.uint64) if want_public else None
        self._chk(self.lib.glp_witness_place_batch(self.ctx, layout, _ptr(d_values), value_stride, r.ctypes.data if B else None, B, _ptr(d_wires),
                                                   wire_stride_words, pub.ctypes.data if pub is not None and pub.size else None),
                  "glp_witness_place_batch")
        return pub

    def witness_last_place_counts(self):
        """(launches, stream synchronises) of the last witness_place_batch on this prover"""
        v = [ctypes.c_uint32() for _ in range(2)]
        self._chk(self.lib.glp_witness_last_place_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_witness_last_place_counts")
        return tuple(x.value for x in v)

    def ed25519_witness(self, pubs, sigs, msgs):
        """pubs/sigs/msgs: lists of bytes.  Returns [n][37] u64 records (glprover.h)."""
        n = len(pubs)
        stride = max(1, max((len(m) for m in msgs), default=1))
        P = np.zeros((n, 32), dtype=np.uint8)
        S = np.zeros((n, 64), dtype=np.uint8)
        M = np.zeros((n, stride), dtype=np.uint8)
        Ln = np.zeros(n, dtype=np.uint32)
        for i in range(n):
            P[i] = np.frombuffer(pubs[i], dtype=np.uint8)
            S[i] = np.frombuffer(sigs[i], dtype=np.uint8)
            M[i, :len(msgs[i])] = np.frombuffer(msgs[i], dtype=np.uint8)
            Ln[i] = len(msgs[i])
        dp, ds, dm, dl = (self.to_device(a) for a in (P, S, M, Ln))
        do = self.alloc(max(8, n * 37 * 8))
        self._chk(self.lib.glp_ed25519_witness(self.ctx, dp.ptr, ds.ptr, dm.ptr, stride, dl.ptr, n, do.ptr), "glp_ed25519_witness")
        out = do.download((n, 37))
        for b in (dp, ds, dm, dl, do):
            b.free()
        return out

    def ed25519_leaf_inputs(self, layout, pubs, sigs, msgs, flags=None, dummy=None, out=None):
        """the input vectors of a signature leaf for B slots, built ON THE DEVICE (glp_ed25519_leaf_inputs): (DeviceBuffer of [B][layout.n_words()]
        u64, status int32[B] of ED25519_IN_*).  Row i equals ed25519_circuit.witness_inputs of slot i; a row whose status is not OK is zero.
        pubs / sigs / msgs: lists of bytes (a sig may be None where its flag is 0); flags: one truth value per slot (None in the plain form);
        dummy: the (pub, sig, msg) triple an unflagged slot verifies (ed25519_circuit.dummy_signature).  out: a DeviceBuffer to reuse."""
        n, width = len(pubs), layout.n_words()
        stride = max(1, max((len(m) for m in msgs), default=1))
        P = np.zeros((n, 32), dtype=np.uint8)
        S = np.zeros((n, 64), dtype=np.uint8)
        M = np.zeros((n, stride), dtype=np.uint8)
        Ln = np.zeros(n, dtype=np.uint32)
        for i in range(n):
            P[i] = np.frombuffer(bytes(pubs[i]), dtype=np.uint8)
            if sigs[i] is not None:
                S[i] = np.frombuffer(bytes(sigs[i]), dtype=np.uint8)
            M[i, :len(msgs[i])] = np.frombuffer(bytes(msgs[i]), dtype=np.uint8)
            Ln[i] = len(msgs[i])
        parts = [Ln.view(np.uint8), P.reshape(-1), S.reshape(-1), M.reshape(-1)]
        if layout.form != ED25519_FORM_PLAIN:
            if flags is None or dummy is None or len(flags) != n:
                raise GlpError("the flagged forms take one flag per slot and the dummy triple")
            parts += [np.array([1 if f else 0 for f in flags], dtype=np.uint8), np.frombuffer(b"".join(bytes(x) for x in dummy), dtype=np.uint8)]
            if parts[-1].size != 96 + layout.msg_len_min:
                raise GlpError("the dummy triple is pub[32], sig[64] and a message of msg_len_min bytes")
        # one upload: every array at an 8-byte offset of one block
        offs, total = [], 0
        for p in parts:
            offs.append(total)
            total += (p.size + 7) & ~7
        host = np.zeros(max(8, total), dtype=np.uint8)
        for o, p in zip(offs, parts):
            host[o:o + p.size] = p
        need = max(8, n * width * 8)
        if out is None or out.ptr is None or out.nbytes < need:
            out = self.alloc(need)
        status = np.zeros(max(1, n), dtype=np.int32)
        d = self.to_device(host)
        at = [d.ptr + o for o in offs] + [None, None]
        try:
            self._chk(self.lib.glp_ed25519_leaf_inputs(self.ctx, ctypes.byref(layout), at[1], at[2], at[3], stride, at[0], at[4], at[5], n, out.ptr,
                                                       width, status.ctypes.data), "glp_ed25519_leaf_inputs")
        finally:
            d.free()
        return out, status[:n]

    def ed25519_last_input_counts(self):
        """(launches, stream synchronises) of the last ed25519_leaf_inputs on this prover"""
        v = [ctypes.c_uint32() for _ in range(2)]
        self._chk(self.lib.glp_ed25519_last_input_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_ed25519_last_input_counts")
        return tuple(x.value for x in v)

    def ed25519_half_scalars(self, ks):
        """ed25519_circuit.half_size_pair of each scalar on the device (glp_ed25519_half_scalars): ks = integers below 2^256; returns [n][8] u64
        = u[3] v[3] neg status (ED25519_IN_OK, _NO_PAIR where the Python raises, _INVALID for k >= L)"""
        n = len(ks)
        a = np.array([[(int(k) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for k in ks], dtype=np.uint64).reshape(n, 4)
        if n == 0:
            return np.zeros((0, 8), dtype=np.uint64)
        dk, do = self.to_device(a), self.alloc(n * 64)
        try:
            self._chk(self.lib.glp_ed25519_half_scalars(self.ctx, dk.ptr, n, do.ptr), "glp_ed25519_half_scalars")
            return do.download((n, 8))
        finally:
            dk.free()
            do.free()

    def tm_merkle_root(self, leaves: bytes, leaf_len: int) -> bytes:
        """Tendermint simple Merkle root of fixed-size leaves (validator set / header fields)"""
        n = len(leaves) // leaf_len if leaf_len else 0
        assert n * leaf_len == len(leaves)
        d = self.to_device(np.frombuffer(leaves, dtype=np.uint8)) if n else None
        out = ctypes.create_string_buffer(32)
        self._chk(self.lib.glp_tm_merkle_root(self.ctx, d.ptr if d else None, leaf_len, n, out), "glp_tm_merkle_root")
        if d:
            d.free()
        return out.raw

    def tm_merkle_root_var(self, leaves) -> bytes:
        """Tendermint simple Merkle root of leaves of different lengths (a list of bytes)"""
        n = len(leaves)
        out = ctypes.create_string_buffer(32)
        if n == 0:
            self._chk(self.lib.glp_tm_merkle_root_var(self.ctx, None, 0, None, 0, out), "glp_tm_merkle_root_var")
            return out.raw
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in leaves])
        blob = b"".join(leaves) or b"\0"
        d = self.to_device(np.frombuffer(blob, dtype=np.uint8))
        do = self.to_device(offs)
        self._chk(self.lib.glp_tm_merkle_root_var(self.ctx, d.ptr, len(blob), do.ptr, n, out), "glp_tm_merkle_root_var")
        d.free()
        do.free()
        return out.raw

    def tm_merkle_root_batch(self, trees, download=True):
        """the Tendermint simple Merkle roots of SEVERAL trees in one call (glp_tm_merkle_root_batch: two launches, one synchronise): trees =
        a list of lists of leaves (bytes), of any leaf counts (<= TM_BATCH_MAX_LEAVES each) and lengths.  Returns the list of 32-byte roots;
        download=False: the DeviceBuffer [B][32] in place of the host copy.  The C call then does not synchronise (its counter reads 0), but
        this wrapper does, once, before it frees the leaf bytes it uploaded: a caller that needs no synchronise at all keeps its bytes resident
        and calls glp_tm_merkle_root_batch itself."""
        B = len(trees)
        leaves = [bytes(x) for t in trees for x in t]
        first = np.zeros(B + 1, dtype=np.uint64)
        first[1:] = np.cumsum([len(t) for t in trees])
        offs = np.zeros(len(leaves) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in leaves])
        blob = b"".join(leaves) or b"\0"
        d = self.to_device(np.frombuffer(blob, dtype=np.uint8))
        d_roots = self.alloc(max(8, 32 * B))
        out = np.zeros((B, 32), dtype=np.uint8)
        try:
            self._chk(self.lib.glp_tm_merkle_root_batch(self.ctx, d.ptr, len(blob), offs.ctypes.data, first.ctypes.data, len(leaves), B,
                                                        d_roots.ptr, out.ctypes.data if download else None), "glp_tm_merkle_root_batch")
        finally:
            if not download:
                self.sync()                     # the blob is freed below: the kernels that read it must be done
            d.free()
        if not download:
            return d_roots
        d_roots.free()
        return [out[i].tobytes() for i in range(B)]

    def tm_merkle_root_batch_last_counts(self):
        """(launches, stream synchronises) of the last glp_tm_merkle_root_batch on this prover"""
        v = [ctypes.c_uint32() for _ in range(2)]
        self._chk(self.lib.glp_tm_merkle_root_batch_last_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_tm_merkle_root_batch_last_counts")
        return tuple(x.value for x in v)

    def tm_forest(self, trees, roots=False):
        """the Tendermint simple Merkle trees of `trees` (a list of lists of leaves, any counts up to TM_FOREST_MAX_LEAVES and any lengths) with
        EVERY LEVEL KEPT on the device (glp_tm_forest_create): a TmForest that hands out roots and audit paths until .free().  roots=True: the
        call copies the roots to the host at once (its one synchronise)."""
        return TmForest(self, trees, roots)

    def tm_verify_inclusion_batch(self, roots, proofs, leaves, root_of=None):
        """check n inclusion proofs in one launch (glp_tm_verify_inclusion_batch): roots = list of 32-byte roots, proofs[p] = (total, index,
        leaf_hash, aunts) as TmForest.proofs gives them (the leaf hash is NOT read: leaves[p], the leaf BYTES, are hashed on the device),
        root_of[p] = the root proof p is checked against (None: root 0).  Returns int32[n] of TM_INCLUSION_OK / _BAD_SHAPE / _BAD_ROOT."""
        n = len(proofs)
        if len(leaves) != n or (root_of is not None and len(root_of) != n):
            raise GlpError("tm_verify_inclusion_batch: proofs, leaves and root_of differ in length")
        status = np.zeros(n, dtype=np.int32)
        if n == 0:
            return status
        stride = max(1, max(len(p[3]) for p in proofs))
        aunts = np.zeros((n, stride, 32), dtype=np.uint8)
        for i, p in enumerate(proofs):
            for k, a in enumerate(p[3]):
                aunts[i, k] = np.frombuffer(bytes(a), dtype=np.uint8)
        return self.tm_verify_inclusion_arrays(roots, leaves, [p[1] for p in proofs], [p[0] for p in proofs], aunts, [len(p[3]) for p in proofs], root_of)

    def tm_verify_inclusion_arrays(self, roots, leaves, index, total, aunts, n_aunts, root_of=None):
        """the array form of tm_verify_inclusion_batch: aunts uint8 [n][aunt_stride][32], index / total / n_aunts the proofs' own (untrusted) words"""
        n = len(leaves)
        aunts = np.ascontiguousarray(aunts, dtype=np.uint8)
        stride = aunts.shape[1] if aunts.ndim == 3 else 0
        status = np.full(n, -1, dtype=np.int32)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in leaves])
        blob = b"".join(bytes(x) for x in leaves) or b"\0"
        ro = None if root_of is None else np.ascontiguousarray(root_of, dtype=np.uint32)
        bufs = [self.to_device(np.frombuffer(b"".join(bytes(r) for r in roots) or b"\0", dtype=np.uint8)), self.to_device(np.frombuffer(blob, dtype=np.uint8)),
                self.to_device(np.asarray(index, dtype=np.uint64)), self.to_device(np.asarray(total, dtype=np.uint64)), self.to_device(aunts),
                self.to_device(np.asarray(n_aunts, dtype=np.uint32))]
        try:
            self._chk(self.lib.glp_tm_verify_inclusion_batch(self.ctx, bufs[0].ptr, len(roots), None if ro is None else ro.ctypes.data, bufs[1].ptr,
                                                             int(offs[-1]), offs.ctypes.data, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, stride, bufs[5].ptr, n,
                                                             status.ctypes.data), "glp_tm_verify_inclusion_batch")
        finally:
            for b in bufs:
                b.free()
        return status

    def tm_forest_last_counts(self):
        """(launches, stream synchronises) of the last glp_tm_forest_create / _proofs / glp_tm_verify_inclusion_batch on this prover"""
        v = [ctypes.c_uint32() for _ in range(2)]
        self._chk(self.lib.glp_tm_forest_last_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_tm_forest_last_counts")
        return tuple(x.value for x in v)

    def header_chain_leaf_inputs(self, layout, d_headers, start_hash, first_height, n, out=None, hashes=None):
        """the input vectors of the header-chain leaves of n headers that lie on the device (glp_header_chain_leaf_inputs: at most 4 launches,
        one synchronise): (DeviceBuffer [n / leaf_headers][layout.n_words()] u64, status int32[n] of HEADER_CHAIN_*, DeviceBuffer [n + 1][32] of
        the start hash and every header's hash).  Row l equals data_commitment_mr._chain_leaf_inputs of leaf l; the row of a leaf with a refused
        header is zero.  d_headers: n * layout.header_bytes() bytes (DeviceBuffer / pointer).  out / hashes: DeviceBuffers to reuse."""
        width, n = layout.n_words(), int(n)
        if n % layout.leaf_headers:
            raise GlpError("the chain is not a whole number of leaves")
        start = np.frombuffer(bytes(start_hash), dtype=np.uint8).copy()
        if start.size != 32:
            raise GlpError("the start hash has 32 bytes")
        need = max(8, (n // layout.leaf_headers) * width * 8)
        own = []                                                    # what this call allocates: freed again when the C call refuses
        if out is None or out.ptr is None or out.nbytes < need:
            out = self.alloc(need)
            own.append(out)
        if hashes is None or hashes.ptr is None or hashes.nbytes < 32 * (n + 1):
            hashes = self.alloc(32 * (n + 1))
            own.append(hashes)
        status = np.zeros(max(1, n), dtype=np.int32)
        try:
            self._chk(self.lib.glp_header_chain_leaf_inputs(self.ctx, ctypes.byref(layout), _ptr(d_headers), start.ctypes.data, int(first_height), n,
                                                            out.ptr, width, hashes.ptr, status.ctypes.data), "glp_header_chain_leaf_inputs")
        except Exception:
            for b in own:
                b.free()
            raise
        return out, status[:n], hashes

    def header_chain_last_input_counts(self):
        """(launches, stream synchronises) of the last header_chain_leaf_inputs on this prover"""
        v = [ctypes.c_uint32() for _ in range(2)]
        self._chk(self.lib.glp_header_chain_last_input_counts(self.ctx, *[ctypes.byref(x) for x in v]), "glp_header_chain_last_input_counts")
        return tuple(x.value for x in v)

    def transpose(self, mat):
        m = np.ascontiguousarray(mat, dtype=np.uint64)
        rows, cols = m.shape
        d_in = self.to_device(m)
        d_out = self.alloc(m.nbytes)
        self.transpose_(d_in, d_out, rows, cols)
        out = d_out.download((cols, rows))
        d_in.free()
        d_out.free()
        return out


def sha_pad(msg: bytes, block: int, blocks: int = None) -> bytes:
    """FIPS 180-4 padding to whole blocks (block = 64 for SHA-256, 128 for SHA-512); when
    `blocks` is given the message must fit exactly that many blocks (fixed-shape batches)."""
    lenbytes = 8 if block == 64 else 16
    need = (len(msg) + 1 + lenbytes + block - 1) // block
    if blocks is not None:
        assert need == blocks, "message does not pad to the requested number of blocks"
    pad = need * block - len(msg) - 1 - lenbytes
    return msg + b"\x80" + b"\x00" * pad + (8 * len(msg)).to_bytes(lenbytes, "big")


class TmForest:
    """B Tendermint simple Merkle trees with every level kept on the device (glp_tm_forest_*).  The proof format is BUILD-DEFINED (Tendermint's
    crypto/merkle.Proof restated from memory, unpinned): a proof is the tuple (total, index, leaf_hash, aunts) with the aunts bottom-up."""

    def __init__(self, prover, trees, roots=False):
        self.prover, self.handle = prover, None
        self.counts = [len(t) for t in trees]
        B = len(trees)
        leaves = [bytes(x) for t in trees for x in t]
        self.first = np.zeros(B + 1, dtype=np.uint64)
        self.first[1:] = np.cumsum(self.counts)
        offs = np.zeros(len(leaves) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in leaves])
        blob = b"".join(leaves) or b"\0"
        d = prover.to_device(np.frombuffer(blob, dtype=np.uint8))
        h = _vp()
        self._roots = np.zeros((B, 32), dtype=np.uint8) if roots else None
        try:
            prover._chk(prover.lib.glp_tm_forest_create(prover.ctx, d.ptr, int(offs[-1]), offs.ctypes.data, self.first.ctypes.data, len(leaves), B,
                                                        self._roots.ctypes.data if roots and B else None, ctypes.byref(h)), "glp_tm_forest_create")
            self.create_counts = prover.tm_forest_last_counts()
        finally:
            if not roots:
                prover.sync()                   # the blob is freed below: the kernels that read it must be done
            d.free()
        self.handle = h
        prover._circuits.append(self)           # holds a pool block of the ctx: freed before it (Prover.close)

    def info(self):
        """(trees, leaves, max_aunts, device bytes held)"""
        v = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()]
        self.prover._chk(self.prover.lib.glp_tm_forest_info(self.handle, *[ctypes.byref(x) for x in v]), "glp_tm_forest_info")
        return tuple(x.value for x in v)

    def roots_ptr(self):
        """the device array [n_trees][32], valid until free()"""
        p = _vp()
        self.prover._chk(self.prover.lib.glp_tm_forest_roots(self.handle, ctypes.byref(p)), "glp_tm_forest_roots")
        return p.value

    def roots(self):
        """the list of 32-byte roots (copied from the device once, then kept)"""
        if self._roots is None:
            B = len(self.counts)
            self._roots = np.zeros((B, 32), dtype=np.uint8)
            if B:
                self.prover._chk(self.prover.lib.glp_d2h(self.prover.ctx, self._roots.ctypes.data, self.roots_ptr(), 32 * B), "glp_d2h")
        return [self._roots[t].tobytes() for t in range(len(self.counts))]

    def proofs_arrays(self, queries=None, aunt_stride=None):
        """(aunts uint8 [n][aunt_stride][32], n_aunts uint32 [n], leaf_hashes uint8 [n][32]) of the queries [(tree, leaf)], or of every leaf in
        numbering order (queries=None): one launch (glp_tm_forest_proofs)"""
        pr = self.prover
        n = int(self.first[-1]) if queries is None else len(queries)
        if aunt_stride is None:
            aunt_stride = self.info()[2]
        aunts, na, lh = np.zeros((n, aunt_stride, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros((n, 32), dtype=np.uint8)
        qt = ql = None
        if queries is not None:
            qt, ql = np.array([q[0] for q in queries], dtype=np.uint64), np.array([q[1] for q in queries], dtype=np.uint64)
        bufs = [pr.alloc(max(8, aunts.nbytes)), pr.alloc(max(8, na.nbytes)), pr.alloc(max(8, lh.nbytes))]
        try:
            pr._chk(pr.lib.glp_tm_forest_proofs(pr.ctx, self.handle, None if qt is None else qt.ctypes.data, None if ql is None else ql.ctypes.data, n,
                                                bufs[0].ptr, aunt_stride, bufs[1].ptr, bufs[2].ptr), "glp_tm_forest_proofs")
            self.proofs_counts = pr.tm_forest_last_counts()
            if n:
                if aunts.nbytes:
                    aunts = bufs[0].download(aunts.shape, dtype=np.uint8)
                na, lh = bufs[1].download(na.shape, dtype=np.uint32), bufs[2].download(lh.shape, dtype=np.uint8)
        finally:
            for b in bufs:
                b.free()
        return aunts, na, lh

    def proofs(self, queries=None):
        """the proofs (total, index, leaf_hash, aunts) of the queries [(tree, leaf)], or of every leaf in numbering order (queries=None)"""
        aunts, na, lh = self.proofs_arrays(queries)
        if queries is None:
            queries = [(t, i) for t, c in enumerate(self.counts) for i in range(c)]
        return [(self.counts[t], i, lh[q].tobytes(), [aunts[q, k].tobytes() for k in range(int(na[q]))]) for q, (t, i) in enumerate(queries)]

    def free(self):
        if self.handle is not None:
            self.prover.lib.glp_tm_forest_destroy(self.handle)
            self.handle = None
            if self in self.prover._circuits:
                self.prover._circuits.remove(self)


class PlonkCircuit:
    """Preprocessed build-defined circuit (glp_plonk_setup_ex): constant columns and sigma columns committed once;
    prove(wires, public) returns the proof bytes.  DESIGN.md §3.6.
      consts: [6][n] = (q_arith, c0, c1, c2, q_pi, q_pos) row values — or the round-1 form [3][n] = (q, c0, c1)
      sigmas: [n_routed][n];  n_wires: total wire columns (default: all routed);  n_public: rows 0..n_public-1 expose wire 0
      poseidon: q_pos rows carry a permutation (needs n_wires >= 130, n_routed >= 24)
      sha: SHA-256 rows (consts [10][n]: + q_she, q_sha, q_shw, q_add; n_wires >= 144, n_routed >= 16)
      ext: extension-arithmetic rows (one more column, q_ext, LAST: consts [7][n] or [11][n])"""

    def __init__(self, prover, consts, sigmas, rate_bits=3, cap_height=4, n_wires=None, n_public=0, poseidon=False, sha=False, ext=False):
        self.prover = prover
        c = np.ascontiguousarray(consts, dtype=np.uint64)
        s = np.ascontiguousarray(sigmas, dtype=np.uint64)
        self.n_routed, n = s.shape
        self.n_wires = self.n_routed if n_wires is None else int(n_wires)
        self.n_public = int(n_public)
        self.flags = (CIRCUIT_POSEIDON_GATE if poseidon else 0) | (CIRCUIT_SHA_GATES if sha else 0) | (CIRCUIT_EXT_GATE if ext else 0)
        self.log_n = n.bit_length() - 1
        nc = PLONK_NCONST + (4 if sha else 0) + (1 if ext else 0)
        assert 1 << self.log_n == n and (c.shape == (nc, n) or (not ext and c.shape in ((3, n), (PLONK_NCONST, n))))
        if c.shape[0] < nc:
            c = np.concatenate([c, np.zeros((nc - c.shape[0], n), dtype=np.uint64)])
        dc, ds = prover.to_device(c), prover.to_device(s)
        h = _vp()
        shape = CircuitShape(self.log_n, self.n_wires, self.n_routed, self.n_public, rate_bits, cap_height, self.flags)
        try:
            prover._chk(prover.lib.glp_plonk_setup_ex(prover.ctx, ctypes.byref(shape), dc.ptr, ds.ptr, ctypes.byref(h)), "glp_plonk_setup_ex")
        finally:
            dc.free()
            ds.free()
        self.h = h
        prover._circuits.append(self)

    def cap(self):
        """the preprocessed commitment (constants + sigmas): the circuit's verifying key"""
        n = ctypes.c_size_t(0)
        self.prover._chk(self.prover.lib.glp_plonk_circuit_cap(self.h, None, ctypes.byref(n)), "glp_plonk_circuit_cap")
        out = np.zeros(n.value, dtype=np.uint64)
        self.prover._chk(self.prover.lib.glp_plonk_circuit_cap(self.h, out.ctypes.data, ctypes.byref(n)), "glp_plonk_circuit_cap")
        return out

    def verify(self, proof, min_queries=28, min_pow_bits=16, public=None):
        """bound to this circuit and to the statement `public` (None: no public inputs; UNBOUND: any)"""
        if public is None and self.n_public:
            raise GlpError("verify: this circuit has public inputs — pass the expected ones (or UNBOUND)")
        return self.prover.plonk_verify(proof, self.cap(), min_queries, min_pow_bits, public=public)

    def verify_batch(self, proofs, min_queries=28, min_pow_bits=16, publics=None, want_digests=False):
        """B proofs bound to this circuit in one call (Prover.plonk_verify_batch); publics: one row of expected public inputs per proof
        (None: the circuit has none; UNBOUND: any)"""
        if publics is None and self.n_public:
            raise GlpError("verify_batch: this circuit has public inputs — pass the expected ones (or UNBOUND)")
        if publics is None:
            publics = [[] for _ in proofs]
        return self.prover.plonk_verify_batch(proofs, self.cap(), min_queries, min_pow_bits, publics=publics, want_digests=want_digests)

    def _public_words(self, public):
        pub = np.ascontiguousarray([] if public is None else [int(v) for v in public], dtype=np.uint64)
        if pub.size != self.n_public:
            raise GlpError(f"{pub.size} public inputs given, the circuit has {self.n_public}")
        return pub if pub.size else None

    def prove(self, wires, num_queries=28, pow_bits=16, public=None):
        w = np.ascontiguousarray(wires, dtype=np.uint64)
        assert w.shape == (self.n_wires, 1 << self.log_n)
        dw = self.prover.to_device(w)
        try:
            return self.prove_(dw, num_queries, pow_bits, public=public)
        finally:
            dw.free()

    def prove_(self, d_wires, num_queries=28, pow_bits=16, public=None):
        proof = _vp()
        ln = ctypes.c_size_t()
        pub = self._public_words(public)
        self.prover._chk(self.prover.lib.glp_plonk_prove_ex(self.prover.ctx, self.h, _ptr(d_wires), pub.ctypes.data if pub is not None else None,
                                                            num_queries, pow_bits, ctypes.byref(proof), ctypes.byref(ln)), "glp_plonk_prove_ex")
        data = ctypes.string_at(proof.value, ln.value)
        self.prover.lib.glp_free_host(proof)
        return data

    def prove_batch_(self, d_wires_list, publics=None, num_queries=28, pow_bits=16):
        """B proofs of this circuit in one call (glp_plonk_prove_batch).  d_wires_list: B device wire matrices (DeviceBuffers or addresses; read
        only, the same one may appear twice); publics: B lists of public values (None when the circuit has none).  Returns the B proofs, each
        byte for byte what prove_ returns for that instance alone; any error fails the whole call (GlpError names the instance at fault)."""
        B = len(d_wires_list)
        if B == 0:
            return []
        if publics is None:
            publics = [None] * B
        if len(publics) != B:
            raise GlpError(f"{len(publics)} public-input lists given for {B} instances")
        rows = [self._public_words(p) for p in publics]
        pub = np.ascontiguousarray(np.stack(rows), dtype=np.uint64) if self.n_public else None
        ptrs = (_vp * B)(*[_ptr(d) for d in d_wires_list])
        proofs = (_vp * B)()
        lens = (ctypes.c_size_t * B)()
        self.prover._chk(self.prover.lib.glp_plonk_prove_batch(self.prover.ctx, self.h, ptrs, pub.ctypes.data if pub is not None else None, B,
                                                               num_queries, pow_bits, proofs, lens), "glp_plonk_prove_batch")
        out = []
        for i in range(B):
            out.append(ctypes.string_at(proofs[i], lens[i]))
            self.prover.lib.glp_free_host(proofs[i])
        return out

    def prove_batch(self, wires_list, publics=None, num_queries=28, pow_bits=16):
        """prove_batch_ for host arrays: B wire matrices [n_wires][n]"""
        n = 1 << self.log_n
        bufs = []
        try:
            for w in wires_list:
                w = np.ascontiguousarray(w, dtype=np.uint64)
                assert w.shape == (self.n_wires, n)
                bufs.append(self.prover.to_device(w))
            return self.prove_batch_(bufs, publics, num_queries, pow_bits)
        finally:
            for b in bufs:
                b.free()

    # ---- witness checker (glp_plonk_check_witness[_batch]): never raises for a bad witness, only for unusable arguments or a bad key ----
    def check_batch_(self, d_wires_list, publics=None, max_list=16):
        """B device wire matrices of this circuit against its constraints in one call.  Returns B CheckResults (ok, summary, violations)."""
        B = len(d_wires_list)
        if B == 0:
            return []
        if publics is None:
            publics = [None] * B
        if len(publics) != B:
            raise GlpError(f"{len(publics)} public-input lists given for {B} instances")
        rows = [self._public_words(p) for p in publics]
        pub = np.ascontiguousarray(np.stack(rows), dtype=np.uint64) if self.n_public else None
        ptrs = (_vp * B)(*[_ptr(d) for d in d_wires_list])
        status = (ctypes.c_int32 * B)()
        sums = (CheckSummary * B)()
        lists = (CheckViolation * max(B * max_list, 1))()
        self.prover._chk(self.prover.lib.glp_plonk_check_witness_batch(self.prover.ctx, self.h, ptrs, pub.ctypes.data if pub is not None else None, B,
                                                                       status, sums, lists if max_list else None, max_list),
                         "glp_plonk_check_witness_batch")
        return [CheckResult(status[b] == 0, sums[b].as_dict(), [lists[b * max_list + k].as_dict() for k in range(sums[b].n_listed)]) for b in range(B)]

    def require_satisfied_(self, d_wires_list, publics=None, names=None):
        """check_batch_ for callers that must not prove a bad witness (the check_witness=True paths of the MapReduce classes): ValueError naming
        the first failing instance (names[i], default 'instance i'), its row, the kind and the index"""
        for i, res in enumerate(self.check_batch_(d_wires_list, publics, max_list=1)):
            if not res.ok:
                raise ValueError(f"check_witness: {names[i] if names else f'instance {i}'}: witness not satisfied: {res.describe()}")

    def check_(self, d_wires, public=None, max_list=16):
        """one device wire matrix (glp_plonk_check_witness) -> CheckResult"""
        pub = self._public_words(public)
        sm = CheckSummary()
        lst = (CheckViolation * max(max_list, 1))()
        rc = self.prover.lib.glp_plonk_check_witness(self.prover.ctx, self.h, _ptr(d_wires), pub.ctypes.data if pub is not None else None,
                                                     ctypes.byref(sm), lst if max_list else None, max_list)
        if rc not in (0, -7):
            self.prover._chk(rc, "glp_plonk_check_witness")
        return CheckResult(rc == 0, sm.as_dict(), [lst[k].as_dict() for k in range(sm.n_listed)])

    def check(self, wires, public=None, max_list=16):
        """check_ for a host array [n_wires][n]"""
        w = np.ascontiguousarray(wires, dtype=np.uint64)
        assert w.shape == (self.n_wires, 1 << self.log_n)
        dw = self.prover.to_device(w)
        try:
            return self.check_(dw, public, max_list)
        finally:
            dw.free()

    def debug_stage(self, wires, which, challenges, public=None):
        """parity hook (glp_plonk_debug_stage): which = "zs" -> [2*M][n] Z / partial products on the trace domain for
        challenges (beta0, beta1, gamma0, gamma1); which = "quotient" -> [2][8n] quotient evaluations on the LDE coset
        (bit-reversed order) for (beta0, beta1, gamma0, gamma1, alpha0, alpha1)"""
        w = np.ascontiguousarray(wires, dtype=np.uint64)
        n = 1 << self.log_n
        assert w.shape == (self.n_wires, n)
        ch = np.ascontiguousarray(challenges, dtype=np.uint64)
        kind = {"zs": 0, "quotient": 1}[which]
        assert ch.size == (4 if kind == 0 else 6)
        shape = (2 * (self.n_routed // 8), n) if kind == 0 else (2, 8 * n)
        pub = self._public_words(public)
        dw = self.prover.to_device(w)
        do = self.prover.alloc(shape[0] * shape[1] * 8)
        try:
            self.prover._chk(self.prover.lib.glp_plonk_debug_stage(self.prover.ctx, self.h, dw.ptr, pub.ctypes.data if pub is not None else None,
                                                                   kind, ch.ctypes.data, do.ptr), "glp_plonk_debug_stage")
            return do.download(shape)
        finally:
            dw.free()
            do.free()

    def free(self):
        if getattr(self, "h", None):
            if getattr(self.prover, "ctx", None):        # after glp_destroy the pool (and the blocks) are gone
                self.prover.lib.glp_plonk_free(self.h)
            self.h = None
            if self in self.prover._circuits:
                self.prover._circuits.remove(self)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Challenger:
    """Host-side Fiat-Shamir transcript of the library (glp_challenger_*)"""

    def __init__(self, prover):
        self.lib = prover.lib
        h = _vp()
        prover._chk(self.lib.glp_challenger_new(prover.ctx, ctypes.byref(h)), "glp_challenger_new")
        self.h = h

    def observe(self, elems):
        a = np.ascontiguousarray(elems, dtype=np.uint64).reshape(-1)
        if self.lib.glp_challenger_observe(self.h, a.ctypes.data, a.size) != 0:
            raise GlpError("glp_challenger_observe: non-canonical element")

    def challenges(self, n):
        out = np.zeros(n, dtype=np.uint64)
        self.lib.glp_challenger_challenges(self.h, out.ctypes.data, n)
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.glp_challenger_free(self.h)
            self.h = None


class PolynomialBatch:
    """Commitment to a batch of polynomials (upstream name recalled:
    plonky2::fri::oracle::PolynomialBatch, file:line NONE — absent from the mount).

    from_values: values on <w_n> -> coefficients (inverse NTT) -> from_coeffs.
    from_coeffs: coset LDE by 2^rate_bits on shift*<w_N> (N = n << rate_bits), stored
    polynomial-major [n_polys][N] with the evaluation index BIT-REVERSED, then a Poseidon
    Merkle tree whose leaf i is column i of that matrix (hashed straight from the
    polynomial-major layout: no transpose pass).  Everything stays resident in HBM."""

    def __init__(self, prover, n_polys, log_n, rate_bits, cap_height):
        self.prover, self.n_polys, self.log_n, self.rate_bits, self.cap_height = prover, n_polys, log_n, rate_bits, cap_height
        self.coeffs = self.lde = self.digests = None
        self.cap = None

    @classmethod
    def from_coeffs(cls, prover, d_coeffs, n_polys, log_n, rate_bits, cap_height, keep_coeffs=True):
        self = cls(prover, n_polys, log_n, rate_bits, cap_height)
        log_N = log_n + rate_bits
        self.coeffs = d_coeffs if keep_coeffs else None
        self.lde = prover.alloc(n_polys * (8 << log_N))
        prover.lde_coset_(d_coeffs, self.lde, log_n, rate_bits, n_polys, COSET_SHIFT, NTT_BITREV)
        self.digests = prover.alloc(8 * Prover.merkle_digest_len(log_N, cap_height))
        self.cap = prover.merkle_(self.lde, n_polys, log_N, cap_height, self.digests, poly_major=True, poly_stride=1 << log_N)
        return self

    @classmethod
    def from_values(cls, prover, values, rate_bits, cap_height):
        v = np.ascontiguousarray(values, dtype=np.uint64)
        n_polys, n = v.shape
        log_n = n.bit_length() - 1
        assert 1 << log_n == n
        d = prover.to_device(v)
        prover.ntt_(d, log_n, n_polys, inverse=True)
        return cls.from_coeffs(prover, d, n_polys, log_n, rate_bits, cap_height)

    @classmethod
    def from_values_batch(cls, prover, values, rate_bits, cap_height):
        """values [B][n_polys][n] -> B PolynomialBatch objects committed in ONE call (glp_commit_values_batch: one inverse NTT, one LDE, B
        Merkle trees built together, one copy of all caps).  The B objects are views: coeffs / lde / digests are integer device addresses
        into three slabs shared by the whole batch and owned by one holder object (view.slabs; slabs.free() releases them, as closing the
        prover does); free() on a view releases nothing."""
        v = np.ascontiguousarray(values, dtype=np.uint64)
        assert v.ndim == 3
        B, n_polys, n = v.shape
        log_n = n.bit_length() - 1
        assert 1 << log_n == n
        log_N = log_n + rate_bits
        nd = Prover.merkle_digest_len(log_N, cap_height)
        slabs = _BatchSlabs(prover.to_device(v), prover.alloc(max(8, B * n_polys * (8 << log_N))), prover.alloc(max(8, B * nd * 8)))
        caps = np.zeros((B, 1 << cap_height, 4), dtype=np.uint64)
        try:
            prover._chk(prover.lib.glp_commit_values_batch(prover.ctx, slabs.coeffs.ptr, n_polys, log_n, rate_bits, cap_height, B, slabs.lde.ptr,
                                                           slabs.digests.ptr, nd, caps.ctypes.data if B else None), "glp_commit_values_batch")
        except GlpError:
            slabs.free()
            raise
        out = []
        for b in range(B):
            pb = cls(prover, n_polys, log_n, rate_bits, cap_height)
            pb.slabs = slabs
            pb.coeffs = slabs.coeffs.ptr + b * n_polys * (8 << log_n)
            pb.lde = slabs.lde.ptr + b * n_polys * (8 << log_N)
            pb.digests = slabs.digests.ptr + b * nd * 8
            pb.cap = caps[b]
            out.append(pb)
        return out

    def free(self):
        for b in (self.coeffs, self.lde, self.digests):
            if isinstance(b, DeviceBuffer):
                b.free()
        self.coeffs = self.lde = self.digests = None


class _BatchSlabs:
    """the three device slabs behind the views of one PolynomialBatch.from_values_batch call"""

    def __init__(self, coeffs, lde, digests):
        self.coeffs, self.lde, self.digests = coeffs, lde, digests

    def free(self):
        for b in (self.coeffs, self.lde, self.digests):
            if b is not None:
                b.free()
        self.coeffs = self.lde = self.digests = None
