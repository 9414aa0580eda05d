"""TEST INFRASTRUCTURE: the reference of the witness checker (glp_plonk_check_witness), written against tests/plonk_ref.py and sharing no code
with the product.  Every trace row of a circuit dict (pref.build_circuit) in Python integers: the public-input constraint, the arithmetic /
extension slots of every chunk, the Poseidon block (pref.poseidon_constraints) times q_pos, the SHA block (pref.sha_constraints), numbered as
the quotient numbers them, and the copy constraints cell by cell after decoding sigma through a dictionary {k_j * w^i: (j, i)}.
check() returns the summary and the COMPLETE sorted violation list in the product's field names, so a test compares word for word."""
import fri_verifier as fv
import plonk_ref as pref

P = pref.P
GATE, COPY = 0, 1


class SigmaError(ValueError):
    pass


def domain(log_n, R, w=None):
    """{k_j * w^i: (j, i)} for the routed cells; w defaults to the generator-7 root the circuit generator uses"""
    n = 1 << log_n
    w = fv.root(log_n) if w is None else w
    ks = pref.ks_of(R)
    out, x = {}, 1
    for i in range(n):
        for j in range(R):
            out[ks[j] * x % P] = (j, i)
        x = x * w % P
    return out


def decode_sigma(sigmas, log_n, w=None):
    """[R][n] of (j', i'); SigmaError naming the first cell (wire-major order) whose value is no routed cell, or — when all decode — the first cell
    that is not the image of exactly one cell"""
    R, n = len(sigmas), 1 << log_n
    dom = domain(log_n, R, w)
    cells = [[None] * n for _ in range(R)]
    hits = {}
    for j in range(R):
        for i in range(n):
            t = dom.get(int(sigmas[j][i]))
            if t is None:
                raise SigmaError(f"no domain point: wire {j}, row {i}")
            cells[j][i] = t
            hits[t] = hits.get(t, 0) + 1
    for j in range(R):
        for i in range(n):
            if hits.get((j, i), 0) != 1:
                raise SigmaError(f"not a bijection: wire {j}, row {i}")
    return cells


def encode_sigma(cells, log_n, w):
    """the sigma values of decoded cells on the root w (a build with another two-adic generator stores other values for the same routing)"""
    R, n = len(cells), 1 << log_n
    ks = pref.ks_of(R)
    wp = [1] * n
    for i in range(1, n):
        wp[i] = wp[i - 1] * w % P
    return [[ks[jj] * wp[ii] % P for (jj, ii) in row] for row in cells]


class RefChecker:
    """one circuit (its constants and sigma), any number of witnesses.  Row results are cached by the row's wire values: a batch of single-cell
    mutations re-evaluates one row per instance."""

    def __init__(self, circ, w=None):
        self.log_n, self.W, self.R, self.flags = circ["log_n"], circ["W"], circ["R"], circ["flags"]
        self.n = 1 << self.log_n
        self.M = self.R // pref.CHUNK
        self.consts = [[int(v) for v in r] for r in circ["consts"]]
        self.n_public = circ["n_public"]
        self.pos_consts = pref.int_consts(circ["pos_consts"]) if self.flags & pref.FLAG_POSEIDON else None
        self.cells = decode_sigma(circ["sigmas"], self.log_n, w)
        self.first_pos = 2 + 3 * self.M
        self.first_sha = self.first_pos + (pref.POS_CONSTRAINTS if self.flags & pref.FLAG_POSEIDON else 0)
        self._cache = {}

    def gate_row(self, i, col, pi):
        """[(index, value)] of the failing gate constraints of row i (col = its W wire values), ascending by index"""
        key = (i, pi, tuple(col))
        if key in self._cache:
            return self._cache[key]
        F = pref.Base
        c = [r[i] for r in self.consts]
        q, c0, c1, c2, q_pi, q_pos = c[:6]
        q_ext = c[-1] if self.flags & pref.FLAG_EXT else None
        vals = [(1, F.sub(F.mul(q_pi, col[0]), pi))]
        for ch in range(self.M):
            w8 = col[ch * 8:ch * 8 + 8]
            gate = lambda x, y, z, w: F.mul(q, F.sub(F.add(F.add(F.mul(c0, F.mul(x, y)), F.mul(c1, z)), c2), w))
            g0, g1 = gate(*w8[0:4]), gate(*w8[4:8])
            if q_ext is not None:
                x0, x1, y0, y1, z0, z1, w0, w1 = w8
                e0 = F.sub(F.add(F.add(F.mul(x0, y0), F.scale(F.mul(x1, y1), 7)), z0), w0)
                e1 = F.sub(F.add(F.add(F.mul(x0, y1), F.mul(x1, y0)), z1), w1)
                g0, g1 = F.add(g0, F.mul(q_ext, e0)), F.add(g1, F.mul(q_ext, e1))
            vals += [(3 + 3 * ch, g0), (4 + 3 * ch, g1)]
        if self.pos_consts is not None and q_pos:                  # q_pos = 0: every term of the block is 0
            vals += [(self.first_pos + k, F.mul(q_pos, v)) for k, v in enumerate(pref.poseidon_constraints(F, col[:pref.POS_WIRES], self.pos_consts))]
        if self.flags & pref.FLAG_SHA and any(c[6:10]):            # all four selectors 0: every slot is 0
            vals += [(self.first_sha + k, v) for k, v in enumerate(pref.sha_constraints(F, col[:pref.SHA_WIRES], c[6:10], c2))]
        out = [(k, v) for k, v in vals if v]
        self._cache[key] = out
        return out

    def check(self, wires, public=None, max_list=None):
        """(summary dict, violation list) of one witness [W][n]; the list is complete unless max_list cuts it (as the product's does)"""
        n = self.n
        wires = [[int(v) for v in r] for r in wires]
        public = [int(v) for v in (public or [])]
        assert len(wires) == self.W and len(public) == self.n_public
        out = []
        n_gate_bad = n_copy_bad = n_gate_rows = n_copy_rows = 0
        for i in range(n):
            col = [wires[j][i] for j in range(self.W)]
            bad = self.gate_row(i, col, public[i] if i < self.n_public else 0)
            if bad:
                n_gate_bad += len(bad)
                n_gate_rows += 1
                out.append({"kind": GATE, "row": i, "index": bad[0][0], "n_in_row": len(bad), "peer_wire": 0, "peer_row": 0, "value": bad[0][1],
                            "peer_value": 0})
            cb = []
            for j in range(self.R):
                jj, ii = self.cells[j][i]
                if wires[j][i] != wires[jj][ii]:
                    cb.append((j, jj, ii))
            if cb:
                j, jj, ii = cb[0]
                n_copy_bad += len(cb)
                n_copy_rows += 1
                out.append({"kind": COPY, "row": i, "index": j, "n_in_row": len(cb), "peer_wire": jj, "peer_row": ii, "value": wires[j][i],
                            "peer_value": wires[jj][ii]})
        if max_list is not None:
            out = out[:max_list]
        summary = {"n_gate_bad": n_gate_bad, "n_copy_bad": n_copy_bad, "n_gate_rows": n_gate_rows, "n_copy_rows": n_copy_rows, "n_listed": len(out)}
        return summary, out


def check(circ, wires=None, public=None, max_list=None):
    return RefChecker(circ).check(circ["wires"] if wires is None else wires, circ["public"] if public is None else public, max_list)


# ---- mutation targets: the wire that each constraint of a block pins ------------------------------------------------------------------------
def poseidon_target(k):
    """(wire, new value or None = add 1) whose change makes Poseidon constraint k the row's lowest failing one: the swap bit (2 is not
    boolean), a delta, an S-box input, an output"""
    if k == 0:
        return pref.POS_SWAP, 2
    if k < 5:
        return pref.POS_DELTA0 + k - 1, None
    if k < 111:
        return pref.POS_ADV0 + k - 5, None
    return 12 + k - 111, None


def sha_kinds(circ):
    """row -> kind of the circuit's SHA rows"""
    out = {}
    for kind in range(4):
        for i, v in enumerate(circ["consts"][6 + kind]):
            if int(v):
                out[i] = kind
    return out


def sha_target(k, kinds):
    """(row, wire, new value or None = add 1) for SHA constraint k: the bit or carry wire of a boolean slot (on a row of kind k mod 4), and for
    the eight shared slots a routed word that only that slot (and later ones) reads — E rows for slots 0..5, ADD rows for slots 6 and 7"""
    by_kind = {kd: sorted(i for i, x in kinds.items() if x == kd) for kd in range(4)}
    assert all(by_kind[kd] for kd in range(4)), "the circuit needs SHA rows of all four kinds"
    if k < 132:
        return by_kind[k % 4][0], 12 + k, 2
    s = k - 132
    if s < 6:
        return by_kind[pref.SHA_E][0], [0, 1, 2, 7, 6, 4][s], None
    return by_kind[pref.SHA_ADD][0], [6, 9][s - 6], None


def mutate(wires, row, wire, value=None):
    w = wires.copy()
    w[wire, row] = (int(w[wire, row]) + 1) % P if value is None else value
    return w
