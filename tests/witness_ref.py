"""An independent interpreter of the witness program (the 15 op kinds documented above witness_run in csrc/verify.hip), in Python integers
(a helper module, not a conftest).

It shares nothing with the product: no ctypes call into the library and nothing from the package.  The Poseidon permutation is
plonk_ref.poseidon_row with the injected constants, the SHA-256 functions are written from FIPS 180-4 §4.1.2, the quadratic extension is
F_p[X]/(X^2 - 7), and NNF_MUL is divmod by q = 2^255 - 19 followed by the 21 carries of the column identity in the header of csrc/nnf25519.h.

run() has the two behaviours the product documents for a refused op: the host evaluators stop there, the kernels write 0 to the op's
results, flag the instance and go on (csrc/witness_kernels.cuh), so that every word of a refused instance has an expected value too."""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonk_ref  # noqa: E402

P = 2**64 - 2**32 + 1
Q = 2**255 - 19
NONE = 2**64 - 1
OK, INVALID, REJECT = 0, -1, -7
OP_LEN = (8, 3, 4, 3, 5, 2, 25, 10, 6, 6, 4, 5, 26, 9, 24)
M32 = 0xFFFFFFFF


# ---- FIPS 180-4 §4.1.2, on 32-bit words ------------------------------------------------------------------------------------------------------
def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def big_sigma0(x):
    return _rotr(x, 2) ^ _rotr(x, 13) ^ _rotr(x, 22)


def big_sigma1(x):
    return _rotr(x, 6) ^ _rotr(x, 11) ^ _rotr(x, 25)


def small_sigma0(x):
    return _rotr(x, 7) ^ _rotr(x, 18) ^ (x >> 3)


def small_sigma1(x):
    return _rotr(x, 17) ^ _rotr(x, 19) ^ (x >> 10)


def ch(x, y, z):
    return (x & y) ^ (~x & M32 & z)


def maj(x, y, z):
    return (x & y) ^ (x & z) ^ (y & z)


# ---- the quadratic extension F_p[X]/(X^2 - 7) ---------------------------------------------------------------------------------------------
def ext_mul(x, y):
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def ext_inv(x):
    """1 / (a + b X) = (a - b X) / (a^2 - 7 b^2); 0 -> 0 (7 is no square: the norm of a non-zero element is non-zero)"""
    n = pow((x[0] * x[0] - 7 * x[1] * x[1]) % P, P - 2, P)
    return (x[0] * n % P, (-x[1]) * n % P)


# ---- NNF_MUL ------------------------------------------------------------------------------------------------------------------------------
def limbs_value(limbs):
    return sum(int(v) << (24 * i) for i, v in enumerate(limbs))


@functools.lru_cache(maxsize=None)
def nnf_mul(a, b):
    """the 44 words (r[11], k[12], c_0..c_20) of the product of two operands given as tuples of 11 limbs, or None when a limb is >= 2^28"""
    if any(v >> 28 for v in a + b):
        return None
    k, r = divmod(limbs_value(a) * limbs_value(b), Q)
    rl = [(r >> (24 * i)) & 0xFFFFFF for i in range(11)]
    kl = [(k >> (24 * i)) & 0xFFFFFF for i in range(12)]
    assert k >> 288 == 0
    out, carry = rl + kl, 0
    for t in range(22):
        col = sum(a[i] * b[t - i] for i in range(max(0, t - 10), min(t, 10) + 1)) + carry
        if t < 12:
            col += 19 * kl[t]
        if 10 <= t:
            col -= kl[t - 10] << 15
        if t < 11:
            col -= rl[t]
        assert col % (1 << 24) == 0
        carry = col >> 24
        assert abs(carry) < 1 << 62
        if t < 21:
            out.append(carry if carry >= 0 else P - (-carry))
    assert carry == 0
    return tuple(out)


def nnf_path(a, b):
    """(folds, subtract, negative carries, largest |carry| in bits) of an accepted product: how often Hi * 2^255 + Lo -> Lo + 19 Hi has to be
    applied until the remainder is below 2^255, whether that remainder is still >= q, and the signs of the carries — counted here, from the
    integers alone, so that a test can say which paths of any implementation its cases reach"""
    rem, folds = limbs_value(a) * limbs_value(b), 0
    while rem >> 255:
        rem = (rem & ((1 << 255) - 1)) + 19 * (rem >> 255)
        folds += 1
    carries = [c if c < P // 2 else c - P for c in nnf_mul(a, b)[23:]]
    return folds, rem >= Q, sum(c < 0 for c in carries), max(abs(c).bit_length() for c in carries)


# ---- Poseidon -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _permute(consts, state, swap):
    return tuple(plonk_ref.poseidon_row(list(state), consts, swap)[12:24])


# ---- the interpreter ----------------------------------------------------------------------------------------------------------------------
def run(prog, inputs, n_values, eq_pairs, consts, mode):
    """(rc, first_bad, values) of a well-formed program.  rc: 0, -1 (an input word >= p) or -7; first_bad: the lowest failing copy pair, NONE
    when an op refused or nothing failed.  mode "host": stop at the first refused op (the values are then unfinished and only the verdict
    means something); mode "device": a refused op's results are 0, the rest runs, -1 wins over -7."""
    assert mode in ("host", "device")
    prog, inputs, eq_pairs = [int(w) for w in prog], [int(w) for w in inputs], [int(w) for w in eq_pairs]
    key = tuple(tuple(int(c) for c in part) for part in consts)
    v = [0] * n_values                                                     # a variable no op writes is 0
    refused = []
    pc = 0
    while pc < len(prog):
        kind = prog[pc]
        a = prog[pc + 1: pc + OP_LEN[kind]]
        pc += OP_LEN[kind]
        rc, outs = OK, None
        if kind == 0:
            outs = {a[0]: (a[4] * v[a[1]] * v[a[2]] + a[5] * v[a[3]] + a[6]) % P}
        elif kind == 1:
            x = inputs[a[1]]
            rc, outs = (OK, {a[0]: x}) if x < P else (INVALID, {a[0]: 0})
        elif kind == 2:
            outs = {a[0]: (v[a[1]] >> a[2]) & 1}
        elif kind == 3:
            outs = {a[0]: pow(v[a[1]], P - 2, P)}
        elif kind == 4:
            w = ext_inv((v[a[2]], v[a[3]]))
            outs = {a[0]: w[0], a[1]: w[1]}
        elif kind == 5:
            outs = {a[0]: 0}
        elif kind in (6, 12):
            swap = v[a[24]] if kind == 12 else 0
            if swap > 1:
                rc, outs = REJECT, {w: 0 for w in a[:12]}
            else:
                outs = dict(zip(a[:12], _permute(key, tuple(v[i] for i in a[12:24]), swap)))
        elif kind == 7:
            e, f, g, h, d, w = (v[i] for i in a[2:8])
            if max(e, f, g, h, d, w) > M32:
                rc, outs = REJECT, {a[0]: 0, a[1]: 0}
            else:
                t1 = h + big_sigma1(e) + ch(e, f, g) + a[8] + w
                outs = {a[0]: t1, a[1]: (d + t1) & M32}
        elif kind == 8:
            x, y, z, t1 = (v[i] for i in a[1:5])
            if max(x, y, z) > M32 or t1 >= 1 << 35:
                rc, outs = REJECT, {a[0]: 0}
            else:
                outs = {a[0]: (t1 + big_sigma0(x) + maj(x, y, z)) & M32}
        elif kind == 9:
            w16, w15, w7, w2 = (v[i] for i in a[1:5])
            if max(w16, w15, w7, w2) > M32:
                rc, outs = REJECT, {a[0]: 0}
            else:
                outs = {a[0]: (w16 + small_sigma0(w15) + w7 + small_sigma1(w2)) & M32}
        elif kind == 10:
            x, y = v[a[1]], v[a[2]]
            rc, outs = (REJECT, {a[0]: 0}) if max(x, y) > M32 else (OK, {a[0]: (x + y) & M32})
        elif kind == 11:
            outs = {a[0]: (v[a[1]] >> a[2]) % (1 << a[3])}
        elif kind == 13:
            w = ext_mul((v[a[2]], v[a[3]]), (v[a[4]], v[a[5]]))
            outs = {a[0]: (w[0] + v[a[6]]) % P, a[1]: (w[1] + v[a[7]]) % P}
        else:
            assert kind == 14
            out = nnf_mul(tuple(v[i] for i in a[1:12]), tuple(v[i] for i in a[12:23]))
            rc = OK if out is not None else REJECT
            outs = {a[0] + i: (out[i] if out is not None else 0) for i in range(44)}
        if rc != OK:
            if mode == "host":
                return rc, NONE, v
            refused.append(rc)
        for var, val in outs.items():
            v[var] = val
    if refused:
        return (INVALID if INVALID in refused else REJECT), NONE, v
    for k in range(len(eq_pairs) // 2):
        if v[eq_pairs[2 * k]] != v[eq_pairs[2 * k + 1]]:
            return REJECT, k, v
    return OK, NONE, v
