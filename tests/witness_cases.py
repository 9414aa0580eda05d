"""Edge-value inputs for the witness evaluator's 15 op kinds (a helper module, not a conftest).

edge_program() is one program whose op operands are all direct inputs, so that an instance chooses every operand freely; the same words with
the segment bounds it returns are its segmented twin (prefix | two segments | tail).  edge_batch() is about 300 seeded instances: one or a
few edge choices each, the other inputs random in range.  The NNF_MUL operands come from the classes N0..N7 below, which are sorted by what
tests/witness_ref.py alone says about them (fold count of the 2^255 reduction, the final subtraction, negative carries) and rotated over the
70 NNF_MUL slots.  reference() runs tests/witness_ref.py over the batch once per process."""
import functools
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import witness_ref as ref  # noqa: E402

P, Q, NONE = ref.P, ref.Q, ref.NONE
M32 = 0xFFFFFFFF
SENTINEL = 0xABCD                                     # what the tests fill the value slab with before a kernel runs
N_NNF = 70
NNF_SPLIT = (4, 30, 30, 6)                            # NNF_MUL ops in the prefix, segment A, segment B and the tail
FIELD_EDGES = (0, 1, 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63, P - 2**32, P - 2, P - 1)
BIT_EDGES = (0, 1, 2**63, P - 1, 2**32 - 1, 2**32)
ARITH_CONSTS = ((P - 1, P - 1, P - 1), (0, 0, 0), (1, 1, 0), (2, 2**32 - 1, 2**32), (2**32, P - 1, 1), (P - 1, 0, 2), (0, P - 1, P - 1),
                (1, 2, 2**32 - 1), (0x9E3779B97F4A7C15 % P, 0xC2B2AE3D27D4EB4F % P, 0x165667B19E3779F9 % P), (2**32 - 1, 2**32, 0xD6E8FEB86659FD93 % P))
BIT_KS = (0, 1, 31, 32, 62, 63)
BITS_GRID = ((0, 1), (0, 32), (0, 63), (0, 64), (31, 2), (32, 32), (40, 32), (1, 63), (63, 1), (63, 64))
SHA_KS = (0, 0xFFFFFFFF, 0x428A2F98)


# ---- the program ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_program():
    """(prog, n_inputs, n_values, eq_pairs, seg_bounds, slots).  slots: name -> the input indices of that operand group (variable i holds input
    i); slots["unwritten"]: the three variables no op writes; slots["nnf_first"][s]: the first of the 44 result variables of NNF_MUL slot s."""
    slots, n_in = {}, [0]

    def inp(name, n):
        slots[name] = list(range(n_in[0], n_in[0] + n))
        n_in[0] += n
        return slots[name]
    for k in range(len(ARITH_CONSTS)):
        inp(f"arith{k}", 3)
    for k in range(len(BIT_KS)):
        inp(f"bit{k}", 1)
    for k in range(len(BITS_GRID)):
        inp(f"bits{k}", 1)
    inp("inv", 1)
    inp("einv", 2)
    for k in range(2):
        inp(f"pos{k}", 12)
    for k in range(2):
        inp(f"swap{k}", 13)                                                # the state, then the swap cell
    for k in range(len(SHA_KS)):
        inp(f"sha_e{k}", 6)                                                # e f g h d w
    inp("sha_a_computed", 3)                                               # a b c (T1 is SHA_E 1's: K = 0xFFFFFFFF)
    inp("sha_a_free", 4)                                                   # a b c T1
    inp("sha_w", 4)
    inp("add32", 2)
    inp("extmuladd", 6)
    inp("copy0", 2)                                                        # copy pair 0: two inputs
    inp("copy2", 1)                                                        # copy pair 2: this input and BITS (0, 64) of bits3's operand
    for s in range(N_NNF):
        inp(f"nnf{s}", 22)
    n_inputs = n_in[0]
    prog, nv, cuts, results = [], [n_inputs], [], []

    def new(n=1):
        v = nv[0]
        nv[0] += n
        return v

    def arith(k):
        w = new()
        prog.extend([0, w, *slots[f"arith{k}"], *ARITH_CONSTS[k]])
        results.append(w)

    def nnf(s):
        first = new(44)
        prog.extend([14, first, *slots[f"nnf{s}"]])
        slots.setdefault("nnf_first", []).append(first)
        results.append(first + (5 * s) % 44)

    for i in reversed(range(n_inputs)):
        prog.extend([1, i, i])
    # ---- prefix
    zero = new()
    prog.extend([5, zero])
    results.append(zero)
    for k in range(0, 4):
        arith(k)
    for s in range(0, NNF_SPLIT[0]):
        nnf(s)
    cuts.append(len(prog))
    # ---- segment A
    for k, bit in enumerate(BIT_KS):
        w = new()
        prog.extend([2, w, slots[f"bit{k}"][0], bit])
        results.append(w)
    for k, (shift, bits) in enumerate(BITS_GRID):
        w = new()
        prog.extend([11, w, slots[f"bits{k}"][0], shift, bits])
        results.append(w)
        if (shift, bits) == (0, 64):
            whole = w
    w = new()
    prog.extend([3, w, slots["inv"][0]])
    results.append(w)
    w = new(2)
    prog.extend([4, w, w + 1, *slots["einv"]])
    results.extend([w, w + 1])
    for k in range(2):
        w = new(12)
        prog.extend([6, *range(w, w + 12), *slots[f"pos{k}"]])
        results.append(w + 3 + 7 * k)
    for k in range(4, 7):
        arith(k)
    for s in range(NNF_SPLIT[0], NNF_SPLIT[0] + NNF_SPLIT[1]):
        nnf(s)
    cuts.append(len(prog))
    # ---- segment B
    for k in range(2):
        w = new(12)
        prog.extend([12, *range(w, w + 12), *slots[f"swap{k}"]])
        results.append(w + 1 + 4 * k)
    t1 = {}
    for k, K in enumerate(SHA_KS):
        w = new(2)
        prog.extend([7, w, w + 1, *slots[f"sha_e{k}"], K])
        results.extend([w, w + 1])
        t1[K] = w
    w = new()
    prog.extend([8, w, *slots["sha_a_computed"], t1[0xFFFFFFFF]])
    results.append(w)
    w = new()
    prog.extend([8, w, *slots["sha_a_free"]])
    results.append(w)
    w = new()
    prog.extend([9, w, *slots["sha_w"]])
    results.append(w)
    w = new()
    prog.extend([10, w, *slots["add32"]])
    results.append(w)
    w = new(2)
    prog.extend([13, w, w + 1, *slots["extmuladd"]])
    results.extend([w, w + 1])
    for k in range(7, 10):
        arith(k)
    for s in range(NNF_SPLIT[0] + NNF_SPLIT[1], N_NNF - NNF_SPLIT[3]):
        nnf(s)
    cuts.append(len(prog))
    # ---- tail: the last NNF_MUL level, then a row of ARITH ops that reads a result of every op above
    for s in range(N_NNF - NNF_SPLIT[3], N_NNF):
        nnf(s)
    closing = []
    for k, r in enumerate(results):
        w = new()
        prog.extend([0, w, r, results[(k + 1) % len(results)], results[(k + 7) % len(results)], 1 + k, P - 1 - k, 3 + k])
        closing.append(w)
    slots["closing"] = closing
    slots["unwritten"] = [new(), new(), new()]
    eq = [slots["copy0"][0], slots["copy0"][1], zero, slots["unwritten"][1], slots["copy2"][0], whole]
    return (np.array(prog, dtype=np.uint64), n_inputs, nv[0], np.array(eq, dtype=np.uint64), np.array(cuts, dtype=np.uint64), slots)


# ---- NNF_MUL operands -----------------------------------------------------------------------------------------------------------------------
def limbs_of(value):
    """canonical 24-bit limbs, the top limb taking the rest (below 2^28 for a value below 2^268)"""
    assert 0 <= value < 1 << 268
    return tuple((value >> (24 * i)) & 0xFFFFFF for i in range(10)) + (value >> 240,)


@functools.lru_cache(maxsize=None)
def nnf_classes(seed=7):
    """name -> list of (a limbs, b limbs); every case accepted except N7_refused"""
    rng = random.Random(seed)
    full = (2**28 - 1,) * 11
    out = {"N0": [(limbs_of(0), limbs_of(rng.randrange(Q))), (limbs_of(rng.randrange(Q)), limbs_of(0)), (limbs_of(0), limbs_of(0))],
           "N1": [(full, full)],
           "N2": [(limbs_of(a), limbs_of(b)) for a in (Q, Q + 1, Q + 18, Q - 1, 2**255, 2 * Q) for b in (1, 3)]}

    def congruent(s, folds):                                               # A * B = s (mod q), both near 2^268; redrawn until the reference
        while True:                                                        # counts the wanted folds (s = 2^34 needs A * B above 2^535.8)
            b = rng.randrange(1 << 267, 1 << 268)
            a0 = s * pow(b, Q - 2, Q) % Q
            j = rng.randrange(1 if a0 == 0 else 0, ((1 << 268) - a0 + Q - 1) // Q)
            assert a0 + j * Q < 1 << 268
            a_limbs, b_limbs = limbs_of(a0 + j * Q), limbs_of(b)
            if ref.nnf_path(a_limbs, b_limbs)[0] == folds:
                return a_limbs, b_limbs
    out["N3"] = [congruent(s, 2) for s in range(19)]
    out["N4"] = [congruent(s, 3) for s in list(range(19, 40)) + [2**20, 2**34]]

    def picked():
        return tuple(rng.choice((0, 1, 2**24 - 1, 2**24, 2**28 - 1, rng.randrange(1 << 28))) for _ in range(11))
    out["N5"] = [(picked(), picked()) for _ in range(120)]
    out["N6"] = [(limbs_of(rng.randrange(Q)), limbs_of(rng.randrange(Q))) for _ in range(40)]
    out["N7_accepted"], out["N7_refused"] = [], []
    for pos in range(22):
        for value, name in ((2**28, "N7_refused"), (2**28 - 1, "N7_accepted")):
            ab = list(limbs_of(rng.randrange(Q)) + limbs_of(rng.randrange(Q)))
            ab[pos] = value
            out[name].append((tuple(ab[:11]), tuple(ab[11:])))
    return out


@functools.lru_cache(maxsize=None)
def nnf_paths(seed=7):
    """the accepted cases sorted by the path the reference says they take: "f0".."f3" (folds, no final subtraction) and "sub" (the final
    subtraction, whatever the folds), and the counts the issue asks for"""
    groups = {"f0": [], "f1": [], "f2": [], "f3": [], "sub": []}
    stats = {"folds": [0, 0, 0, 0], "subtract": 0, "three_folds": 0, "negative_carry": 0, "carry_bits": 0, "accepted": 0}
    for name, cases in nnf_classes(seed).items():
        if name == "N7_refused":
            continue
        for a, b in cases:
            folds, sub, neg, bits = ref.nnf_path(a, b)
            groups["sub" if sub else f"f{folds}"].append((a, b))
            stats["folds"][folds] += 1
            stats["subtract"] += sub
            stats["three_folds"] += folds == 3
            stats["negative_carry"] += neg > 0
            stats["carry_bits"] = max(stats["carry_bits"], bits)
            stats["accepted"] += 1
    return groups, stats


# ---- the instances --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_batch(seed=7):
    """(inputs [B][n_inputs] uint64, notes [B]): see the module docstring.  The two last instances hold ONE path in all 70 NNF_MUL slots (three
    folds; the final subtraction): wavefronts that do not diverge, next to the others' that do."""
    _, n_inputs, _, _, _, slots = edge_program()
    rng = random.Random(seed)
    groups, _ = nnf_paths(seed)
    order = ("f0", "f1", "f2", "f3", "sub")
    used = {g: 0 for g in order}
    rows, notes = [], []
    sha_words = [i for k in range(len(SHA_KS)) for i in slots[f"sha_e{k}"]] + slots["sha_a_computed"] + slots["sha_a_free"][:3] + slots["sha_w"] + slots["add32"]
    field_ops = [i for k in range(len(ARITH_CONSTS)) for i in slots[f"arith{k}"]] + slots["inv"] + slots["einv"] + slots["extmuladd"]
    bit_ops = [slots[f"bit{k}"][0] for k in range(len(BIT_KS))] + [slots[f"bits{k}"][0] for k in range(len(BITS_GRID))]

    def base(uniform=None):
        v = [rng.randrange(P) for _ in range(n_inputs)]
        for i in sha_words:
            v[i] = rng.randrange(1 << 32)
        v[slots["sha_a_free"][3]] = rng.randrange(1 << 35)
        for k in range(2):
            v[slots[f"swap{k}"][12]] = rng.randrange(2)
        v[slots["copy0"][1]] = v[slots["copy0"][0]]
        b = len(rows)
        for s in range(N_NNF):                                             # neighbouring slots: different paths; over the batch every slot sees every path
            g = uniform or order[(s + b) % len(order)]
            a_limbs, b_limbs = groups[g][used[g] % len(groups[g])]
            used[g] += 1
            v[slots[f"nnf{s}"][0]: slots[f"nnf{s}"][0] + 22] = a_limbs + b_limbs
        return v

    def add(note, edits=(), uniform=None, pair2=True):
        v = base(uniform)
        for idx, value in edits:
            v[idx] = value
        if pair2:                                                          # copy pair 2 holds: the input equals BITS (0, 64) of bits3's operand
            v[slots["copy2"][0]] = v[slots["bits3"][0]]
        rows.append(v)
        notes.append(note)

    # field operands
    for e in FIELD_EDGES:
        add(f"field operands all {e:#x}", [(i, e) for i in field_ops])
    for r in range(len(FIELD_EDGES)):
        add(f"field operands cycling through the edges from {r}", [(i, FIELD_EDGES[(n + r) % len(FIELD_EDGES)]) for n, i in enumerate(field_ops)])
    for pair in ((0, 0), (rng.randrange(1, P), 0), (0, rng.randrange(1, P)), (P - 1, P - 1)):
        add(f"EINV of {pair}", list(zip(slots["einv"], pair)))
    # inputs that are no field elements: refused with -1, alone and next to a refused row
    for bad in (P, 2**64 - 1):
        add(f"INPUT {bad:#x}", [(slots["arith5"][1], bad)])
        add(f"INPUT {bad:#x} and a swap cell of 2", [(slots["arith5"][1], bad), (slots["swap1"][12], 2)])
    add("INPUT p in an NNF limb and a SHA word of 2^32", [(slots["nnf33"][4], P), (slots["sha_w"][1], 2**32)])
    add("INPUT p - 1 everywhere a field element goes", [(i, P - 1) for i in field_ops + bit_ops + slots["pos0"] + slots["swap0"][:12] + slots["copy0"]])
    # bit ops
    for e in BIT_EDGES:
        add(f"bit operands all {e:#x}", [(i, e) for i in bit_ops])
    # SHA words
    add("SHA words all 0", [(i, 0) for i in sha_words] + [(slots["sha_a_free"][3], 0)])
    add("SHA words all 0xFFFFFFFF", [(i, M32) for i in sha_words] + [(slots["sha_a_free"][3], 2**35 - 1)])
    for i in sha_words:
        add(f"SHA word 2^32 at input {i}", [(i, 2**32)])
    add("free T1 2^35 - 1", [(slots["sha_a_free"][3], 2**35 - 1)])
    add("free T1 2^35", [(slots["sha_a_free"][3], 2**35)])
    add("free T1 2^32", [(slots["sha_a_free"][3], 2**32)])
    for i in (slots["sha_e0"][2], slots["sha_a_free"][1], slots["sha_a_free"][3], slots["sha_w"][3], slots["add32"][0]):
        add(f"2^63 at SHA input {i}", [(i, 2**63)])
    # swap cells
    for k in range(2):
        for e in (0, 1, 2, P - 1):
            add(f"swap cell {k} = {e:#x}", [(slots[f"swap{k}"][12], e)])
    # copy pairs
    add("copy pair 0 fails", [(slots["copy0"][1], 5), (slots["copy0"][0], 6)])
    add("copy pair 2 fails", [(slots["copy2"][0], 11), (slots["bits3"][0], 12)], pair2=False)
    add("copy pairs 0 and 2 fail", [(slots["copy0"][1], 5), (slots["copy0"][0], 6), (slots["copy2"][0], 11), (slots["bits3"][0], 12)], pair2=False)
    add("copy pair 0 fails next to a refused row", [(slots["copy0"][1], 5), (slots["copy0"][0], 6), (slots["add32"][1], 2**32)])
    # NNF limbs of 2^28: one refused product per instance, the slot moving
    for n, (a_limbs, b_limbs) in enumerate(nnf_classes(seed)["N7_refused"]):
        s = (3 * n + 1) % N_NNF
        add(f"NNF limb {n} = 2^28 in slot {s}", list(zip(slots[f"nnf{s}"], a_limbs + b_limbs)))
    while len(rows) < 298:
        add("random operands")
    add("all 70 NNF_MUL slots fold three times", uniform="f3")
    add("all 70 NNF_MUL slots take the final subtraction", uniform="sub")
    assert all(n >= len(groups[g]) for g, n in used.items())               # every accepted case sits in some slot
    return np.array(rows, dtype=np.uint64), notes


def consts_ints(consts):
    return tuple(tuple(int(v) for v in part) for part in consts)


_reference = {}


def reference(kind, consts, mode):
    """[(rc, first_bad, values uint64[n_values])] of witness_ref.run over edge_batch(), once per process for each (constant kind, mode)"""
    if (kind, mode) not in _reference:
        prog, _, n_values, eq, _, _ = edge_program()
        batch, _ = edge_batch()
        words, pairs, ints = prog.tolist(), eq.tolist(), consts_ints(consts)
        out = []
        for row in batch.tolist():
            rc, bad, values = ref.run(words, row, n_values, pairs, ints, mode)
            out.append((rc, bad, np.array(values, dtype=np.uint64)))
        _reference[(kind, mode)] = out
    return _reference[(kind, mode)]
