// witness_plan.h — a recorded circuit's witness program (verify.hip: the 15 op kinds of witness_run) compiled into a LEVEL SCHEDULE.
//
// The program is straight-line: each op defines new variables from earlier ones.  The level of an op is 0 when it reads no variable
// (INPUT, ZERO) and 1 + the highest level among the producers of its operands otherwise; ops of one level are independent.  A signature leaf
// is 1.2 M ops in 8 k levels (profiles/witness_depth.py), so one workgroup walks an instance level by level with a barrier
// between levels (witness_kernels.cuh) instead of one lane walking 1.2 M dependent ops.
//
// glp_wit_compile does ALL structural checks of witness_run once (indices < n_values, constants < p, shift / bit counts, op lengths, every
// operand written by an earlier op, every variable written at most once): the executors below index memory without bounds checks.
//
// Device stream (u32 words), ops ordered by (level, kind, program order):
//   ARITH   w x y z d          d = index into the dictionary of distinct (c0, c1, c2) triples (u64[3] each; a signature leaf has 1.05 M ARITH
//                              ops and a few hundred triples: 20 bytes per op where the host program spends 64)
//   others  the op's words after the kind, each narrowed to 32 bits (variable indices, input index, bit / shift counts, the SHA round constant)
// A variable that NO op writes (a recorded circuit may hold some; they can sit in wire cells) is 0: the host evaluator leaves such a word as the
// caller passed it and WitnessProgram.evaluate passes zeros, so the plan lists those variables and its executors write the zeros themselves.
// A RUN is a maximal range of one level's ops of one kind: {kind, count, word offset}; level l owns runs [level_run[l], level_run[l + 1]).
// PARTS.  A recursion node is one instance whose ops are fan-in mutually independent verifier segments (the seg_bounds of glp_witness_eval_mt:
// n_seg + 1 ascending word offsets on op boundaries).  glp_wit_compile_ex cuts such a program into n_seg + 2 parts — the prefix
// [0, seg_bounds[0]), one part per segment, the tail — and gives each part its OWN level schedule: the level of an op counts only producers
// inside its part (what an earlier part wrote is simply there).  The parts' levels are laid one after the other in the one level_run / runs /
// stream, part s owning levels [part_level[s], part_level[s + 1]): walking all levels in order runs the parts in order (glp_wit_run_host, and
// the single-workgroup kernel, stay correct on a segmented plan), while glp_witness_eval_part_kernel gives every segment a workgroup of its own.
// The independence claim (an op of segment s reads only what the prefix or segment s wrote) is checked HERE: the kernel has no checks.
// This header is host + device C++ with no HIP runtime dependency: the CPU emulation (tests/emu_witness, tests/emu_witness_seg) compiles it
// unchanged.
#pragma once
#include <stdint.h>
#include <map>
#include <tuple>
#include <vector>
#include "../../include/glprover.h"
#include "gl_field.cuh"
#include "hash_kernels.cuh"
#include "plonk_gates.h"
#include "nnf25519.h"

#define GLP_WIT_KINDS 15
#ifndef GLP_WIT_WG
#define GLP_WIT_WG 256        // workgroup size of glp_witness_eval_kernel (the `steps` of glp_witness_plan_stats are counted at this width)
#endif
// words per op in the HOST program, kind included (the table witness_run decodes with)
static const uint32_t GLP_WIT_OP_LEN[GLP_WIT_KINDS] = {8, 3, 4, 3, 5, 2, 25, 10, 6, 6, 4, 5, 26, 9, 2 + 2 * GLP_NNF_LIMBS};
// words per record in the device stream
GL_HD u32 glp_wit_rec_len(u32 kind) {
    constexpr u32 L[GLP_WIT_KINDS] = {5, 2, 3, 2, 4, 1, 24, 9, 5, 5, 3, 4, 25, 8, 1 + 2 * GLP_NNF_LIMBS};
    return L[kind];
}

struct glp_wit_run { u32 kind, count, off; };

struct glp_wit_view {           // what an executor reads (host vectors or their device copies)
    const u32* stream;
    const glp_wit_run* runs;
    const u32* level_run;       // depth + 1 entries
    const u64* dict;            // 3 words per ARITH constant triple
    const u32* eq;              // 2 * n_eq variable indices
    const u32* zero;            // the variables no op writes: set to 0 before level 0
    u32 depth, n_eq, n_inputs, n_values, n_zero;
};

GL_HD gl_ext2 glp_wit_ext_inv(gl_ext2 x) {       // 1 / (a + b X) in F_p[X]/(X^2 - 7): the formula of verify.hip's ext_inv
    const u64 nrm = gl_sub(gl_mul(x.a, x.a), gl_mul(7, gl_mul(x.b, x.b)));
    const u64 ni = gl_inv(nrm);
    return {gl_mul(x.a, ni), gl_mul(gl_neg(x.b), ni)};
}

// One op of the device stream on instance values `v`: the per-op bodies of witness_run.  Returns GLP_OK, or the refusal witness_run gives for a
// VALUE (GLP_E_REJECT: an operand no row can hold; GLP_E_INVALID: an input word >= p) after writing 0 to the op's results — the caller decides
// whether to stop (host) or to flag the instance and go on (device).  No index is computed from a value.
template <bool SMALL>
GL_HD int glp_wit_exec(u32 kind, const u32* __restrict__ r, const u64* __restrict__ dict, const u64* __restrict__ in, u64* v,
                       const GlpPoseidonConsts& pk) {
    switch (kind) {
        case 0: {
            const u64* c = dict + 3 * (size_t)r[4];
            v[r[0]] = gl_add(gl_add(gl_mul(c[0], gl_mul(v[r[1]], v[r[2]])), gl_mul(c[1], v[r[3]])), c[2]);
            return GLP_OK;
        }
        case 1: {
            const u64 x = in[r[1]];
            v[r[0]] = x < GL_P ? x : 0;
            return x < GL_P ? GLP_OK : GLP_E_INVALID;
        }
        case 2: v[r[0]] = (v[r[1]] >> r[2]) & 1ull; return GLP_OK;
        case 3: { const u64 x = v[r[1]]; v[r[0]] = x ? gl_inv(x) : 0; return GLP_OK; }
        case 4: {
            const gl_ext2 x{v[r[2]], v[r[3]]};
            const gl_ext2 w = (x.a || x.b) ? glp_wit_ext_inv(x) : gl_ext2{0, 0};
            v[r[0]] = w.a; v[r[1]] = w.b;
            return GLP_OK;
        }
        case 5: v[r[0]] = 0; return GLP_OK;
        case 6: case 12: {
            u64 st[12];
            for (int i = 0; i < 12; i++) st[i] = v[r[12 + i]];
            bool bad = false;
            if (kind == 12) {
                const u64 sw = v[r[24]];
                bad = sw > 1;
                if (sw == 1) for (int i = 0; i < 4; i++) { const u64 t = st[i]; st[i] = st[4 + i]; st[4 + i] = t; }
            }
            glp_poseidon_permute<SMALL>(st, pk);
            for (int i = 0; i < 12; i++) v[r[i]] = bad ? 0 : st[i];
            return bad ? GLP_E_REJECT : GLP_OK;
        }
        case 7: {   // SHA_E  T1 e_new | e f g h d w | K
            u64 x[6], any = 0;
            for (int i = 0; i < 6; i++) { x[i] = v[r[2 + i]]; any |= x[i]; }
            const bool bad = (any >> 32) != 0;
            const u64 t1 = x[3] + glp_sha_S1(x[0]) + glp_sha_ch(x[0], x[1], x[2]) + (u64)r[8] + x[5];
            v[r[0]] = bad ? 0 : t1;
            v[r[1]] = bad ? 0 : ((x[4] + t1) & 0xFFFFFFFFull);
            return bad ? GLP_E_REJECT : GLP_OK;
        }
        case 8: {   // SHA_A  a_new | a b c T1
            const u64 a = v[r[1]], b = v[r[2]], c = v[r[3]], t1 = v[r[4]];
            const bool bad = ((a | b | c) >> 32) || (t1 >> 35);
            v[r[0]] = bad ? 0 : ((t1 + glp_sha_S0(a) + glp_sha_maj(a, b, c)) & 0xFFFFFFFFull);
            return bad ? GLP_E_REJECT : GLP_OK;
        }
        case 9: {   // SHA_W  w_new | w16 w15 w7 w2
            const u64 w16 = v[r[1]], w15 = v[r[2]], w7 = v[r[3]], w2 = v[r[4]];
            const bool bad = ((w16 | w15 | w7 | w2) >> 32) != 0;
            v[r[0]] = bad ? 0 : ((w16 + glp_sha_s0(w15) + w7 + glp_sha_s1(w2)) & 0xFFFFFFFFull);
            return bad ? GLP_E_REJECT : GLP_OK;
        }
        case 10: {
            const u64 x = v[r[1]], y = v[r[2]];
            const bool bad = ((x | y) >> 32) != 0;
            v[r[0]] = bad ? 0 : ((x + y) & 0xFFFFFFFFull);
            return bad ? GLP_E_REJECT : GLP_OK;
        }
        case 11: {
            const u64 sh = v[r[1]] >> r[2];
            v[r[0]] = r[3] >= 64 ? sh : (sh & ((1ull << r[3]) - 1));
            return GLP_OK;
        }
        case 13: {
            const gl_ext2 x{v[r[2]], v[r[3]]}, y{v[r[4]], v[r[5]]}, z{v[r[6]], v[r[7]]};
            const gl_ext2 w = gl_ext_add(gl_ext_mul(x, y), z);
            v[r[0]] = w.a; v[r[1]] = w.b;
            return GLP_OK;
        }
        default: {  // 14 NNF_MUL  first | a0..a10 | b0..b10
            u64 va[GLP_NNF_LIMBS], vb[GLP_NNF_LIMBS], out[GLP_NNF_OUT];
            for (int i = 0; i < GLP_NNF_LIMBS; i++) { va[i] = v[r[1 + i]]; vb[i] = v[r[1 + GLP_NNF_LIMBS + i]]; }
            const bool ok = glp_nnf::mul_hints(va, vb, out);
            for (int i = 0; i < GLP_NNF_OUT; i++) v[(size_t)r[0] + i] = ok ? out[i] : 0;
            return ok ? GLP_OK : GLP_E_REJECT;
        }
    }
}

struct glp_wit_part { u64 n_ops, steps; u32 depth; };       // one part's share of the schedule (steps at GLP_WIT_WG lanes)

struct glp_wit_compiled {
    std::vector<u32> stream;
    std::vector<glp_wit_run> runs;
    std::vector<u32> level_run;
    std::vector<u32> part_level;          // parts + 1 entries: part s owns levels [part_level[s], part_level[s + 1]); a plain plan is ONE part
    std::vector<glp_wit_part> parts;
    std::vector<u64> dict;
    std::vector<u32> eq;
    std::vector<u32> zero;
    u64 n_ops = 0, steps = 0;
    u32 depth = 0, n_inputs = 0, n_values = 0;
    glp_wit_view view() const {
        return glp_wit_view{stream.data(), runs.data(), level_run.data(), dict.data(), eq.data(), zero.data(), depth, (u32)(eq.size() / 2), n_inputs, n_values,
                            (u32)zero.size()};
    }
    size_t stream_bytes() const {
        return stream.size() * 4 + runs.size() * sizeof(glp_wit_run) + level_run.size() * 4 + dict.size() * 8 + (eq.size() + zero.size()) * 4 +
               (parts.size() > 1 ? part_level.size() * 4 : 0);
    }
};

// program -> schedule.  GLP_E_INVALID for a program witness_run would refuse on structure (or one that reads a variable nobody wrote / writes one
// twice: witness_run checks those for the segments of glp_witness_eval_mt), GLP_E_UNSUPPORTED when an index does not fit 32 bits.
// seg_bounds / n_seg: the independent segments (see PARTS above); n_seg < 2 compiles the plain plan — one part, seg_bounds not looked at.  With
// segments also GLP_E_INVALID for an offset that is not an op boundary, descending or past the program, and for a false independence claim.
inline int glp_wit_compile_ex(const u64* prog, size_t prog_words, size_t n_inputs, size_t n_values, const u64* eq_pairs, size_t n_eq,
                              const u64* seg_bounds, size_t n_seg, glp_wit_compiled& out) {
    if ((!prog && prog_words) || (!eq_pairs && n_eq)) return GLP_E_INVALID;
    if (n_values >= 0xFFFFFFFFull || n_inputs >= 0xFFFFFFFFull || n_eq >= 0x7FFFFFFFull) return GLP_E_UNSUPPORTED;
    if (n_seg < 2) n_seg = 0;
    if (n_seg) {
        if (!seg_bounds || n_seg >= 0xFFFE) return GLP_E_INVALID;
        for (size_t k = 0; k <= n_seg; k++)
            if (seg_bounds[k] > prog_words || (k && seg_bounds[k] < seg_bounds[k - 1])) return GLP_E_INVALID;
    }
    const u32 n_parts = n_seg ? (u32)n_seg + 2 : 1;
    const u32 NONE = 0xFFFFFFFFu;
    std::vector<u32> lvl(n_values, NONE);                      // level, inside its part, of the op that wrote the variable
    std::vector<uint16_t> owner(n_seg ? n_values : 0, 0);      // ... and that part
    struct Op { u64 pc; u32 level; u32 kind; };                // level: inside the part while scanning, in the whole schedule afterwards
    std::vector<Op> ops;
    ops.reserve(prog_words / 7 + 1);
    std::vector<u32> part_ops(n_parts + 1, 0);                 // part s = ops [part_ops[s], part_ops[s + 1])
    std::vector<u32> part_depth(n_parts, 0);
    u32 part = 0;
    size_t bound = 0;                                          // seg_bounds[bound] is the next offset the scan has to land on
    size_t pc = 0;
    for (;;) {
        while (n_seg && bound <= n_seg && seg_bounds[bound] == pc) {      // (an empty segment: two offsets at one op boundary)
            part_ops[++part] = (u32)ops.size();
            bound++;
        }
        if (pc >= prog_words) break;
        if (n_seg && bound <= n_seg && seg_bounds[bound] < pc) return GLP_E_INVALID;          // an offset inside the op just scanned
        const u64 kind = prog[pc];
        if (kind >= GLP_WIT_KINDS || pc + GLP_WIT_OP_LEN[kind] > prog_words) return GLP_E_INVALID;
        if (ops.size() >= 0xFFFFFFFEull) return GLP_E_UNSUPPORTED;
        const u64* a = prog + pc + 1;
        u32 level = 0;
        bool ok = true;
        const bool in_segment = n_seg && part >= 1 && part <= n_seg;
        auto rd = [&](u64 var) {                               // an operand: in range and written by an earlier op
            if (var >= n_values || lvl[var] == NONE) { ok = false; return; }
            if (n_seg && owner[var] != part) {                 // an earlier part's: there before this part starts — unless it is ANOTHER SEGMENT's
                if (in_segment && owner[var] != 0) ok = false;
                return;
            }
            if (lvl[var] + 1 > level) level = lvl[var] + 1;
        };
        u64 wr[GLP_NNF_OUT];
        int n_wr = 0;
        switch (kind) {
            case 0: rd(a[1]); rd(a[2]); rd(a[3]); wr[n_wr++] = a[0]; ok = ok && a[4] < GL_P && a[5] < GL_P && a[6] < GL_P; break;
            case 1: wr[n_wr++] = a[0]; ok = a[1] < n_inputs; break;
            case 2: rd(a[1]); wr[n_wr++] = a[0]; ok = ok && a[2] < 64; break;
            case 3: rd(a[1]); wr[n_wr++] = a[0]; break;
            case 4: rd(a[2]); rd(a[3]); wr[n_wr++] = a[0]; wr[n_wr++] = a[1]; break;
            case 5: wr[n_wr++] = a[0]; break;
            case 6: case 12:
                for (int i = 0; i < 12; i++) { rd(a[12 + i]); wr[n_wr++] = a[i]; }
                if (kind == 12) rd(a[24]);
                break;
            case 7: for (int i = 2; i < 8; i++) rd(a[i]); wr[n_wr++] = a[0]; wr[n_wr++] = a[1]; ok = ok && a[8] <= 0xFFFFFFFFull; break;
            case 8: case 9: for (int i = 1; i < 5; i++) rd(a[i]); wr[n_wr++] = a[0]; break;
            case 10: rd(a[1]); rd(a[2]); wr[n_wr++] = a[0]; break;
            case 11: rd(a[1]); wr[n_wr++] = a[0]; ok = ok && a[2] < 64 && a[3] >= 1 && a[3] <= 64; break;
            case 13: for (int i = 2; i < 8; i++) rd(a[i]); wr[n_wr++] = a[0]; wr[n_wr++] = a[1]; break;
            default:
                for (int i = 0; i < 2 * GLP_NNF_LIMBS; i++) rd(a[1 + i]);
                if (a[0] >= n_values || a[0] + GLP_NNF_OUT > n_values) ok = false;
                else for (int i = 0; i < GLP_NNF_OUT; i++) wr[n_wr++] = a[0] + i;
                break;
        }
        if (!ok) return GLP_E_INVALID;
        for (int i = 0; i < n_wr; i++) {
            if (wr[i] >= n_values || lvl[wr[i]] != NONE) return GLP_E_INVALID;      // out of range, or written twice (by another op or by this one)
            lvl[wr[i]] = level;
            if (n_seg) owner[wr[i]] = (uint16_t)part;
        }
        ops.push_back(Op{pc, level, (u32)kind});
        if (level + 1 > part_depth[part]) part_depth[part] = level + 1;
        pc += GLP_WIT_OP_LEN[kind];
    }
    if (n_seg && bound <= n_seg) return GLP_E_INVALID;          // an offset inside the last op
    for (u32 s = part + 1; s <= n_parts; s++) part_ops[s] = (u32)ops.size();
    for (size_t k = 0; k < 2 * n_eq; k++) if (eq_pairs[k] >= n_values) return GLP_E_INVALID;
    // the parts' levels one after the other
    std::vector<u32> part_level(n_parts + 1, 0);
    for (u32 s = 0; s < n_parts; s++) {
        if ((u64)part_level[s] + part_depth[s] >= NONE) return GLP_E_UNSUPPORTED;
        part_level[s + 1] = part_level[s] + part_depth[s];
        for (u32 k = part_ops[s]; k < part_ops[s + 1]; k++) ops[k].level += part_level[s];
    }
    const u32 depth = part_level[n_parts];
    // counting sort by (level, kind), program order kept inside a run
    std::vector<u64> start((size_t)depth * GLP_WIT_KINDS + 1, 0);
    for (const Op& o : ops) start[(size_t)o.level * GLP_WIT_KINDS + o.kind + 1]++;
    u64 words = 0;
    out = glp_wit_compiled();
    out.level_run.assign((size_t)depth + 1, 0);
    out.parts.resize(n_parts);
    for (u32 s = 0; s < n_parts; s++) out.parts[s] = glp_wit_part{(u64)part_ops[s + 1] - part_ops[s], 0, part_depth[s]};
    std::vector<u64> word_at((size_t)depth * GLP_WIT_KINDS, 0);
    u32 cur = 0;
    for (u32 l = 0; l < depth; l++) {
        while (part_level[cur + 1] <= l) cur++;
        out.level_run[l] = (u32)out.runs.size();
        u64 width = 0;
        for (u32 k = 0; k < GLP_WIT_KINDS; k++) {
            const u64 cnt = start[(size_t)l * GLP_WIT_KINDS + k + 1];
            word_at[(size_t)l * GLP_WIT_KINDS + k] = words;
            if (!cnt) continue;
            if (words > 0xFFFFFFFFull || cnt > 0xFFFFFFFFull) return GLP_E_UNSUPPORTED;
            out.runs.push_back(glp_wit_run{k, (u32)cnt, (u32)words});
            words += cnt * glp_wit_rec_len(k);
            width += cnt;
        }
        out.parts[cur].steps += (width + GLP_WIT_WG - 1) / GLP_WIT_WG;
        out.steps += (width + GLP_WIT_WG - 1) / GLP_WIT_WG;
    }
    if (words > 0xFFFFFFFFull) return GLP_E_UNSUPPORTED;
    out.level_run[depth] = (u32)out.runs.size();
    out.stream.resize(words);
    std::map<std::tuple<u64, u64, u64>, u32> dict;
    for (const Op& o : ops) {
        u64& at = word_at[(size_t)o.level * GLP_WIT_KINDS + o.kind];
        u32* rec = out.stream.data() + at;
        const u64* a = prog + o.pc + 1;
        if (o.kind == 0) {
            auto it = dict.emplace(std::make_tuple(a[4], a[5], a[6]), (u32)dict.size()).first;
            for (int i = 0; i < 4; i++) rec[i] = (u32)a[i];
            rec[4] = it->second;
        } else {
            for (u32 i = 0; i + 1 < GLP_WIT_OP_LEN[o.kind]; i++) rec[i] = (u32)a[i];
        }
        at += glp_wit_rec_len(o.kind);
    }
    out.dict.resize(3 * dict.size() + 3, 0);
    for (const auto& kv : dict) {
        out.dict[3 * (size_t)kv.second] = std::get<0>(kv.first);
        out.dict[3 * (size_t)kv.second + 1] = std::get<1>(kv.first);
        out.dict[3 * (size_t)kv.second + 2] = std::get<2>(kv.first);
    }
    for (size_t i = 0; i < n_values; i++) if (lvl[i] == NONE) out.zero.push_back((u32)i);
    out.eq.resize(2 * n_eq);
    for (size_t k = 0; k < 2 * n_eq; k++) out.eq[k] = (u32)eq_pairs[k];
    out.part_level = part_level;
    out.n_ops = ops.size();
    out.depth = depth;
    out.n_inputs = (u32)n_inputs;
    out.n_values = (u32)n_values;
    return GLP_OK;
}
inline int glp_wit_compile(const u64* prog, size_t prog_words, size_t n_inputs, size_t n_values, const u64* eq_pairs, size_t n_eq, glp_wit_compiled& out) {
    return glp_wit_compile_ex(prog, prog_words, n_inputs, n_values, eq_pairs, n_eq, nullptr, 0, out);
}

// the REORDERED stream, serially, on the host: the check of the schedule on a machine without a GPU (not a product path).  Stops at the first
// refused op like witness_run does; then the copy constraints.
template <bool SMALL>
inline int glp_wit_run_host(const glp_wit_view& p, const GlpPoseidonConsts& pk, const u64* inputs, u64* values, size_t* first_bad) {
    if (first_bad) *first_bad = (size_t)-1;
    for (u32 k = 0; k < p.n_zero; k++) values[p.zero[k]] = 0;
    for (u32 l = 0; l < p.depth; l++)
        for (u32 r = p.level_run[l]; r < p.level_run[l + 1]; r++) {
            const glp_wit_run run = p.runs[r];
            const u32 len = glp_wit_rec_len(run.kind);
            for (u32 k = 0; k < run.count; k++) {
                const int rc = glp_wit_exec<SMALL>(run.kind, p.stream + run.off + (size_t)k * len, p.dict, inputs, values, pk);
                if (rc != GLP_OK) return rc;
            }
        }
    for (u32 k = 0; k < p.n_eq; k++)
        if (values[p.eq[2 * k]] != values[p.eq[2 * k + 1]]) { if (first_bad) *first_bad = k; return GLP_E_REJECT; }
    return GLP_OK;
}

// WORD CHECKS: the facts a recorded circuit ties between words of its inputs that are NOT program inputs and variables it computes (the
// wc_var / wc_bits tables of WitnessProgram.check_words).  Check k < n_var: v[var_idx[k]] is the wanted word; check n_var + j: the bits
// v[bit_vars[i]], i in [bit_start[j], bit_start[j + 1]), packed little-endian (the sum of v << position, mod 2^64) are the wanted word.
// var_want / bit_want are the instance's n_var / n_bits wanted words.  A variable index >= row_words, the words of an instance's row (no table a
// recording makes holds one), fails the check instead of being read.
struct glp_wit_words {
    const u32* var_idx;
    const u32* bit_vars;
    const u32* bit_start;         // n_bits + 1 ascending entries
    u32 n_var, n_bits;
};
GL_HD bool glp_wit_word_ok(const glp_wit_words& t, const u64* v, u64 row_words, const u64* var_want, const u64* bit_want, u32 k) {
    if (k < t.n_var) return t.var_idx[k] < row_words && v[t.var_idx[k]] == var_want[k];
    const u32 j = k - t.n_var;
    u64 packed = 0;
    for (u32 i = t.bit_start[j]; i < t.bit_start[j + 1]; i++) {
        if (t.bit_vars[i] >= row_words) return false;
        const u32 sh = i - t.bit_start[j];
        packed += sh < 64 ? v[t.bit_vars[i]] << sh : 0;
    }
    return packed == bit_want[j];
}
// every check of B instances, serially on the host: the lowest failing index of each kind per instance, ~0 when none fails
inline void glp_wit_check_words_host(const glp_wit_words& t, const u64* values, size_t value_stride, u32 B, const u64* var_want, const u64* bit_want,
                                     u64* first_bad_var, u64* first_bad_bits) {
    for (u32 b = 0; b < B; b++) {
        first_bad_var[b] = first_bad_bits[b] = ~0ull;
        const u64* v = values + (size_t)b * value_stride;
        const u64 *vw = var_want + (size_t)b * t.n_var, *bw = bit_want + (size_t)b * t.n_bits;
        for (u32 k = 0; k < t.n_var + t.n_bits; k++)
            if (!glp_wit_word_ok(t, v, value_stride, vw, bw, k)) {
                u64& first = k < t.n_var ? first_bad_var[b] : first_bad_bits[b];
                const u64 idx = k < t.n_var ? k : k - t.n_var;
                if (idx < first) first = idx;
            }
    }
}
