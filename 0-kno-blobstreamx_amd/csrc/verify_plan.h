// verify_plan.h — the native verifier's host phase and the plan it writes for the batched query phase.
//
// A verification has a serial part — header and range checks, the transcript replay, proof of work, the query indices, the alpha powers
// and opening sums, the PLONK identity at zeta — and a part that is independent per (proof, query): leaf hashes, Merkle paths, the
// combination, the folds and the final polynomial.  fri_verify below is split accordingly into fri_pre / fri_query / the checks after the
// queries.  The single verifier (glp_plonk_verify*, glp_fri_verify*) runs fri_query for q = 0 .. nq-1 in place; the batched verifier
// (glp_plonk_verify_batch, glp_fri_verify_batch: verify.hip) passes a VerifyPlan, and fri_verify then RECORDS the query phase instead:
// a descriptor per proof (GlpVerifyDesc), its tables (idxs, per-tree offsets, betas, alpha powers ...) and one work item per
// (proof, query, tree) and per (proof, query), which verify_batch_kernels.cuh runs — on the device, or serially on the host.
//
// Every failure the query loop can find has a key (query << 16 | step), the steps numbered in the order the loop tests them
// (glp_vstep_*); the lowest key over all items is the failure the loop would have stopped at.  Every offset the items use is computed
// HERE from the range-checked header and checked against the proof's length: the proof's own words are field data only, the query index
// is the transcript's.  A query that does not lie wholly inside the proof is never handed out: the host runs fri_query on it and records
// its key.  The reason texts live in one table (glp_vr_text) shared by both verifiers.
// Host C++ and GL_HD helpers only, no HIP call: tests/emu_verify_batch compiles this file with a host compiler.
#pragma once
#include <stdio.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../include/glprover.h"
#include "gl_field.cuh"
#include "hash_kernels.cuh"
#include "challenger.h"
#include "plonk_gates.h"

// ---- what the items read (device-visible, laid out in words) ------------------------------------------------------------------------
#define GLP_VB_MAX_ARITY_BITS 4u                 // the fold of one layer leaf (2^a extension values) stays in registers up to here
#define GLP_VB_MAX_OPENINGS 65536u               // alpha powers uploaded per proof: 16 bytes each
#define GLP_VB_KEY_NONE 0xFFFFFFFFFFFFFFFFull
#define GLP_VB_BLOCK 64u                         // one wavefront per workgroup: the lanes of a wave walk the same tree of consecutive queries

// word offsets (o_*) are relative to the proof's block of the table slab; offsets inside the proof are in words from its start
struct GlpVerifyDesc {
    u64 base;                    // the proof's first word in the proof slab
    u64 aux;                     // its tables' first word in the table slab
    u64 shift, w_N;              // coset shift, primitive 2^log_N-th root of unity
    u32 log_N, cap0, a, L, final_bits, nb, n_pts, nq;      // nq: the queries handed out (a prefix of the proof's)
    u32 n_order, pt_used, q0, qwords, fin_off, key_slot;   // q0: first query's offset; every query is qwords long
    u32 o_idx, o_batch, o_layer, o_order, o_ys, o_pts, o_apow, pad;
};
// tables: idx[nq] | per batch {n_polys, leaf offset inside the query, cap offset inside the proof} | per layer {leaf offset inside the
// query, cap offset inside the proof, cap height, log2 of the layer's length, beta.a, beta.b} | order[n_order] (point | batch << 32) |
// Ys[n_pts][2] | points[n_pts][2] | apow[total][2]
#define GLP_VB_BATCH_WORDS 3u
#define GLP_VB_LAYER_WORDS 6u
static_assert(sizeof(GlpVerifyDesc) == 120, "the descriptor is uploaded as words");

// steps of one query, in the order the query loop tests them
GL_HD u32 glp_vstep_index_truncated() { return 0; }
GL_HD u32 glp_vstep_index() { return 1; }
GL_HD u32 glp_vstep_batch(u32 b, u32 k) { return 2 + 3 * b + k; }                         // k: 0 truncated, 1 non-canonical leaf, 2 Merkle path
GL_HD u32 glp_vstep_point(u32 nb) { return 2 + 3 * nb; }
GL_HD u32 glp_vstep_layer(u32 nb, u32 l, u32 k) { return 3 + 3 * nb + 4 * l + k; }        // k: 0 truncated, 1 non-canonical, 2 fold, 3 Merkle path
GL_HD u32 glp_vstep_final(u32 nb, u32 L) { return 3 + 3 * nb + 4 * L; }
GL_HD u64 glp_vkey(u32 q, u32 step) { return ((u64)q << 16) | step; }

static inline const char* glp_vr_text(u32 reason) {
    static const char* const T[GLP_VR_COUNT] = {
        "",
        "truncated",
        "bad tag",
        "bad header",
        "header out of range",
        "rate_bits = 0: a rate-1 code proves nothing",
        "fewer queries or less proof of work than required",
        "lower code rate (rate_bits) than required",
        "bad open masks",
        "bad point multiplier",
        "cap height",
        "non-canonical cap",
        "non-canonical opening",
        "non-canonical layer cap",
        "non-canonical final polynomial",
        "proof of work failed",
        "query index does not match the transcript",
        "non-canonical leaf",
        "Merkle path does not lead to the cap",
        "query point equals an opening point",
        "non-canonical layer leaf",
        "a layer value does not continue the fold",
        "layer Merkle path does not lead to the cap",
        "final polynomial mismatch",
        "trailing data in proof",
        "bad plonk header",
        "non-canonical public input",
        "public inputs differ from the expected statement",
        "preprocessed commitment differs from the circuit's",
        "FRI statement does not match the circuit shape",
        "FRI caps differ from the committed caps",
        "wrong opening points",
        "PLONK identity fails at zeta",
    };
    return reason < GLP_VR_COUNT ? T[reason] : "";
}
static inline u32 glp_vstep_reason(u32 step, u32 nb) {
    if (step == 0) return GLP_VR_TRUNCATED;
    if (step == 1) return GLP_VR_QUERY_INDEX;
    if (step < 2 + 3 * nb) {
        const u32 k = (step - 2) % 3;
        return k == 0 ? GLP_VR_TRUNCATED : k == 1 ? GLP_VR_LEAF_NONCANONICAL : GLP_VR_MERKLE_PATH;
    }
    if (step == 2 + 3 * nb) return GLP_VR_QUERY_AT_POINT;
    const u32 k = (step - 3 - 3 * nb) % 4;
    // the final polynomial's step is 3 + 3 nb + 4 L: k == 0 there as for a truncated layer; glp_vkey_reason, which knows L, tells them apart
    return k == 0 ? GLP_VR_TRUNCATED : k == 1 ? GLP_VR_LAYER_LEAF_NONCANONICAL : k == 2 ? GLP_VR_FOLD : GLP_VR_LAYER_MERKLE_PATH;
}
static inline u32 glp_vkey_reason(u64 key, u32 nb, u32 L) {
    const u32 step = (u32)(key & 0xFFFFu);
    return step == glp_vstep_final(nb, L) ? GLP_VR_FINAL_POLY : glp_vstep_reason(step, nb);
}

GL_HD bool glp_ext_eq(gl_ext2 x, gl_ext2 y) { return x.a == y.a && x.b == y.b; }
GL_HD gl_ext2 glp_ext_inv(gl_ext2 x) {
    const u64 nrm = gl_sub(gl_mul(x.a, x.a), gl_mul(7, gl_mul(x.b, x.b)));   // a^2 - 7 b^2
    const u64 ni = gl_inv(nrm);
    return {gl_mul(x.a, ni), gl_mul(gl_neg(x.b), ni)};
}
GL_HD u64 glp_bitrev(u64 v, u32 bits) {
    u64 r = 0;
    for (u32 i = 0; i < bits; i++) r |= ((v >> i) & 1ull) << (bits - 1 - i);
    return r;
}

namespace glp_verify {
const u64 FRI_TAG = 0x32304952464C4747ull;
const u64 PLONK_TAG = 0x32304B4C504C4747ull;   // "GGLPLK02"
const u32 CHUNK = 8, NCHAL = 2;

struct Reject {
    char* buf;           // receives "proof rejected: <reason text>" (may be null)
    size_t n;
    u32 reason = 0;      // GLP_VR_*
    u32 query = 0xFFFFFFFFu;
    int fail(u32 why, u32 q = 0xFFFFFFFFu) {
        reason = why;
        query = q;
        if (buf && n) snprintf(buf, n, "proof rejected: %s", glp_vr_text(why));
        return GLP_E_REJECT;
    }
};

struct Hasher {
    std::vector<u64> consts;
    bool small_mds;
    GlpPoseidonConsts k() const { return GlpPoseidonConsts{consts.data(), consts.data() + 360, consts.data() + 372, nullptr, nullptr}; }
    void permute(u64 (&s)[12]) const {
        if (small_mds) glp_poseidon_permute<true>(s, k());
        else glp_poseidon_permute<false>(s, k());
    }
    // digest of a leaf: the zero-padded leaf itself up to 4 elements, else the overwrite-mode sponge
    void hash_or_noop(const u64* e, size_t len, u64 (&out)[4]) const {
        if (len <= 4) {
            for (size_t i = 0; i < 4; i++) out[i] = i < len ? e[i] : 0;
            return;
        }
        u64 s[12] = {0};
        for (size_t off = 0; off < len; off += 8) {
            const size_t m = len - off < 8 ? len - off : 8;
            for (size_t i = 0; i < m; i++) s[i] = e[off + i];
            permute(s);
        }
        for (int i = 0; i < 4; i++) out[i] = s[i];
    }
    void two_to_one(const u64* l, const u64* r, u64 (&out)[4]) const {
        u64 s[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
        permute(s);
        for (int i = 0; i < 4; i++) out[i] = s[i];
    }
};

inline bool ext_eq(gl_ext2 x, gl_ext2 y) { return glp_ext_eq(x, y); }
inline gl_ext2 ext_inv(gl_ext2 x) { return glp_ext_inv(x); }
inline u64 bitrev(u64 v, u32 bits) { return glp_bitrev(v, bits); }

struct Reader {
    const u64* w;
    size_t n, pos;
    bool take(size_t k, const u64** out) {
        if (k > n - pos) return false;
        *out = w + pos;
        pos += k;
        return true;
    }
};

inline bool merkle_check(const Hasher& h, const u64 (&leaf_digest)[4], u64 index, const u64* path, u32 path_len, const u64* cap, u64 cap_len) {
    u64 cur[4] = {leaf_digest[0], leaf_digest[1], leaf_digest[2], leaf_digest[3]};
    for (u32 lvl = 0; lvl < path_len; lvl++) {
        u64 nxt[4];
        if (((index >> lvl) & 1ull) == 0) h.two_to_one(cur, path + 4 * lvl, nxt);
        else h.two_to_one(path + 4 * lvl, cur, nxt);
        memcpy(cur, nxt, sizeof(cur));
    }
    const u64 ci = index >> path_len;
    return ci < cap_len && memcmp(cur, cap + 4 * ci, sizeof(cur)) == 0;
}

struct FriInfo {
    u32 log_n = 0, rb = 0, cap0 = 0, n_pts = 0, nb = 0, nq = 0, pow_bits = 0;
    u64 shift = 0;
    u64 mults[4] = {0, 0, 0, 0};
    size_t caps_off = 0, openings_off = 0;       // word offsets inside the proof
    gl_ext2 zeta{0, 0};
    std::vector<gl_ext2> points;                 // zeta * mult[p]
    std::vector<u64> n_polys, masks;
    std::vector<const u64*> caps;                // per batch, 4 << cap0 words inside the proof
    std::vector<std::pair<u32, u32>> order;      // (point, batch) in opening order
    std::vector<size_t> open_off;                // offset into openings per order entry
    std::vector<gl_ext2> openings;
};

// what the query loop reads besides the proof's query words: everything fri_pre derived from the header and the transcript
struct FriQueries {
    u32 log_N = 0, cap0 = 0, a = 0, L = 0, final_bits = 0, nb = 0, n_pts = 0, nq = 0;
    u64 shift = 0, w_N = 0, inv2 = 0;
    const FriInfo* fi = nullptr;
    std::vector<gl_ext2> apow, Ys, betas;
    std::vector<bool> pt_used;
    std::vector<const u64*> layer_caps;
    std::vector<u32> layer_log, layer_caph;
    const u64* fin = nullptr;
    std::vector<u64> idxs;
    u64 query_words() const {                    // every query of a proof has the same length: the header fixes it
        u64 w = 1;
        for (u32 b = 0; b < nb; b++) w += fi->n_polys[b] + 4ull * (log_N - cap0);
        for (u32 l = 0; l < L; l++) w += (2ull << a) + 4ull * (layer_log[l] - a - layer_caph[l]);
        return w;
    }
};

// The plan of a batched call: descriptors, tables and items of the proofs whose query phase was recorded instead of run.
struct VerifyPlan {
    std::vector<GlpVerifyDesc> desc;
    std::vector<u64> aux;
    struct Item { u32 desc, q; };
    std::vector<std::vector<Item>> by_tree;      // Merkle items, tree-major: by_tree[t] = the (proof, query) pairs of the proofs that have a tree t
    std::vector<Item> arith;                     // (proof, query)
    // the proof being planned (reset per proof by the batched driver)
    bool recorded = false;                       // fri_verify recorded this proof's queries
    bool unsupported = false;                    // ... or ran them in place: a shape the items do not take
    u64 host_key = GLP_VB_KEY_NONE;              // a failure inside the query loop that the host found (truncated, index mismatch)
    size_t slab_words = 0;                       // proof slab: the sum of the recorded proofs' used words
    void begin_proof() { recorded = unsupported = false; host_key = GLP_VB_KEY_NONE; }
    size_t n_merkle() const { size_t s = 0; for (auto& v : by_tree) s += v.size(); return s; }
};
const int FRI_STOP = 1;                          // fri_verify with a plan: the host phase found a failure inside the query loop (plan.host_key)

// header .. query indices: everything before the query loop
inline int fri_pre(Reject& rj, const Hasher& h, glp_challenger& ch, Reader& rd, u32 min_queries, u32 min_pow_bits, u32 min_rate_bits, FriInfo& fi,
                   FriQueries& Q) {
    const u64* hd;
    if (!rd.take(11, &hd)) return rj.fail(GLP_VR_TRUNCATED);
    const u64 tag = hd[0], log_n = hd[1], rb = hd[2], cap0 = hd[3], a = hd[4], fb = hd[5], nq = hd[6], pow_bits = hd[7], shift = hd[8],
              nb = hd[9], n_pts = hd[10];
    if (tag != FRI_TAG) return rj.fail(GLP_VR_BAD_TAG);
    if (n_pts < 1 || n_pts > 4 || nb == 0 || nb > 64) return rj.fail(GLP_VR_BAD_HEADER);
    if (log_n > 32 || rb > 8 || log_n + rb > 32 || a == 0 || a > 8 || fb > 12 || nq == 0 || nq > 1024 || pow_bits > 40 || shift == 0 ||
        shift >= GL_P)
        return rj.fail(GLP_VR_HEADER_RANGE);
    // rate 1 (rate_bits = 0) is no proximity test at all: every word of length n is a codeword of degree < n, so ANY
    // claimed opening passes.  Never accepted, whatever the caller asks for.
    if (rb == 0) return rj.fail(GLP_VR_RATE_ONE);
    if (nq < min_queries || pow_bits < min_pow_bits) return rj.fail(GLP_VR_WEAK_PARAMS);
    if (rb < min_rate_bits) return rj.fail(GLP_VR_LOW_RATE);
    const u64 *mults, *pm;
    if (!rd.take(n_pts, &mults) || !rd.take(2 * nb, &pm)) return rj.fail(GLP_VR_TRUNCATED);
    bool first_point_used = false;
    for (u64 b = 0; b < nb; b++) {
        const u64 np = pm[2 * b], m = pm[2 * b + 1];
        if (np == 0 || np > (1u << 20) || m == 0 || (m >> n_pts)) return rj.fail(GLP_VR_OPEN_MASKS);
        if (m & 1) first_point_used = true;
    }
    if (!first_point_used) return rj.fail(GLP_VR_OPEN_MASKS);
    for (u64 p = 0; p < n_pts; p++)
        if (mults[p] == 0 || mults[p] >= GL_P) return rj.fail(GLP_VR_POINT_MULT);
    for (int i = 0; i < 11; i++) ch.observe(hd[i] % GL_P);
    for (u64 i = 0; i < n_pts; i++) ch.observe(mults[i]);
    for (u64 i = 0; i < 2 * nb; i++) ch.observe(pm[i]);
    const u32 log_N = (u32)(log_n + rb);
    const u64 N = 1ull << log_N;
    if (cap0 > log_N) return rj.fail(GLP_VR_CAP_HEIGHT);
    const u32 L = log_n > fb ? (u32)((log_n - fb) / a) : 0;
    const u32 final_bits = (u32)(log_n - a * L);
    fi.log_n = (u32)log_n; fi.rb = (u32)rb; fi.cap0 = (u32)cap0; fi.n_pts = (u32)n_pts; fi.nb = (u32)nb; fi.nq = (u32)nq; fi.pow_bits = (u32)pow_bits;
    fi.shift = shift;
    for (u64 p = 0; p < n_pts; p++) fi.mults[p] = mults[p];
    fi.caps_off = rd.pos;
    for (u64 b = 0; b < nb; b++) {
        const u64* cp;
        if (!rd.take((size_t)4 << cap0, &cp)) return rj.fail(GLP_VR_TRUNCATED);
        for (size_t i = 0; i < ((size_t)4 << cap0); i++) {
            if (cp[i] >= GL_P) return rj.fail(GLP_VR_CAP_NONCANONICAL);
            ch.observe(cp[i]);
        }
        fi.caps.push_back(cp);
        fi.n_polys.push_back(pm[2 * b]);
        fi.masks.push_back(pm[2 * b + 1]);
    }
    fi.zeta = ch.ext_challenge();
    size_t total = 0;
    for (u32 p = 0; p < n_pts; p++)
        for (u32 b = 0; b < nb; b++)
            if ((fi.masks[b] >> p) & 1) {
                fi.order.push_back({p, b});
                fi.open_off.push_back(total);
                total += fi.n_polys[b];
            }
    const u64* op;
    fi.openings_off = rd.pos;
    if (!rd.take(2 * total, &op)) return rj.fail(GLP_VR_TRUNCATED);
    fi.openings.resize(total);
    for (size_t k = 0; k < total; k++) {
        if (op[2 * k] >= GL_P || op[2 * k + 1] >= GL_P) return rj.fail(GLP_VR_OPENING_NONCANONICAL);
        ch.observe(op[2 * k]);
        ch.observe(op[2 * k + 1]);
        fi.openings[k] = {op[2 * k], op[2 * k + 1]};
    }
    const gl_ext2 alpha = ch.ext_challenge();
    std::vector<gl_ext2>& apow = Q.apow;
    apow.resize(total);
    apow[0] = {1, 0};
    for (size_t k = 1; k < total; k++) apow[k] = gl_ext_mul(apow[k - 1], alpha);
    Q.Ys.assign(n_pts, gl_ext2{0, 0});
    Q.pt_used.assign(n_pts, false);
    fi.points.resize(n_pts);
    for (u32 p = 0; p < n_pts; p++) fi.points[p] = gl_ext_scale(fi.zeta, mults[p]);
    {
        size_t kk = 0;
        for (auto& pb : fi.order) {
            Q.pt_used[pb.first] = true;
            for (u64 j = 0; j < fi.n_polys[pb.second]; j++, kk++) Q.Ys[pb.first] = gl_ext_add(Q.Ys[pb.first], gl_ext_mul(apow[kk], fi.openings[kk]));
        }
    }
    Q.layer_caps.resize(L); Q.betas.resize(L); Q.layer_log.resize(L); Q.layer_caph.resize(L);
    {
        u32 log_len = log_N;
        for (u32 l = 0; l < L; l++) {
            const u32 log_leaves = log_len - (u32)a;
            const u32 chh = cap0 < log_leaves ? (u32)cap0 : log_leaves;
            const u64* cp;
            if (!rd.take((size_t)4 << chh, &cp)) return rj.fail(GLP_VR_TRUNCATED);
            for (size_t i = 0; i < ((size_t)4 << chh); i++) {
                if (cp[i] >= GL_P) return rj.fail(GLP_VR_LAYER_CAP_NONCANONICAL);
                ch.observe(cp[i]);
            }
            Q.layer_caps[l] = cp;
            Q.betas[l] = ch.ext_challenge();
            Q.layer_log[l] = log_len;
            Q.layer_caph[l] = chh;
            log_len -= (u32)a;
        }
    }
    const u64* fin;
    if (!rd.take((size_t)2 << final_bits, &fin)) return rj.fail(GLP_VR_TRUNCATED);
    for (size_t i = 0; i < ((size_t)2 << final_bits); i++) {
        if (fin[i] >= GL_P) return rj.fail(GLP_VR_FINAL_NONCANONICAL);
        ch.observe(fin[i]);
    }
    u64 seed[4];
    for (int i = 0; i < 4; i++) seed[i] = ch.challenge();
    const u64* noncep;
    if (!rd.take(1, &noncep)) return rj.fail(GLP_VR_TRUNCATED);
    const u64 nonce = noncep[0] % GL_P;
    if (pow_bits) {
        u64 s[12] = {seed[0], seed[1], seed[2], seed[3], nonce, 0, 0, 0, 0, 0, 0, 0};
        h.permute(s);
        if (s[0] >> (64 - pow_bits)) return rj.fail(GLP_VR_POW);
    }
    ch.observe(nonce);
    Q.idxs.resize(nq);
    for (u64 q = 0; q < nq; q++) Q.idxs[q] = ch.challenge() & (N - 1);
    Q.log_N = log_N; Q.cap0 = (u32)cap0; Q.a = (u32)a; Q.L = L; Q.final_bits = final_bits; Q.nb = (u32)nb; Q.n_pts = (u32)n_pts; Q.nq = (u32)nq;
    Q.shift = shift; Q.w_N = gl_root_of_unity(log_N); Q.inv2 = gl_inv(2);
    Q.fi = &fi; Q.fin = fin;
    return GLP_OK;
}

// one query, read at rd.pos: -1 when every check holds, else the step (glp_vstep_*) of the first that does not
inline int fri_query(const Hasher& h, const FriQueries& Q, Reader& rd, u64 q) {
    const FriInfo& fi = *Q.fi;
    const u32 log_N = Q.log_N, cap0 = Q.cap0, nb = Q.nb, n_pts = Q.n_pts, L = Q.L, final_bits = Q.final_bits;
    const u64 a = Q.a, shift = Q.shift, inv2 = Q.inv2;
    const u64* ip;
    if (!rd.take(1, &ip)) return (int)glp_vstep_index_truncated();
    const u64 idx = ip[0];
    if (idx != Q.idxs[q]) return (int)glp_vstep_index();
    const u64 x = gl_mul(shift, gl_pow(Q.w_N, bitrev(idx, log_N)));
    std::vector<const u64*> leaves(nb);
    for (u32 b = 0; b < nb; b++) {
        const u64 *leaf, *path;
        if (!rd.take(fi.n_polys[b], &leaf) || !rd.take((size_t)4 * (log_N - cap0), &path)) return (int)glp_vstep_batch(b, 0);
        for (u64 j = 0; j < fi.n_polys[b]; j++)
            if (leaf[j] >= GL_P) return (int)glp_vstep_batch(b, 1);
        u64 dg[4];
        h.hash_or_noop(leaf, fi.n_polys[b], dg);
        if (!merkle_check(h, dg, idx, path, (u32)(log_N - cap0), fi.caps[b], 1ull << cap0)) return (int)glp_vstep_batch(b, 2);
        leaves[b] = leaf;
    }
    std::vector<gl_ext2> accs(n_pts, gl_ext2{0, 0}), vals, nxt;
    {
        size_t k = 0;
        for (auto& pb : fi.order)
            for (u64 j = 0; j < fi.n_polys[pb.second]; j++, k++) accs[pb.first] = gl_ext_add(accs[pb.first], gl_ext_scale(Q.apow[k], leaves[pb.second][j]));
    }
    gl_ext2 cur{0, 0};
    for (u32 p = 0; p < n_pts; p++)
        if (Q.pt_used[p]) {
            const gl_ext2 den = gl_ext_sub(gl_ext2{x, 0}, fi.points[p]);
            if (den.a == 0 && den.b == 0) return (int)glp_vstep_point(nb);
            cur = gl_ext_add(cur, gl_ext_mul(gl_ext_sub(accs[p], Q.Ys[p]), ext_inv(den)));
        }
    u64 sh = shift;
    for (u32 l = 0; l < L; l++) {
        const u32 ll = Q.layer_log[l];
        const u64 *leaf, *path;
        const u32 log_leaves = ll - (u32)a;
        if (!rd.take((size_t)2 << a, &leaf) || !rd.take((size_t)4 * (log_leaves - Q.layer_caph[l]), &path)) return (int)glp_vstep_layer(nb, l, 0);
        vals.assign((size_t)1 << a, gl_ext2{0, 0});
        for (size_t j = 0; j < ((size_t)1 << a); j++) {
            if (leaf[2 * j] >= GL_P || leaf[2 * j + 1] >= GL_P) return (int)glp_vstep_layer(nb, l, 1);
            vals[j] = {leaf[2 * j], leaf[2 * j + 1]};
        }
        const u64 p_l = idx >> (a * l);
        const u64 leaf_idx = p_l >> a;
        if (!ext_eq(vals[p_l & ((1ull << a) - 1)], cur)) return (int)glp_vstep_layer(nb, l, 2);
        u64 dg[4];
        h.hash_or_noop(leaf, (size_t)2 << a, dg);
        if (!merkle_check(h, dg, leaf_idx, path, log_leaves - Q.layer_caph[l], Q.layer_caps[l], 1ull << Q.layer_caph[l])) return (int)glp_vstep_layer(nb, l, 3);
        gl_ext2 beta = Q.betas[l];
        u64 base = leaf_idx << a;
        u32 cl = ll;
        for (u64 s = 0; s < a; s++) {
            const u64 wl = gl_root_of_unity(cl);
            nxt.resize(vals.size() / 2);
            for (size_t i = 0; i < vals.size() / 2; i++) {
                const u64 xi = gl_mul(sh, gl_pow(wl, bitrev(base + 2 * i, cl)));
                const gl_ext2 f0 = vals[2 * i], f1 = vals[2 * i + 1];
                const gl_ext2 sm = gl_ext_scale(gl_ext_add(f0, f1), inv2);
                const gl_ext2 d = gl_ext_scale(gl_ext_sub(f0, f1), gl_mul(inv2, gl_inv(xi)));
                nxt[i] = gl_ext_add(sm, gl_ext_mul(beta, d));
            }
            vals.swap(nxt);
            base >>= 1;
            cl -= 1;
            beta = gl_ext_mul(beta, beta);
            sh = gl_mul(sh, sh);
        }
        cur = vals[0];
    }
    const u32 fl = (u32)(log_N - a * L);
    const u64 xf = gl_mul(sh, gl_pow(gl_root_of_unity(fl), bitrev(idx >> (a * L), fl)));
    gl_ext2 ev{0, 0};
    for (size_t j = (size_t)1 << final_bits; j-- > 0;) ev = gl_ext_add(gl_ext_scale(ev, xf), gl_ext2{Q.fin[2 * j], Q.fin[2 * j + 1]});
    if (!ext_eq(ev, cur)) return (int)glp_vstep_final(nb, L);
    return -1;
}

// does the query phase of this proof fit the items (verify_batch_kernels.cuh)?  Everything else runs fri_query in place.
inline bool plan_supports(const FriQueries& Q, const Reader& rd) {
    if (Q.a > GLP_VB_MAX_ARITY_BITS || Q.apow.size() > GLP_VB_MAX_OPENINGS) return false;
    const u64 qw = Q.query_words();
    return rd.n < (1ull << 31) && rd.pos + qw * Q.nq < (1ull << 31);
}

// Record the query phase of the proof whose queries start at rd.pos.  Handed out: the longest prefix of queries that lie wholly inside the
// proof and whose index word is the transcript's; the first query that is not — if any — is settled here (fri_query on what is there) and
// leaves plan.host_key.  Offsets are computed from the header's range-checked shape only.
inline void plan_queries(const Hasher& h, const FriQueries& Q, Reader& rd, VerifyPlan& P) {
    const FriInfo& fi = *Q.fi;
    const u64 qw = Q.query_words();
    const size_t q0 = rd.pos;
    u32 nq_dev = 0;
    for (u32 q = 0; q < Q.nq; q++) {
        if (qw > rd.n - rd.pos) {                                   // does not lie inside the proof: the host settles it
            Reader part = rd;
            const int step = fri_query(h, Q, part, q);
            P.host_key = glp_vkey(q, (u32)step);                    // a truncated query fails somewhere: step >= 0
            break;
        }
        if (rd.w[rd.pos] != Q.idxs[q]) { P.host_key = glp_vkey(q, glp_vstep_index()); break; }
        rd.pos += (size_t)qw;
        nq_dev++;
    }
    P.recorded = true;
    GlpVerifyDesc d;
    memset(&d, 0, sizeof(d));
    const u32 me = (u32)P.desc.size();
    d.base = P.slab_words;
    d.aux = P.aux.size();
    d.shift = Q.shift; d.w_N = Q.w_N;
    d.log_N = Q.log_N; d.cap0 = Q.cap0; d.a = Q.a; d.L = Q.L; d.final_bits = Q.final_bits; d.nb = Q.nb; d.n_pts = Q.n_pts; d.nq = nq_dev;
    d.n_order = (u32)fi.order.size();
    for (u32 p = 0; p < Q.n_pts; p++) d.pt_used |= Q.pt_used[p] ? 1u << p : 0u;
    d.q0 = (u32)q0; d.qwords = (u32)qw; d.fin_off = (u32)(Q.fin - rd.w); d.key_slot = me;
    std::vector<u64>& A = P.aux;
    const size_t a0 = A.size();
    d.o_idx = 0;
    for (u32 q = 0; q < nq_dev; q++) A.push_back(Q.idxs[q]);
    d.o_batch = (u32)(A.size() - a0);
    u64 rel = 1;
    for (u32 b = 0; b < Q.nb; b++) {
        A.push_back(fi.n_polys[b]); A.push_back(rel); A.push_back((u64)(fi.caps[b] - rd.w));
        rel += fi.n_polys[b] + 4ull * (Q.log_N - Q.cap0);
    }
    d.o_layer = (u32)(A.size() - a0);
    for (u32 l = 0; l < Q.L; l++) {
        A.push_back(rel); A.push_back((u64)(Q.layer_caps[l] - rd.w)); A.push_back(Q.layer_caph[l]); A.push_back(Q.layer_log[l]);
        A.push_back(Q.betas[l].a); A.push_back(Q.betas[l].b);
        rel += (2ull << Q.a) + 4ull * (Q.layer_log[l] - Q.a - Q.layer_caph[l]);
    }
    d.o_order = (u32)(A.size() - a0);
    for (auto& pb : fi.order) A.push_back((u64)pb.first | ((u64)pb.second << 32));
    d.o_ys = (u32)(A.size() - a0);
    for (u32 p = 0; p < Q.n_pts; p++) { A.push_back(Q.Ys[p].a); A.push_back(Q.Ys[p].b); }
    d.o_pts = (u32)(A.size() - a0);
    for (u32 p = 0; p < Q.n_pts; p++) { A.push_back(fi.points[p].a); A.push_back(fi.points[p].b); }
    d.o_apow = (u32)(A.size() - a0);
    for (auto& v : Q.apow) { A.push_back(v.a); A.push_back(v.b); }
    P.slab_words += q0 + (size_t)qw * nq_dev;                       // the words the items can reach: header .. the last query handed out
    P.desc.push_back(d);
    const u32 trees = Q.nb + Q.L;
    if (P.by_tree.size() < trees) P.by_tree.resize(trees);
    for (u32 t = 0; t < trees; t++)
        for (u32 q = 0; q < nq_dev; q++) P.by_tree[t].push_back({me, q});
    for (u32 q = 0; q < nq_dev; q++) P.arith.push_back({me, q});
}

// The FRI opening proof starting at rd.pos, continuing the transcript `ch` (fresh for a stand-alone proof).  With a plan the query phase is
// recorded (plan->recorded) instead of run when its shape fits the items; FRI_STOP then says that the host found a failure inside the
// query loop (plan->host_key), a GLP_E_REJECT after the recording one that counts only when no item fails.
inline int fri_verify(Reject& rj, const Hasher& h, glp_challenger& ch, Reader& rd, bool allow_trailing, u32 min_queries, u32 min_pow_bits,
                      u32 min_rate_bits, FriInfo& fi, VerifyPlan* plan = nullptr) {
    FriQueries Q;
    int rc = fri_pre(rj, h, ch, rd, min_queries, min_pow_bits, min_rate_bits, fi, Q);
    if (rc != GLP_OK) return rc;
    if (plan && plan_supports(Q, rd)) {
        plan_queries(h, Q, rd, *plan);
        if (plan->host_key != GLP_VB_KEY_NONE) return FRI_STOP;
    } else {
        if (plan) plan->unsupported = true;
        for (u64 q = 0; q < Q.nq; q++) {
            const int step = fri_query(h, Q, rd, q);
            if (step >= 0) return rj.fail(glp_vkey_reason((u64)step, Q.nb, Q.L), (u32)q);
        }
    }
    if (rd.pos != rd.n && !allow_trailing) return rj.fail(GLP_VR_TRAILING);
    return GLP_OK;
}

inline void init_hasher(const std::vector<u64>& consts, bool small_mds, Hasher& h, glp_challenger& ch) {
    h.consts = consts;
    h.small_mds = small_mds;
    memset(ch.state, 0, sizeof(ch.state));
    ch.n_in = ch.n_out = 0;
    ch.consts = consts;
    ch.small_mds = small_mds;
}
// constants passed explicitly (the ctx-less entry points): same validity rules as glp_set_poseidon_constants
inline bool make_hasher_from(const u64* rc, const u64* circ, const u64* diag, Hasher& h, glp_challenger& ch) {
    if (!rc || !circ || !diag) return false;
    std::vector<u64> all(384);
    for (int i = 0; i < 360; i++) { if (rc[i] >= GL_P) return false; all[i] = rc[i]; }
    unsigned __int128 sum = 0;
    u64 maxdiag = 0;
    bool small = true;
    for (int i = 0; i < 12; i++) {
        if (circ[i] >= GL_P || diag[i] >= GL_P) return false;
        all[360 + i] = circ[i]; all[372 + i] = diag[i];
        sum += circ[i];
        if (diag[i] > maxdiag) maxdiag = diag[i];
        if (circ[i] >> 24 || diag[i] >> 24) small = false;
    }
    if (sum + maxdiag >= ((unsigned __int128)1 << 24)) small = false;
    init_hasher(all, small, h, ch);
    return true;
}
inline void reset_challenger(glp_challenger& ch) {
    memset(ch.state, 0, sizeof(ch.state));
    ch.n_in = ch.n_out = 0;
}

// sum_idx alpha_t^idx * C_idx at zeta for challenge t (the constraint list of plonk_kernels.cuh / DESIGN.md §3.6), extension field
inline gl_ext2 constraint_sum(u32 t, gl_ext2 x, gl_ext2 xn, u64 n, u32 R, bool poseidon, bool sha, const gl_ext2* q_ext, const u64* pos_consts, const std::vector<u64>& ks, const u64* beta,
                              const u64* gamma, const u64* alpha, const gl_ext2* consts, const gl_ext2* sigmas, const gl_ext2* wires, const gl_ext2* zs,
                              const gl_ext2* z_next, gl_ext2 pi_at_x) {
    typedef GlpGateExt O;
    const u32 M = R / CHUNK;
    const gl_ext2 one{1, 0};
    // L_1(x) = (x^n - 1) / (n (x - 1))
    const gl_ext2 l1 = gl_ext_mul(gl_ext_sub(xn, one), ext_inv(gl_ext_scale(gl_ext_sub(x, one), n % GL_P)));
    const gl_ext2 q = consts[0], c0 = consts[1], c1 = consts[2], c2 = consts[3], q_pi = consts[4], q_pos = consts[5];
    gl_ext2 acc = gl_ext_mul(l1, gl_ext_sub(zs[t * M], one));
    u64 ap = alpha[t];
    acc = gl_ext_add(acc, gl_ext_scale(gl_ext_sub(gl_ext_mul(q_pi, wires[0]), pi_at_x), ap));       // public inputs, alpha^1
    gl_ext2 prev = zs[t * M];
    const gl_ext2 bx = gl_ext_scale(x, beta[t]);
    for (u32 cidx = 0; cidx < M; cidx++) {
        gl_ext2 num = one, den = one;
        for (u32 j = cidx * CHUNK; j < (cidx + 1) * CHUNK; j++) {
            const gl_ext2 wg = gl_ext_add(wires[j], gl_ext2{gamma[t], 0});
            num = gl_ext_mul(num, gl_ext_add(wg, gl_ext_scale(bx, ks[j])));
            den = gl_ext_mul(den, gl_ext_add(wg, gl_ext_scale(sigmas[j], beta[t])));
        }
        const gl_ext2 nx = cidx + 1 < M ? zs[t * M + 1 + cidx] : z_next[t];
        const gl_ext2 perm = gl_ext_sub(gl_ext_mul(prev, num), gl_ext_mul(nx, den));
        const gl_ext2* w8 = wires + cidx * CHUNK;
        gl_ext2 g0 = gl_ext_mul(q, glp_arith_gate<O>(c0, c1, c2, w8[0], w8[1], w8[2], w8[3]));
        gl_ext2 g1 = gl_ext_mul(q, glp_arith_gate<O>(c0, c1, c2, w8[4], w8[5], w8[6], w8[7]));
        if (q_ext) {
            const gl_ext2 ww[8] = {w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7]};
            gl_ext2 e0, e1;
            glp_ext_gate<O>(ww, e0, e1);
            g0 = gl_ext_add(g0, gl_ext_mul(*q_ext, e0));
            g1 = gl_ext_add(g1, gl_ext_mul(*q_ext, e1));
        }
        const gl_ext2 cons[3] = {perm, g0, g1};
        for (int i = 0; i < 3; i++) {
            ap = gl_mul(ap, alpha[t]);
            acc = gl_ext_add(acc, gl_ext_scale(cons[i], ap));
        }
        prev = nx;
    }
    if (poseidon) {
        gl_ext2 pacc{0, 0};
        glp_poseidon_gate_constraints<O>([&](int j) -> gl_ext2 { return wires[j]; }, pos_consts, pos_consts + 360, pos_consts + 372,
                                         [&](gl_ext2 con) {
                                             ap = gl_mul(ap, alpha[t]);
                                             pacc = gl_ext_add(pacc, gl_ext_scale(con, ap));
                                         });
        acc = gl_ext_add(acc, gl_ext_mul(q_pos, pacc));
    }
    if (sha) {                                   // consts then has GLP_PLONK_NCONST_SHA entries; the constraints arrive selector-weighted
        const gl_ext2 qs[4] = {consts[6], consts[7], consts[8], consts[9]};
        glp_sha_gate_constraints<O>([&](int j) -> gl_ext2 { return wires[j]; }, qs, c2, [&](gl_ext2 con) {
            ap = gl_mul(ap, alpha[t]);
            acc = gl_ext_add(acc, gl_ext_scale(con, ap));
        });
    }
    return acc;
}

// PI(x) = sum_i pi_i * L_i(x),  L_i(x) = w^i (x^n - 1) / (n (x - w^i))   (the polynomial that is pi_i on row i < n_public, 0 elsewhere)
inline gl_ext2 public_input_poly_at(const u64* pub, u64 n_pub, gl_ext2 x, gl_ext2 xn, u32 log_n) {
    if (n_pub == 0) return gl_ext2{0, 0};
    const u64 n = 1ull << log_n, w = gl_root_of_unity(log_n);
    const gl_ext2 zh_over_n = gl_ext_scale(gl_ext_sub(xn, gl_ext2{1, 0}), gl_inv(n % GL_P));
    gl_ext2 acc{0, 0};
    u64 wi = 1;
    for (u64 i = 0; i < n_pub; i++) {
        const gl_ext2 li = gl_ext_mul(gl_ext_scale(zh_over_n, wi), ext_inv(gl_ext_sub(x, gl_ext2{wi, 0})));
        acc = gl_ext_add(acc, gl_ext_scale(li, pub[i]));
        wi = gl_mul(wi, w);
    }
    return acc;
}

inline bool proof_args_ok(const uint8_t* proof, size_t len) { return proof && len && len % 8 == 0 && ((uintptr_t)proof & 7) == 0; }

inline int fri_verify_entry(Reject& rj, const Hasher& h, glp_challenger& ch, const uint8_t* proof, size_t len, uint32_t min_queries,
                            uint32_t min_pow_bits, uint32_t min_rate_bits, glp_fri_statement* st, VerifyPlan* plan = nullptr) {
    Reader rd{(const u64*)proof, len / 8, 0};
    FriInfo fi;
    if (st) memset(st, 0, sizeof(*st));
    int rc = fri_verify(rj, h, ch, rd, false, min_queries, min_pow_bits, min_rate_bits, fi, plan);
    if (rc == GLP_OK && st) {     // WHAT was proven: the caller compares it with the statement it expects
        st->log_n = fi.log_n; st->rate_bits = fi.rb; st->cap_height = fi.cap0; st->n_batches = fi.nb; st->n_points = fi.n_pts;
        st->num_queries = fi.nq; st->pow_bits = fi.pow_bits; st->shift = fi.shift;
        st->zeta[0] = fi.zeta.a; st->zeta[1] = fi.zeta.b;
        for (u32 p = 0; p < 4; p++) st->point_mult[p] = fi.mults[p];
        st->caps_word_off = fi.caps_off; st->cap_words = (size_t)4 << fi.cap0;
        st->openings_word_off = fi.openings_off; st->n_openings = fi.openings.size();
        u32 np = 0;
        for (u32 b = 0; b < fi.nb && b < 64; b++) { st->n_polys[b] = (u32)fi.n_polys[b]; st->open_mask[b] = (u32)fi.masks[b]; np += (u32)fi.n_polys[b]; }
        st->total_polys = np;
    }
    return rc;
}

inline int plonk_verify_entry(Reject& rj, const Hasher& h, glp_challenger& ch, const uint8_t* proof, size_t len, const uint64_t* h_circuit_cap,
                              size_t cap_words, const uint64_t* h_public, size_t n_public_expected, uint32_t min_queries, uint32_t min_pow_bits,
                              VerifyPlan* plan = nullptr) {
    Reader rd{(const u64*)proof, len / 8, 0};
    auto take_obs = [&](size_t k, const u64** out) -> bool {
        if (!rd.take(k, out)) return false;
        for (size_t i = 0; i < k; i++) ch.observe((*out)[i] % GL_P);
        return true;
    };
    const u64* hd;
    if (!take_obs(8, &hd)) return rj.fail(GLP_VR_TRUNCATED);
    const u64 tag = hd[0], log_n = hd[1], W = hd[2], R = hd[3], rb = hd[4], cap_h = hd[5], n_pub = hd[6], flags = hd[7];
    if (tag != PLONK_TAG || rb != 3 || W % 8 || W < 8 || W > 160 || R % 8 || R < 8 || R > W || log_n < 3 || log_n > 24 ||
        n_pub > (1ull << log_n) || (flags & ~(u64)(GLP_CIRCUIT_POSEIDON_GATE | GLP_CIRCUIT_SHA_GATES | GLP_CIRCUIT_EXT_GATE)))
        return rj.fail(GLP_VR_PLONK_HEADER);
    const bool poseidon = (flags & GLP_CIRCUIT_POSEIDON_GATE) != 0, sha = (flags & GLP_CIRCUIT_SHA_GATES) != 0;
    if (poseidon && (W < GLP_POS_GATE_WIRES || R < 24)) return rj.fail(GLP_VR_PLONK_HEADER);
    if (sha && (W < GLP_SHA_GATE_WIRES || R < 16)) return rj.fail(GLP_VR_PLONK_HEADER);
    const u64 n_const = (u64)glp_plonk_n_const((u32)flags);
    const u64 n = 1ull << log_n;
    const u32 log_N = (u32)(log_n + rb), M = (u32)(R / CHUNK);
    const u64* pub;
    if (!rd.take((size_t)n_pub, &pub)) return rj.fail(GLP_VR_TRUNCATED);
    for (u64 i = 0; i < n_pub; i++) {
        if (pub[i] >= GL_P) return rj.fail(GLP_VR_PUBLIC_NONCANONICAL);
        ch.observe(pub[i]);
    }
    // the proof must be about THIS statement: the caller's public inputs, word for word
    if (h_public && (n_public_expected != n_pub || memcmp(h_public, pub, (size_t)n_pub * 8) != 0)) return rj.fail(GLP_VR_PUBLIC_DIFFER);
    const size_t capw = (size_t)4 << (cap_h < log_N ? cap_h : log_N);
    const u64 *cap_pre, *cap_wires, *cap_zs, *cap_q;
    if (cap_h > 32 || !take_obs(capw, &cap_pre) || !take_obs(capw, &cap_wires)) return rj.fail(GLP_VR_TRUNCATED);
    // ... and about THIS circuit: its preprocessed commitment is the verifying key
    if (h_circuit_cap && (cap_words != capw || memcmp(h_circuit_cap, cap_pre, capw * 8) != 0)) return rj.fail(GLP_VR_CIRCUIT_DIFFER);
    u64 beta[NCHAL], gamma[NCHAL], alpha[NCHAL];
    for (u32 t = 0; t < NCHAL; t++) beta[t] = ch.challenge();
    for (u32 t = 0; t < NCHAL; t++) gamma[t] = ch.challenge();
    if (!take_obs(capw, &cap_zs)) return rj.fail(GLP_VR_TRUNCATED);
    for (u32 t = 0; t < NCHAL; t++) alpha[t] = ch.challenge();
    if (!take_obs(capw, &cap_q)) return rj.fail(GLP_VR_TRUNCATED);
    FriInfo fi;
    int rc = fri_verify(rj, h, ch, rd, false, min_queries, min_pow_bits, 1, fi, plan);
    if (rc != GLP_OK) return rc;
    // the FRI part must be about exactly these commitments, shapes and points
    const u64 want_polys[4] = {n_const + R, W, (u64)NCHAL * M, (u64)NCHAL << rb};
    if (fi.nb != 4 || fi.log_n != log_n || fi.rb != rb || fi.cap0 != (cap_h < log_N ? cap_h : log_N)) return rj.fail(GLP_VR_FRI_SHAPE);
    const u64* want_caps[4] = {cap_pre, cap_wires, cap_zs, cap_q};
    for (int b = 0; b < 4; b++) {
        if (fi.n_polys[b] != want_polys[b]) return rj.fail(GLP_VR_FRI_SHAPE);
        if (memcmp(fi.caps[b], want_caps[b], capw * 8) != 0) return rj.fail(GLP_VR_FRI_CAPS);
    }
    const u64 g = gl_root_of_unity((unsigned)log_n);
    if (fi.n_pts != 2 || !ext_eq(fi.points[0], fi.zeta) || !ext_eq(fi.points[1], gl_ext_scale(fi.zeta, g))) return rj.fail(GLP_VR_POINTS);
    const std::pair<u32, u32> want_order[5] = {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {1, 2}};
    if (fi.order.size() != 5) return rj.fail(GLP_VR_POINTS);
    for (int i = 0; i < 5; i++)
        if (fi.order[i] != want_order[i]) return rj.fail(GLP_VR_POINTS);
    const gl_ext2* pre = fi.openings.data() + fi.open_off[0];
    const gl_ext2* wires = fi.openings.data() + fi.open_off[1];
    const gl_ext2* zs = fi.openings.data() + fi.open_off[2];
    const gl_ext2* quot = fi.openings.data() + fi.open_off[3];
    const gl_ext2* zs_next = fi.openings.data() + fi.open_off[4];
    std::vector<u64> ks(R);
    {
        u64 t = 1;
        for (u64 j = 0; j < R; j++) { ks[j] = t; t = gl_mul(t, 7); }
    }
    gl_ext2 zn = fi.zeta;
    for (u64 i = 0; i < log_n; i++) zn = gl_ext_mul(zn, zn);
    const gl_ext2 zh = gl_ext_sub(zn, gl_ext2{1, 0});
    const gl_ext2 pi_z = public_input_poly_at(pub, n_pub, fi.zeta, zn, (u32)log_n);
    gl_ext2 z_next[NCHAL];
    for (u32 t = 0; t < NCHAL; t++) z_next[t] = zs_next[t * M];
    for (u32 t = 0; t < NCHAL; t++) {
        const gl_ext2 lhs = constraint_sum(t, fi.zeta, zn, n, (u32)R, poseidon, sha, (flags & GLP_CIRCUIT_EXT_GATE) ? pre + n_const - 1 : nullptr, h.consts.data(), ks, beta, gamma, alpha, pre,
                                           pre + n_const,
                                           wires, zs, z_next, pi_z);
        gl_ext2 tz{0, 0}, zp{1, 0};
        for (u32 cc = 0; cc < (1u << rb); cc++) {
            tz = gl_ext_add(tz, gl_ext_mul(zp, quot[t * (1u << rb) + cc]));
            zp = gl_ext_mul(zp, zn);
        }
        if (!ext_eq(lhs, gl_ext_mul(zh, tz))) return rj.fail(GLP_VR_IDENTITY);
    }
    return GLP_OK;
}

// digest of a circuit proof's STATEMENT AND COMMITMENTS: hash_no_pad(header (8) || public inputs || the four caps).  The caps bind every
// committed polynomial, so two proofs with equal digests are proofs about the same circuit, inputs and witness commitment; this is the
// leaf value of the Reduce step's aggregation tree (recursion.py).  No verification.
inline int proof_digest(const Hasher& h, const uint8_t* proof, size_t len, uint64_t* out4) {
    const u64* w = (const u64*)proof;
    const size_t nw = len / 8;
    if (nw < 8 || w[0] != PLONK_TAG || w[1] > 24 || w[4] != 3 || w[5] > 12 || w[6] > (1ull << 24)) return GLP_E_INVALID;
    const u32 log_N = (u32)(w[1] + w[4]);
    const size_t capw = (size_t)4 << (w[5] < log_N ? w[5] : log_N);
    const size_t total = 8 + (size_t)w[6] + 4 * capw;
    if (total > nw) return GLP_E_INVALID;
    std::vector<u64> buf(total);
    for (size_t i = 0; i < total; i++) buf[i] = w[i] % GL_P;
    u64 d[4];
    h.hash_or_noop(buf.data(), total, d);
    memcpy(out4, d, 32);
    return GLP_OK;
}

// ---- the batched verifiers' host side (verify.hip drives the device with it, tests/emu_verify_batch the emulation) --------------------
// what the host phase left per proof
struct ProofState {
    int pre_rc = GLP_OK;            // GLP_E_REJECT: refused before the query loop (wins outright)
    u32 pre_reason = 0, pre_query = 0xFFFFFFFFu;     // pre_query: set when the queries ran in place (fallback)
    u32 post_reason = 0;            // refused after the loop: counts only when no key was set
    u64 host_key = GLP_VB_KEY_NONE;
    int desc = -1;                  // its descriptor in the plan, -1: the queries were not recorded
    bool fallback = false;
    u32 nb = 0, L = 0;
    glp_fri_statement st;
};

// plonk = true: glp_plonk_verify_batch's arguments, else glp_fri_verify_batch's
struct BatchArgs {
    bool plonk;
    const uint8_t* const* proofs;
    const size_t* lens;
    u32 B;
    const uint64_t* cap; size_t cap_words;
    const uint64_t* pub; size_t n_public;
    u32 min_queries, min_pow_bits, min_rate_bits;
    glp_verify_verdict* verdicts;
    uint64_t* digests;
    glp_fri_statement* statements;
};

inline const char* batch_args_bad(const BatchArgs& A) {
    if (!A.proofs || !A.lens || !A.verdicts) return "null argument";
    for (u32 i = 0; i < A.B; i++)
        if (!proof_args_ok(A.proofs[i], A.lens[i])) return "a proof is null, empty or not 8-byte aligned words";
    return nullptr;
}

// the host phase of proofs [i0, i1): one ProofState each, the recorded query phases in P.  ch: a challenger that holds h's constants (reset here
// per proof); neither is copied
inline void host_phase(const BatchArgs& A, const Hasher& h, glp_challenger& ch, u32 i0, u32 i1, std::vector<ProofState>& S, VerifyPlan& P) {
    for (u32 i = i0; i < i1; i++) {
        ProofState& s = S[i];
        reset_challenger(ch);
        P.begin_proof();
        Reject rj{nullptr, 0};
        memset(&s.st, 0, sizeof(s.st));
        const size_t n_desc = P.desc.size();
        int rc;
        if (A.plonk)
            rc = plonk_verify_entry(rj, h, ch, A.proofs[i], A.lens[i], A.cap, A.cap_words, A.pub ? A.pub + (size_t)i * A.n_public : nullptr, A.n_public,
                                    A.min_queries, A.min_pow_bits, &P);
        else
            rc = fri_verify_entry(rj, h, ch, A.proofs[i], A.lens[i], A.min_queries, A.min_pow_bits, A.min_rate_bits, &s.st, &P);
        s.fallback = P.unsupported;
        if (P.recorded) {
            s.desc = (int)n_desc;
            s.nb = P.desc[n_desc].nb; s.L = P.desc[n_desc].L;
            s.host_key = P.host_key;
            if (rc == GLP_E_REJECT) s.post_reason = rj.reason;
        } else if (rc == GLP_E_REJECT) {
            s.pre_rc = rc; s.pre_reason = rj.reason; s.pre_query = rj.query;
        }
        if (A.digests) {
            uint64_t* dg = A.digests + (size_t)i * 4;
            if (proof_digest(h, A.proofs[i], A.lens[i], dg) != GLP_OK) memset(dg, 0, 32);
        }
    }
}

// verdicts from the host phase's findings and the keys the items left
inline void settle(const BatchArgs& A, const std::vector<ProofState>& S, const unsigned long long* keys, u32 i0, u32 i1, u32* n_on_device, u32* n_fallback) {
    for (u32 i = i0; i < i1; i++) {
        const ProofState& s = S[i];
        glp_verify_verdict& v = A.verdicts[i];
        v.status = GLP_OK; v.reason = GLP_VR_NONE; v.query = 0xFFFFFFFFu; v.on_device = s.desc >= 0 ? 1u : 0u;
        if (s.desc >= 0) (*n_on_device)++;
        if (s.fallback) (*n_fallback)++;
        if (s.pre_rc == GLP_E_REJECT) { v.status = GLP_E_REJECT; v.reason = s.pre_reason; v.query = s.pre_query; }
        else if (s.desc >= 0) {
            u64 key = keys[s.desc];
            if (s.host_key < key) key = s.host_key;
            if (key != GLP_VB_KEY_NONE) { v.status = GLP_E_REJECT; v.reason = glp_vkey_reason(key, s.nb, s.L); v.query = (u32)(key >> 16); }
            else if (s.post_reason) { v.status = GLP_E_REJECT; v.reason = s.post_reason; }
        }
        if (A.statements) {
            if (v.status == GLP_OK) A.statements[i] = s.st;
            else memset(&A.statements[i], 0, sizeof(glp_fri_statement));
        }
    }
}

// the Merkle items of P.by_tree and the arithmetic items as the device reads them: desc | query << 32
inline void flatten_items(const VerifyPlan& P, std::vector<u64>& items, std::vector<u32>& tree_first) {
    tree_first.clear();
    for (auto& v : P.by_tree) {
        tree_first.push_back((u32)items.size());
        for (auto& it : v) items.push_back((u64)it.desc | ((u64)it.q << 32));
    }
    tree_first.push_back((u32)items.size());
}
}  // namespace glp_verify
