// tests/emu_tm_proofs/emu_tm_proofs.cpp — TEST INFRASTRUCTURE.  The kernels of glp_tm_forest_create, glp_tm_forest_proofs and
// glp_tm_verify_inclusion_batch (csrc/tm_proof_kernels.cuh) on the CPU, unchanged, with the checks and the plan the driver uses (csrc/tm.hip)
// and through the driver's own launch sequences (glp_tm_forest_create_launches, glp_tm_path_launch, glp_tm_verify_launch of that header),
// issued by GlpEmuLaunch of ../emu/hip_emu.h: the top kernel with real threads and barriers, the kernels without a barrier with their
// work-items one after the other.  This file only sets up buffers and fills the argument structs with host pointers.
// The host forms are exported beside them.  Never part of the product.  With -DGLP_EMU_TM_PROOFS_MAIN the
// file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that runs a corpus of forests, paths and tampered
// proofs through both forms, every buffer a heap block of exactly its length, against a separate byte-wise SHA-256 and the RECURSIVE tree.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/tm_proof_kernels.cuh"

// glp_tm_forest_create + glp_tm_forest_proofs: 0, -1 (GLP_E_INVALID) or -5 (GLP_E_UNSUPPORTED); nothing is written on a refusal.  roots may be
// NULL; launches[0] = launches of create, launches[1] = of proofs (may be NULL)
extern "C" int emu_tm_forest_proofs(const uint8_t* data, u64 data_len, const u64* offs, const u64* tree_first, u64 total, u64 n_trees, const u32* k256,
                                    const u64* query_tree, const u64* query_leaf, u64 n_queries, uint8_t* roots, uint8_t* aunts, u32 aunt_stride,
                                    u32* n_aunts, uint8_t* leaf_hashes, u32* launches) {
    if (launches) launches[0] = launches[1] = 0;
    if (n_trees == 0) return n_queries || total ? -1 : 0;
    const int bad = glp_tm_forest_check(offs, tree_first, total, n_trees, data_len);
    if (bad) return bad == 1 ? -1 : -5;
    GlpTmForestPlan plan;
    glp_tm_forest_plan(tree_first, n_trees, plan);
    if (glp_tm_forest_check_queries(tree_first, n_trees, plan.max_aunts, query_tree, query_leaf, n_queries, aunt_stride)) return -1;
    std::vector<u32> slab((size_t)plan.total_nodes * 8);                // exact size: ASan sees any overrun
    std::vector<uint8_t> own_roots;
    if (!roots) { own_roots.resize((size_t)n_trees * 32); roots = own_roots.data(); }
    GlpTmForestArgs a;
    std::memset(&a, 0, sizeof(a));
    a.tree_first = tree_first; a.upper_base = plan.upper_base.data(); a.n_trees = n_trees; a.total_leaves = total; a.slab = slab.data();
    a.roots = roots; a.k256 = k256;
    GlpEmuLaunch create, proofs;
    glp_tm_forest_create_launches(create, a, glp_tm_forest_leaf_args(a, data, offs), plan, [&](size_t l) { return plan.level_pre[l].data(); });
    if (launches) launches[0] = create.n;
    if (n_queries == 0) return 0;
    GlpTmPathArgs p;
    std::memset(&p, 0, sizeof(p));
    p.f = a;
    p.query_tree = query_tree; p.query_leaf = query_leaf; p.n_queries = n_queries; p.aunts = aunts; p.n_aunts = n_aunts; p.leaf_hash = leaf_hashes;
    p.aunt_stride = aunt_stride;
    glp_tm_path_launch(proofs, p);
    if (launches) launches[1] = proofs.n;
    return 0;
}

// glp_tm_forest_proofs_host
extern "C" int emu_tm_forest_proofs_host(const uint8_t* data, u64 data_len, const u64* offs, const u64* tree_first, u64 total, u64 n_trees,
                                         const u32* k256, const u64* query_tree, const u64* query_leaf, u64 n_queries, uint8_t* roots, uint8_t* aunts,
                                         u32 aunt_stride, u32* n_aunts, uint8_t* leaf_hashes, u32* launches) {
    if (launches) launches[0] = launches[1] = 0;
    const int bad = glp_tm_forest_proofs_host_impl(data, data_len, offs, tree_first, total, n_trees, query_tree, query_leaf, n_queries, roots, aunts,
                                                   aunt_stride, n_aunts, leaf_hashes, k256);
    return bad == 0 ? 0 : bad == 1 ? -1 : -5;
}

// glp_tm_verify_inclusion_batch: 0 or -1
extern "C" int emu_tm_verify(const uint8_t* roots, u64 n_roots, const u32* root_of, const uint8_t* data, u64 data_len, const u64* offs, const u64* index,
                             const u64* total, const uint8_t* aunts, u32 aunt_stride, const u32* n_aunts, u64 n, const u32* k256, int32_t* status) {
    if (n == 0) return 0;
    if (glp_tm_verify_check(offs, n, data_len, root_of, n_roots)) return -1;
    GlpTmVerifyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.roots = roots; a.root_of = root_of; a.data = data; a.leaf_off = offs; a.index = index; a.total = total; a.aunts = aunts; a.n_aunts = n_aunts;
    a.n = n; a.status = status; a.k256 = k256; a.aunt_stride = aunt_stride;
    GlpEmuLaunch l;
    glp_tm_verify_launch(l, a);
    return 0;
}

// glp_tm_verify_inclusion_batch_host
extern "C" int emu_tm_verify_host(const uint8_t* roots, u64 n_roots, const u32* root_of, const uint8_t* data, u64 data_len, const u64* offs,
                                  const u64* index, const u64* total, const uint8_t* aunts, u32 aunt_stride, const u32* n_aunts, u64 n, const u32* k256,
                                  int32_t* status) {
    return glp_tm_verify_inclusion_host_impl(roots, n_roots, root_of, data, data_len, offs, index, total, aunts, aunt_stride, n_aunts, n, status, k256)
               ? -1 : 0;
}

#ifdef GLP_EMU_TM_PROOFS_MAIN
#include <algorithm>
#include <cstdio>
#include <map>
// ---- a separate reference: SHA-256 over a padded byte buffer, the RFC 6962 tree, its PATH and Tendermint's computeHashFromAunts by recursion ----
typedef std::vector<uint8_t> Bytes;
static u32 KREF[64];
static void make_k() {       // the first 32 bits of the fractional parts of the cube roots of the first 64 primes, by integer bisection
    int p = 2;
    for (int i = 0; i < 64; p++) {
        bool prime = true;
        for (int d = 2; d * d <= p; d++) if (p % d == 0) prime = false;
        if (!prime) continue;
        unsigned __int128 lo = 0, hi = (unsigned __int128)1 << 36;      // the largest x with x^3 <= p * 2^96: x = cbrt(p) * 2^32 < 2^36
        while (hi - lo > 1) {
            const unsigned __int128 mid = (lo + hi) / 2;
            if (mid * mid * mid <= ((unsigned __int128)p << 96)) lo = mid; else hi = mid;
        }
        KREF[i++] = (u32)lo;
    }
}
static u32 rotr(u32 x, int r) { return (x >> r) | (x << (32 - r)); }
static Bytes sha256(const Bytes& msg) {
    Bytes m = msg;
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    const u64 bits = (u64)msg.size() * 8;
    for (int i = 7; i >= 0; i--) m.push_back((uint8_t)(bits >> (8 * i)));
    u32 h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    for (size_t b = 0; b < m.size(); b += 64) {
        u32 w[64];
        for (int i = 0; i < 16; i++) w[i] = ((u32)m[b + 4 * i] << 24) | ((u32)m[b + 4 * i + 1] << 16) | ((u32)m[b + 4 * i + 2] << 8) | m[b + 4 * i + 3];
        for (int i = 16; i < 64; i++)
            w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        u32 s[8];
        for (int i = 0; i < 8; i++) s[i] = h[i];
        for (int i = 0; i < 64; i++) {
            const u32 t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + KREF[i] + w[i];
            const u32 t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
            for (int j = 7; j > 0; j--) s[j] = s[j - 1];
            s[4] += t1;
            s[0] = t1 + t2;
        }
        for (int i = 0; i < 8; i++) h[i] += s[i];
    }
    Bytes out;
    for (int i = 0; i < 8; i++) for (int j = 3; j >= 0; j--) out.push_back((uint8_t)(h[i] >> (8 * j)));
    return out;
}
static Bytes leaf_hash(const Bytes& x) { Bytes m(1, 0); m.insert(m.end(), x.begin(), x.end()); return sha256(m); }
static Bytes inner_hash(const Bytes& l, const Bytes& r) { Bytes m(1, 1); m.insert(m.end(), l.begin(), l.end()); m.insert(m.end(), r.begin(), r.end()); return sha256(m); }
static size_t split(size_t n) { size_t k = 1; while (2 * k < n) k *= 2; return k; }
static std::map<std::pair<size_t, size_t>, Bytes> tree_memo;       // of the forest under test: cleared by check_forest
static Bytes tree(const std::vector<Bytes>& xs, size_t lo, size_t hi) {
    if (hi == lo) return sha256(Bytes());
    if (hi - lo == 1) return leaf_hash(xs[lo]);
    const auto key = std::make_pair(lo, hi);
    const auto it = tree_memo.find(key);
    if (it != tree_memo.end()) return it->second;
    const size_t k = split(hi - lo);
    return tree_memo[key] = inner_hash(tree(xs, lo, lo + k), tree(xs, lo + k, hi));
}
// RFC 6962 PATH(m, D[lo:hi)), reordered bottom-up: the deeper subtree's path first, then the sibling subtree's root
static void path(const std::vector<Bytes>& xs, size_t lo, size_t hi, size_t m, std::vector<Bytes>& out) {
    if (hi - lo <= 1) return;
    const size_t k = split(hi - lo);
    if (m < k) { path(xs, lo, lo + k, m, out); out.push_back(tree(xs, lo + k, hi)); }
    else { path(xs, lo + k, hi, m - k, out); out.push_back(tree(xs, lo, lo + k)); }
}
// computeHashFromAunts, recalled: false = refused
static bool from_aunts(u64 index, u64 total, const Bytes& lh, const std::vector<Bytes>& aunts, size_t n, Bytes& out) {
    if (index >= total || total == 0) return false;
    if (total == 1) { if (n != 0) return false; out = lh; return true; }
    if (n == 0) return false;
    u64 k = 1;
    while (2 * k < total) k *= 2;
    Bytes sub;
    if (index < k) { if (!from_aunts(index, k, lh, aunts, n - 1, sub)) return false; out = inner_hash(sub, aunts[n - 1]); }
    else { if (!from_aunts(index - k, total - k, lh, aunts, n - 1, sub)) return false; out = inner_hash(aunts[n - 1], sub); }
    return true;
}
static int ref_status(const Bytes& root, const Bytes& leaf, u64 index, u64 total, const std::vector<Bytes>& aunts, u64 n_aunts, u32 stride) {
    if (n_aunts > stride || n_aunts > aunts.size()) return GLP_TM_INC_BAD_SHAPE;
    Bytes got;
    if (!from_aunts(index, total, leaf_hash(leaf), aunts, (size_t)n_aunts, got)) return GLP_TM_INC_BAD_SHAPE;
    return got == root ? GLP_TM_INC_OK : GLP_TM_INC_BAD_ROOT;
}
static u64 next_word(u64& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    u64 z = st ^ (st >> 29);
    z *= 0xBF58476D1CE4E5B9ull;
    return z ^ (z >> 32);
}
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

typedef int (*ProofsFn)(const uint8_t*, u64, const u64*, const u64*, u64, u64, const u32*, const u64*, const u64*, u64, uint8_t*, uint8_t*, u32, u32*,
                        uint8_t*, u32*);
typedef int (*VerifyFn)(const uint8_t*, u64, const u32*, const uint8_t*, u64, const u64*, const u64*, const u64*, const uint8_t*, u32, const u32*, u64,
                        const u32*, int32_t*);

// one forest of the given leaf counts; leaf i has lens[i % lens.size()] bytes, its first bytes spell i (pairwise distinct leaves); paths of every
// leaf (trees <= 130) or of the first, last, middle and split-point leaves, through both forms; then a tampered copy of every proof through both
// verifiers against the recursive verdict
static int check_forest(const std::vector<u64>& counts, const std::vector<u64>& lens, u64& st) {
    tree_memo.clear();
    std::vector<Bytes> leaves;
    std::vector<u64> first(1, 0), offs(1, 0);
    Bytes data;
    for (u64 c : counts) {
        for (u64 i = 0; i < c; i++) {
            Bytes x(lens[leaves.size() % lens.size()]);
            for (auto& b : x) b = (uint8_t)next_word(st);
            for (size_t k = 0; k < 3 && k < x.size(); k++) x[k] = (uint8_t)(leaves.size() >> (8 * k));
            data.insert(data.end(), x.begin(), x.end());
            offs.push_back(data.size());
            leaves.push_back(x);
        }
        first.push_back(leaves.size());
    }
    std::vector<u64> qt, ql;
    u32 stride = 0;
    for (size_t t = 0; t < counts.size(); t++) {
        const u64 n = counts[t];
        std::vector<u64> which;
        if (n <= 130) for (u64 i = 0; i < n; i++) which.push_back(i);
        else { const u64 k = split(n); which = {0, n - 1, n / 2, k - 1, k}; }
        for (u64 i : which) { qt.push_back(t); ql.push_back(i); }
        if (!which.empty()) stride = std::max(stride, glp_tm_ceil_log2(n));
    }
    stride += 1;                                                        // one slot more than any row needs: it must come back zero
    const u64 nq = qt.size();
    Bytes exact(data);
    exact.shrink_to_fit();
    const ProofsFn forms[2] = {emu_tm_forest_proofs, emu_tm_forest_proofs_host};
    Bytes aunts0, roots0;
    std::vector<u32> na0;
    for (int form = 0; form < 2; form++) {
        Bytes roots(counts.size() * 32, 0xEE), aunts((size_t)nq * stride * 32, 0xEE), lh((size_t)nq * 32, 0xEE);
        std::vector<u32> na(nq, 0xEEEEEEEEu);
        REQUIRE(forms[form](exact.data(), exact.size(), offs.data(), first.data(), leaves.size(), counts.size(), KREF, qt.data(), ql.data(), nq,
                            roots.data(), aunts.data(), stride, na.data(), lh.data(), nullptr) == 0);
        for (size_t t = 0; t < counts.size(); t++) {
            const Bytes want = tree(leaves, first[t], first[t + 1]);
            REQUIRE(std::memcmp(want.data(), roots.data() + 32 * t, 32) == 0);
        }
        for (u64 q = 0; q < nq; q++) {
            std::vector<Bytes> want;
            path(leaves, first[qt[q]], first[qt[q] + 1], ql[q], want);
            REQUIRE(na[q] == want.size());
            for (size_t k = 0; k < stride; k++) {
                const Bytes w = k < want.size() ? want[k] : Bytes(32, 0);
                REQUIRE(std::memcmp(w.data(), aunts.data() + ((size_t)q * stride + k) * 32, 32) == 0);
            }
            const Bytes l = leaf_hash(leaves[first[qt[q]] + ql[q]]);
            REQUIRE(std::memcmp(l.data(), lh.data() + 32 * q, 32) == 0);
        }
        if (form == 0) { aunts0 = aunts; roots0 = roots; na0 = na; }
        else REQUIRE(aunts == aunts0 && roots == roots0 && na == na0);
    }
    if (nq == 0) return 0;
    // ---- verification: proof q as it is, then one tamper chosen by q % 10 ----
    std::vector<u64> index, total, voffs(1, 0);
    std::vector<u32> vna, root_of;
    Bytes vdata, vaunts;
    std::vector<int> want;
    for (int pass = 0; pass < 2; pass++)
        for (u64 q = 0; q < nq; q++) {
            const u64 t = qt[q], n = counts[t];
            Bytes leaf = leaves[first[t] + ql[q]];
            u64 idx = ql[q], tot = n, cnt = na0[q];
            Bytes row(aunts0.begin() + (size_t)q * stride * 32, aunts0.begin() + (size_t)(q + 1) * stride * 32);
            u32 ro = (u32)t;
            if (pass == 1) switch (q % 10) {
                case 0: if (cnt) row[(next_word(st) % cnt) * 32 + 7] ^= 0x04; else leaf.push_back(1); break;
                case 1: if (leaf.empty()) leaf.push_back(0); else leaf[next_word(st) % leaf.size()] ^= 0x80; break;
                case 2: ro = (u32)((t + 1) % counts.size()); break;                                     // another tree's root (the same one when B = 1)
                case 3: idx ^= 1; break;                                                                // may reach total: then BAD_SHAPE
                case 4: tot += 1; break;
                case 5: tot -= 1; break;
                case 6: cnt += 1; break;
                case 7: cnt = cnt ? cnt - 1 : stride + 1; break;
                case 8: idx = tot + (next_word(st) % 3); break;
                case 9: tot = 0; break;
            }
            std::vector<Bytes> as;
            for (u32 k = 0; k < stride; k++) as.push_back(Bytes(row.begin() + k * 32, row.begin() + (k + 1) * 32));
            want.push_back(ref_status(Bytes(roots0.begin() + 32 * ro, roots0.begin() + 32 * ro + 32), leaf, idx, tot, as, cnt, stride));
            index.push_back(idx); total.push_back(tot); vna.push_back((u32)cnt); root_of.push_back(ro);
            vdata.insert(vdata.end(), leaf.begin(), leaf.end());
            voffs.push_back(vdata.size());
            vaunts.insert(vaunts.end(), row.begin(), row.end());
        }
    vdata.shrink_to_fit();
    vaunts.shrink_to_fit();
    const VerifyFn vforms[2] = {emu_tm_verify, emu_tm_verify_host};
    for (int form = 0; form < 2; form++) {
        std::vector<int32_t> status(want.size(), -1);
        REQUIRE(vforms[form](roots0.data(), counts.size(), root_of.data(), vdata.data(), vdata.size(), voffs.data(), index.data(), total.data(),
                             vaunts.data(), stride, vna.data(), want.size(), KREF, status.data()) == 0);
        for (size_t p = 0; p < want.size(); p++) {
            if (status[p] != want[p]) std::printf("proof %zu (query %zu, tamper %d): status %d, reference %d\n", p, p % nq, p < nq ? -1 : (int)(p % nq % 10), status[p], want[p]);
            REQUIRE(status[p] == want[p]);
            if (p < nq) REQUIRE(status[p] == GLP_TM_INC_OK);
        }
    }
    return 0;
}

int main() {
    make_k();
    REQUIRE(KREF[0] == 0x428a2f98u && KREF[63] == 0xc67178f2u);
    u64 st = 20261021;
    const std::vector<u64> counts = {0, 1, 2, 3, 5, 7, 8, 9, 14, 100, 127, 128, 129, 511, 512, 513, 1024, 1025, 4096};
    const std::vector<u64> lens = {0, 1, 54, 55, 56, 118, 119, 120, 300};
    for (u64 c : counts)
        if (check_forest({c}, c > 600 ? std::vector<u64>{40, 55} : lens, st)) return 1;
    for (u64 len : lens)
        if (check_forest({3}, {len}, st)) return 1;
    for (u64 B : {2, 65, 130}) {
        std::vector<u64> mix;
        for (u64 t = 0; t < B; t++) mix.push_back(B == 2 ? (t ? 5 : 129) : counts[(t * 5 + 1) % (B == 130 ? 9 : 13)]);
        if (check_forest(mix, lens, st)) return 1;
    }
    if (check_forest({2, 1025, 0, 7}, {40, 1, 55}, st)) return 1;      // a wide tree beside small ones: the small ones sit the level launches out
    // ---- refusals: nothing is written ----
    {
        Bytes data(10, 1), roots(64, 0xEE), aunts(4 * 2 * 32, 0xEE);
        std::vector<u32> na(4, 0xEEEEEEEEu);
        u64 bad_offs[4] = {0, 4, 2, 10}, first[3] = {0, 1, 3}, ok_offs[4] = {0, 2, 4, 10}, short_first[3] = {0, 1, 2};
        u64 qt[2] = {0, 1}, ql[2] = {0, 1}, ql_bad[2] = {0, 2}, qt_bad[2] = {0, 2}, ql_one[2] = {1, 1};
        for (ProofsFn fn : {(ProofsFn)emu_tm_forest_proofs, (ProofsFn)emu_tm_forest_proofs_host}) {
            REQUIRE(fn(data.data(), 10, bad_offs, first, 3, 2, KREF, qt, ql, 2, roots.data(), aunts.data(), 2, na.data(), nullptr, nullptr) == -1);
            REQUIRE(fn(data.data(), 10, ok_offs, short_first, 3, 2, KREF, qt, ql, 2, roots.data(), aunts.data(), 2, na.data(), nullptr, nullptr) == -1);
            REQUIRE(fn(data.data(), 9, ok_offs, first, 3, 2, KREF, qt, ql, 2, roots.data(), aunts.data(), 2, na.data(), nullptr, nullptr) == -1);
            REQUIRE(fn(data.data(), 10, ok_offs, first, 3, 2, KREF, qt, ql_bad, 2, roots.data(), aunts.data(), 2, na.data(), nullptr, nullptr) == -1);
            REQUIRE(fn(data.data(), 10, ok_offs, first, 3, 2, KREF, qt_bad, ql, 2, roots.data(), aunts.data(), 2, na.data(), nullptr, nullptr) == -1);
            REQUIRE(fn(data.data(), 10, ok_offs, first, 3, 2, KREF, qt, ql_one, 2, roots.data(), aunts.data(), 2, na.data(), nullptr, nullptr) == -1);   // tree 0 has one leaf
            REQUIRE(fn(data.data(), 10, ok_offs, first, 3, 2, KREF, qt, ql, 2, roots.data(), aunts.data(), 0, na.data(), nullptr, nullptr) == -1);      // stride 0 < 1
            REQUIRE(fn(data.data(), 10, ok_offs, first, 3, 2, KREF, nullptr, nullptr, 2, roots.data(), aunts.data(), 2, na.data(), nullptr, nullptr) == -1);
            for (auto b : roots) REQUIRE(b == 0xEE);
            for (auto b : aunts) REQUIRE(b == 0xEE);
            for (auto v : na) REQUIRE(v == 0xEEEEEEEEu);
            REQUIRE(fn(data.data(), 10, ok_offs, first, 3, 2, KREF, nullptr, nullptr, 3, nullptr, aunts.data(), 2, na.data(), nullptr, nullptr) == 0);
            REQUIRE(na[0] == 0 && na[1] == 1 && na[2] == 1);
            std::fill(aunts.begin(), aunts.end(), 0xEE);
            std::fill(na.begin(), na.end(), 0xEEEEEEEEu);
        }
    }
    std::printf("emu_tm_proofs_san ok\n");
    return 0;
}
#endif
