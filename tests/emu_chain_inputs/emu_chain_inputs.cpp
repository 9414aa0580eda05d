// tests/emu_chain_inputs/emu_chain_inputs.cpp — TEST INFRASTRUCTURE.  The kernels of glp_tm_merkle_root_batch (csrc/tm_batch_kernels.cuh) and
// of glp_header_chain_leaf_inputs (csrc/chain_inputs.cuh) on the CPU, unchanged, through the launch sequences the driver (csrc/tm.hip) runs
// (glp_tm_batch_launches, glp_header_chain_launches of those headers), issued by GlpEmuLaunch of ../emu/hip_emu.h: the fold kernel with real
// threads and barriers, the kernels without a barrier with their work-items one after the other.  This file only sets up buffers and fills
// the argument structs with host pointers.  The host forms are exported beside them.  Never part
// of the product.  With -DGLP_EMU_CHAIN_INPUTS_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined:
// `make sanitized`) that runs a corpus of trees and chains through both forms, every buffer a heap block of exactly its length, against a
// separate byte-wise SHA-256 and a recursive tree.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/chain_inputs.cuh"

// glp_tm_merkle_root_batch: 0, -1 (GLP_E_INVALID) or -5 (GLP_E_UNSUPPORTED); nothing is written on a refusal
extern "C" int emu_tm_root_batch(const uint8_t* data, u64 data_len, const u64* offs, const u64* tree_first, u64 total, u64 n_trees, const u32* k256,
                                 uint8_t* roots) {
    if (n_trees == 0) return 0;
    const int bad = glp_tm_batch_check(offs, tree_first, total, n_trees, data_len);
    if (bad) return bad == 1 ? -1 : -5;
    std::vector<u32> nodes((size_t)total * 8);                      // exact size: ASan sees any overrun
    GlpTmBatchArgs a;
    std::memset(&a, 0, sizeof(a));
    a.data = data; a.leaf_off = offs; a.tree_first = tree_first; a.n_trees = n_trees; a.total_leaves = total; a.nodes = nodes.data(); a.roots = roots;
    a.k256 = k256;
    GlpEmuLaunch l;
    glp_tm_batch_launches(l, a, glp_tm_batch_max_tree(tree_first, n_trees));
    return 0;
}

// glp_tm_merkle_root_batch_host
extern "C" int emu_tm_root_batch_host(const uint8_t* data, u64 data_len, const u64* offs, const u64* tree_first, u64 total, u64 n_trees,
                                      const u32* k256, uint8_t* roots) {
    if (n_trees == 0) return 0;
    const int bad = glp_tm_batch_check(offs, tree_first, total, n_trees, data_len);
    if (bad) return bad == 1 ? -1 : -5;
    GlpTmBatchArgs a;
    std::memset(&a, 0, sizeof(a));
    a.data = data; a.leaf_off = offs; a.tree_first = tree_first; a.n_trees = n_trees; a.total_leaves = total; a.roots = roots; a.k256 = k256;
    std::vector<u32> scratch(8 * GLP_TM_BATCH_MAX_LEAVES);
    for (u64 t = 0; t < n_trees; t++) glp_tm_batch_tree_host(a, t, scratch.data());
    return 0;
}

extern "C" u64 emu_chain_input_words(const u32* field_len, u32 leaf_headers, u32 n_groups) {
    const u64 per = glp_chain_words_per_header(field_len, leaf_headers, n_groups);
    return per ? GLP_CHAIN_ROW_HEAD + per * leaf_headers : 0;
}

// the launches of glp_header_chain_leaf_inputs: out [n / leaf_headers][out_stride], hashes [n + 1][32], status [n]
extern "C" int emu_chain_inputs(const u32* field_len, u32 leaf_headers, u32 n_groups, const uint8_t* headers, const uint8_t* start32, u64 first_height,
                                u64 n, const u32* k256, u64* out, u64 out_stride, uint8_t* hashes, int32_t* status) {
    const u64 width = emu_chain_input_words(field_len, leaf_headers, n_groups);
    if (!width || out_stride < width || n % leaf_headers) return -1;
    if (n == 0) return 0;
    GlpChainArgs a;
    GlpTmBatchArgs t;
    std::memset(&t, 0, sizeof(t));
    std::vector<u32> nodes((size_t)n * GLP_CHAIN_FIELDS * 8);       // exact size: ASan sees any overrun
    if (glp_header_chain_fill_args(a, t, field_len, leaf_headers, n_groups, headers, start32, first_height, n, out, out_stride, hashes, status,
                                   nodes.data(), k256)) return -1;
    GlpEmuLaunch l;
    glp_header_chain_launches(l, a, t);
    return 0;
}

// glp_header_chain_leaf_inputs_host
extern "C" int emu_chain_inputs_host(const u32* field_len, u32 leaf_headers, u32 n_groups, const uint8_t* headers, const uint8_t* start32,
                                     u64 first_height, u64 n, const u32* k256, u64* out, u64 out_stride, uint8_t* hashes, int32_t* status) {
    const u64 width = emu_chain_input_words(field_len, leaf_headers, n_groups);
    if (!width || out_stride < width || n % leaf_headers) return -1;
    if (n == 0) return 0;
    return glp_header_chain_leaf_inputs_host_impl(field_len, leaf_headers, n_groups, headers, start32, first_height, n, out, out_stride, hashes,
                                                  status, k256);
}

#ifdef GLP_EMU_CHAIN_INPUTS_MAIN
#include <cstdio>
// ---- a separate reference: SHA-256 over a padded byte buffer, the RFC 6962 tree by recursion ----
typedef std::vector<uint8_t> Bytes;
static u32 KREF[64];
static void make_k() {       // the first 32 bits of the fractional parts of the cube roots of the first 64 primes, by integer bisection
    int p = 2;
    for (int i = 0; i < 64; p++) {
        bool prime = true;
        for (int d = 2; d * d <= p; d++) if (p % d == 0) prime = false;
        if (!prime) continue;
        // the largest x with x^3 <= p * 2^96: x = cbrt(p) * 2^32
        unsigned __int128 lo = 0, hi = (unsigned __int128)1 << 36;
        const unsigned __int128 target_hi = (unsigned __int128)p;     // p * 2^96, compared through x^3 >> 96 without overflow: x < 2^36
        while (hi - lo > 1) {
            const unsigned __int128 mid = (lo + hi) / 2;
            // mid^3 < 2^108 fits 128 bits
            if (mid * mid * mid <= (target_hi << 96)) lo = mid; else hi = mid;
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
static Bytes tree(const std::vector<Bytes>& xs, size_t lo, size_t hi) {
    if (hi == lo) return sha256(Bytes());
    Bytes m;
    if (hi - lo == 1) { m.push_back(0); m.insert(m.end(), xs[lo].begin(), xs[lo].end()); return sha256(m); }
    size_t k = 1;
    while (2 * k < hi - lo) k *= 2;
    const Bytes l = tree(xs, lo, lo + k), r = tree(xs, lo + k, hi);
    m.push_back(1); m.insert(m.end(), l.begin(), l.end()); m.insert(m.end(), r.begin(), r.end());
    return sha256(m);
}
static u64 next_word(u64& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    u64 z = st ^ (st >> 29);
    z *= 0xBF58476D1CE4E5B9ull;
    return z ^ (z >> 32);
}
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// one call of both forms over trees of the given leaf counts; leaf i has lens[i % lens.size()] bytes
static int check_trees(const std::vector<u64>& counts, const std::vector<u64>& lens, u64& st) {
    std::vector<Bytes> leaves;
    std::vector<u64> first(1, 0), offs(1, 0);
    Bytes data;
    for (u64 c : counts) {
        for (u64 i = 0; i < c; i++) {
            Bytes x(lens[leaves.size() % lens.size()]);
            for (auto& b : x) b = (uint8_t)next_word(st);
            data.insert(data.end(), x.begin(), x.end());
            offs.push_back(data.size());
            leaves.push_back(x);
        }
        first.push_back(leaves.size());
    }
    Bytes exact(data);                                                // a heap block of exactly data.size() bytes
    exact.shrink_to_fit();
    Bytes r1(counts.size() * 32, 0xEE), r2(counts.size() * 32, 0xEE);
    REQUIRE(emu_tm_root_batch(exact.data(), exact.size(), offs.data(), first.data(), leaves.size(), counts.size(), KREF, r1.data()) == 0);
    REQUIRE(emu_tm_root_batch_host(exact.data(), exact.size(), offs.data(), first.data(), leaves.size(), counts.size(), KREF, r2.data()) == 0);
    for (size_t t = 0; t < counts.size(); t++) {
        const Bytes want = tree(leaves, first[t], first[t + 1]);
        REQUIRE(std::memcmp(want.data(), r1.data() + 32 * t, 32) == 0);
        REQUIRE(std::memcmp(want.data(), r2.data() + 32 * t, 32) == 0);
    }
    return 0;
}

static Bytes varint(u64 v) { Bytes o; while (v >= 0x80) { o.push_back((uint8_t)(v | 0x80)); v >>= 7; } o.push_back((uint8_t)v); return o; }

// a well-formed chain of n headers at the layout, with one optional tamper (header `at`, kind 0 none, 1 link bit, 2 link prefix, 3 height + 1,
// 4 over-long varint, 5 data prefix 0a 21, 6 a height one group too long for the layout spelled by its low groups); both forms must agree with the expectation built here
static int check_chain(const u32 (&fl)[14], u32 B, u32 g, u64 first, u64 n, int kind, u64 at, u64& st) {
    u32 hdr = 0, pre[15] = {0};
    for (int j = 0; j < 14; j++) { pre[j + 1] = pre[j] + fl[j]; }
    hdr = pre[14];
    Bytes headers((size_t)n * hdr), start(32);
    for (auto& b : start) b = (uint8_t)next_word(st);
    std::vector<Bytes> hashes(1, start);
    std::vector<int32_t> want_status(n, 0);
    for (u64 k = 0; k < n; k++) {
        uint8_t* h = headers.data() + k * hdr;
        for (u32 i = 0; i < hdr; i++) h[i] = (uint8_t)next_word(st);
        Bytes v = varint(first + k);
        if (kind == 6 && k == at) {                                   // the height has g + 1 groups: its g low ones in the layout's bytes
            REQUIRE(v.size() == g + 1);
            v.resize(g);
            v[g - 1] &= 0x7f;
            want_status[k] = GLP_CHAIN_BAD_HEIGHT;
        }
        REQUIRE(v.size() == g && fl[2] == 1 + g);
        h[pre[2]] = 0x08;
        std::memcpy(h + pre[2] + 1, v.data(), g);
        h[pre[4]] = 0x0a; h[pre[4] + 1] = 0x20;
        std::memcpy(h + pre[4] + 2, hashes[k].data(), 32);
        h[pre[6]] = 0x0a; h[pre[6] + 1] = 0x20;
        if (kind && k == at) {
            if (kind == 1) { h[pre[4] + 2 + 17] ^= 0x10; want_status[k] = GLP_CHAIN_BAD_LINK; }
            if (kind == 2) { h[pre[4] + 1] = 0x21; want_status[k] = GLP_CHAIN_BAD_LINK; }
            if (kind == 3) { const Bytes w = varint(first + k + 1); std::memcpy(h + pre[2] + 1, w.data(), g); want_status[k] = GLP_CHAIN_BAD_HEIGHT; }
            if (kind == 4) { h[pre[2] + g] |= 0x80; want_status[k] = GLP_CHAIN_BAD_HEIGHT; }
            if (kind == 5) { h[pre[6] + 1] = 0x21; want_status[k] = GLP_CHAIN_BAD_DATA_FIELD; }
        }
        std::vector<Bytes> fields;
        for (int j = 0; j < 14; j++) fields.push_back(Bytes(h + pre[j], h + pre[j + 1]));
        hashes.push_back(tree(fields, 0, 14));
        // a tampered header changes its own hash, so its successor no longer links: the chain is rebuilt on the tampered hash, as a caller
        // who serves consistent headers would, and only header `at` is refused
    }
    const u64 width = emu_chain_input_words(fl, B, g), stride = width + 2;
    REQUIRE(width != 0);
    for (int form = 0; form < 2; form++) {
        std::vector<u64> out((size_t)(n / B) * stride, 0x5E5E5E5E5E5E5E5Eull);
        Bytes hs((size_t)(n + 1) * 32, 0xEE);
        std::vector<int32_t> status(n, -1);
        Bytes exact(headers);
        exact.shrink_to_fit();
        REQUIRE((form ? emu_chain_inputs_host : emu_chain_inputs)(fl, B, g, exact.data(), start.data(), first, n, KREF, out.data(), stride, hs.data(),
                                                                 status.data()) == 0);
        for (u64 k = 0; k <= n; k++) REQUIRE(std::memcmp(hs.data() + 32 * k, hashes[k].data(), 32) == 0);
        for (u64 k = 0; k < n; k++) REQUIRE(status[k] == want_status[k]);
        for (u64 l = 0; l < n / B; l++) {
            bool ok = true;
            for (u64 k = l * B; k < (l + 1) * B; k++) ok = ok && want_status[k] == 0;
            std::vector<u64> want;
            for (int w = 0; w < 8; w++) {
                const uint8_t* s = hashes[l * B].data() + 4 * w;
                want.push_back(((u64)s[0] << 24) | ((u64)s[1] << 16) | ((u64)s[2] << 8) | s[3]);
            }
            want.push_back(first + l * B);
            for (u64 k = l * B; k < (l + 1) * B; k++) {
                const uint8_t* h = headers.data() + k * hdr;
                for (u32 j = 0; j < g; j++) want.push_back(((first + k) >> (7 * j)) & 0x7f);
                for (u32 i = 2; i < 34; i++) want.push_back(h[pre[6] + i]);
                for (u32 i = 34; i < fl[4]; i++) want.push_back(h[pre[4] + i]);
                for (int j = 0; j < 14; j++)
                    if (j != 2 && j != 4 && j != 6)
                        for (u32 i = 0; i < fl[j]; i++) want.push_back(h[pre[j] + i]);
            }
            REQUIRE(want.size() == width);
            for (u64 w = 0; w < width; w++) REQUIRE(out[l * stride + w] == (ok ? want[w] : 0));
            REQUIRE(out[l * stride + width] == 0x5E5E5E5E5E5E5E5Eull && out[l * stride + width + 1] == 0x5E5E5E5E5E5E5E5Eull);
        }
    }
    return 0;
}

int main() {
    make_k();
    REQUIRE(KREF[0] == 0x428a2f98u && KREF[63] == 0xc67178f2u);
    u64 st = 20261020;
    // ---- trees: every leaf count of the list alone, then mixed calls of 2, 65 and 130 trees; leaf lengths at the padding edges ----
    const std::vector<u64> counts = {0, 1, 2, 3, 5, 7, 8, 9, 14, 100, 127, 128, 129, GLP_TM_BATCH_MAX_LEAVES};
    const std::vector<u64> lens = {0, 1, 54, 55, 56, 118, 119, 120, 300};
    for (u64 c : counts)
        if (check_trees({c}, lens, st)) return 1;
    for (u64 len : lens)
        if (check_trees({3}, {len}, st)) return 1;
    for (u64 B : {2, 65, 130}) {                                       // 2: a 129-leaf tree beside a small one (256 lanes); 65: up to 128 leaves; 130: small trees
        std::vector<u64> mix;
        for (u64 t = 0; t < B; t++) mix.push_back(B == 2 ? (t ? 5 : 129) : counts[(t * 5 + 1) % (B == 130 ? 9 : 12)]);
        if (check_trees(mix, lens, st)) return 1;
    }
    // ---- refusals: nothing is written ----
    {
        Bytes data(10, 1), roots(64, 0xEE);
        u64 offs[4] = {0, 4, 2, 10}, first[3] = {0, 1, 3};
        REQUIRE(emu_tm_root_batch(data.data(), 10, offs, first, 3, 2, KREF, roots.data()) == -1);
        u64 ok_offs[4] = {0, 2, 4, 10}, short_first[3] = {0, 1, 2};
        REQUIRE(emu_tm_root_batch(data.data(), 10, ok_offs, short_first, 3, 2, KREF, roots.data()) == -1);
        REQUIRE(emu_tm_root_batch(data.data(), 9, ok_offs, first, 3, 2, KREF, roots.data()) == -1);
        std::vector<u64> many(GLP_TM_BATCH_MAX_LEAVES + 2, 0);
        u64 big_first[2] = {0, GLP_TM_BATCH_MAX_LEAVES + 1};
        REQUIRE(emu_tm_root_batch(data.data(), 10, many.data(), big_first, GLP_TM_BATCH_MAX_LEAVES + 1, 1, KREF, roots.data()) == -5);
        for (auto b : roots) REQUIRE(b == 0xEE);
    }
    // ---- chains: the default lengths at 1, 2 and 4 varint bytes, leaves of 1, 2 and 8 headers; every tamper on the first, a middle and the
    // last header of the second leaf (2-header leaves at 4 varint bytes, 8-header leaves at 2) ----
    const struct { u32 g; u64 first; } heights[] = {{1, 100}, {2, 128}, {2, 16383 - 23}, {4, 1ull << 21}, {4, (1ull << 28) - 24}};
    for (const auto& hg : heights)
        for (u32 B : {1u, 2u, 8u}) {
            const u32 fl[14] = {4, 12, 1 + hg.g, 13, 72, 34, 34, 34, 34, 34, 34, 34, 34, 22};
            if (check_chain(fl, B, hg.g, hg.first, 3 * B, 0, 0, st)) return 1;
            if (!((hg.first == 1ull << 21 && B == 2) || (hg.first == 128 && B == 8))) continue;
            for (int kind = 1; kind <= 5; kind++)
                for (u64 at : {(u64)B, (u64)B + B / 2, (u64)2 * B - 1})
                    if (check_chain(fl, B, hg.g, hg.first, 2 * B, kind, at, st)) return 1;
        }
    // ---- the first height that does not fit the layout, on the last header: 16384 as 08 80 00 at 2 bytes, 128 as 08 00 at 1 byte ----
    for (u32 g : {2u, 1u}) {
        const u32 fl[14] = {4, 12, 1 + g, 13, 72, 34, 34, 34, 34, 34, 34, 34, 34, 22};
        if (check_chain(fl, 2, g, (1ull << (7 * g)) - 5, 6, 6, 5, st)) return 1;
    }
    std::printf("emu_chain_inputs_san ok\n");
    return 0;
}
#endif
