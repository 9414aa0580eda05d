// tests/cpp/host_chain_leaves.cpp — the MAP step of the header-chain MapReduce from a compiled host (g++, C ABI only: no hipcc, no Python): the
// raw bytes of n headers (each the concatenation of its 14 field encodings) and ONE exported leaf recording
// (recursion.WitnessProgram.export_raw of data_commitment_mr.HeaderChainMapReduce's leaf) go
//     glp_header_chain_leaf_inputs   the headers' bytes -> header hashes, link / height / data-field tests, [n / B][n_inputs] input rows on the
//                                    device (at most 4 launches, 1 synchronise)
//     glp_tm_merkle_root_batch       the same n header hashes once more as n trees of 14 leaves given by offsets: they must equal d_hashes
//     glp_witness_plan_create / glp_witness_eval_device     the rows, where they lie -> a slab of witnesses
//     glp_witness_layout_create / glp_witness_place_batch   slab rows -> wire matrices + their public values
//     glp_plonk_prove_batch          one prover call for the leaves
// and each proof must be accepted by glp_plonk_verify_ex for the recording's key and ITS public values.  Nothing of a header is computed on the
// host.  Prints the counts, the statuses, the end hash, the public values per leaf and OK; proof i goes to <out prefix><i>.bin.  The Reduce is
// not done here.
// chain file: u32 field_len[14], leaf_headers, n_groups, n; u64 first_height; start hash [32]; headers [n][sum of field_len]
// usage: host_chain_leaves <poseidon consts: 384 u64> <queries> <pow bits> <recording dir> <chain file> <out prefix>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "glprover.h"

static glp_ctx* ctx = nullptr;
#define CHECK(x) do { int rc__ = (x); if (rc__ != GLP_OK) { std::printf("FAIL %s -> %d: %s\n", #x, rc__, ctx ? glp_last_error(ctx) : ""); std::exit(1); } } while (0)

template <class T>
static std::vector<T> load(const std::string& dir, const std::string& name, size_t n) {
    std::vector<T> v(n);
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
    if (n && !f.read((char*)v.data(), (std::streamsize)(n * sizeof(T)))) { std::printf("FAIL: cannot read %s/%s\n", dir.c_str(), name.c_str()); std::exit(1); }
    return v;
}
template <class T>
static std::vector<T> take(std::ifstream& f, size_t n) {
    std::vector<T> v(n);
    if (n && !f.read((char*)v.data(), (std::streamsize)(n * sizeof(T)))) { std::printf("FAIL: the chain file is short\n"); std::exit(1); }
    return v;
}
template <class T>
static T* to_device(const std::vector<T>& v) {
    T* d = nullptr;
    CHECK(glp_alloc(ctx, (void**)&d, v.size() * sizeof(T) + 8));
    if (!v.empty()) CHECK(glp_h2d(ctx, d, v.data(), v.size() * sizeof(T)));
    return d;
}

int main(int argc, char** argv) {
    if (argc != 7) { std::printf("usage: host_chain_leaves <consts> <queries> <pow bits> <recording dir> <chain file> <out prefix>\n"); return 2; }
    std::vector<uint64_t> PC(384);
    { std::ifstream f(argv[1], std::ios::binary); if (!f.read((char*)PC.data(), 384 * 8)) { std::printf("FAIL: constants\n"); return 1; } }
    const uint32_t NQ = (uint32_t)std::atoi(argv[2]), PW = (uint32_t)std::atoi(argv[3]);
    const std::string dir = argv[4];
    std::map<std::string, uint64_t> meta, sizes;
    {
        std::ifstream f(dir + "/manifest.txt");
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream ss(line);
            std::string k;
            ss >> k;
            if (k == "array") { std::string name; uint64_t cnt; ss >> name >> cnt; sizes[name] = cnt; }
            else { uint64_t v; ss >> v; meta[k] = v; }
        }
    }
    const uint32_t log_n = (uint32_t)meta["log_n"], W = (uint32_t)meta["n_wires"], R = (uint32_t)meta["n_routed"], n_pub = (uint32_t)meta["n_public"];
    const size_t n = (size_t)1 << log_n, n_values = meta["n_values"], n_inputs = meta["n_inputs"], cells = (size_t)W * n;
    auto consts = load<uint64_t>(dir, "consts", sizes["consts"]);
    auto sigma = load<uint64_t>(dir, "sigma", sizes["sigma"]);
    auto cell = load<uint32_t>(dir, "cell_index", sizes["cell_index"]);
    auto prog = load<uint64_t>(dir, "prog", sizes["prog"]);
    auto eq = load<uint64_t>(dir, "eq_pairs", sizes["eq_pairs"]);
    auto fixed = load<uint64_t>(dir, "fixed_values", sizes["fixed_values"]);
    auto pos_rows = load<uint32_t>(dir, "pos_rows", sizes["pos_rows"]);
    auto sha_rows = load<uint32_t>(dir, "sha_rows", sizes["sha_rows"]);
    auto sha_kinds = load<uint32_t>(dir, "sha_kinds", sizes["sha_kinds"]);
    auto pub_vars64 = load<uint64_t>(dir, "public_vars", sizes["public_vars"]);
    if (cell.size() != cells || sigma.size() != (size_t)R * n || consts.size() != meta["n_const"] * n || pub_vars64.size() != n_pub || sha_rows.size() != sha_kinds.size()) {
        std::printf("FAIL: manifest and arrays disagree\n");
        return 1;
    }
    // ---- the chain ----
    std::ifstream cf(argv[5], std::ios::binary);
    const auto head = take<uint32_t>(cf, 17);
    glp_header_chain_layout lay;
    uint32_t hdr_len = 0;
    for (int j = 0; j < 14; j++) { lay.field_len[j] = head[j]; hdr_len += head[j]; }
    lay.leaf_headers = head[14]; lay.n_groups = head[15];
    const uint32_t H = head[16];
    const uint64_t first_height = take<uint64_t>(cf, 1)[0];
    if (H == 0 || H > 4096 || hdr_len == 0 || hdr_len > (1u << 16) || lay.leaf_headers == 0 || H % lay.leaf_headers) { std::printf("FAIL: chain header\n"); return 1; }
    const auto start = take<uint8_t>(cf, 32), headers = take<uint8_t>(cf, (size_t)H * hdr_len);
    const uint32_t B = H / lay.leaf_headers;                       // leaves
    uint64_t row_words = 0;
    if (glp_header_chain_leaf_input_words(&lay, &row_words) != GLP_OK || row_words != n_inputs) {
        std::printf("FAIL: the layout's rows have %llu words, the recording takes %llu inputs\n", (unsigned long long)row_words, (unsigned long long)n_inputs);
        return 1;
    }

    // ---- host only: the layout and the plan (no ctx yet) ----
    const size_t n_src = n_values + fixed.size();
    std::vector<uint32_t> pub_vars(n_pub);
    for (uint32_t i = 0; i < n_pub; i++) pub_vars[i] = (uint32_t)pub_vars64[i];
    char why[256];
    glp_witness_layout* layout = nullptr;
    int rc = glp_witness_layout_create(log_n, W, cell.data(), n_src, pos_rows.data(), (uint32_t)pos_rows.size(), sha_rows.data(), sha_kinds.data(),
                                       (uint32_t)sha_rows.size(), pub_vars.data(), n_pub, &layout, why, sizeof(why));
    if (rc != GLP_OK) { std::printf("FAIL glp_witness_layout_create -> %d: %s\n", rc, why); return 1; }
    glp_witness_plan* plan = nullptr;
    rc = glp_witness_plan_create(prog.data(), prog.size(), n_inputs, n_values, eq.empty() ? nullptr : eq.data(), eq.size() / 2, &plan);
    if (rc != GLP_OK) { std::printf("FAIL glp_witness_plan_create -> %d\n", rc); return 1; }

    CHECK(glp_create(&ctx, 0));
    CHECK(glp_set_poseidon_constants(ctx, PC.data(), 360, PC.data() + 360, PC.data() + 372));
    glp_circuit_shape sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.log_n = log_n; sh.n_wires = W; sh.n_routed = R; sh.n_public = n_pub; sh.rate_bits = 3; sh.cap_height = (uint32_t)meta["cap_height"]; sh.flags = (uint32_t)meta["flags"];
    glp_plonk_circuit* ck = nullptr;
    {
        uint64_t *d_consts = to_device(consts), *d_sigma = to_device(sigma);
        CHECK(glp_plonk_setup_ex(ctx, &sh, d_consts, d_sigma, &ck));
        CHECK(glp_free(ctx, d_consts));
        CHECK(glp_free(ctx, d_sigma));
    }
    size_t capw = 0;
    CHECK(glp_plonk_circuit_cap(ck, nullptr, &capw));
    std::vector<uint64_t> key(capw);
    CHECK(glp_plonk_circuit_cap(ck, key.data(), &capw));

    // ---- the input rows, on the device from the headers' bytes ----
    uint8_t* d_headers = to_device(headers);
    uint8_t *d_hashes = nullptr, *d_roots = nullptr;
    uint64_t* d_in = nullptr;
    CHECK(glp_alloc(ctx, (void**)&d_in, (size_t)B * n_inputs * 8));
    CHECK(glp_alloc(ctx, (void**)&d_hashes, (size_t)(H + 1) * 32));
    CHECK(glp_alloc(ctx, (void**)&d_roots, (size_t)H * 32));
    std::vector<int32_t> st(H, 99);
    CHECK(glp_header_chain_leaf_inputs(ctx, &lay, d_headers, start.data(), first_height, H, d_in, n_inputs, d_hashes, st.data()));
    uint32_t launches = 99, syncs = 99;
    CHECK(glp_header_chain_last_input_counts(ctx, &launches, &syncs));
    std::printf("input launches %u syncs %u\nstatus", launches, syncs);
    for (uint32_t k = 0; k < H; k++) std::printf(" %d", st[k]);
    std::printf("\n");
    if (launches > 4 || syncs != 1) { std::printf("FAIL: counts\n"); return 1; }
    for (uint32_t k = 0; k < H; k++)
        if (st[k] != GLP_HEADER_CHAIN_OK) { std::printf("FAIL: header %u is refused (%d)\n", k, st[k]); return 1; }
    std::vector<uint8_t> hashes((size_t)(H + 1) * 32);
    CHECK(glp_d2h(ctx, hashes.data(), d_hashes, hashes.size()));
    // the same hashes as H trees of 14 leaves through the offsets form: one call, one synchronise
    {
        std::vector<uint64_t> offs((size_t)H * 14 + 1, 0), firsts(H + 1, 0);
        for (uint32_t k = 0; k < H; k++) {
            firsts[k + 1] = (uint64_t)(k + 1) * 14;
            for (int j = 0; j < 14; j++) offs[(size_t)k * 14 + j + 1] = offs[(size_t)k * 14 + j] + lay.field_len[j];
        }
        std::vector<uint8_t> roots((size_t)H * 32);
        CHECK(glp_tm_merkle_root_batch(ctx, d_headers, headers.size(), offs.data(), firsts.data(), (uint64_t)H * 14, H, d_roots, roots.data()));
        CHECK(glp_tm_merkle_root_batch_last_counts(ctx, &launches, &syncs));
        std::printf("tree launches %u syncs %u\n", launches, syncs);
        if (launches != 2 || syncs != 1 || std::memcmp(roots.data(), hashes.data() + 32, roots.size()) != 0 || std::memcmp(hashes.data(), start.data(), 32) != 0) {
            std::printf("FAIL: the batched trees and the chain call disagree on the header hashes\n");
            return 1;
        }
    }
    std::printf("end_hash ");
    for (int i = 0; i < 32; i++) std::printf("%02x", hashes[(size_t)H * 32 + i]);
    std::printf("\n");

    // ---- evaluate on the device: slab [B][n_src + 3], the fixed values behind the variables of each row ----
    const size_t stride = n_src + 3, wstride = cells + 2;
    uint64_t *d_slab = nullptr, *d_wires = nullptr;
    CHECK(glp_alloc(ctx, (void**)&d_slab, B * stride * 8));
    CHECK(glp_alloc(ctx, (void**)&d_wires, B * wstride * 8));
    for (uint32_t b = 0; b < B && !fixed.empty(); b++) CHECK(glp_h2d(ctx, d_slab + b * stride + n_values, fixed.data(), fixed.size() * 8));
    std::vector<int32_t> status(B, 99);
    std::vector<uint64_t> first_bad(B, 0);
    CHECK(glp_witness_eval_device(ctx, plan, d_in, d_slab, stride, B, status.data(), first_bad.data()));
    for (uint32_t b = 0; b < B; b++)
        if (status[b] != GLP_OK) { std::printf("FAIL: leaf %u does not satisfy the circuit (%d, %llu)\n", b, status[b], (unsigned long long)first_bad[b]); return 1; }

    // ---- place and prove: leaf i <- slab row i ----
    std::vector<uint32_t> rows(B);
    for (uint32_t b = 0; b < B; b++) rows[b] = b;
    std::vector<uint64_t> pub((size_t)B * n_pub);
    CHECK(glp_witness_place_batch(ctx, layout, d_slab, stride, rows.data(), B, d_wires, wstride, pub.empty() ? nullptr : pub.data()));
    std::vector<const uint64_t*> mats(B);
    for (uint32_t b = 0; b < B; b++) mats[b] = d_wires + b * wstride;
    std::vector<uint8_t*> proofs(B, nullptr);
    std::vector<size_t> plen(B, 0);
    CHECK(glp_plonk_prove_batch(ctx, ck, mats.data(), pub.empty() ? nullptr : pub.data(), B, NQ, PW, proofs.data(), plen.data()));
    for (uint32_t i = 0; i < B; i++) {
        const uint64_t* mine = pub.data() + (size_t)i * n_pub;
        if (glp_plonk_verify_ex(ctx, proofs[i], plen[i], key.data(), key.size(), mine, n_pub, NQ, PW) != GLP_OK) {
            std::printf("FAIL: proof %u rejected: %s\n", i, glp_last_error(ctx));
            return 1;
        }
        std::ofstream f(std::string(argv[6]) + std::to_string(i) + ".bin", std::ios::binary);
        f.write((const char*)proofs[i], (std::streamsize)plen[i]);
        std::printf("public%u", i);
        for (uint32_t k = 0; k < n_pub; k++) std::printf(" %llu", (unsigned long long)mine[k]);
        std::printf("\n");
        glp_free_host(proofs[i]);
    }
    std::printf("key0 %llu\n", (unsigned long long)key[0]);
    CHECK(glp_sync(ctx));
    glp_witness_layout_destroy(layout);
    glp_witness_plan_destroy(plan);
    glp_plonk_free(ck);
    for (void* p : {(void*)d_headers, (void*)d_hashes, (void*)d_roots, (void*)d_in, (void*)d_slab, (void*)d_wires})
        CHECK(glp_free(ctx, p));
    glp_destroy(ctx);
    std::printf("OK\n");
    return 0;
}
