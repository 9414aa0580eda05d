// tests/cpp/host_place.cpp — batched witness placement from a compiled host (g++, C ABI only: no hipcc, no Python): two instances of ONE exported
// recording (recursion.WitnessProgram.export_raw) go
//     glp_witness_layout_create   the recording's placement arrays, every index checked on the host
//     glp_witness_eval_device     both input vectors -> a slab of two rows on the device (the fixed values written behind each row first)
//     glp_witness_place_batch     slab rows {1, 0} -> two wire matrices side by side + their public values: at most 4 launches, 1 synchronise
//     glp_plonk_prove_batch       one prover call for the two
// and each proof must be accepted by glp_plonk_verify_ex for the recording's key and ITS public values.  Instance i is slab row 1 - i, so a
// row mix-up shows as a proof for the wrong statement.  Prints the public values per instance and OK; proof i goes to <out prefix><i>.bin.
// usage: host_place <poseidon consts: 384 u64> <queries> <pow bits> <recording dir> <inputs: 2 * n_inputs u64> <out prefix>
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

int main(int argc, char** argv) {
    if (argc != 7) { std::printf("usage: host_place <consts> <queries> <pow bits> <recording dir> <inputs> <out prefix>\n"); return 2; }
    std::vector<uint64_t> PC(384);
    { std::ifstream f(argv[1], std::ios::binary); if (!f.read((char*)PC.data(), 384 * 8)) { std::printf("FAIL: constants\n"); return 1; } }
    const uint32_t NQ = (uint32_t)std::atoi(argv[2]), PW = (uint32_t)std::atoi(argv[3]), B = 2;
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
    std::vector<uint64_t> inputs(B * n_inputs);
    { std::ifstream f(argv[5], std::ios::binary); if (!f.read((char*)inputs.data(), (std::streamsize)(inputs.size() * 8))) { std::printf("FAIL: inputs\n"); return 1; } }

    // ---- host only: the layout and the plan (no ctx yet) ----
    const size_t n_src = n_values + fixed.size();
    std::vector<uint32_t> pub_vars(n_pub);
    for (uint32_t i = 0; i < n_pub; i++) pub_vars[i] = (uint32_t)pub_vars64[i];
    char why[256];
    glp_witness_layout* layout = nullptr;
    int rc = glp_witness_layout_create(log_n, W, cell.data(), n_src, pos_rows.data(), (uint32_t)pos_rows.size(), sha_rows.data(), sha_kinds.data(),
                                       (uint32_t)sha_rows.size(), pub_vars.data(), n_pub, &layout, why, sizeof(why));
    if (rc != GLP_OK) { std::printf("FAIL glp_witness_layout_create -> %d: %s\n", rc, why); return 1; }
    {   // a cell that names a source past the row is refused here, with a reason, not on the device
        std::vector<uint32_t> bad = cell;
        bad[cells / 2] = (uint32_t)n_src;
        glp_witness_layout* none = nullptr;
        rc = glp_witness_layout_create(log_n, W, bad.data(), n_src, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, &none, why, sizeof(why));
        if (rc != GLP_E_INVALID || none || !why[0]) { std::printf("FAIL: an out-of-range cell was not refused (%d)\n", rc); return 1; }
    }
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
        uint64_t *d_consts = nullptr, *d_sigma = nullptr;
        CHECK(glp_alloc(ctx, (void**)&d_consts, consts.size() * 8));
        CHECK(glp_alloc(ctx, (void**)&d_sigma, sigma.size() * 8));
        CHECK(glp_h2d(ctx, d_consts, consts.data(), consts.size() * 8));
        CHECK(glp_h2d(ctx, d_sigma, sigma.data(), sigma.size() * 8));
        CHECK(glp_plonk_setup_ex(ctx, &sh, d_consts, d_sigma, &ck));
        CHECK(glp_free(ctx, d_consts));
        CHECK(glp_free(ctx, d_sigma));
    }
    size_t capw = 0;
    CHECK(glp_plonk_circuit_cap(ck, nullptr, &capw));
    std::vector<uint64_t> key(capw);
    CHECK(glp_plonk_circuit_cap(ck, key.data(), &capw));

    // ---- evaluate both instances on the device: slab [B][n_src + 3], the fixed values behind the variables of each row ----
    const size_t stride = n_src + 3, wstride = cells + 2;
    uint64_t *d_in = nullptr, *d_slab = nullptr, *d_wires = nullptr;
    CHECK(glp_alloc(ctx, (void**)&d_in, inputs.size() * 8 + 8));
    CHECK(glp_alloc(ctx, (void**)&d_slab, B * stride * 8));
    CHECK(glp_alloc(ctx, (void**)&d_wires, B * wstride * 8));
    if (!inputs.empty()) CHECK(glp_h2d(ctx, d_in, inputs.data(), inputs.size() * 8));
    for (uint32_t b = 0; b < B && !fixed.empty(); b++) CHECK(glp_h2d(ctx, d_slab + b * stride + n_values, fixed.data(), fixed.size() * 8));
    int32_t status[2] = {99, 99};
    uint64_t first_bad[2] = {0, 0};
    CHECK(glp_witness_eval_device(ctx, plan, d_in, d_slab, stride, B, status, first_bad));
    for (uint32_t b = 0; b < B; b++)
        if (status[b] != GLP_OK) { std::printf("FAIL: instance %u does not satisfy the circuit (%d, %llu)\n", b, status[b], (unsigned long long)first_bad[b]); return 1; }

    // ---- place: instance i <- slab row 1 - i ----
    const uint32_t rows[2] = {1, 0};
    std::vector<uint64_t> pub((size_t)B * n_pub);
    uint32_t launches = 99, syncs = 99;
    CHECK(glp_witness_place_batch(ctx, layout, d_slab, stride, rows, 0, d_wires, wstride, nullptr));                  // B = 0: nothing
    CHECK(glp_witness_last_place_counts(ctx, &launches, &syncs));
    if (launches != 0 || syncs != 0) { std::printf("FAIL: B = 0 issued %u launches, %u synchronises\n", launches, syncs); return 1; }
    CHECK(glp_witness_place_batch(ctx, layout, d_slab, stride, rows, B, d_wires, wstride, pub.empty() ? nullptr : pub.data()));
    CHECK(glp_witness_last_place_counts(ctx, &launches, &syncs));
    std::printf("place launches %u syncs %u\n", launches, syncs);
    const uint32_t want_launches = 1 + (pos_rows.empty() ? 0 : 1) + (sha_rows.empty() ? 0 : 1) + (n_pub ? 1 : 0);
    if (launches != want_launches || launches > 4 || syncs != (n_pub ? 1u : 0u)) { std::printf("FAIL: counts (%u, %u), expected (%u, %u)\n", launches, syncs, want_launches, n_pub ? 1u : 0u); return 1; }
    if (glp_witness_place_batch(ctx, layout, d_slab, n_src - 1, rows, B, d_wires, wstride, nullptr) != GLP_E_INVALID ||
        glp_witness_place_batch(ctx, layout, d_slab, stride, rows, B, d_wires, cells - 1, nullptr) != GLP_E_INVALID) {
        std::printf("FAIL: a stride below the layout's was accepted\n");
        return 1;
    }

    // ---- one prover call for the two ----
    const uint64_t* mats[2] = {d_wires, d_wires + wstride};
    uint8_t* proofs[2] = {nullptr, nullptr};
    size_t lens[2] = {0, 0};
    CHECK(glp_plonk_prove_batch(ctx, ck, mats, pub.empty() ? nullptr : pub.data(), B, NQ, PW, proofs, lens));
    for (uint32_t i = 0; i < B; i++) {
        const uint64_t* mine = pub.data() + (size_t)i * n_pub;
        if (glp_plonk_verify_ex(ctx, proofs[i], lens[i], key.data(), key.size(), mine, n_pub, NQ, PW) != GLP_OK) {
            std::printf("FAIL: proof %u rejected: %s\n", i, glp_last_error(ctx));
            return 1;
        }
        if (n_pub) {
            const uint64_t* other = pub.data() + (size_t)(1 - i) * n_pub;
            if (std::memcmp(mine, other, (size_t)n_pub * 8) && glp_plonk_verify_ex(ctx, proofs[i], lens[i], key.data(), key.size(), other, n_pub, NQ, PW) != GLP_E_REJECT) {
                std::printf("FAIL: proof %u accepted for the other instance's statement\n", i);
                return 1;
            }
        }
        std::ofstream f(std::string(argv[6]) + std::to_string(i) + ".bin", std::ios::binary);
        f.write((const char*)proofs[i], (std::streamsize)lens[i]);
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
    CHECK(glp_free(ctx, d_in));
    CHECK(glp_free(ctx, d_slab));
    CHECK(glp_free(ctx, d_wires));
    glp_destroy(ctx);
    std::printf("OK\n");
    return 0;
}
