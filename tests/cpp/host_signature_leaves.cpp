// tests/cpp/host_signature_leaves.cpp — the MAP step of the signature MapReduce from a compiled host (g++, C ABI only: no hipcc, no Python): the
// raw bytes of n slots (keys, signatures, votes, flags, the circuit's dummy triple) and ONE exported leaf recording
// (recursion.WitnessProgram.export_raw of signature_mr's leaf) go
//     glp_ed25519_leaf_inputs     the slots' bytes -> [n][n_inputs] input rows on the device (witness kernel + input kernel: 2 launches, 1 synchronise)
//     glp_witness_plan_create / glp_witness_eval_device     the rows, where they lie -> a slab of n witnesses
//     glp_witness_layout_create / glp_witness_place_batch   slab rows -> n wire matrices + their public values
//     glp_plonk_prove_batch       one prover call for the n leaves
// and each proof must be accepted by glp_plonk_verify_ex for the recording's key and ITS public values.  Nothing of a slot is computed on the
// host.  Prints the statuses, the public values per leaf and OK; proof i goes to <out prefix><i>.bin.  The Reduce is not done here.
// slots file: u32 form, msg_len_min, msg_len_max, split_scalars, n, msg_stride; pubs [n][32]; sigs [n][64]; msgs [n][msg_stride]; u32 lens [n];
//             u8 flags [n]; dummy = pub[32] sig[64] msg[msg_len_min]
// usage: host_signature_leaves <poseidon consts: 384 u64> <queries> <pow bits> <recording dir> <slots file> <out prefix>
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
    if (n && !f.read((char*)v.data(), (std::streamsize)(n * sizeof(T)))) { std::printf("FAIL: the slots file is short\n"); std::exit(1); }
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
    if (argc != 7) { std::printf("usage: host_signature_leaves <consts> <queries> <pow bits> <recording dir> <slots file> <out prefix>\n"); return 2; }
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
    // ---- the slots ----
    std::ifstream sf(argv[5], std::ios::binary);
    const auto head = take<uint32_t>(sf, 6);
    glp_ed25519_input_layout lay;
    lay.form = head[0]; lay.msg_len_min = head[1]; lay.msg_len_max = head[2]; lay.split_scalars = head[3];
    const uint32_t B = head[4], msg_stride = head[5];
    if (B == 0 || B > 64 || msg_stride == 0 || msg_stride > 4096) { std::printf("FAIL: slots header\n"); return 1; }
    const auto pubs = take<uint8_t>(sf, (size_t)B * 32), sigs = take<uint8_t>(sf, (size_t)B * 64), msgs = take<uint8_t>(sf, (size_t)B * msg_stride);
    const auto lens = take<uint32_t>(sf, B);
    const auto flags = take<uint8_t>(sf, B), dummy = take<uint8_t>(sf, 96 + (size_t)lay.msg_len_min);
    uint64_t row_words = 0;
    if (glp_ed25519_leaf_input_words(&lay, &row_words) != GLP_OK || row_words != n_inputs) {
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

    // ---- the input rows, on the device from the slots' bytes ----
    uint8_t *d_pubs = to_device(pubs), *d_sigs = to_device(sigs), *d_msgs = to_device(msgs), *d_flags = to_device(flags), *d_dummy = to_device(dummy);
    uint32_t* d_lens = to_device(lens);
    uint64_t* d_in = nullptr;
    CHECK(glp_alloc(ctx, (void**)&d_in, (size_t)B * n_inputs * 8));
    std::vector<int32_t> st(B, 99);
    const bool plain = lay.form == GLP_ED25519_FORM_PLAIN;
    CHECK(glp_ed25519_leaf_inputs(ctx, &lay, d_pubs, d_sigs, d_msgs, msg_stride, d_lens, plain ? nullptr : d_flags, plain ? nullptr : d_dummy, B, d_in,
                                  n_inputs, st.data()));
    uint32_t launches = 99, syncs = 99;
    CHECK(glp_ed25519_last_input_counts(ctx, &launches, &syncs));
    std::printf("input launches %u syncs %u\nstatus", launches, syncs);
    for (uint32_t b = 0; b < B; b++) std::printf(" %d", st[b]);
    std::printf("\n");
    if (launches != 2 || syncs != 1) { std::printf("FAIL: counts\n"); return 1; }
    for (uint32_t b = 0; b < B; b++)
        if (st[b] != GLP_ED25519_IN_OK) { std::printf("FAIL: slot %u is refused (%d)\n", b, st[b]); return 1; }

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
    for (void* p : {(void*)d_pubs, (void*)d_sigs, (void*)d_msgs, (void*)d_flags, (void*)d_dummy, (void*)d_lens, (void*)d_in, (void*)d_slab, (void*)d_wires})
        CHECK(glp_free(ctx, p));
    glp_destroy(ctx);
    std::printf("OK\n");
    return 0;
}
