// tests/emu_verify_batch/emu_verify_batch.cpp — TEST INFRASTRUCTURE.  The batched verifier (glp_plonk_verify_batch / glp_fri_verify_batch) on
// the CPU: the host phase of csrc/verify_plan.h as the driver (csrc/verify.hip) runs it, then the two kernels of csrc/verify_batch_kernels.cuh,
// unchanged, through ../emu/hip_emu.h with the driver's grids (64 lanes, ceil(items / 64) workgroups, the staging block laid out as the driver
// lays it out, in a heap block of exactly its size) and the driver's settling of the verdicts.  The kernels have no barrier: the work-items run
// one after the other.  Never part of the product.
// With -DGLP_EMU_VERIFY_BATCH_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that reads
// a corpus file (tests/test_emu_verify_batch.py writes it: the golden proofs with every tamper and truncation) and runs it through the
// emulation and through the single verifier, comparing the verdicts.
#include "../emu/hip_emu.h"
#include <memory>
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/verify_batch_kernels.cuh"

using namespace glp_verify;

namespace {
// csrc/verify.hip::device_phase with the copies replaced by one exact-size heap block
void emu_device_phase(const VerifyPlan& P, const std::vector<const u64*>& words, const Hasher& h, std::vector<unsigned long long>& keys, u32* counts) {
    const size_t nd = P.desc.size();
    keys.assign(nd, GLP_VB_KEY_NONE);
    if (nd == 0 || P.arith.empty()) return;
    std::vector<u64> items;
    std::vector<u32> tree_first;
    flatten_items(P, items, tree_first);
    const size_t n_merkle = items.size(), n_arith = P.arith.size();
    for (auto& it : P.arith) items.push_back((u64)it.desc | ((u64)it.q << 32));
    const size_t w_desc = nd * (sizeof(GlpVerifyDesc) / 8), w_aux = P.aux.size(), w_items = items.size(), w_tree = (tree_first.size() + 1) / 2, w_keys = nd;
    const size_t o_aux = w_desc, o_items = o_aux + w_aux, o_tree = o_items + w_items, o_keys = o_tree + w_tree, o_slab = o_keys + w_keys;
    const size_t total = o_slab + P.slab_words;
    std::unique_ptr<u64[]> up(new u64[total]);                   // exact size: ASan sees any read past the staging block
    memset(up.get(), 0, total * 8);
    memcpy(up.get(), P.desc.data(), w_desc * 8);
    if (w_aux) memcpy(up.get() + o_aux, P.aux.data(), w_aux * 8);
    memcpy(up.get() + o_items, items.data(), w_items * 8);
    memcpy(up.get() + o_tree, tree_first.data(), tree_first.size() * 4);
    for (size_t k = 0; k < nd; k++) up[o_keys + k] = GLP_VB_KEY_NONE;
    for (size_t k = 0; k < nd; k++) {
        const size_t used = (k + 1 < nd ? P.desc[k + 1].base : P.slab_words) - P.desc[k].base;
        memcpy(up.get() + o_slab + P.desc[k].base, words[k], used * 8);
    }
    GlpVerifyArgs a;
    memset(&a, 0, sizeof(a));
    a.desc = reinterpret_cast<const GlpVerifyDesc*>(up.get());
    a.aux = up.get() + o_aux; a.items = up.get() + o_items; a.tree_first = reinterpret_cast<const u32*>(up.get() + o_tree);
    a.keys = reinterpret_cast<unsigned long long*>(up.get() + o_keys); a.slab = up.get() + o_slab;
    a.n_trees = (u32)P.by_tree.size(); a.n_items = n_merkle;
    a.k = h.k();
    if (n_merkle) {
        const unsigned g = (unsigned)((n_merkle + GLP_VB_BLOCK - 1) / GLP_VB_BLOCK);
        if (h.small_mds) glp_emu_launch_seq(g, GLP_VB_BLOCK, [&] { glp_verify_merkle_kernel<true>(a); });
        else glp_emu_launch_seq(g, GLP_VB_BLOCK, [&] { glp_verify_merkle_kernel<false>(a); });
        counts[0]++;
    }
    a.items = up.get() + o_items + n_merkle; a.n_items = n_arith;
    glp_emu_launch_seq((unsigned)((n_arith + GLP_VB_BLOCK - 1) / GLP_VB_BLOCK), GLP_VB_BLOCK, [&] { glp_verify_arith_kernel<0>(a); });
    counts[0]++;
    for (size_t k = 0; k < nd; k++) keys[k] = a.keys[k];
    counts[1]++;
}
}  // namespace

// plonk != 0: glp_plonk_verify_batch's arguments, else glp_fri_verify_batch's (cap .. n_public ignored).  counts[4]: launches, synchronises,
// proofs on the device, proofs verified in place.  0, or -1 for unusable constants or arguments.
extern "C" int emu_verify_batch(const u64* rc, const u64* circ, const u64* diag, int plonk, const uint8_t* const* proofs, const size_t* lens, u32 B,
                                const u64* cap, size_t cap_words, const u64* pub, size_t n_public, u32 min_queries, u32 min_pow_bits, u32 min_rate_bits,
                                glp_verify_verdict* verdicts, u64* digests, u32* counts) {
    Hasher h;
    glp_challenger ch;
    if (!make_hasher_from(rc, circ, diag, h, ch)) return -1;
    const BatchArgs A{plonk != 0, proofs, lens, B, cap, cap_words, pub, n_public, min_queries, min_pow_bits, plonk ? 1u : min_rate_bits, verdicts,
                      plonk ? digests : nullptr, nullptr};
    for (int k = 0; k < 4; k++) counts[k] = 0;
    if (B == 0) return 0;
    if (batch_args_bad(A)) return -1;
    std::vector<ProofState> S(B);
    VerifyPlan P;
    std::vector<const u64*> words;
    for (u32 i = 0; i < B; i++) {
        const size_t nd = P.desc.size();
        host_phase(A, h, ch, i, i + 1, S, P);
        if (P.desc.size() > nd) words.push_back((const u64*)proofs[i]);
    }
    std::vector<unsigned long long> keys;
    emu_device_phase(P, words, h, keys, counts);
    settle(A, S, keys.data(), 0, B, &counts[2], &counts[3]);
    return 0;
}

// the single verifier on the same bytes: status, reason and failing query as the batched verdict carries them
extern "C" int emu_verify_single(const u64* rc, const u64* circ, const u64* diag, int plonk, const uint8_t* proof, size_t len, const u64* cap,
                                 size_t cap_words, const u64* pub, size_t n_public, u32 min_queries, u32 min_pow_bits, u32 min_rate_bits,
                                 glp_verify_verdict* v) {
    Hasher h;
    glp_challenger ch;
    if (!proof_args_ok(proof, len) || !make_hasher_from(rc, circ, diag, h, ch)) return -1;
    Reject rj{nullptr, 0};
    const int r = plonk ? plonk_verify_entry(rj, h, ch, proof, len, cap, cap_words, pub, n_public, min_queries, min_pow_bits)
                        : fri_verify_entry(rj, h, ch, proof, len, min_queries, min_pow_bits, min_rate_bits, nullptr);
    v->status = r; v->reason = r == GLP_OK ? GLP_VR_NONE : rj.reason; v->query = r == GLP_OK ? 0xFFFFFFFFu : rj.query; v->on_device = 0;
    return 0;
}

#ifdef GLP_EMU_VERIFY_BATCH_MAIN
#include <cstdio>
// corpus file, u64 words: rc[360] circ[12] diag[12] | n_groups | per group: plonk, min_queries, min_pow_bits, min_rate_bits, cap_words,
// cap[cap_words], n_cases | per case: n_bytes, ceil(n_bytes / 8) words.  Every group is one batched call.
int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<u64> w;
    u64 buf[4096];
    size_t got;
    while ((got = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    std::fclose(f);
    size_t pos = 384;
    if (w.size() < 385) { std::printf("short corpus\n"); return 2; }
    const u64 n_groups = w[pos++];
    size_t n_total = 0, n_bad = 0;
    for (u64 g = 0; g < n_groups; g++) {
        const int plonk = (int)w[pos]; const u32 mq = (u32)w[pos + 1], mp = (u32)w[pos + 2], mr = (u32)w[pos + 3];
        const size_t cap_words = (size_t)w[pos + 4];
        pos += 5;
        std::vector<u64> cap(w.begin() + pos, w.begin() + pos + cap_words);
        pos += cap_words;
        const u64 n_cases = w[pos++];
        // every case in a heap block of exactly its length: ASan sees a read one word past a truncated proof
        std::vector<std::unique_ptr<u64[]>> store;
        std::vector<const uint8_t*> ptrs;
        std::vector<size_t> lens;
        for (u64 k = 0; k < n_cases; k++) {
            const size_t nbytes = (size_t)w[pos++], nw = (nbytes + 7) / 8;
            store.emplace_back(new u64[nw ? nw : 1]);
            memcpy(store.back().get(), w.data() + pos, nw * 8);
            pos += nw;
            ptrs.push_back((const uint8_t*)store.back().get());
            lens.push_back(nbytes);
        }
        std::vector<glp_verify_verdict> vb(n_cases);
        std::vector<u64> dg(4 * n_cases);
        u32 counts[4];
        if (emu_verify_batch(w.data(), w.data() + 360, w.data() + 372, plonk, ptrs.data(), lens.data(), (u32)n_cases, cap_words ? cap.data() : nullptr, cap_words,
                             nullptr, 0, mq, mp, mr, vb.data(), dg.data(), counts) != 0) { std::printf("group %llu: refused\n", (unsigned long long)g); return 1; }
        for (u64 k = 0; k < n_cases; k++) {
            glp_verify_verdict vs;
            emu_verify_single(w.data(), w.data() + 360, w.data() + 372, plonk, ptrs[k], lens[k], cap_words ? cap.data() : nullptr, cap_words, nullptr, 0, mq, mp, mr, &vs);
            n_total++;
            if (vs.status != vb[k].status || vs.reason != vb[k].reason || vs.query != vb[k].query) {
                if (n_bad++ < 10)
                    std::printf("group %llu case %llu: single (%d, %s, %u) batch (%d, %s, %u)\n", (unsigned long long)g, (unsigned long long)k, vs.status, glp_vr_text(vs.reason),
                                vs.query, vb[k].status, glp_vr_text(vb[k].reason), vb[k].query);
            }
        }
    }
    if (n_bad) { std::printf("FAILED: %zu of %zu verdicts differ\n", n_bad, n_total); return 1; }
    std::printf("emu_verify_batch_san ok: %zu cases\n", n_total);
    return 0;
}
#endif
