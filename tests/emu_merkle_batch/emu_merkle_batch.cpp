// tests/emu_merkle_batch/emu_merkle_batch.cpp — TEST INFRASTRUCTURE.  glp_merkle_batch on the CPU: the three kernels of
// csrc/merkle_batch_kernels.cuh, unchanged, launched through ../emu/hip_emu.h (every work-item a real thread, __syncthreads() a barrier, one
// workgroup after the other) in the steps of the product's own plan (csrc/merkle_plan.h) — the launches' order is the only ordering between
// the levels, as on the stream.  Never part of the product.
// With -DGLP_EMU_MERKLE_BATCH_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that checks
// the fused plans against the unfused one on small shapes.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/merkle_batch_kernels.cuh"
#include "../../0-kno-blobstreamx_amd/csrc/merkle_plan.h"
#include "../../0-kno-blobstreamx_amd/csrc/poseidon_precomp.h"

// Arguments as glp_merkle_batch, on host arrays.  consts384 = rc[360] | circ[12] | diag[12]; small != 0: fast MDS path, small == 2: also the
// grouped partial rounds.  caps (may be NULL): [B][4 << cap_h].  n_launches / n_fused (may be NULL): what was launched.
// Returns 0, or -1 for the arguments glp_merkle_batch refuses (the product's own rule: glp_merkle_batch_check).
extern "C" int emu_merkle_batch(const u64* src, u64 src_tree_stride, int poly_major, u64 poly_stride, u32 leaf_len, u32 log_leaves, u32 cap_h, u32 B,
                                u32 fuse_max_log, u64* digests, u64 digest_tree_stride, u64* caps, const u64* consts384, int small, u32* n_launches,
                                u32* n_fused) {
    if (B == 0) return 0;
    if (!src || !digests || log_leaves > 20) return -1;
    if (glp_merkle_batch_check(src_tree_stride, poly_major, poly_stride, leaf_len, log_leaves, cap_h, digest_tree_stride)) return -1;
    const u64 nl = 1ull << log_leaves;
    std::vector<u32> cf; std::vector<u64> cs;
    GlpPoseidonConsts k{consts384, consts384 + 360, consts384 + 372, nullptr, nullptr};
    if (small == 2 && glp_poseidon_group_tables(consts384, cf, cs)) { k.pg_coef = cf.data(); k.pg_cst = cs.data(); }
    std::vector<glp_merkle_step> steps;
    glp_merkle_plan_steps(log_leaves, cap_h, fuse_max_log, steps);
    const u64 stride = poly_major ? poly_stride : (u64)leaf_len;
    const u32 leaf_bpt = (u32)((nl + 255) / 256);
    auto leaves = [&](auto sm_, auto pm_) {
        constexpr bool SM = decltype(sm_)::value != 0, PM = decltype(pm_)::value != 0;
        glp_emu_launch(leaf_bpt * B, 256, 0, [&] {
            glp_hash_leaves_batch_kernel<SM, PM>(src, src_tree_stride, stride, leaf_len, nl, leaf_bpt, digests, digest_tree_stride, k);
        });
    };
    if (small) { if (poly_major) leaves(glp_ic<1>{}, glp_ic<1>{}); else leaves(glp_ic<1>{}, glp_ic<0>{}); }
    else { if (poly_major) leaves(glp_ic<0>{}, glp_ic<1>{}); else leaves(glp_ic<0>{}, glp_ic<0>{}); }
    u32 nf = 0;
    for (const glp_merkle_step& s : steps) {
        const u32 bpt = (u32)glp_merkle_step_blocks(s);
        const u64 in_off = glp_merkle_level_offset(log_leaves, s.in_log);
        if (s.fused) {
            nf++;
            if (small) glp_emu_launch(bpt * B, 256, 0, [&] { glp_merkle_subtree_kernel<true>(digests, digest_tree_stride, in_off, s.in_log, s.s_log, s.n_levels, bpt, k); });
            else glp_emu_launch(bpt * B, 256, 0, [&] { glp_merkle_subtree_kernel<false>(digests, digest_tree_stride, in_off, s.in_log, s.s_log, s.n_levels, bpt, k); });
        } else {
            const u64 count = 1ull << (s.in_log - 1);
            if (small) glp_emu_launch(bpt * B, 256, 0, [&] { glp_merkle_level_batch_kernel<true>(digests, digest_tree_stride, in_off, count, bpt, k); });
            else glp_emu_launch(bpt * B, 256, 0, [&] { glp_merkle_level_batch_kernel<false>(digests, digest_tree_stride, in_off, count, bpt, k); });
        }
    }
    if (caps)
        for (u32 b = 0; b < B; b++)
            memcpy(caps + ((size_t)b * 4 << cap_h), digests + b * digest_tree_stride + glp_merkle_level_offset(log_leaves, cap_h), (size_t)32 << cap_h);
    if (n_launches) *n_launches = 1 + (u32)steps.size();
    if (n_fused) *n_fused = nf;
    return 0;
}

#ifdef GLP_EMU_MERKLE_BATCH_MAIN
#include <cstdio>
// Self-made constants (any canonical words do for a fused-against-unfused comparison): a small-integer MDS for the fast path, 64-bit entries
// for the generic one.
static u64 next_word(u64& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    u64 z = st ^ (st >> 29);
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 32;
    return z % GL_P;
}

int main() {
    struct Shape { u32 log_leaves, cap_h, B, leaf_len; };
    // the shapes of tests/test_emu_merkle_batch.py
    const Shape shapes[] = {{0, 0, 2, 7}, {5, 5, 2, 9}, {3, 0, 3, 3}, {9, 0, 2, 8}, {10, 2, 2, 135}, {12, 0, 1, 5}, {12, 3, 1, 5}};
    int bad = 0;
    // the generic MDS path on leaf-major rows over every shape; the fast path with grouped partial rounds on polynomial-major columns over
    // the first four, which differ from it only in the permutation and the leaf addressing (an emulated fused workgroup costs seconds: 256
    // threads meeting at some 10^4 wave barriers; the two 12-level shapes are 9 and 8 of them per plan)
    for (int small = 0; small <= 2; small += 2) {
        const int pm = small ? 1 : 0;
        u64 st = 99 + small;
        std::vector<u64> c384(384);
        for (int i = 0; i < 360; i++) c384[i] = next_word(st);
        for (int i = 360; i < 384; i++) c384[i] = small ? 1 + next_word(st) % 40 : next_word(st);
        for (const Shape& sh : shapes) {
            if (small && sh.log_leaves > 9) continue;
            const u64 nl = 1ull << sh.log_leaves, tree = 4 * ((2ull << sh.log_leaves) - (1ull << sh.cap_h));
            const u64 dstride = tree + 5, pstride = nl + 3, sstride = (u64)sh.leaf_len * pstride + 7;
            const u64 fill = 0x5e5e5e5e5e5e5e5eull;
            std::vector<u64> src(sstride * sh.B);
            for (u64& w : src) w = next_word(st);
            std::vector<u64> ref(dstride * sh.B, fill), cap_ref((size_t)sh.B * 4 << sh.cap_h);
            if (emu_merkle_batch(src.data(), sstride, pm, pstride, sh.leaf_len, sh.log_leaves, sh.cap_h, sh.B, 0, ref.data(), dstride, cap_ref.data(),
                                 c384.data(), small, nullptr, nullptr)) { printf("unfused run refused\n"); return 2; }
            for (u32 b = 0; b < sh.B; b++)
                for (u64 w = tree; w < dstride; w++)
                    if (ref[b * dstride + w] != fill) { printf("gap overwritten (unfused) tree %u\n", b); bad++; }
            std::vector<glp_merkle_step> unfused, done, plan;
            glp_merkle_plan_steps(sh.log_leaves, sh.cap_h, 0, unfused);
            const u32 fuses[] = {sh.log_leaves, GLP_MERKLE_FUSE_DEFAULT};
            for (u32 f : fuses) {
                glp_merkle_plan_steps(sh.log_leaves, sh.cap_h, f, plan);
                auto same = [](const std::vector<glp_merkle_step>& a, const std::vector<glp_merkle_step>& b) {
                    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(glp_merkle_step)));
                };
                if (same(plan, unfused) || same(plan, done)) continue;      // a plan already run
                done = plan;
                std::vector<u64> got(dstride * sh.B, fill), cap((size_t)sh.B * 4 << sh.cap_h);
                u32 nlaunch = 0, nfused = 0;
                if (emu_merkle_batch(src.data(), sstride, pm, pstride, sh.leaf_len, sh.log_leaves, sh.cap_h, sh.B, f, got.data(), dstride, cap.data(),
                                     c384.data(), small, &nlaunch, &nfused)) { printf("fused run refused\n"); return 2; }
                if (got != ref || cap != cap_ref) {
                    u64 w = 0;
                    while (w < got.size() && got[w] == ref[w]) w++;
                    printf("DIFF small=%d pm=%d log_leaves=%u cap_h=%u B=%u leaf_len=%u fuse=%u first word %llu\n", small, pm, sh.log_leaves, sh.cap_h, sh.B,
                           sh.leaf_len, f, (unsigned long long)w);
                    bad++;
                }
                if (nfused == 0) { printf("no fused launch at fuse=%u\n", f); bad++; }
            }
        }
    }
    printf(bad ? "emu_merkle_batch_san: %d differences\n" : "emu_merkle_batch_san: fused == unfused on every shape\n", bad);
    return bad ? 1 : 0;
}
#endif
