// merkle_plan.h — the launch plan of glp_merkle_batch (hash.hip), header-only and host-only: the product and the CPU emulation
// (tests/emu_merkle_batch) both walk the steps this function returns, so the two cannot drift.
//
// A tree of 2^log_leaves leaves is built down to its cap level of 2^cap_h nodes.  After the leaf launch every step takes the level of
// 2^in_log nodes as input:
//   level step : one launch builds the next level (2^(in_log - 1) nodes), one permutation per lane;
//   fused step : one launch of glp_merkle_subtree_kernel builds n_levels <= 9 levels.  Each workgroup owns a slice of
//                S = 2^s_log = min(2^in_log, 512) consecutive input digests; level l of slice g lands g * (S >> l) nodes into its level.
// A level is fused when it has at most 2^fuse_max_log nodes (fuse_max_log 0 = never).  Once one level qualifies every narrower one does,
// so a plan is: level steps, then fused steps down to the cap.
#pragma once
#include <stdint.h>
#include <vector>

#define GLP_MERKLE_SLICE_LOG 9u            // 512 digests in, 256 lanes: the first fused level is one permutation per lane
#ifndef GLP_MERKLE_FUSE_DEFAULT
#define GLP_MERKLE_FUSE_DEFAULT 0xFFFFFFFFu
#endif
// what GLP_MERKLE_FUSE_DEFAULT resolves to: measured, profiles/merkle_batch.json (DESIGN.md "Batched Merkle trees")
#define GLP_MERKLE_FUSE_LOG_MEASURED 15u

struct glp_merkle_step {
    uint32_t fused;      // 0 = level step, 1 = fused step
    uint32_t in_log;     // the input level has 2^in_log nodes per tree
    uint32_t s_log;      // fused: slice of 2^s_log input digests per workgroup
    uint32_t n_levels;   // levels this launch builds (1 for a level step)
};

// first word of the level of 2^lvl_log nodes inside one tree's digest block (layout of glp_merkle: leaf digests first)
static inline uint64_t glp_merkle_level_offset(uint32_t log_leaves, uint32_t lvl_log) {
    return 4ull * ((2ull << log_leaves) - (2ull << lvl_log));
}
// workgroups (of 256 lanes) per tree of a step; the grid is B times this
static inline uint64_t glp_merkle_step_blocks(const glp_merkle_step& s) {
    if (s.fused) return 1ull << (s.in_log - s.s_log);
    return ((1ull << (s.in_log - 1)) + 255) / 256;
}

// the shape rules of glp_merkle_batch, shared with the emulation: nullptr when the shape is acceptable, otherwise what is wrong with it.
// The footprint of one tree's leaves is computed in 128 bits, so a product that would wrap 64 bits is refused and not compared.
static inline const char* glp_merkle_batch_check(uint64_t src_tree_stride, int poly_major, uint64_t poly_stride, uint32_t leaf_len,
                                                 uint32_t log_leaves, uint32_t cap_h, uint64_t digest_tree_stride) {
    if (log_leaves > 40 || cap_h > log_leaves || leaf_len == 0) return "bad argument";
    const uint64_t nl = 1ull << log_leaves;
    if (digest_tree_stride < 4 * ((2ull << log_leaves) - (1ull << cap_h))) return "digest_tree_stride < one tree's digests";
    if (poly_major && poly_stride < nl) return "poly_stride < leaves";
    // [leaf_len][poly_stride] rows of which the last needs only its first 2^log_leaves words, or dense leaf rows
    const unsigned __int128 footprint = poly_major ? (unsigned __int128)(leaf_len - 1) * poly_stride + nl : (unsigned __int128)nl * leaf_len;
    if (footprint >> 64) return "one tree's leaves exceed 2^64 words";
    if (src_tree_stride < (uint64_t)footprint) return "src_tree_stride < one tree's leaves";
    return nullptr;
}

// the steps after the leaf launch.  log_leaves <= 40 and cap_h <= log_leaves are the caller's to check.
static inline void glp_merkle_plan_steps(uint32_t log_leaves, uint32_t cap_h, uint32_t fuse_max_log, std::vector<glp_merkle_step>& steps) {
    if (fuse_max_log == GLP_MERKLE_FUSE_DEFAULT) fuse_max_log = GLP_MERKLE_FUSE_LOG_MEASURED;
    steps.clear();
    uint32_t lvl = log_leaves;
    while (lvl > cap_h) {
        if (fuse_max_log && lvl - 1 <= fuse_max_log) {
            const uint32_t s_log = lvl < GLP_MERKLE_SLICE_LOG ? lvl : GLP_MERKLE_SLICE_LOG;
            const uint32_t n = lvl - cap_h < s_log ? lvl - cap_h : s_log;
            steps.push_back({1u, lvl, s_log, n});
            lvl -= n;
        } else {
            steps.push_back({0u, lvl, 0u, 1u});
            lvl -= 1;
        }
    }
}
