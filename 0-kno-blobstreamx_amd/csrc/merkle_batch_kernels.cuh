// merkle_batch_kernels.cuh — B Poseidon Merkle trees of one shape per launch (glp_merkle_batch, hash.hip; plan: merkle_plan.h).
// 1-D grids throughout: a launch has B * blocks_per_tree workgroups of 256 lanes and the tree index is blockIdx.x / blocks_per_tree.
// Tree b reads its leaves at src + b * src_tree_stride and owns the digest block at digests + b * digest_tree_stride, laid out as
// glp_merkle lays it out (leaf digests, then every level down to the cap).  The permutations are those of hash_kernels.cuh, unchanged.
//
// Plain HIP C++ without AMD builtins: tests/emu_merkle_batch runs these bodies on the CPU.
#pragma once
#include "hash_kernels.cuh"

// glp_hash_leaves_kernel over B trees (same leaf rules: leaf_len <= 4 is the zero-padded leaf, otherwise the overwrite-mode sponge)
template <bool SMALL, bool POLY_MAJOR>
__global__ void __launch_bounds__(256) glp_hash_leaves_batch_kernel(const u64* __restrict__ src, u64 src_tree_stride, u64 stride, u32 leaf_len,
                                                                    u64 n_leaves, u32 blocks_per_tree, u64* __restrict__ digests,
                                                                    u64 digest_tree_stride, GlpPoseidonConsts k) {
    const u32 b = blockIdx.x / blocks_per_tree;
    const u64 i = (u64)(blockIdx.x - b * blocks_per_tree) * 256 + threadIdx.x;
    if (i >= n_leaves) return;
    const u64* __restrict__ tsrc = src + (u64)b * src_tree_stride;
    u64* __restrict__ out = digests + (u64)b * digest_tree_stride;
    auto at = [&](u32 j) -> u64 { return POLY_MAJOR ? tsrc[(u64)j * stride + i] : tsrc[i * stride + j]; };
    u64 s[12];
    glp_hfor<0, 12>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = 0; });
    if (leaf_len <= 4) {
        glp_hfor<0, 4>([&](auto j_) { constexpr int j = decltype(j_)::value; if ((u32)j < leaf_len) s[j] = at(j); });
    } else {
        u32 off = 0;
        for (; off + GLP_POS_RATE <= leaf_len; off += GLP_POS_RATE) {
            glp_hfor<0, 8>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = at(off + j); });
            glp_poseidon_permute<SMALL>(s, k);
        }
        if (off < leaf_len) {
            glp_hfor<0, 8>([&](auto j_) { constexpr int j = decltype(j_)::value; if (off + j < leaf_len) s[j] = at(off + j); });
            glp_poseidon_permute<SMALL>(s, k);
        }
    }
    glp_hfor<0, 4>([&](auto j_) { constexpr int j = decltype(j_)::value; out[i * 4 + j] = s[j]; });
}

// one level of B trees, one permutation per lane (the wide levels): the level of 2 * count nodes at word in_off of every tree's digest
// block -> the `count` nodes right after it
template <bool SMALL>
__global__ void __launch_bounds__(256) glp_merkle_level_batch_kernel(u64* __restrict__ digests, u64 digest_tree_stride, u64 in_off, u64 count,
                                                                     u32 blocks_per_tree, GlpPoseidonConsts k) {
    const u32 b = blockIdx.x / blocks_per_tree;
    const u64 i = (u64)(blockIdx.x - b * blocks_per_tree) * 256 + threadIdx.x;
    if (i >= count) return;
    const u64* prev = digests + (u64)b * digest_tree_stride + in_off;
    u64* cur = digests + (u64)b * digest_tree_stride + in_off + 8 * count;
    u64 s[12];
    glp_hfor<0, 8>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = prev[i * 8 + j]; });
    glp_hfor<8, 12>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = 0; });
    glp_poseidon_permute<SMALL>(s, k);
    glp_hfor<0, 4>([&](auto j_) { constexpr int j = decltype(j_)::value; cur[i * 4 + j] = s[j]; });
}

// n_levels <= s_log <= 9 levels of B trees in one launch.  Workgroup (b, g) owns slice g of S = 2^s_log consecutive digests of the level
// of 2^in_log nodes (at word in_off of tree b's block) and everything above that slice: level l (1-based) of the slice has S >> l nodes and
// is stored g * (S >> l) nodes into its level, where glp_merkle keeps it.  The first level is read from memory, every later one from LDS
// (two buffers in turn: level l writes buf[l & 1] while it reads buf[(l - 1) & 1]).
// A level of >= 64 nodes per slice runs one permutation per lane: the lanes beyond the level idle in whole waves.  Below that the
// dependency chain of one permutation is all there is to wait for, and it is spread over 16 lanes (glp_poseidon_permute_coop: a quarter of
// the chain at four times the instructions, a good trade once three of four waves would idle): 16 nodes per pass of the 256 lanes.  At 64
// nodes four passes cost what one per-lane permutation costs, hence the switch below 64.
// Every lane of a wave that calls the lane-cooperative permutation calls it (only whole waves sit a pass out: a wave holds 4 nodes), and
// every __syncthreads() is reached by all 256 lanes: no lane returns before the last level.
#define GLP_SUBTREE_COOP_BELOW 64u
template <bool SMALL>
__global__ void __launch_bounds__(256) glp_merkle_subtree_kernel(u64* __restrict__ digests, u64 digest_tree_stride, u64 in_off, u32 in_log,
                                                                 u32 s_log, u32 n_levels, u32 slices_per_tree, GlpPoseidonConsts k) {
    __shared__ u64 buf[2][256 * 4];                  // 2 x 8 KiB: the widest level kept is the first one, 256 nodes
    const u32 b = blockIdx.x / slices_per_tree, g = blockIdx.x - b * slices_per_tree;
    const u32 tid = threadIdx.x, r = tid & 15u, lane_base = (tid & 63u) & ~15u, wave_node = (tid >> 6) << 2;
    u64* tree = digests + (u64)b * digest_tree_stride;
    const u64* in = tree + in_off + ((u64)g << (s_log + 2));
    u64 lvl_off = in_off, lvl_cnt = 1ull << in_log;
    for (u32 l = 1; l <= n_levels; l++) {
        const u32 cnt = 1u << (s_log - l);           // nodes of this slice at this level
        lvl_off += 4 * lvl_cnt;
        lvl_cnt >>= 1;
        u64* out = tree + lvl_off + (u64)g * cnt * 4;
        const u64* from = l == 1 ? in : buf[(l - 1) & 1];
        u64* keep = buf[l & 1];
        if (cnt >= GLP_SUBTREE_COOP_BELOW) {
            if (tid < cnt) {
                u64 s[12];
                glp_hfor<0, 8>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = from[tid * 8 + j]; });
                glp_hfor<8, 12>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = 0; });
                glp_poseidon_permute<SMALL>(s, k);
                glp_hfor<0, 4>([&](auto j_) { constexpr int j = decltype(j_)::value; out[tid * 4 + j] = s[j]; keep[tid * 4 + j] = s[j]; });
            }
        } else {
            for (u32 base = 0; base < cnt; base += 16) {
                const u32 node = base + (tid >> 4);
                const bool active = node < cnt;
                u64 x = 0;
                if (active && r < 8u) x = from[node * 8 + r];
                if (base + wave_node < cnt) x = glp_poseidon_permute_coop<SMALL>(x, r, lane_base, k);      // wave-uniform
                if (active && r < 4u) { out[node * 4 + r] = x; keep[node * 4 + r] = x; }
            }
        }
        __syncthreads();
    }
}
