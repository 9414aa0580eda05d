// tm_batch_kernels.cuh — B Tendermint "simple" Merkle trees (RFC 6962 prefixes) per call: glp_tm_merkle_root_batch and the header hashes of
// glp_header_chain_leaf_inputs (tm.hip).  Two kernels, both 1-D grids:
//   glp_tm_batch_leaf_kernel   one work-item per leaf over ALL trees: nodes[i] = SHA256(00 || leaf i), streamed block by block, any length
//   glp_tm_batch_fold_kernel   one workgroup of LANES lanes per tree (tree = blockIdx.x): level 0 pairs the leaf hashes straight from global
//                              memory, every later level folds in place in 32 * LANES bytes of LDS (01 || l || r, an odd last node promoted
//                              unchanged); lane 0 stores the 32 root bytes.  Every barrier is reached by all lanes: the level loop runs on
//                              the tree's node count, which is the same for the whole workgroup.
// A tree has at most GLP_TM_BATCH_MAX_LEAVES = 512 leaves: then level 0 leaves at most 256 nodes, one per lane, and LDS holds one level.  The
// host launches LANES = 64 (one wave, 2 KiB) when no tree of the call has more than 128 leaves — a header's 14 fields, a validator set of
// up to 128 — and 256 (8 KiB) otherwise: a small tree does not pay for barriers across three idle waves.
// Where the leaves lie: either two arrays (leaf_off [total + 1] byte offsets, tree_first [B + 1] leaf indices — checked by the host before the
// launch) or the UNIFORM form, in which every tree has uni_leaves (<= 16) leaves at fixed offsets uni_pre[] inside records of uni_stride bytes
// (the 14 field encodings of a header): no array is read.  The per-item functions are GL_HD and run unchanged in the host forms.
#pragma once
#include "hash_kernels.cuh"

#define GLP_TM_BATCH_MAX_LEAVES 512
#define GLP_TM_BATCH_LANES 256
#define GLP_TM_BATCH_LANES_SMALL 64
#define GLP_TM_UNIFORM_MAX 16

struct GlpTmBatchArgs {
    const uint8_t* data;
    const u64* leaf_off;        // nullptr in the uniform form
    const u64* tree_first;      // nullptr in the uniform form
    u64 n_trees, total_leaves;
    u32* nodes;                 // [total_leaves][8] leaf hashes, big-endian words
    uint8_t* roots;             // [n_trees][32]
    const u32* k256;
    u32 uni_leaves, uni_stride;
    u32 uni_pre[GLP_TM_UNIFORM_MAX + 1];
};

GL_HD void glp_sha256_iv(u32 (&h)[8]) {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

// h = SHA256(00 || p[0 .. len)), block by block
GL_HD void glp_tm_leaf_hash(const uint8_t* __restrict__ p, u64 len, u32 (&h)[8], const u32* __restrict__ k256) {
    const u64 total = len + 1;                             // with the 0x00 prefix
    const u64 nblk = (total + 9 + 63) / 64;
    glp_sha256_iv(h);
    for (u64 b = 0; b < nblk; b++) {
        u32 m[16];
        for (int wd = 0; wd < 16; wd++) {
            u32 v = 0;
            for (int k = 0; k < 4; k++) {
                const u64 pos = b * 64 + wd * 4 + k;       // byte position in the padded message
                u32 byte = 0;
                if (pos == 0) byte = 0x00;
                else if (pos < total) byte = p[pos - 1];
                else if (pos == total) byte = 0x80;
                else if (pos >= nblk * 64 - 8) { const u64 bits = total * 8; byte = (u32)(bits >> (8 * (nblk * 64 - 1 - pos))) & 0xff; }
                v = (v << 8) | byte;
            }
            m[wd] = v;
        }
        glp_sha256_compress_words(h, m, k256);
    }
}

// h = SHA256(01 || d[0..8) || d[8..16)), the words big-endian: a 65-byte message, two blocks
GL_HD void glp_tm_inner_hash(const u32 (&d)[16], u32 (&h)[8], const u32* __restrict__ k256) {
    u32 m[16];
    glp_sha256_iv(h);
    m[0] = (0x01u << 24) | (d[0] >> 8);
    #pragma unroll
    for (int k = 1; k < 16; k++) m[k] = (d[k - 1] << 24) | (d[k] >> 8);
    glp_sha256_compress_words(h, m, k256);
    #pragma unroll
    for (int k = 0; k < 16; k++) m[k] = 0;
    m[0] = (d[15] << 24) | (0x80u << 16);
    m[15] = 520;
    glp_sha256_compress_words(h, m, k256);
}

// SHA256(""): the root of a tree without leaves, as glp_tm_merkle_root_var has it
GL_HD void glp_tm_empty_root(u32 (&h)[8]) {
    h[0] = 0xe3b0c442u; h[1] = 0x98fc1c14u; h[2] = 0x9afbf4c8u; h[3] = 0x996fb924u;
    h[4] = 0x27ae41e4u; h[5] = 0x649b934cu; h[6] = 0xa495991bu; h[7] = 0x7852b855u;
}

GL_HD void glp_tm_store_root(uint8_t* __restrict__ out, const u32 (&h)[8]) {
    for (int k = 0; k < 8; k++) {
        out[4 * k] = (uint8_t)(h[k] >> 24); out[4 * k + 1] = (uint8_t)(h[k] >> 16); out[4 * k + 2] = (uint8_t)(h[k] >> 8); out[4 * k + 3] = (uint8_t)h[k];
    }
}

// the bytes of leaf i (over all trees): [*lo, *hi) of a.data
GL_HD void glp_tm_batch_leaf_span(const GlpTmBatchArgs& a, u64 i, u64& lo, u64& hi) {
    if (a.leaf_off) { lo = a.leaf_off[i]; hi = a.leaf_off[i + 1]; return; }
    const u64 t = i / a.uni_leaves;
    const u32 j = (u32)(i % a.uni_leaves);
    lo = t * a.uni_stride + a.uni_pre[j];
    hi = t * a.uni_stride + a.uni_pre[j + 1];
}
// the leaves of tree t: [*first, *first + *cnt)
GL_HD void glp_tm_batch_tree_span(const GlpTmBatchArgs& a, u64 t, u64& first, u64& cnt) {
    if (a.tree_first) { first = a.tree_first[t]; cnt = a.tree_first[t + 1] - first; return; }
    first = t * a.uni_leaves;
    cnt = a.uni_leaves;
}

GL_HD void glp_tm_batch_leaf_item(const GlpTmBatchArgs& a, u64 i) {
    u64 lo, hi;
    glp_tm_batch_leaf_span(a, i, lo, hi);
    u32 h[8];
    glp_tm_leaf_hash(a.data + lo, hi - lo, h, a.k256);
    for (int k = 0; k < 8; k++) a.nodes[i * 8 + k] = h[k];
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_tm_batch_leaf_kernel(const GlpTmBatchArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total_leaves) return;
    glp_tm_batch_leaf_item(a, i);
}

// node j of a level of cnt nodes from its children (2j, 2j + 1) read through `get(node, word)`: hashed, or promoted when 2j + 1 == cnt
template <class Get>
GL_HD void glp_tm_fold_node(u64 j, u64 cnt, Get&& get, u32 (&h)[8], const u32* __restrict__ k256) {
    if (2 * j + 1 >= cnt) {
        for (int k = 0; k < 8; k++) h[k] = get(2 * j, k);
        return;
    }
    u32 d[16];
    for (int k = 0; k < 8; k++) { d[k] = get(2 * j, k); d[8 + k] = get(2 * j + 1, k); }
    glp_tm_inner_hash(d, h, k256);
}

template <int LANES>
__global__ void __launch_bounds__(LANES) glp_tm_batch_fold_kernel(const GlpTmBatchArgs a) {
    __shared__ u32 lvl[8 * LANES];                         // word k of node j at lvl[k * LANES + j]: lanes read and write consecutive banks
    const u64 t = blockIdx.x;
    const u32 tid = threadIdx.x;
    u64 first, cnt;
    glp_tm_batch_tree_span(a, t, first, cnt);              // the same for every lane of the workgroup
    uint8_t* root = a.roots + t * 32;
    u32 h[8];
    if (cnt <= 1) {                                        // no fold, no barrier: the whole workgroup leaves here
        if (tid == 0) {
            if (cnt == 0) glp_tm_empty_root(h);
            else for (int k = 0; k < 8; k++) h[k] = a.nodes[first * 8 + k];
            glp_tm_store_root(root, h);
        }
        return;
    }
    const u32* src = a.nodes + first * 8;
    u64 n_out = (cnt + 1) / 2;                             // <= LANES: the host launches LANES >= (largest tree + 1) / 2
    if (tid < n_out) {
        glp_tm_fold_node(tid, cnt, [&](u64 node, int k) { return src[node * 8 + k]; }, h, a.k256);
        for (int k = 0; k < 8; k++) lvl[k * LANES + tid] = h[k];
    }
    __syncthreads();
    cnt = n_out;
    while (cnt > 1) {
        n_out = (cnt + 1) / 2;
        const bool act = tid < n_out;
        if (act) glp_tm_fold_node(tid, cnt, [&](u64 node, int k) { return lvl[k * LANES + node]; }, h, a.k256);
        __syncthreads();                                   // every read of this level is done before any node of the next is stored over it
        if (act)
            for (int k = 0; k < 8; k++) lvl[k * LANES + tid] = h[k];
        __syncthreads();
        cnt = n_out;
    }
    if (tid == 0) {
        for (int k = 0; k < 8; k++) h[k] = lvl[k * LANES];
        glp_tm_store_root(root, h);
    }
}

// ---- what the host checks before a launch, and the host form --------------------------------------------------------------------------------
// 0 = the arrays are sound; 1 = not (GLP_E_INVALID); 2 = a tree has more than max_tree leaves (GLP_E_UNSUPPORTED)
static inline int glp_tm_batch_check(const u64* leaf_off, const u64* tree_first, u64 total_leaves, u64 n_trees, u64 data_len,
                                     u64 max_tree = GLP_TM_BATCH_MAX_LEAVES) {
    if (tree_first[0] != 0 || tree_first[n_trees] != total_leaves) return 1;
    for (u64 t = 0; t < n_trees; t++)
        if (tree_first[t] > tree_first[t + 1]) return 1;
    if (leaf_off[total_leaves] > data_len) return 1;
    for (u64 i = 0; i < total_leaves; i++)
        if (leaf_off[i] > leaf_off[i + 1]) return 1;
    for (u64 t = 0; t < n_trees; t++)
        if (tree_first[t + 1] - tree_first[t] > max_tree) return 2;
    return 0;
}

static inline u64 glp_tm_batch_max_tree(const u64* tree_first, u64 n_trees) {
    u64 m = 0;
    for (u64 t = 0; t < n_trees; t++) m = tree_first[t + 1] - tree_first[t] > m ? tree_first[t + 1] - tree_first[t] : m;
    return m;
}

// The launches of a call, written once for the driver (tm.hip, l = GlpLaunch, device pointers in a) and the CPU emulation (l = GlpEmuLaunch,
// host pointers): the leaves, then the fold over a.n_trees (> 0) trees none of which has more than max_tree leaves.
template <class L> static inline void glp_tm_batch_launches(L& l, const GlpTmBatchArgs& a, u64 max_tree) {
    if (a.total_leaves) l.launch(glp_tm_batch_leaf_kernel<0>, (a.total_leaves + 255) / 256, 256, a);
    if (max_tree <= 2 * GLP_TM_BATCH_LANES_SMALL) l.launch_sync(glp_tm_batch_fold_kernel<GLP_TM_BATCH_LANES_SMALL>, a.n_trees, GLP_TM_BATCH_LANES_SMALL, a);
    else l.launch_sync(glp_tm_batch_fold_kernel<GLP_TM_BATCH_LANES>, a.n_trees, GLP_TM_BATCH_LANES, a);
}

// tree t of `a` serially, with the functions the kernels call; scratch: 8 * (the tree's leaves) words
static inline void glp_tm_batch_tree_host(const GlpTmBatchArgs& a, u64 t, u32* scratch) {
    u64 first, cnt;
    glp_tm_batch_tree_span(a, t, first, cnt);
    u32 h[8];
    if (cnt == 0) { glp_tm_empty_root(h); glp_tm_store_root(a.roots + t * 32, h); return; }
    for (u64 i = 0; i < cnt; i++) {
        u64 lo, hi;
        glp_tm_batch_leaf_span(a, first + i, lo, hi);
        glp_tm_leaf_hash(a.data + lo, hi - lo, h, a.k256);
        for (int k = 0; k < 8; k++) scratch[i * 8 + k] = h[k];
    }
    while (cnt > 1) {
        const u64 n_out = (cnt + 1) / 2;
        for (u64 j = 0; j < n_out; j++) {                  // node j is stored over node j: its children 2j, 2j + 1 >= j are read first
            glp_tm_fold_node(j, cnt, [&](u64 node, int k) { return scratch[node * 8 + k]; }, h, a.k256);
            for (int k = 0; k < 8; k++) scratch[j * 8 + k] = h[k];
        }
        cnt = n_out;
    }
    for (int k = 0; k < 8; k++) h[k] = scratch[k];
    glp_tm_store_root(a.roots + t * 32, h);
}
