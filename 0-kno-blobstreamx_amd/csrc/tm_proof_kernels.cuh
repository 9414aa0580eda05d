// tm_proof_kernels.cuh — Tendermint "simple" Merkle trees (RFC 6962 prefixes) with EVERY LEVEL KEPT, the audit paths read out of them and the
// batched check of such paths: glp_tm_forest_create / glp_tm_forest_proofs / glp_tm_verify_inclusion_batch (tm.hip).  The proof format is
// BUILD-DEFINED (a restatement from memory of Tendermint's crypto/merkle.Proof{Total, Index, LeafHash, Aunts}, unpinned): the aunts of leaf i
// are its sibling hashes bottom-up, 32 bytes each; an odd last node of a level is promoted and contributes no aunt there.
// The slab (node = 8 big-endian words):
//   [ leaf hashes of ALL leaves, in the call's leaf numbering ][ tree 0: level 1, level 2, .., its root ][ tree 1: .. ] ..
// level 0 lies apart so that glp_tm_batch_leaf_kernel (tm_batch_kernels.cuh, included unchanged) writes it as it writes its nodes; the upper
// levels of tree t begin at node total_leaves + upper_base[t].  A tree of n > 1 leaves has levels of n, ceil(n / 2), .., 1 nodes; a tree of one
// leaf has only its leaf hash (which is its root); a tree without leaves has no node, and its root SHA256("") exists in the root array only.
// Kernels, all 1-D grids:
//   glp_tm_batch_leaf_kernel     (tm_batch_kernels.cuh) one work-item per leaf over all trees
//   glp_tm_forest_level_kernel   one work-item per OUTPUT node of one level over all trees: (tree, node) by bisection in that level's prefix
//                                sums; launched while the widest tree has more than GLP_TM_FOREST_TOP_NODES nodes at the level
//   glp_tm_forest_top_kernel     one workgroup of LANES lanes per tree, from level `level` on: the first pairing reads the slab, every later one
//                                folds in 32 * LANES bytes of LDS (word k of node j at lvl[k * LANES + j]) as glp_tm_batch_fold_kernel does, and
//                                every node is ALSO stored to its place in the slab; lane 0 stores the root bytes.  The level loop runs on the
//                                tree's node count, the same for the whole workgroup, so every barrier is reached by all lanes; a tree that is
//                                already down to one node (or has none) only stores its root and leaves before the first barrier.
//   glp_tm_path_kernel           one work-item per query (tree, leaf): aunts, their count, optionally the leaf hash; unused slots zeroed
//   glp_tm_verify_kernel         one work-item per proof: hashes the leaf BYTES (the 00 prefix keeps an inner node from passing as a leaf),
//                                walks (index, total) bottom-up.  index, total and n_aunts are the proof's own untrusted words: the shape is
//                                settled from them before any aunt is read, and at most min(n_aunts, aunt_stride) aunts of the own row are read.
// The per-item functions are GL_HD and run unchanged in the host forms and the CPU emulation.
#pragma once
#include <cstring>
#include <vector>
#include "tm_batch_kernels.cuh"

#define GLP_TM_FOREST_MAX_TREE (1ull << 24)
#define GLP_TM_FOREST_TOP_NODES (2 * GLP_TM_BATCH_LANES)   // 512: after the first pairing one node per lane
#define GLP_TM_INC_OK 0
#define GLP_TM_INC_BAD_SHAPE 1
#define GLP_TM_INC_BAD_ROOT 2

struct GlpTmForestArgs {
    const u64* tree_first;      // [n_trees + 1] leaf indices
    const u64* upper_base;      // [n_trees + 1] nodes above level 0 of the trees before t
    const u64* level_pre;       // level kernel: [n_trees + 1] output nodes of this level of the trees before t
    u64 n_trees, total_leaves;
    u32* slab;
    uint8_t* roots;             // [n_trees][32]
    const u32* k256;
    u32 level;                  // level kernel: the level it reads; top kernel: the level it starts from
};

// where a level of tree t lies: nodes [at, at + n) of the slab
struct GlpTmLevel { u64 at, n, up; u32 l; };
GL_HD GlpTmLevel glp_tm_forest_leaves(const GlpTmForestArgs& a, u64 t) {
    GlpTmLevel v;
    v.at = a.tree_first[t]; v.n = a.tree_first[t + 1] - v.at; v.up = a.total_leaves + a.upper_base[t]; v.l = 0;
    return v;
}
GL_HD u64 glp_tm_level_above(const GlpTmLevel& v) { return v.l == 0 ? v.up : v.at + v.n; }
GL_HD void glp_tm_level_ascend(GlpTmLevel& v) { v.at = glp_tm_level_above(v); v.n = (v.n + 1) / 2; v.l++; }
// level `level` of tree t, or its top level when the tree has fewer
GL_HD GlpTmLevel glp_tm_forest_level(const GlpTmForestArgs& a, u64 t, u32 level) {
    GlpTmLevel v = glp_tm_forest_leaves(a, t);
    while (v.l < level && v.n > 1) glp_tm_level_ascend(v);
    return v;
}
// the largest t in [0, n) with pre[t] <= i (pre ascending, pre[0] = 0 <= i < pre[n])
GL_HD u64 glp_tm_bisect(const u64* __restrict__ pre, u64 n, u64 i) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (pre[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
GL_HD u32 glp_tm_ceil_log2(u64 n) {
    u32 d = 0;
    while (d < 64 && ((u64)1 << d) < n) d++;
    return d;
}

// output node i (over all trees) of the level above a.level
GL_HD void glp_tm_forest_level_item(const GlpTmForestArgs& a, u64 i) {
    const u64 t = glp_tm_bisect(a.level_pre, a.n_trees, i);
    const u64 j = i - a.level_pre[t];
    const GlpTmLevel v = glp_tm_forest_level(a, t, a.level);   // v.n > 1: a tree that is down to one node has no output in level_pre
    const u32* src = a.slab + v.at * 8;
    u32 h[8];
    glp_tm_fold_node(j, v.n, [&](u64 node, int k) { return src[node * 8 + k]; }, h, a.k256);
    u32* dst = a.slab + (glp_tm_level_above(v) + j) * 8;
    for (int k = 0; k < 8; k++) dst[k] = h[k];
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_tm_forest_level_kernel(const GlpTmForestArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.level_pre[a.n_trees]) return;
    glp_tm_forest_level_item(a, i);
}

template <int LANES>
__global__ void __launch_bounds__(LANES) glp_tm_forest_top_kernel(const GlpTmForestArgs a) {
    __shared__ u32 lvl[8 * LANES];                         // word k of node j at lvl[k * LANES + j]
    const u64 t = blockIdx.x;
    const u32 tid = threadIdx.x;
    GlpTmLevel v = glp_tm_forest_level(a, t, a.level);     // the same for every lane of the workgroup
    uint8_t* root = a.roots + t * 32;
    u32 h[8];
    if (v.n <= 1) {                                        // sits out: no fold, no barrier, the whole workgroup leaves here
        if (tid == 0) {
            if (v.n == 0) glp_tm_empty_root(h);
            else for (int k = 0; k < 8; k++) h[k] = a.slab[v.at * 8 + k];
            glp_tm_store_root(root, h);
        }
        return;
    }
    const u32* src = a.slab + v.at * 8;
    u64 cnt = v.n;
    u64 n_out = (cnt + 1) / 2;                             // <= LANES: the host launches LANES >= (widest level + 1) / 2
    u32* dst = a.slab + glp_tm_level_above(v) * 8;
    if (tid < n_out) {
        glp_tm_fold_node(tid, cnt, [&](u64 node, int k) { return src[node * 8 + k]; }, h, a.k256);
        for (int k = 0; k < 8; k++) { lvl[k * LANES + tid] = h[k]; dst[(u64)tid * 8 + k] = h[k]; }
    }
    __syncthreads();
    cnt = n_out;
    while (cnt > 1) {
        dst += cnt * 8;                                    // the level above the one in LDS
        n_out = (cnt + 1) / 2;
        const bool act = tid < n_out;
        if (act) glp_tm_fold_node(tid, cnt, [&](u64 node, int k) { return lvl[k * LANES + node]; }, h, a.k256);
        __syncthreads();                                   // every read of this level is done before any node of the next is stored over it
        if (act)
            for (int k = 0; k < 8; k++) { lvl[k * LANES + tid] = h[k]; dst[(u64)tid * 8 + k] = h[k]; }
        __syncthreads();
        cnt = n_out;
    }
    if (tid == 0) {
        for (int k = 0; k < 8; k++) h[k] = lvl[k * LANES];
        glp_tm_store_root(root, h);
    }
}

// ---- audit paths ----------------------------------------------------------------------------------------------------------------------------
struct GlpTmPathArgs {
    GlpTmForestArgs f;          // tree_first, upper_base, n_trees, total_leaves, slab
    const u64* query_tree;      // [n_queries]; nullptr: query q is leaf q of the numbering over all trees
    const u64* query_leaf;      // [n_queries] leaf inside its tree
    u64 n_queries;
    uint8_t* aunts;             // [n_queries][aunt_stride][32]
    u32* n_aunts;               // [n_queries]
    uint8_t* leaf_hash;         // [n_queries][32] or nullptr
    u32 aunt_stride;
};

GL_HD void glp_tm_path_item(const GlpTmPathArgs& a, u64 q) {
    u64 t, idx;
    if (a.query_tree) { t = a.query_tree[q]; idx = a.query_leaf[q]; }
    else { t = glp_tm_bisect(a.f.tree_first, a.f.n_trees, q); idx = q - a.f.tree_first[t]; }
    GlpTmLevel v = glp_tm_forest_leaves(a.f, t);           // the host checked idx < v.n and aunt_stride >= ceil(log2 v.n)
    u32 h[8];
    if (a.leaf_hash) {
        for (int k = 0; k < 8; k++) h[k] = a.f.slab[(v.at + idx) * 8 + k];
        glp_tm_store_root(a.leaf_hash + q * 32, h);
    }
    uint8_t* row = a.aunts + q * a.aunt_stride * 32;
    u32 used = 0;
    while (v.n > 1) {
        const u64 sib = idx ^ 1;
        if (sib < v.n && used < a.aunt_stride) {
            for (int k = 0; k < 8; k++) h[k] = a.f.slab[(v.at + sib) * 8 + k];
            glp_tm_store_root(row + (u64)used * 32, h);
            used++;
        }
        idx >>= 1;
        glp_tm_level_ascend(v);
    }
    a.n_aunts[q] = used;
    for (u64 b = (u64)used * 32; b < (u64)a.aunt_stride * 32; b++) row[b] = 0;
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_tm_path_kernel(const GlpTmPathArgs a) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n_queries) return;
    glp_tm_path_item(a, q);
}

// ---- batched verification -------------------------------------------------------------------------------------------------------------------
struct GlpTmVerifyArgs {
    const uint8_t* roots;       // [n_roots][32]
    const u32* root_of;         // [n] or nullptr = root 0 (checked by the host: < n_roots)
    const uint8_t* data;
    const u64* leaf_off;        // [n + 1] (checked by the host)
    const u64* index;           // [n] untrusted
    const u64* total;           // [n] untrusted
    const uint8_t* aunts;       // [n][aunt_stride][32]
    const u32* n_aunts;         // [n] untrusted
    u64 n;
    int32_t* status;            // [n]
    const u32* k256;
    u32 aunt_stride;
};

// the number of aunts the pair (index, total) fixes; index < total
GL_HD u32 glp_tm_aunt_count(u64 index, u64 total) {
    u32 c = 0;
    while (total > 1) {
        if ((index ^ 1) < total) c++;
        index >>= 1;
        total = (total + 1) / 2;
    }
    return c;
}

GL_HD int32_t glp_tm_verify_item(const GlpTmVerifyArgs& a, u64 p) {
    u64 idx = a.index[p], n = a.total[p];
    const u32 na = a.n_aunts[p];
    if (n == 0 || idx >= n || na > a.aunt_stride || na != glp_tm_aunt_count(idx, n)) return GLP_TM_INC_BAD_SHAPE;
    u32 h[8], d[16];
    glp_tm_leaf_hash(a.data + a.leaf_off[p], a.leaf_off[p + 1] - a.leaf_off[p], h, a.k256);
    const uint8_t* row = a.aunts + p * a.aunt_stride * 32;
    u32 used = 0;
    while (n > 1) {
        if ((idx ^ 1) < n) {                               // used < na: na is the count of exactly these levels
            const uint8_t* s = row + (u64)used * 32;
            const int mine = (idx & 1) ? 8 : 0, other = 8 - mine;
            for (int k = 0; k < 8; k++) {
                d[mine + k] = h[k];
                d[other + k] = ((u32)s[4 * k] << 24) | ((u32)s[4 * k + 1] << 16) | ((u32)s[4 * k + 2] << 8) | s[4 * k + 3];
            }
            glp_tm_inner_hash(d, h, a.k256);
            used++;
        }
        idx >>= 1;
        n = (n + 1) / 2;
    }
    const uint8_t* r = a.roots + (u64)(a.root_of ? a.root_of[p] : 0) * 32;
    u32 diff = 0;
    for (int k = 0; k < 8; k++) diff |= h[k] ^ (((u32)r[4 * k] << 24) | ((u32)r[4 * k + 1] << 16) | ((u32)r[4 * k + 2] << 8) | r[4 * k + 3]);
    return diff ? GLP_TM_INC_BAD_ROOT : GLP_TM_INC_OK;
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_tm_verify_kernel(const GlpTmVerifyArgs a) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    a.status[p] = glp_tm_verify_item(a, p);
}

// ---- what the host checks and plans before a launch, and the host forms ---------------------------------------------------------------------
// 0 = the arrays are sound; 1 = not (GLP_E_INVALID); 2 = a tree has more than GLP_TM_FOREST_MAX_TREE leaves (GLP_E_UNSUPPORTED)
static inline int glp_tm_forest_check(const u64* leaf_off, const u64* tree_first, u64 total_leaves, u64 n_trees, u64 data_len) {
    return glp_tm_batch_check(leaf_off, tree_first, total_leaves, n_trees, data_len, GLP_TM_FOREST_MAX_TREE);
}

struct GlpTmForestPlan {
    std::vector<u64> upper_base;             // [n_trees + 1]
    std::vector<std::vector<u64>> level_pre; // one [n_trees + 1] per level launch
    u64 max_tree = 0, total_nodes = 0;       // total_nodes: leaves and upper nodes, the slab's length
    u32 max_aunts = 0, top_level = 0, top_width = 0;   // the top kernel starts at top_level, where the widest tree has top_width <= 512 nodes
};
static inline void glp_tm_forest_plan(const u64* tree_first, u64 n_trees, GlpTmForestPlan& p) {
    p.upper_base.assign(n_trees + 1, 0);
    for (u64 t = 0; t < n_trees; t++) {
        u64 n = tree_first[t + 1] - tree_first[t], upper = 0;
        p.max_tree = n > p.max_tree ? n : p.max_tree;
        while (n > 1) { n = (n + 1) / 2; upper += n; }
        p.upper_base[t + 1] = p.upper_base[t] + upper;
    }
    p.total_nodes = tree_first[n_trees] + p.upper_base[n_trees];
    p.max_aunts = glp_tm_ceil_log2(p.max_tree);
    u64 w = p.max_tree;
    for (; w > GLP_TM_FOREST_TOP_NODES; w = (w + 1) / 2) {
        std::vector<u64> pre(n_trees + 1, 0);
        for (u64 t = 0; t < n_trees; t++) {
            u64 n = tree_first[t + 1] - tree_first[t];
            for (u32 l = 0; l < p.top_level && n > 1; l++) n = (n + 1) / 2;
            pre[t + 1] = pre[t] + (n > 1 ? (n + 1) / 2 : 0);
        }
        p.level_pre.push_back(pre);
        p.top_level++;
    }
    p.top_width = (u32)w;
}

// 0 = the queries are sound; 1 = not.  query_tree / query_leaf both nullptr: n_queries must be total_leaves (every leaf in numbering order)
static inline int glp_tm_forest_check_queries(const u64* tree_first, u64 n_trees, u32 max_aunts, const u64* query_tree, const u64* query_leaf,
                                              u64 n_queries, u32 aunt_stride) {
    if (!query_tree != !query_leaf) return 1;
    if (!query_tree) return n_queries != tree_first[n_trees] || (n_queries && aunt_stride < max_aunts);
    for (u64 q = 0; q < n_queries; q++) {
        if (query_tree[q] >= n_trees) return 1;
        const u64 n = tree_first[query_tree[q] + 1] - tree_first[query_tree[q]];
        if (query_leaf[q] >= n || aunt_stride < glp_tm_ceil_log2(n)) return 1;
    }
    return 0;
}

// 0 = sound; 1 = not
static inline int glp_tm_verify_check(const u64* leaf_off, u64 n, u64 data_len, const u32* root_of, u64 n_roots) {
    if (n_roots == 0 || leaf_off[n] > data_len) return 1;
    for (u64 p = 0; p < n; p++)
        if (leaf_off[p] > leaf_off[p + 1] || (root_of && root_of[p] >= n_roots)) return 1;
    return 0;
}

// what the leaf-hash kernel is given to fill level 0 of forest a: the slab's leaf region is its node array
static inline GlpTmBatchArgs glp_tm_forest_leaf_args(const GlpTmForestArgs& a, const uint8_t* data, const u64* leaf_off) {
    GlpTmBatchArgs b;
    memset(&b, 0, sizeof(b));
    b.data = data; b.leaf_off = leaf_off; b.tree_first = a.tree_first; b.n_trees = a.n_trees; b.total_leaves = a.total_leaves; b.nodes = a.slab;
    b.roots = a.roots; b.k256 = a.k256;
    return b;
}

// The launches of the three calls, written once for the driver (tm.hip, l = GlpLaunch, device pointers) and the CPU emulation (l = GlpEmuLaunch,
// host pointers).  A forest of a.n_trees > 0 trees: the leaves, a level launch per entry of plan.level_pre (level_pre(i): where the kernel reads it), the top.
template <class L, class Pre>
static inline void glp_tm_forest_create_launches(L& l, GlpTmForestArgs a, const GlpTmBatchArgs& leaves, const GlpTmForestPlan& plan, Pre level_pre) {
    if (a.total_leaves) l.launch(glp_tm_batch_leaf_kernel<0>, (a.total_leaves + 255) / 256, 256, leaves);
    for (size_t i = 0; i < plan.level_pre.size(); i++) {
        a.level = (u32)i;
        a.level_pre = level_pre(i);
        l.launch(glp_tm_forest_level_kernel<0>, (plan.level_pre[i][a.n_trees] + 255) / 256, 256, a);
    }
    a.level = plan.top_level;
    a.level_pre = nullptr;
    if (plan.top_width <= 2 * GLP_TM_BATCH_LANES_SMALL) l.launch_sync(glp_tm_forest_top_kernel<GLP_TM_BATCH_LANES_SMALL>, a.n_trees, GLP_TM_BATCH_LANES_SMALL, a);
    else l.launch_sync(glp_tm_forest_top_kernel<GLP_TM_BATCH_LANES>, a.n_trees, GLP_TM_BATCH_LANES, a);
}
template <class L> static inline void glp_tm_path_launch(L& l, const GlpTmPathArgs& a) { l.launch(glp_tm_path_kernel<0>, (a.n_queries + 255) / 256, 256, a); }
template <class L> static inline void glp_tm_verify_launch(L& l, const GlpTmVerifyArgs& a) { l.launch(glp_tm_verify_kernel<0>, (a.n + 255) / 256, 256, a); }

// the whole forest serially, with the functions the kernels call; slab: plan.total_nodes * 8 words
static inline void glp_tm_forest_build_host(const GlpTmBatchArgs& leaves, const GlpTmForestArgs& a) {
    for (u64 i = 0; i < a.total_leaves; i++) glp_tm_batch_leaf_item(leaves, i);
    u32 h[8];
    for (u64 t = 0; t < a.n_trees; t++) {
        GlpTmLevel v = glp_tm_forest_leaves(a, t);
        if (v.n == 0) { glp_tm_empty_root(h); glp_tm_store_root(a.roots + t * 32, h); continue; }
        while (v.n > 1) {
            const u32* src = a.slab + v.at * 8;
            u32* dst = a.slab + glp_tm_level_above(v) * 8;
            for (u64 j = 0; j < (v.n + 1) / 2; j++) {
                glp_tm_fold_node(j, v.n, [&](u64 node, int k) { return src[node * 8 + k]; }, h, a.k256);
                for (int k = 0; k < 8; k++) dst[j * 8 + k] = h[k];
            }
            glp_tm_level_ascend(v);
        }
        for (int k = 0; k < 8; k++) h[k] = a.slab[v.at * 8 + k];
        glp_tm_store_root(a.roots + t * 32, h);
    }
}

// glp_tm_forest_proofs_host: 0, 1 (GLP_E_INVALID) or 2 (GLP_E_UNSUPPORTED); nothing is written on a refusal
static inline int glp_tm_forest_proofs_host_impl(const uint8_t* data, u64 data_len, const u64* leaf_offsets, const u64* tree_first, u64 total_leaves,
                                                 u64 n_trees, const u64* query_tree, const u64* query_leaf, u64 n_queries, uint8_t* roots,
                                                 uint8_t* aunts, u32 aunt_stride, u32* n_aunts, uint8_t* leaf_hashes, const u32* k256) {
    if (n_trees == 0) return n_queries || total_leaves ? 1 : 0;
    if (!leaf_offsets || !tree_first || (!data && data_len)) return 1;
    const int bad = glp_tm_forest_check(leaf_offsets, tree_first, total_leaves, n_trees, data_len);
    if (bad) return bad;
    GlpTmForestPlan plan;
    glp_tm_forest_plan(tree_first, n_trees, plan);
    if (glp_tm_forest_check_queries(tree_first, n_trees, plan.max_aunts, query_tree, query_leaf, n_queries, aunt_stride)) return 1;
    if (n_queries && (!n_aunts || (!aunts && aunt_stride))) return 1;
    std::vector<u32> slab((size_t)plan.total_nodes * 8);
    std::vector<uint8_t> own_roots;
    if (!roots) { own_roots.resize((size_t)n_trees * 32); roots = own_roots.data(); }
    GlpTmPathArgs a;
    memset(&a, 0, sizeof(a));
    a.f.tree_first = tree_first; a.f.upper_base = plan.upper_base.data(); a.f.n_trees = n_trees; a.f.total_leaves = total_leaves;
    a.f.slab = slab.data(); a.f.roots = roots; a.f.k256 = k256;
    glp_tm_forest_build_host(glp_tm_forest_leaf_args(a.f, data, leaf_offsets), a.f);
    a.query_tree = query_tree; a.query_leaf = query_leaf; a.n_queries = n_queries; a.aunts = aunts; a.n_aunts = n_aunts; a.leaf_hash = leaf_hashes;
    a.aunt_stride = aunt_stride;
    for (u64 q = 0; q < n_queries; q++) glp_tm_path_item(a, q);
    return 0;
}

// glp_tm_verify_inclusion_batch_host: 0 or 1 (GLP_E_INVALID)
static inline int glp_tm_verify_inclusion_host_impl(const uint8_t* roots, u64 n_roots, const u32* root_of, const uint8_t* data, u64 data_len,
                                                    const u64* leaf_offsets, const u64* index, const u64* total, const uint8_t* aunts,
                                                    u32 aunt_stride, const u32* n_aunts, u64 n, int32_t* status, const u32* k256) {
    if (n == 0) return 0;
    if (!roots || !leaf_offsets || !index || !total || !n_aunts || !status || (!data && data_len) || (!aunts && aunt_stride)) return 1;
    if (glp_tm_verify_check(leaf_offsets, n, data_len, root_of, n_roots)) return 1;
    GlpTmVerifyArgs a;
    memset(&a, 0, sizeof(a));
    a.roots = roots; a.root_of = root_of; a.data = data; a.leaf_off = leaf_offsets; a.index = index; a.total = total; a.aunts = aunts;
    a.n_aunts = n_aunts; a.n = n; a.status = status; a.k256 = k256; a.aunt_stride = aunt_stride;
    for (u64 p = 0; p < n; p++) status[p] = glp_tm_verify_item(a, p);
    return 0;
}
