// chain_inputs.cuh — the header-chain leaf's INPUT VECTORS on the device (glp_header_chain_leaf_inputs, tm.hip): from the raw headers of a
// chain (each the concatenation of its 14 field encodings at the layout's lengths) to the rows glp_witness_eval_device reads, word for word
// what data_commitment_mr._chain_leaf_inputs builds, after the tests of data_commitment_mr.HeaderChainMapReduce._map_chain.  After the header
// hashes (tm_batch_kernels.cuh, uniform form: n trees of 14 leaves) two kernels:
//   glp_header_chain_check_kernel   one work-item per header k: field 4 begins 0a 20 || hash of the predecessor (the start hash for k = 0),
//                                   field 2 is 08 || varint(first_height + k) in exactly n_groups bytes, field 6 begins 0a 20 -> status[k]
//   glp_header_chain_rows_kernel    one wave per header (header = blockIdx.x): its slice of its leaf's row, consecutive lanes storing
//                                   consecutive words; the first header of a leaf also stores the row's 9 leading words.  A leaf with a header
//                                   whose status is not OK gets zeros in every word of its row: none is written partially.
// Neither kernel has a barrier.  The per-item functions are GL_HD and run unchanged in glp_header_chain_leaf_inputs_host.
#pragma once
#include "tm_batch_kernels.cuh"

#define GLP_CHAIN_OK 0
#define GLP_CHAIN_BAD_LINK 1
#define GLP_CHAIN_BAD_HEIGHT 2
#define GLP_CHAIN_BAD_DATA_FIELD 3
#define GLP_CHAIN_FIELDS 14
#define GLP_CHAIN_MAX_LEAF_HEADERS 1024   // every wave of the rows kernel reads its leaf's statuses: leaves of a few headers (the statements use 1 - 8)
#define GLP_CHAIN_ROW_HEAD 9           // the start hash's 8 big-endian words, the leaf's first height

struct GlpChainArgs {
    const uint8_t* headers;            // [n][hdr_len]
    uint8_t* hashes;                   // [n + 1][32]: the start hash, then the hash of every header
    int32_t* status;                   // [n]
    u64* out;                          // [n / B][out_stride]
    u64 n, first_height, out_stride;
    u32 pre[GLP_CHAIN_FIELDS + 1];     // byte offset of field j in a header; pre[14] = hdr_len
    u32 B, g, per;                     // headers per leaf, varint bytes, row words per header
    uint8_t start[32];
};

// row words per header (0 = no leaf statement has this layout) — the count of _chain_leaf_inputs
static inline u64 glp_chain_words_per_header(const u32* field_len, u32 leaf_headers, u32 n_groups) {
    if (leaf_headers < 1 || leaf_headers > GLP_CHAIN_MAX_LEAF_HEADERS || n_groups < 1 || n_groups > 7) return 0;
    if (field_len[4] < 34 || field_len[6] != 34) return 0;            // _chain_leaf_statement refuses other encodings of these two
    u64 per = (u64)n_groups + 32 + (field_len[4] - 34);
    for (int j = 0; j < GLP_CHAIN_FIELDS; j++) {
        if (field_len[j] > (1u << 16)) return 0;
        if (j != 2 && j != 4 && j != 6) per += field_len[j];
    }
    return per;
}

GL_HD const uint8_t* glp_chain_prev_hash(const GlpChainArgs& a, u64 k) { return k == 0 ? a.start : a.hashes + 32 * k; }

// what _map_chain tests of header k, in its order
GL_HD int32_t glp_chain_check_item(const GlpChainArgs& a, u64 k) {
    const uint8_t* hd = a.headers + k * a.pre[GLP_CHAIN_FIELDS];
    const uint8_t* f4 = hd + a.pre[4];
    const uint8_t* prev = glp_chain_prev_hash(a, k);
    u32 diff = (u32)(f4[0] ^ 0x0a) | (u32)(f4[1] ^ 0x20);
    for (int i = 0; i < 32; i++) diff |= (u32)(f4[2 + i] ^ prev[i]);
    if (diff) return GLP_CHAIN_BAD_LINK;
    // 08, then the height in exactly g groups of 7 bits, low group first, the continuation bit on all but the last: the canonical varint has
    // this many bytes only when the top group is not zero (or there is one group) and nothing lies above it
    const u64 h = a.first_height + k;
    const uint8_t* f2 = hd + a.pre[2];
    if (a.pre[3] - a.pre[2] != 1 + a.g || f2[0] != 0x08) return GLP_CHAIN_BAD_HEIGHT;
    if ((h >> (7 * a.g)) != 0 || (a.g > 1 && ((h >> (7 * (a.g - 1))) & 0x7f) == 0)) return GLP_CHAIN_BAD_HEIGHT;
    for (u32 j = 0; j < a.g; j++) {
        const u32 want = (u32)((h >> (7 * j)) & 0x7f) | (j + 1 < a.g ? 0x80u : 0u);
        if (f2[1 + j] != want) return GLP_CHAIN_BAD_HEIGHT;
    }
    const uint8_t* f6 = hd + a.pre[6];
    if (f6[0] != 0x0a || f6[1] != 0x20) return GLP_CHAIN_BAD_DATA_FIELD;
    return GLP_CHAIN_OK;
}

// are all headers of the leaf that holds header k OK
GL_HD bool glp_chain_leaf_ok(const GlpChainArgs& a, u64 k) {
    const u64 lo = k - k % a.B;
    int32_t bad = 0;
    for (u32 j = 0; j < a.B; j++) bad |= a.status[lo + j];
    return bad == 0;
}

// word w (< per) of header k's slice: varint groups, the data hash, the tail of last_block_id, the bytes of the other eleven fields
GL_HD u64 glp_chain_slice_word(const GlpChainArgs& a, u64 k, u32 w) {
    const uint8_t* hd = a.headers + k * a.pre[GLP_CHAIN_FIELDS];
    if (w < a.g) return ((a.first_height + k) >> (7 * w)) & 0x7f;
    w -= a.g;
    if (w < 32) return hd[a.pre[6] + 2 + w];
    w -= 32;
    const u32 tail = a.pre[5] - a.pre[4] - 34;
    if (w < tail) return hd[a.pre[4] + 34 + w];
    w -= tail;
    for (int j = 0; j < GLP_CHAIN_FIELDS; j++) {
        if (j == 2 || j == 4 || j == 6) continue;
        const u32 len = a.pre[j + 1] - a.pre[j];
        if (w < len) return hd[a.pre[j] + w];
        w -= len;
    }
    return 0;                                                         // not reached for w < per
}

// word w (< 9) of the head of the row of the leaf that begins at header k
GL_HD u64 glp_chain_head_word(const GlpChainArgs& a, u64 k, u32 w) {
    if (w == 8) return a.first_height + k;
    const uint8_t* s = glp_chain_prev_hash(a, k) + 4 * w;
    return ((u64)s[0] << 24) | ((u64)s[1] << 16) | ((u64)s[2] << 8) | (u64)s[3];
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_header_chain_check_kernel(const GlpChainArgs a) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    if (k == 0)
        for (int i = 0; i < 32; i++) a.hashes[i] = a.start[i];
    a.status[k] = glp_chain_check_item(a, k);
}

// lanes `lane`, lane + n_lanes, ... of header k's share of its row
GL_HD void glp_chain_rows_item(const GlpChainArgs& a, u64 k, u32 lane, u32 n_lanes) {
    const u64 l = k / a.B;
    const u32 j = (u32)(k % a.B);
    const bool ok = glp_chain_leaf_ok(a, k);
    u64* row = a.out + l * a.out_stride;
    if (j == 0)
        for (u32 w = lane; w < GLP_CHAIN_ROW_HEAD; w += n_lanes) row[w] = ok ? glp_chain_head_word(a, k, w) : 0;
    u64* slice = row + GLP_CHAIN_ROW_HEAD + (u64)j * a.per;
    for (u32 w = lane; w < a.per; w += n_lanes) slice[w] = ok ? glp_chain_slice_word(a, k, w) : 0;
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(64) glp_header_chain_rows_kernel(const GlpChainArgs a) {
    glp_chain_rows_item(a, blockIdx.x, threadIdx.x, blockDim.x);
}

// ---- the three steps serially (no ctx): the header hashes, the tests, the rows --------------------------------------------------------------
// hashes: [n + 1][32] (required here: the caller of the C form passes scratch when it does not want them).  Returns 0, or -1 for a bad layout.
static inline int glp_header_chain_fill_args(GlpChainArgs& a, GlpTmBatchArgs& t, const u32* field_len, u32 leaf_headers, u32 n_groups,
                                             const uint8_t* headers, const uint8_t* start32, u64 first_height, u64 n, u64* out, u64 out_stride,
                                             uint8_t* hashes, int32_t* status, u32* nodes, const u32* k256) {
    const u64 per = glp_chain_words_per_header(field_len, leaf_headers, n_groups);
    if (!per) return -1;
    a.headers = headers; a.hashes = hashes; a.status = status; a.out = out; a.n = n; a.first_height = first_height; a.out_stride = out_stride;
    a.pre[0] = 0;
    for (int j = 0; j < GLP_CHAIN_FIELDS; j++) a.pre[j + 1] = a.pre[j] + field_len[j];
    a.B = leaf_headers; a.g = n_groups; a.per = (u32)per;
    for (int i = 0; i < 32; i++) a.start[i] = start32[i];
    t.data = headers; t.leaf_off = nullptr; t.tree_first = nullptr; t.n_trees = n; t.total_leaves = n * GLP_CHAIN_FIELDS; t.nodes = nodes;
    t.roots = hashes + 32; t.k256 = k256; t.uni_leaves = GLP_CHAIN_FIELDS; t.uni_stride = a.pre[GLP_CHAIN_FIELDS];
    for (int j = 0; j <= GLP_TM_UNIFORM_MAX; j++) t.uni_pre[j] = j <= GLP_CHAIN_FIELDS ? a.pre[j] : 0;
    return 0;
}

// The launches of the call, written once for the driver (tm.hip, l = GlpLaunch, device pointers in a and t) and the CPU emulation
// (l = GlpEmuLaunch, host pointers): the header hashes (t: a.n trees of 14 leaves, uniform form), the tests, the rows.
template <class L> static inline void glp_header_chain_launches(L& l, const GlpChainArgs& a, const GlpTmBatchArgs& t) {
    glp_tm_batch_launches(l, t, GLP_CHAIN_FIELDS);
    l.launch(glp_header_chain_check_kernel<0>, (a.n + 255) / 256, 256, a);
    l.launch(glp_header_chain_rows_kernel<0>, a.n, 64, a);
}

static inline int glp_header_chain_leaf_inputs_host_impl(const u32* field_len, u32 leaf_headers, u32 n_groups, const uint8_t* headers,
                                                         const uint8_t* start32, u64 first_height, u64 n, u64* out, u64 out_stride,
                                                         uint8_t* hashes, int32_t* status, const u32* k256) {
    GlpChainArgs a;
    GlpTmBatchArgs t;
    u32 nodes[8 * GLP_CHAIN_FIELDS];
    if (glp_header_chain_fill_args(a, t, field_len, leaf_headers, n_groups, headers, start32, first_height, n, out, out_stride, hashes, status,
                                   nodes, k256)) return -1;
    for (int i = 0; i < 32; i++) hashes[i] = start32[i];
    for (u64 k = 0; k < n; k++) {
        t.data = headers + k * t.uni_stride;                          // tree 0 of a one-tree call: the scratch holds one header's leaves
        t.roots = hashes + 32 * (k + 1);
        glp_tm_batch_tree_host(t, 0, nodes);
    }
    for (u64 k = 0; k < n; k++) status[k] = glp_chain_check_item(a, k);
    for (u64 k = 0; k < n; k++) glp_chain_rows_item(a, k, 0, 1);
    return 0;
}
