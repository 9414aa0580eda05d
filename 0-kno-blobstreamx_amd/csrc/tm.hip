// tm.hip — C-ABI entry points of the Tendermint side (include/glprover.h): simple Merkle roots, the Ed25519 witness and the signature leaf's
// input vectors, B trees per call, forests with audit paths and batched inclusion checks, the header-chain leaf's input vectors.
// Kernels: hash_kernels.cuh, ed25519_kernels.cuh, ed25519_inputs.cuh, tm_batch_kernels.cuh, tm_proof_kernels.cuh, chain_inputs.cuh, whose
// launch sequences the batched drivers run through GlpLaunch (glp_ctx.h) and the CPU emulation (tests/emu_*) through its own launcher.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "glp_ctx.h"
#include "hash_kernels.cuh"
#include "hash_state.h"
#include "ed25519_kernels.cuh"

// the glp_*_last_*counts calls: counts = {kernel launches (counted by GlpLaunch), stream synchronises} of the last call of the kind
static int last_counts(const glp_ctx* c, uint32_t (glp_ctx::*counts)[2], uint32_t* n_launches, uint32_t* n_host_syncs) {
    if (!c || !n_launches || !n_host_syncs) return GLP_E_INVALID;
    *n_launches = (c->*counts)[0];
    *n_host_syncs = (c->*counts)[1];
    return GLP_OK;
}

// Tendermint simple Merkle root of n fixed-size leaves (RFC 6962: 0x00/0x01 prefixes, split at the
// largest power of two < n == pair adjacent nodes level by level, promoting an odd last node).
static int tm_merkle_root_impl(glp_ctx* c, const uint8_t* d_leaves, uint32_t leaf_len, const uint64_t* d_offsets, uint64_t n, uint8_t* h_root32);

extern "C" int glp_tm_merkle_root(glp_ctx* c, const uint8_t* d_leaves, uint32_t leaf_len, uint64_t n, uint8_t* h_root32) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (!h_root32 || (!d_leaves && n) || leaf_len == 0 || leaf_len > 118 || n > (1ull << 31)) { glp_set_err(c, "glp_tm_merkle_root: bad argument"); return GLP_E_INVALID; }
    return tm_merkle_root_impl(c, d_leaves, leaf_len, nullptr, n, h_root32);
}
// leaves of different lengths: leaf i = d_data[d_offsets[i] .. d_offsets[i+1]) (n + 1 non-decreasing offsets on the device)
extern "C" int glp_tm_merkle_root_var(glp_ctx* c, const uint8_t* d_data, uint64_t data_len, const uint64_t* d_offsets, uint64_t n,
                                      uint8_t* h_root32) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (!h_root32 || ((!d_data || !d_offsets) && n) || n > (1ull << 31)) { glp_set_err(c, "glp_tm_merkle_root_var: bad argument"); return GLP_E_INVALID; }
    if (n) {
        // the kernel trusts the offsets: check them here (n + 1 words, tiny next to the hashing) — non-decreasing and inside the data
        std::vector<u64> offs(n + 1);
        GLP_HIPCHK(c, hipMemcpyAsync(offs.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
        for (u64 i = 0; i < n; i++)
            if (offs[i] > offs[i + 1]) { glp_set_err(c, "glp_tm_merkle_root_var: offsets decrease at leaf %llu", (unsigned long long)i); return GLP_E_INVALID; }
        if (offs[n] > data_len) { glp_set_err(c, "glp_tm_merkle_root_var: offsets reach %llu, past data_len %llu", (unsigned long long)offs[n], (unsigned long long)data_len); return GLP_E_INVALID; }
    }
    return tm_merkle_root_impl(c, d_data, 0, d_offsets, n, h_root32);
}

static int tm_merkle_root_impl(glp_ctx* c, const uint8_t* d_leaves, uint32_t leaf_len, const uint64_t* d_offsets, uint64_t n, uint8_t* h_root32) {
    if (n == 0) {   // SHA256("")
        static const uint8_t e[32] = {0xe3,0xb0,0xc4,0x42,0x98,0xfc,0x1c,0x14,0x9a,0xfb,0xf4,0xc8,0x99,0x6f,0xb9,0x24,0x27,0xae,0x41,0xe4,0x64,0x9b,0x93,0x4c,0xa4,0x95,0x99,0x1b,0x78,0x52,0xb8,0x55};
        memcpy(h_root32, e, 32);
        return GLP_OK;
    }
    int rc = glp_ensure_sha_tables(c);
    if (rc) return rc;
    u32 *a = nullptr, *b = nullptr;
    GLP_HIPCHK(c, hipMalloc((void**)&a, n * 32));
    hipError_t e2 = hipMalloc((void**)&b, ((n + 1) / 2) * 32);
    if (e2 != hipSuccess) { hipFree(a); glp_set_err(c, "glp_tm_merkle_root: alloc"); return GLP_E_NOMEM; }
    if (d_offsets) hipLaunchKernelGGL(glp_tm_leaf_var_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_leaves, d_offsets, n, a, c->hash->d_k256);
    else hipLaunchKernelGGL(glp_tm_leaf_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_leaves, leaf_len, n, a, c->hash->d_k256);
    u64 cnt = n;
    u32 *src = a, *dst = b;
    while (cnt > 1) {
        const u64 nout = (cnt + 1) / 2;
        hipLaunchKernelGGL(glp_tm_inner_kernel<0>, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, c->stream, src, cnt, dst, c->hash->d_k256);
        cnt = nout;
        u32* t = src; src = dst; dst = t;
    }
    u32 hw[8];
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hw, src, 32, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(a); hipFree(b);
    if (e != hipSuccess) { glp_set_err(c, "glp_tm_merkle_root: %s", hipGetErrorString(e)); return GLP_E_HIP; }
    for (int k = 0; k < 8; k++) { h_root32[4*k] = hw[k] >> 24; h_root32[4*k+1] = hw[k] >> 16; h_root32[4*k+2] = hw[k] >> 8; h_root32[4*k+3] = hw[k]; }
    return GLP_OK;
}

// ---- the Ed25519 witness and the signature leaf's input vectors on the device (ed25519_inputs.cuh) ---------------------------------------------
#include "ed25519_inputs.cuh"
static_assert(GLP_ED_IN_OK == GLP_ED25519_IN_OK && GLP_ED_IN_REJECT == GLP_ED25519_IN_REJECT && GLP_ED_IN_NO_PAIR == GLP_ED25519_IN_NO_PAIR &&
              GLP_ED_IN_INVALID == GLP_ED25519_IN_INVALID && GLP_ED_FORM_PLAIN == GLP_ED25519_FORM_PLAIN &&
              GLP_ED_FORM_FLAGGED == GLP_ED25519_FORM_FLAGGED && GLP_ED_FORM_VOTE == GLP_ED25519_FORM_VOTE && GLP_ED_REC == GLP_ED25519_RECORD_WORDS,
              "glprover.h and ed25519_inputs.cuh name the same codes");

// Ed25519 verification witness for a batch of signatures (row a10): pubs [n][32], sigs [n][64],
// msgs [n][msg_stride] with lens[n] (all device); out [n][GLP_ED25519_RECORD_WORDS] u64.
extern "C" int glp_ed25519_witness(glp_ctx* c, const uint8_t* d_pubs, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_stride,
                                   const uint32_t* d_lens, uint64_t n, uint64_t* d_out) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if ((!d_pubs || !d_sigs || !d_msgs || !d_lens || !d_out) && n) { glp_set_err(c, "glp_ed25519_witness: null buffer"); return GLP_E_INVALID; }
    if (n == 0) return GLP_OK;
    if (msg_stride == 0 || n > (1ull << 30)) { glp_set_err(c, "glp_ed25519_witness: bad size"); return GLP_E_INVALID; }
    int rc = glp_ensure_sha_tables(c);
    if (rc) return rc;
    uint32_t uncounted = 0;
    GlpLaunch l{c, &uncounted};
    glp_ed25519_witness_launch(l, d_pubs, d_sigs, d_msgs, msg_stride, d_lens, n, c->hash->d_k512, d_out);
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

extern "C" int glp_ed25519_leaf_input_words(const glp_ed25519_input_layout* layout, uint64_t* n_words) {
    if (!layout || !n_words) return GLP_E_INVALID;
    const u64 w = glp_ed25519_input_words(layout->form, layout->msg_len_min, layout->msg_len_max, layout->split_scalars);
    if (!w) return GLP_E_INVALID;
    *n_words = w;
    return GLP_OK;
}

extern "C" int glp_ed25519_leaf_inputs(glp_ctx* c, const glp_ed25519_input_layout* layout, const uint8_t* d_pubs, const uint8_t* d_sigs,
                                       const uint8_t* d_msgs, uint32_t msg_stride, const uint32_t* d_lens, const uint8_t* d_flags,
                                       const uint8_t* d_dummy, uint64_t n, uint64_t* d_inputs, size_t input_stride, int32_t* h_status) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    c->ed_input_counts[0] = c->ed_input_counts[1] = 0;
    uint64_t width = 0;
    if (glp_ed25519_leaf_input_words(layout, &width) != GLP_OK) { glp_set_err(c, "glp_ed25519_leaf_inputs: no statement has this layout"); return GLP_E_INVALID; }
    if (n == 0) return GLP_OK;
    const bool flagged = layout->form != GLP_ED25519_FORM_PLAIN;
    if (!d_pubs || !d_sigs || !d_msgs || !d_lens || !d_inputs || !h_status || (flagged && (!d_flags || !d_dummy))) {
        glp_set_err(c, "glp_ed25519_leaf_inputs: null buffer");
        return GLP_E_INVALID;
    }
    if (msg_stride == 0 || n > (1ull << 30) || input_stride < width) { glp_set_err(c, "glp_ed25519_leaf_inputs: bad size"); return GLP_E_INVALID; }
    int rc = glp_ensure_sha_tables(c);
    if (rc) return rc;
    GlpPoolBuf recs(c), stat(c);
    if (recs.alloc((size_t)n * GLP_ED_REC * sizeof(u64)) != hipSuccess || stat.alloc((size_t)n * sizeof(int32_t)) != hipSuccess) return GLP_E_HIP;
    GlpEdInputsArgs a;
    a.pubs = d_pubs; a.sigs = d_sigs; a.msgs = d_msgs; a.lens = d_lens; a.flags = d_flags; a.dummy = d_dummy; a.recs = recs.u();
    a.k512 = c->hash->d_k512; a.out = d_inputs; a.status = (int32_t*)stat.p; a.n = n; a.out_stride = input_stride; a.msg_stride = msg_stride;
    a.form = layout->form; a.lo = layout->msg_len_min; a.hi = layout->msg_len_max; a.split = layout->split_scalars ? 1u : 0u;
    GlpLaunch l{c, &c->ed_input_counts[0]};
    glp_ed25519_leaf_inputs_launches(l, a, recs.u());
    GLP_HIPCHK(c, hipGetLastError());
    GLP_HIPCHK(c, hipMemcpyAsync(h_status, stat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->ed_input_counts[1] = 1;
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    return GLP_OK;
}

extern "C" int glp_ed25519_last_input_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    return last_counts(c, &glp_ctx::ed_input_counts, n_launches, n_host_syncs);
}

extern "C" int glp_ed25519_half_scalars(glp_ctx* c, const uint64_t* d_k, uint64_t n, uint64_t* d_out) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if ((!d_k || !d_out) && n) { glp_set_err(c, "glp_ed25519_half_scalars: null buffer"); return GLP_E_INVALID; }
    if (n == 0) return GLP_OK;
    if (n > (1ull << 30)) { glp_set_err(c, "glp_ed25519_half_scalars: bad size"); return GLP_E_INVALID; }
    uint32_t uncounted = 0;
    GlpLaunch l{c, &uncounted};
    glp_ed25519_half_scalars_launch(l, d_k, n, d_out);
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

// ---- B Tendermint trees per call (tm_batch_kernels.cuh) and the header-chain leaf's input vectors (chain_inputs.cuh) -------------------------
#include "chain_inputs.cuh"
static_assert(GLP_CHAIN_OK == GLP_HEADER_CHAIN_OK && GLP_CHAIN_BAD_LINK == GLP_HEADER_CHAIN_BAD_LINK &&
              GLP_CHAIN_BAD_HEIGHT == GLP_HEADER_CHAIN_BAD_HEIGHT && GLP_CHAIN_BAD_DATA_FIELD == GLP_HEADER_CHAIN_BAD_DATA_FIELD &&
              GLP_CHAIN_FIELDS == sizeof(((glp_header_chain_layout*)0)->field_len) / sizeof(uint32_t),
              "glprover.h and chain_inputs.cuh name the same codes");

// what the tree launches over a.total_leaves leaves and a.n_trees (> 0) trees need: the size limits, the SHA tables, a.nodes, a.k256
static int tm_batch_prepare(glp_ctx* c, GlpTmBatchArgs& a, GlpPoolBuf& nodes) {
    if (a.n_trees > 0x7fffffffull || a.total_leaves > (1ull << 36)) { glp_set_err(c, "glp_tm_merkle_root_batch: too many trees or leaves"); return GLP_E_UNSUPPORTED; }
    int rc = glp_ensure_sha_tables(c);
    if (rc) return rc;
    if (nodes.alloc((size_t)(a.total_leaves ? a.total_leaves : 1) * 32) != hipSuccess) return GLP_E_NOMEM;
    a.nodes = (u32*)nodes.p;
    a.k256 = c->hash->d_k256;
    return GLP_OK;
}

extern "C" int glp_tm_merkle_root_batch(glp_ctx* c, const uint8_t* d_data, uint64_t data_len, const uint64_t* h_leaf_offsets,
                                        const uint64_t* h_tree_first, uint64_t total_leaves, uint64_t n_trees, uint8_t* d_roots,
                                        uint8_t* h_roots) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    c->tm_batch_counts[0] = c->tm_batch_counts[1] = 0;
    if (n_trees == 0) return GLP_OK;
    if (!h_leaf_offsets || !h_tree_first || !d_roots || (!d_data && data_len)) { glp_set_err(c, "glp_tm_merkle_root_batch: null argument"); return GLP_E_INVALID; }
    const int bad = glp_tm_batch_check(h_leaf_offsets, h_tree_first, total_leaves, n_trees, data_len);
    if (bad == 1) { glp_set_err(c, "glp_tm_merkle_root_batch: offsets decrease, pass data_len, or the trees do not cover the leaves"); return GLP_E_INVALID; }
    if (bad == 2) { glp_set_err(c, "glp_tm_merkle_root_batch: a tree has more than %d leaves", GLP_TM_BATCH_MAX_LEAVES); return GLP_E_UNSUPPORTED; }
    // the kernels read the checked words themselves: uploaded here, stream-ordered, into scratch of the ctx
    GlpPoolBuf nodes(c), arrays(c);
    const size_t n_off = (size_t)total_leaves + 1, n_first = (size_t)n_trees + 1;
    if (arrays.alloc((n_off + n_first) * 8) != hipSuccess) return GLP_E_NOMEM;
    GLP_HIPCHK(c, hipMemcpyAsync(arrays.u(), h_leaf_offsets, n_off * 8, hipMemcpyHostToDevice, c->stream));
    GLP_HIPCHK(c, hipMemcpyAsync(arrays.u() + n_off, h_tree_first, n_first * 8, hipMemcpyHostToDevice, c->stream));
    GlpTmBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.data = d_data; a.leaf_off = arrays.u(); a.tree_first = arrays.u() + n_off; a.n_trees = n_trees; a.total_leaves = total_leaves; a.roots = d_roots;
    int rc = tm_batch_prepare(c, a, nodes);
    if (rc) return rc;
    GlpLaunch l{c, &c->tm_batch_counts[0]};
    glp_tm_batch_launches(l, a, glp_tm_batch_max_tree(h_tree_first, n_trees));
    GLP_HIPCHK(c, hipGetLastError());
    if (h_roots) {
        GLP_HIPCHK(c, hipMemcpyAsync(h_roots, d_roots, (size_t)n_trees * 32, hipMemcpyDeviceToHost, c->stream));
        c->tm_batch_counts[1] = 1;
        GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GLP_OK;
}

extern "C" int glp_tm_merkle_root_batch_last_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    return last_counts(c, &glp_ctx::tm_batch_counts, n_launches, n_host_syncs);
}

extern "C" int glp_tm_merkle_root_batch_host(const uint8_t* data, uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* tree_first,
                                             uint64_t total_leaves, uint64_t n_trees, uint8_t* roots) {
    if (n_trees == 0) return GLP_OK;
    if (!leaf_offsets || !tree_first || !roots || (!data && data_len)) return GLP_E_INVALID;
    const int bad = glp_tm_batch_check(leaf_offsets, tree_first, total_leaves, n_trees, data_len);
    if (bad) return bad == 1 ? GLP_E_INVALID : GLP_E_UNSUPPORTED;
    GlpTmBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.data = data; a.leaf_off = leaf_offsets; a.tree_first = tree_first; a.n_trees = n_trees; a.total_leaves = total_leaves; a.roots = roots; a.k256 = glp_k256;
    std::vector<u32> scratch(8 * GLP_TM_BATCH_MAX_LEAVES);
    for (u64 t = 0; t < n_trees; t++) glp_tm_batch_tree_host(a, t, scratch.data());
    return GLP_OK;
}

// ---- trees with every level kept, audit paths, batched inclusion checks (tm_proof_kernels.cuh) ------------------------------------------------
#include "tm_proof_kernels.cuh"
static_assert(GLP_TM_INC_OK == GLP_TM_INCLUSION_OK && GLP_TM_INC_BAD_SHAPE == GLP_TM_INCLUSION_BAD_SHAPE && GLP_TM_INC_BAD_ROOT == GLP_TM_INCLUSION_BAD_ROOT &&
              GLP_TM_FOREST_MAX_TREE == GLP_TM_FOREST_MAX_LEAVES, "glprover.h and tm_proof_kernels.cuh name the same codes");

struct glp_tm_forest {
    glp_ctx* c = nullptr;
    void* block = nullptr;                   // one pool block: slab | roots | tree_first | upper_base
    u32* slab = nullptr;
    uint8_t* roots = nullptr;
    u64 *d_tree_first = nullptr, *d_upper_base = nullptr;
    std::vector<u64> tree_first;             // the checked host copy: what glp_tm_forest_proofs validates queries against
    GlpTmForestPlan plan;
    u64 n_trees = 0, total_leaves = 0, bytes = 0;
};

static void tm_forest_args(const glp_tm_forest* f, GlpTmForestArgs& a) {
    memset(&a, 0, sizeof(a));
    a.tree_first = f->d_tree_first; a.upper_base = f->d_upper_base; a.n_trees = f->n_trees; a.total_leaves = f->total_leaves;
    a.slab = f->slab; a.roots = f->roots; a.k256 = f->c->hash->d_k256;
}

extern "C" int glp_tm_forest_create(glp_ctx* c, const uint8_t* d_data, uint64_t data_len, const uint64_t* h_leaf_offsets, const uint64_t* h_tree_first,
                                    uint64_t total_leaves, uint64_t n_trees, uint8_t* h_roots, glp_tm_forest** out) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    c->tm_forest_counts[0] = c->tm_forest_counts[1] = 0;
    if (!out) { glp_set_err(c, "glp_tm_forest_create: null argument"); return GLP_E_INVALID; }
    if (n_trees && (!h_leaf_offsets || !h_tree_first || (!d_data && data_len))) { glp_set_err(c, "glp_tm_forest_create: null argument"); return GLP_E_INVALID; }
    static const u64 none[1] = {0};
    if (n_trees == 0) {                      // an empty forest: a handle that admits no query
        if (total_leaves) { glp_set_err(c, "glp_tm_forest_create: leaves without a tree"); return GLP_E_INVALID; }
        h_tree_first = none;
    } else {
        const int bad = glp_tm_forest_check(h_leaf_offsets, h_tree_first, total_leaves, n_trees, data_len);
        if (bad == 1) { glp_set_err(c, "glp_tm_forest_create: offsets decrease, pass data_len, or the trees do not cover the leaves"); return GLP_E_INVALID; }
        if (bad == 2) { glp_set_err(c, "glp_tm_forest_create: a tree has more than 2^24 leaves"); return GLP_E_UNSUPPORTED; }
        if (n_trees > 0x7fffffffull || total_leaves > (1ull << 36)) { glp_set_err(c, "glp_tm_forest_create: too many trees or leaves"); return GLP_E_UNSUPPORTED; }
    }
    int rc = glp_ensure_sha_tables(c);
    if (rc) return rc;
    glp_tm_forest* f = new glp_tm_forest;
    f->c = c; f->n_trees = n_trees; f->total_leaves = total_leaves;
    f->tree_first.assign(h_tree_first, h_tree_first + n_trees + 1);
    glp_tm_forest_plan(f->tree_first.data(), n_trees, f->plan);
    const size_t n_first = (size_t)n_trees + 1, n_off = (size_t)total_leaves + 1, n_lvl = f->plan.level_pre.size();
    const size_t slab_bytes = (size_t)f->plan.total_nodes * 32, root_bytes = (size_t)n_trees * 32;
    f->bytes = slab_bytes + root_bytes + 2 * n_first * 8;
    GlpPoolBuf keep(c), arrays(c);           // arrays: the leaf offsets and the level prefixes, needed by this call's launches only
    if (keep.alloc(f->bytes) != hipSuccess || arrays.alloc((n_off + n_lvl * n_first) * 8) != hipSuccess) { delete f; return GLP_E_NOMEM; }
    f->slab = (u32*)keep.p;
    f->roots = (uint8_t*)keep.p + slab_bytes;
    f->d_tree_first = (u64*)(f->roots + root_bytes);
    f->d_upper_base = f->d_tree_first + n_first;
    hipError_t e = hipMemcpyAsync(f->d_tree_first, f->tree_first.data(), n_first * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_upper_base, f->plan.upper_base.data(), n_first * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_trees) e = hipMemcpyAsync(arrays.u(), h_leaf_offsets, n_off * 8, hipMemcpyHostToDevice, c->stream);
    for (size_t l = 0; l < n_lvl && e == hipSuccess; l++)
        e = hipMemcpyAsync(arrays.u() + n_off + l * n_first, f->plan.level_pre[l].data(), n_first * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_trees) {
        GlpTmForestArgs a;
        tm_forest_args(f, a);
        GlpLaunch l{c, &c->tm_forest_counts[0]};
        glp_tm_forest_create_launches(l, a, glp_tm_forest_leaf_args(a, d_data, arrays.u()), f->plan,
                                      [&](size_t lvl) { return arrays.u() + n_off + lvl * n_first; });
        e = hipGetLastError();
        if (e == hipSuccess && h_roots) {
            e = hipMemcpyAsync(h_roots, f->roots, root_bytes, hipMemcpyDeviceToHost, c->stream);
            c->tm_forest_counts[1] = 1;
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
    }
    if (e != hipSuccess) { glp_set_err(c, "glp_tm_forest_create: %s", hipGetErrorString(e)); delete f; return GLP_E_HIP; }
    f->block = keep.release();
    *out = f;
    return GLP_OK;
}

extern "C" int glp_tm_forest_info(const glp_tm_forest* f, uint64_t* n_trees, uint64_t* total_leaves, uint32_t* max_aunts, uint64_t* bytes) {
    if (!f) return GLP_E_INVALID;
    if (n_trees) *n_trees = f->n_trees;
    if (total_leaves) *total_leaves = f->total_leaves;
    if (max_aunts) *max_aunts = f->plan.max_aunts;
    if (bytes) *bytes = f->bytes;
    return GLP_OK;
}

extern "C" int glp_tm_forest_roots(const glp_tm_forest* f, const uint8_t** d_roots) {
    if (!f || !d_roots) return GLP_E_INVALID;
    *d_roots = f->roots;
    return GLP_OK;
}

extern "C" int glp_tm_forest_destroy(glp_tm_forest* f) {
    if (!f) return GLP_OK;
    if (f->block) glp_pool_release(f->c, f->block);      // stream-ordered reuse: work of the ctx's stream that still reads it comes first
    delete f;
    return GLP_OK;
}

extern "C" int glp_tm_forest_proofs(glp_ctx* c, const glp_tm_forest* f, const uint64_t* h_query_tree, const uint64_t* h_query_leaf, uint64_t n_queries,
                                    uint8_t* d_aunts, uint32_t aunt_stride, uint32_t* d_n_aunts, uint8_t* d_leaf_hashes) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    c->tm_forest_counts[0] = c->tm_forest_counts[1] = 0;
    if (!f || f->c != c) { glp_set_err(c, "glp_tm_forest_proofs: not a forest of this ctx"); return GLP_E_INVALID; }
    if (glp_tm_forest_check_queries(f->tree_first.data(), f->n_trees, f->plan.max_aunts, h_query_tree, h_query_leaf, n_queries, aunt_stride)) {
        glp_set_err(c, "glp_tm_forest_proofs: a query names no leaf of the forest, or aunt_stride is below the aunts of a queried tree");
        return GLP_E_INVALID;
    }
    if (n_queries == 0) return GLP_OK;
    if (!d_n_aunts || (!d_aunts && aunt_stride)) { glp_set_err(c, "glp_tm_forest_proofs: null argument"); return GLP_E_INVALID; }
    if (n_queries > (1ull << 36)) { glp_set_err(c, "glp_tm_forest_proofs: too many queries"); return GLP_E_UNSUPPORTED; }
    GlpPoolBuf q(c);
    GlpTmPathArgs a;
    memset(&a, 0, sizeof(a));
    tm_forest_args(f, a.f);
    if (h_query_tree) {
        if (q.alloc((size_t)n_queries * 16) != hipSuccess) return GLP_E_NOMEM;
        GLP_HIPCHK(c, hipMemcpyAsync(q.u(), h_query_tree, (size_t)n_queries * 8, hipMemcpyHostToDevice, c->stream));
        GLP_HIPCHK(c, hipMemcpyAsync(q.u() + n_queries, h_query_leaf, (size_t)n_queries * 8, hipMemcpyHostToDevice, c->stream));
        a.query_tree = q.u(); a.query_leaf = q.u() + n_queries;
    }
    a.n_queries = n_queries; a.aunts = d_aunts; a.n_aunts = d_n_aunts; a.leaf_hash = d_leaf_hashes; a.aunt_stride = aunt_stride;
    GlpLaunch l{c, &c->tm_forest_counts[0]};
    glp_tm_path_launch(l, a);
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

extern "C" int glp_tm_verify_inclusion_batch(glp_ctx* c, const uint8_t* d_roots, uint64_t n_roots, const uint32_t* h_root_of, const uint8_t* d_data,
                                             uint64_t data_len, const uint64_t* h_leaf_offsets, const uint64_t* d_index, const uint64_t* d_total,
                                             const uint8_t* d_aunts, uint32_t aunt_stride, const uint32_t* d_n_aunts, uint64_t n, int32_t* h_status) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    c->tm_forest_counts[0] = c->tm_forest_counts[1] = 0;
    if (n == 0) return GLP_OK;
    if (!d_roots || !h_leaf_offsets || !d_index || !d_total || !d_n_aunts || !h_status || (!d_data && data_len) || (!d_aunts && aunt_stride)) {
        glp_set_err(c, "glp_tm_verify_inclusion_batch: null argument");
        return GLP_E_INVALID;
    }
    if (glp_tm_verify_check(h_leaf_offsets, n, data_len, h_root_of, n_roots)) {
        glp_set_err(c, "glp_tm_verify_inclusion_batch: offsets decrease or pass data_len, or a proof names no root");
        return GLP_E_INVALID;
    }
    if (n > (1ull << 36)) { glp_set_err(c, "glp_tm_verify_inclusion_batch: too many proofs"); return GLP_E_UNSUPPORTED; }
    int rc = glp_ensure_sha_tables(c);
    if (rc) return rc;
    GlpPoolBuf arrays(c), stat(c);
    const size_t n_off = (size_t)n + 1;
    if (arrays.alloc(n_off * 8 + (h_root_of ? (size_t)n * 4 : 0)) != hipSuccess || stat.alloc((size_t)n * sizeof(int32_t)) != hipSuccess) return GLP_E_NOMEM;
    GLP_HIPCHK(c, hipMemcpyAsync(arrays.u(), h_leaf_offsets, n_off * 8, hipMemcpyHostToDevice, c->stream));
    if (h_root_of) GLP_HIPCHK(c, hipMemcpyAsync(arrays.u() + n_off, h_root_of, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    GlpTmVerifyArgs a;
    memset(&a, 0, sizeof(a));
    a.roots = d_roots; a.root_of = h_root_of ? (const u32*)(arrays.u() + n_off) : nullptr; a.data = d_data; a.leaf_off = arrays.u();
    a.index = d_index; a.total = d_total; a.aunts = d_aunts; a.n_aunts = d_n_aunts; a.n = n; a.status = (int32_t*)stat.p;
    a.k256 = c->hash->d_k256; a.aunt_stride = aunt_stride;
    GlpLaunch l{c, &c->tm_forest_counts[0]};
    glp_tm_verify_launch(l, a);
    GLP_HIPCHK(c, hipGetLastError());
    GLP_HIPCHK(c, hipMemcpyAsync(h_status, stat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->tm_forest_counts[1] = 1;
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    return GLP_OK;
}

extern "C" int glp_tm_forest_last_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    return last_counts(c, &glp_ctx::tm_forest_counts, n_launches, n_host_syncs);
}

extern "C" int glp_tm_forest_proofs_host(const uint8_t* data, uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* tree_first,
                                         uint64_t total_leaves, uint64_t n_trees, const uint64_t* query_tree, const uint64_t* query_leaf,
                                         uint64_t n_queries, uint8_t* roots, uint8_t* aunts, uint32_t aunt_stride, uint32_t* n_aunts,
                                         uint8_t* leaf_hashes) {
    const int bad = glp_tm_forest_proofs_host_impl(data, data_len, leaf_offsets, tree_first, total_leaves, n_trees, query_tree, query_leaf, n_queries,
                                                   roots, aunts, aunt_stride, n_aunts, leaf_hashes, glp_k256);
    return bad == 0 ? GLP_OK : bad == 1 ? GLP_E_INVALID : GLP_E_UNSUPPORTED;
}

extern "C" int glp_tm_verify_inclusion_batch_host(const uint8_t* roots, uint64_t n_roots, const uint32_t* root_of, const uint8_t* data,
                                                  uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* index, const uint64_t* total,
                                                  const uint8_t* aunts, uint32_t aunt_stride, const uint32_t* n_aunts, uint64_t n, int32_t* status) {
    return glp_tm_verify_inclusion_host_impl(roots, n_roots, root_of, data, data_len, leaf_offsets, index, total, aunts, aunt_stride, n_aunts, n,
                                             status, glp_k256) ? GLP_E_INVALID : GLP_OK;
}

extern "C" int glp_header_chain_leaf_input_words(const glp_header_chain_layout* layout, uint64_t* n_words) {
    if (!layout || !n_words) return GLP_E_INVALID;
    const u64 per = glp_chain_words_per_header(layout->field_len, layout->leaf_headers, layout->n_groups);
    if (!per) return GLP_E_INVALID;
    *n_words = GLP_CHAIN_ROW_HEAD + per * layout->leaf_headers;
    return GLP_OK;
}

extern "C" int glp_header_chain_leaf_inputs(glp_ctx* c, const glp_header_chain_layout* layout, const uint8_t* d_headers, const uint8_t* start_hash32,
                                            uint64_t first_height, uint64_t n, uint64_t* d_inputs, size_t input_stride, uint8_t* d_hashes,
                                            int32_t* h_status) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    c->chain_input_counts[0] = c->chain_input_counts[1] = 0;
    uint64_t width = 0;
    if (glp_header_chain_leaf_input_words(layout, &width) != GLP_OK) { glp_set_err(c, "glp_header_chain_leaf_inputs: no leaf statement has this layout"); return GLP_E_INVALID; }
    if (n == 0) return GLP_OK;
    if (!d_headers || !start_hash32 || !d_inputs || !h_status) { glp_set_err(c, "glp_header_chain_leaf_inputs: null argument"); return GLP_E_INVALID; }
    if (n % layout->leaf_headers || input_stride < width || n > (1ull << 30) || first_height >= (1ull << 49)) {
        glp_set_err(c, "glp_header_chain_leaf_inputs: n is not a whole number of leaves or above 2^30, the stride is below the row, or first_height is 2^49 or more");
        return GLP_E_INVALID;
    }
    GlpPoolBuf nodes(c), stat(c), hashes(c);
    if (stat.alloc((size_t)n * sizeof(int32_t)) != hipSuccess) return GLP_E_NOMEM;
    if (!d_hashes) {
        if (hashes.alloc((size_t)(n + 1) * 32) != hipSuccess) return GLP_E_NOMEM;
        d_hashes = (uint8_t*)hashes.p;
    }
    GlpChainArgs a;
    GlpTmBatchArgs t;
    memset(&t, 0, sizeof(t));
    if (glp_header_chain_fill_args(a, t, layout->field_len, layout->leaf_headers, layout->n_groups, d_headers, start_hash32, first_height, n, d_inputs,
                                   input_stride, d_hashes, (int32_t*)stat.p, nullptr, nullptr)) return GLP_E_INVALID;
    int rc = tm_batch_prepare(c, t, nodes);
    if (rc) return rc;
    GlpLaunch l{c, &c->chain_input_counts[0]};
    glp_header_chain_launches(l, a, t);
    GLP_HIPCHK(c, hipGetLastError());
    GLP_HIPCHK(c, hipMemcpyAsync(h_status, stat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->chain_input_counts[1] = 1;
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    return GLP_OK;
}

extern "C" int glp_header_chain_last_input_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    return last_counts(c, &glp_ctx::chain_input_counts, n_launches, n_host_syncs);
}

extern "C" int glp_header_chain_leaf_inputs_host(const glp_header_chain_layout* layout, const uint8_t* headers, const uint8_t* start_hash32,
                                                 uint64_t first_height, uint64_t n, uint64_t* inputs, size_t input_stride, uint8_t* hashes,
                                                 int32_t* status) {
    uint64_t width = 0;
    if (glp_header_chain_leaf_input_words(layout, &width) != GLP_OK) return GLP_E_INVALID;
    if (n == 0) return GLP_OK;
    if (!headers || !start_hash32 || !inputs || !status || n % layout->leaf_headers || input_stride < width || first_height >= (1ull << 49)) return GLP_E_INVALID;
    std::vector<uint8_t> own;
    if (!hashes) { own.resize((size_t)(n + 1) * 32); hashes = own.data(); }
    return glp_header_chain_leaf_inputs_host_impl(layout->field_len, layout->leaf_headers, layout->n_groups, headers, start_hash32, first_height, n,
                                                  inputs, input_stride, hashes, status, glp_k256) ? GLP_E_INVALID : GLP_OK;
}
