// hash.hip — C-ABI entry points for Poseidon / Merkle / FRI fold / SHA-2 witness traces
// (include/glprover.h).  Kernels: hash_kernels.cuh.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "glp_ctx.h"
#include "hash_kernels.cuh"
#include "merkle_batch_kernels.cuh"
#include "merkle_plan.h"

#include "hash_state.h"
#include "poseidon_precomp.h"
#include "ed25519_kernels.cuh"

int glp_ntt_table(glp_ctx* c, int log_N, int inv, const u64** lo, const u64** hi);   // glprover.hip

static const u32 K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
static const u64 K512[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
    0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
    0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
    0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
    0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
    0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
    0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
    0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
    0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
    0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
    0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
    0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

glp_hash_state* glp_hash_get(glp_ctx* c) {
    if (!c->hash) c->hash = new glp_hash_state();
    return c->hash;
}
static glp_hash_state* hs(glp_ctx* c) { return glp_hash_get(c); }

void glp_hash_destroy(glp_ctx* c) {
    if (!c || !c->hash) return;
    if (c->hash->d_consts) hipFree(c->hash->d_consts);
    if (c->hash->d_k256) hipFree(c->hash->d_k256);
    if (c->hash->d_k512) hipFree(c->hash->d_k512);
    if (c->hash->d_pg_coef) hipFree(c->hash->d_pg_coef);
    if (c->hash->d_pg_cst) hipFree(c->hash->d_pg_cst);
    delete c->hash;
    c->hash = nullptr;
}

static GlpPoseidonConsts consts_of(glp_hash_state* h) { return glp_dev_consts(h); }

extern "C" int glp_set_poseidon_constants(glp_ctx* c, const uint64_t* rc, size_t n_rc, const uint64_t* circ, const uint64_t* diag) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (!rc || !circ || !diag || n_rc != 360) { glp_set_err(c, "glp_set_poseidon_constants: need 360 round constants, 12 + 12 MDS entries"); return GLP_E_INVALID; }
    std::vector<u64> all(384);
    for (int i = 0; i < 360; i++) { if (rc[i] >= GL_P) { glp_set_err(c, "round constant %d not canonical", i); return GLP_E_INVALID; } all[i] = rc[i]; }
    unsigned __int128 sum = 0;
    u64 maxdiag = 0;
    bool small = true;
    for (int i = 0; i < 12; i++) {
        if (circ[i] >= GL_P || diag[i] >= GL_P) { glp_set_err(c, "MDS entry %d not canonical", i); return GLP_E_INVALID; }
        all[360 + i] = circ[i]; all[372 + i] = diag[i];
        sum += circ[i];
        if (diag[i] > maxdiag) maxdiag = diag[i];
        if (circ[i] >> 24 || diag[i] >> 24) small = false;
    }
    if (sum + maxdiag >= ((unsigned __int128)1 << 24)) small = false;   // bound the fast MDS path relies on (hash_kernels.cuh)
    glp_hash_state* h = hs(c);
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!h->d_consts) GLP_HIPCHK(c, hipMalloc((void**)&h->d_consts, 384 * 8));
    GLP_HIPCHK(c, hipMemcpy(h->d_consts, all.data(), 384 * 8, hipMemcpyHostToDevice));
    h->h_consts = all;
    h->have_consts = true;
    h->small_mds = small;
    // grouped partial rounds: only for small-integer MDS whose cubes stay small
    if (h->d_pg_coef) { hipFree(h->d_pg_coef); h->d_pg_coef = nullptr; }
    if (h->d_pg_cst) { hipFree(h->d_pg_cst); h->d_pg_cst = nullptr; }
    h->h_pg_coef.clear(); h->h_pg_cst.clear();
    if (small && glp_poseidon_group_tables(all.data(), h->h_pg_coef, h->h_pg_cst)) {
        GLP_HIPCHK(c, hipMalloc((void**)&h->d_pg_coef, h->h_pg_coef.size() * 4));
        GLP_HIPCHK(c, hipMalloc((void**)&h->d_pg_cst, h->h_pg_cst.size() * 8));
        GLP_HIPCHK(c, hipMemcpy(h->d_pg_coef, h->h_pg_coef.data(), h->h_pg_coef.size() * 4, hipMemcpyHostToDevice));
        GLP_HIPCHK(c, hipMemcpy(h->d_pg_cst, h->h_pg_cst.data(), h->h_pg_cst.size() * 8, hipMemcpyHostToDevice));
    } else {
        h->h_pg_coef.clear(); h->h_pg_cst.clear();
    }
    return GLP_OK;
}

static int need_consts(glp_ctx* c) {
    if (!c->hash || !c->hash->have_consts) { glp_set_err(c, "Poseidon constants not set (glp_set_poseidon_constants)"); return GLP_E_STATE; }
    return GLP_OK;
}

extern "C" int glp_poseidon_permute(glp_ctx* c, uint64_t* d_states, uint64_t n) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (!d_states && n) { glp_set_err(c, "glp_poseidon_permute: null states"); return GLP_E_INVALID; }
    int rc = need_consts(c);
    if (rc) return rc;
    if (n == 0) return GLP_OK;
    const u64 blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffull) return GLP_E_UNSUPPORTED;
    glp_hash_state* h = c->hash;
    if (h->small_mds) hipLaunchKernelGGL(glp_poseidon_permute_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_states, n, consts_of(h));
    else hipLaunchKernelGGL(glp_poseidon_permute_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_states, n, consts_of(h));
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

static int merkle_impl(glp_ctx* c, const u64* src, u64 stride, bool poly_major, u32 leaf_len, u32 log_leaves, u32 cap_h,
                       u64* digests, u64* h_cap) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (!src || !digests || log_leaves > 40 || cap_h > log_leaves || leaf_len == 0) { glp_set_err(c, "glp_merkle: bad argument"); return GLP_E_INVALID; }
    int rc = need_consts(c);
    if (rc) return rc;
    glp_hash_state* h = c->hash;
    const GlpPoseidonConsts k = consts_of(h);
    const u64 nl = 1ull << log_leaves;
    u64 blocks = (nl + 255) / 256;
    if (blocks > 0x7fffffffull) return GLP_E_UNSUPPORTED;
    const dim3 g((unsigned)blocks), b(256);
    if (h->small_mds) {
        if (poly_major) hipLaunchKernelGGL((glp_hash_leaves_kernel<true, true>), g, b, 0, c->stream, src, stride, leaf_len, nl, digests, k);
        else hipLaunchKernelGGL((glp_hash_leaves_kernel<true, false>), g, b, 0, c->stream, src, stride, leaf_len, nl, digests, k);
    } else {
        if (poly_major) hipLaunchKernelGGL((glp_hash_leaves_kernel<false, true>), g, b, 0, c->stream, src, stride, leaf_len, nl, digests, k);
        else hipLaunchKernelGGL((glp_hash_leaves_kernel<false, false>), g, b, 0, c->stream, src, stride, leaf_len, nl, digests, k);
    }
    GLP_HIPCHK(c, hipGetLastError());
    u64* prev = digests;
    u64 cnt = nl;
    // levels of <= coop_max nodes leave most of the chip idle and are latency-bound: there a permutation is spread over 12 lanes
    // (glp_poseidon_permute_coop), and the last levels (<= 64 nodes) run in one launch.  GLP_COOP_MAX_NODES=0 turns both off.
    static const u64 coop_max = [] { const char* e = getenv("GLP_COOP_MAX_NODES"); return e ? (u64)atoll(e) : (u64)16384; }();
    for (u32 lvl = log_leaves; lvl > cap_h; lvl--) {
        u64* cur = prev + 4 * cnt;
        const u64 out = cnt >> 1;
        if (coop_max && out <= GLP_COOP_TOP_NODES && out <= coop_max) {          // the rest of the tree in one launch
            const u32 n_levels = lvl - cap_h;
            if (h->small_mds) hipLaunchKernelGGL(glp_merkle_top_coop_kernel<true>, dim3(1), dim3(1024), 0, c->stream, prev, cnt, n_levels, k);
            else hipLaunchKernelGGL(glp_merkle_top_coop_kernel<false>, dim3(1), dim3(1024), 0, c->stream, prev, cnt, n_levels, k);
            GLP_HIPCHK(c, hipGetLastError());
            for (u32 l = 0; l < n_levels; l++) { prev += 4 * cnt; cnt >>= 1; }
            break;
        }
        cnt = out;
        if (coop_max && cnt <= coop_max) {
            blocks = (cnt * 16 + 255) / 256;
            if (h->small_mds) hipLaunchKernelGGL(glp_merkle_level_coop_kernel<true>, dim3((unsigned)blocks), b, 0, c->stream, prev, cur, cnt, k);
            else hipLaunchKernelGGL(glp_merkle_level_coop_kernel<false>, dim3((unsigned)blocks), b, 0, c->stream, prev, cur, cnt, k);
        } else {
            blocks = (cnt + 255) / 256;
            if (h->small_mds) hipLaunchKernelGGL(glp_merkle_level_kernel<true>, dim3((unsigned)blocks), b, 0, c->stream, prev, cur, cnt, k);
            else hipLaunchKernelGGL(glp_merkle_level_kernel<false>, dim3((unsigned)blocks), b, 0, c->stream, prev, cur, cnt, k);
        }
        GLP_HIPCHK(c, hipGetLastError());
        prev = cur;
    }
    if (h_cap) {
        GLP_HIPCHK(c, hipMemcpyAsync(h_cap, prev, (size_t)32 << cap_h, hipMemcpyDeviceToHost, c->stream));
        GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GLP_OK;
}

extern "C" int glp_merkle(glp_ctx* c, const uint64_t* d_leaves, uint32_t leaf_len, uint32_t log_leaves, uint32_t cap_h,
                          uint64_t* d_digests, uint64_t* h_cap) {
    return merkle_impl(c, d_leaves, leaf_len, false, leaf_len, log_leaves, cap_h, d_digests, h_cap);
}
extern "C" int glp_merkle_from_polys(glp_ctx* c, const uint64_t* d_polys, uint64_t poly_stride, uint32_t leaf_len,
                                     uint32_t log_leaves, uint32_t cap_h, uint64_t* d_digests, uint64_t* h_cap) {
    if (c && log_leaves <= 40 && poly_stride < (1ull << log_leaves)) { glp_set_err(c, "glp_merkle_from_polys: stride < leaves"); return GLP_E_INVALID; }
    return merkle_impl(c, d_polys, poly_stride, true, leaf_len, log_leaves, cap_h, d_digests, h_cap);
}

// ---- B trees of one shape per launch (kernels: merkle_batch_kernels.cuh; plan: merkle_plan.h) -------------------------------------
extern "C" int glp_merkle_batch_plan(uint32_t log_leaves, uint32_t cap_h, uint32_t fuse_max_log, uint32_t* n_launches, uint32_t* n_fused) {
    if (log_leaves > 40 || cap_h > log_leaves) return GLP_E_INVALID;
    std::vector<glp_merkle_step> steps;
    glp_merkle_plan_steps(log_leaves, cap_h, fuse_max_log, steps);
    u32 nf = 0;
    for (const glp_merkle_step& s : steps) nf += s.fused;
    if (n_launches) *n_launches = 1 + (u32)steps.size();      // the leaf launch
    if (n_fused) *n_fused = nf;
    return GLP_OK;
}

extern "C" int glp_merkle_batch(glp_ctx* c, const uint64_t* d_src, uint64_t src_tree_stride, int poly_major, uint64_t poly_stride,
                                uint32_t leaf_len, uint32_t log_leaves, uint32_t cap_h, uint32_t B, uint32_t fuse_max_log, uint64_t* d_digests,
                                uint64_t digest_tree_stride, uint64_t* h_caps) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (B == 0) return GLP_OK;
    if (!d_src || !d_digests) { glp_set_err(c, "glp_merkle_batch: null buffer"); return GLP_E_INVALID; }
    if (const char* why = glp_merkle_batch_check(src_tree_stride, poly_major, poly_stride, leaf_len, log_leaves, cap_h, digest_tree_stride)) {
        glp_set_err(c, "glp_merkle_batch: %s", why);
        return GLP_E_INVALID;
    }
    const u64 nl = 1ull << log_leaves;
    int rc = need_consts(c);
    if (rc) return rc;
    glp_hash_state* h = c->hash;
    const GlpPoseidonConsts k = consts_of(h);
    std::vector<glp_merkle_step> steps;
    glp_merkle_plan_steps(log_leaves, cap_h, fuse_max_log, steps);
    const u64 leaf_bpt = (nl + 255) / 256;
    u64 max_blocks = leaf_bpt * B;
    for (const glp_merkle_step& s : steps) if (glp_merkle_step_blocks(s) * B > max_blocks) max_blocks = glp_merkle_step_blocks(s) * B;
    if (max_blocks > 0x7fffffffull) { glp_set_err(c, "glp_merkle_batch: a launch of %llu workgroups", (unsigned long long)max_blocks); return GLP_E_UNSUPPORTED; }
    const dim3 blk(256);
    const u64 stride = poly_major ? poly_stride : (u64)leaf_len;
    {
        const dim3 g((unsigned)(leaf_bpt * B));
        const u32 bpt = (u32)leaf_bpt;
        if (h->small_mds) {
            if (poly_major) hipLaunchKernelGGL((glp_hash_leaves_batch_kernel<true, true>), g, blk, 0, c->stream, d_src, src_tree_stride, stride, leaf_len, nl, bpt, d_digests, digest_tree_stride, k);
            else hipLaunchKernelGGL((glp_hash_leaves_batch_kernel<true, false>), g, blk, 0, c->stream, d_src, src_tree_stride, stride, leaf_len, nl, bpt, d_digests, digest_tree_stride, k);
        } else {
            if (poly_major) hipLaunchKernelGGL((glp_hash_leaves_batch_kernel<false, true>), g, blk, 0, c->stream, d_src, src_tree_stride, stride, leaf_len, nl, bpt, d_digests, digest_tree_stride, k);
            else hipLaunchKernelGGL((glp_hash_leaves_batch_kernel<false, false>), g, blk, 0, c->stream, d_src, src_tree_stride, stride, leaf_len, nl, bpt, d_digests, digest_tree_stride, k);
        }
        GLP_HIPCHK(c, hipGetLastError());
    }
    for (const glp_merkle_step& s : steps) {
        const u32 bpt = (u32)glp_merkle_step_blocks(s);
        const dim3 g((unsigned)((u64)bpt * B));
        const u64 in_off = glp_merkle_level_offset(log_leaves, s.in_log);
        if (s.fused) {
            if (h->small_mds) hipLaunchKernelGGL(glp_merkle_subtree_kernel<true>, g, blk, 0, c->stream, d_digests, digest_tree_stride, in_off, s.in_log, s.s_log, s.n_levels, bpt, k);
            else hipLaunchKernelGGL(glp_merkle_subtree_kernel<false>, g, blk, 0, c->stream, d_digests, digest_tree_stride, in_off, s.in_log, s.s_log, s.n_levels, bpt, k);
        } else {
            const u64 count = 1ull << (s.in_log - 1);
            if (h->small_mds) hipLaunchKernelGGL(glp_merkle_level_batch_kernel<true>, g, blk, 0, c->stream, d_digests, digest_tree_stride, in_off, count, bpt, k);
            else hipLaunchKernelGGL(glp_merkle_level_batch_kernel<false>, g, blk, 0, c->stream, d_digests, digest_tree_stride, in_off, count, bpt, k);
        }
        GLP_HIPCHK(c, hipGetLastError());
    }
    if (h_caps) {     // the B caps sit one digest_tree_stride apart: one strided copy
        const size_t cap_bytes = (size_t)32 << cap_h;
        GLP_HIPCHK(c, hipMemcpy2DAsync(h_caps, cap_bytes, d_digests + glp_merkle_level_offset(log_leaves, cap_h), digest_tree_stride * 8, cap_bytes, B,
                                       hipMemcpyDeviceToHost, c->stream));
        GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GLP_OK;
}

extern "C" int glp_commit_values_batch(glp_ctx* c, uint64_t* d_vals, uint32_t n_polys, uint32_t log_n, uint32_t rate_bits, uint32_t cap_h, uint32_t B,
                                       uint64_t* d_lde, uint64_t* d_digests, uint64_t digest_tree_stride, uint64_t* h_caps) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (B == 0) return GLP_OK;
    const u32 log_N = log_n + rate_bits;
    if (!d_vals || !d_lde || !d_digests || n_polys == 0 || log_n > 32 || rate_bits > 8 || cap_h > log_N || (u64)B * n_polys > 0xffffffffull) {
        glp_set_err(c, "glp_commit_values_batch: bad argument");
        return GLP_E_INVALID;
    }
    const u32 rows = B * n_polys;
    int rc = glp_ntt(c, d_vals, log_n, rows, 1);
    if (rc) return rc;
    rc = glp_lde_coset(c, d_vals, d_lde, log_n, rate_bits, rows, 7, GLP_NTT_BITREV);
    if (rc) return rc;
    const u64 N = 1ull << log_N;
    return glp_merkle_batch(c, d_lde, (u64)n_polys * N, 1, N, n_polys, log_N, cap_h, B, GLP_MERKLE_FUSE_DEFAULT, d_digests, digest_tree_stride, h_caps);
}

extern "C" int glp_fri_fold2(glp_ctx* c, const uint64_t* d_evals, uint64_t* d_out, uint32_t log_n, uint64_t shift,
                             const uint64_t* h_beta) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (!d_evals || !d_out || !h_beta || log_n == 0 || log_n > 32 || shift == 0 || shift >= GL_P || h_beta[0] >= GL_P || h_beta[1] >= GL_P) {
        glp_set_err(c, "glp_fri_fold2: bad argument");
        return GLP_E_INVALID;
    }
    const u64* lo = nullptr; const u64* hi = nullptr;
    int rc = glp_ntt_table(c, (int)log_n, 1, &lo, &hi);
    if (rc) return rc;
    const u64 half = 1ull << (log_n - 1);
    const u64 half_inv = gl_inv(2), cc = gl_inv(gl_mul(2, shift));
    hipLaunchKernelGGL(glp_fri_fold2_kernel<0>, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, c->stream, d_evals, d_out, log_n,
                       half_inv, cc, gl_ext2{h_beta[0], h_beta[1]}, lo, hi);
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

static int ensure_sha_tables(glp_ctx* c) {
    glp_hash_state* h = hs(c);
    if (h->d_k256) return GLP_OK;
    GLP_HIPCHK(c, hipMalloc((void**)&h->d_k256, sizeof(K256)));
    GLP_HIPCHK(c, hipMemcpy(h->d_k256, K256, sizeof(K256), hipMemcpyHostToDevice));
    GLP_HIPCHK(c, hipMalloc((void**)&h->d_k512, sizeof(K512)));
    GLP_HIPCHK(c, hipMemcpy(h->d_k512, K512, sizeof(K512), hipMemcpyHostToDevice));
    return GLP_OK;
}

extern "C" int glp_sha256_trace(glp_ctx* c, const uint8_t* d_blocks, uint64_t n_msgs, uint32_t bpm, uint32_t* d_digests,
                                uint32_t* d_trace) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if ((!d_blocks || !d_digests) && n_msgs) { glp_set_err(c, "glp_sha256_trace: null buffer"); return GLP_E_INVALID; }
    if (n_msgs == 0) return GLP_OK;
    if (bpm == 0 || (n_msgs + 63) / 64 > 0x7fffffffull) { glp_set_err(c, "glp_sha256_trace: bad size"); return GLP_E_INVALID; }
    int rc = ensure_sha_tables(c);
    if (rc) return rc;
    hipLaunchKernelGGL(glp_sha256_trace_kernel<0>, dim3((unsigned)((n_msgs + 63) / 64)), dim3(64), 0, c->stream, d_blocks, n_msgs, bpm,
                       d_digests, d_trace, c->hash->d_k256);
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

extern "C" int glp_sha512_trace(glp_ctx* c, const uint8_t* d_blocks, uint64_t n_msgs, uint32_t bpm, uint64_t* d_digests,
                                uint64_t* d_trace) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if ((!d_blocks || !d_digests) && n_msgs) { glp_set_err(c, "glp_sha512_trace: null buffer"); return GLP_E_INVALID; }
    if (n_msgs == 0) return GLP_OK;
    if (bpm == 0 || (n_msgs + 63) / 64 > 0x7fffffffull) { glp_set_err(c, "glp_sha512_trace: bad size"); return GLP_E_INVALID; }
    int rc = ensure_sha_tables(c);
    if (rc) return rc;
    hipLaunchKernelGGL(glp_sha512_trace_kernel<0>, dim3((unsigned)((n_msgs + 63) / 64)), dim3(64), 0, c->stream, d_blocks, n_msgs, bpm,
                       d_digests, d_trace, c->hash->d_k512);
    GLP_HIPCHK(c, hipGetLastError());
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
    int rc = ensure_sha_tables(c);
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

// Ed25519 verification witness for a batch of signatures (row a10): pubs [n][32], sigs [n][64],
// msgs [n][msg_stride] with lens[n] (all device); out [n][GLP_ED25519_RECORD_WORDS] u64.
extern "C" int glp_ed25519_witness(glp_ctx* c, const uint8_t* d_pubs, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_stride,
                                   const uint32_t* d_lens, uint64_t n, uint64_t* d_out) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if ((!d_pubs || !d_sigs || !d_msgs || !d_lens || !d_out) && n) { glp_set_err(c, "glp_ed25519_witness: null buffer"); return GLP_E_INVALID; }
    if (n == 0) return GLP_OK;
    if (msg_stride == 0 || n > (1ull << 30)) { glp_set_err(c, "glp_ed25519_witness: bad size"); return GLP_E_INVALID; }
    int rc = ensure_sha_tables(c);
    if (rc) return rc;
    hipLaunchKernelGGL(glp_ed25519_witness_kernel<0>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, d_pubs, d_sigs, d_msgs, msg_stride,
                       d_lens, n, c->hash->d_k512, d_out);
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

// ---- the signature leaf's input vectors on the device (ed25519_inputs.cuh) --------------------------------------------------------------------
#include "ed25519_inputs.cuh"
static_assert(GLP_ED_IN_OK == GLP_ED25519_IN_OK && GLP_ED_IN_REJECT == GLP_ED25519_IN_REJECT && GLP_ED_IN_NO_PAIR == GLP_ED25519_IN_NO_PAIR &&
              GLP_ED_IN_INVALID == GLP_ED25519_IN_INVALID && GLP_ED_FORM_PLAIN == GLP_ED25519_FORM_PLAIN &&
              GLP_ED_FORM_FLAGGED == GLP_ED25519_FORM_FLAGGED && GLP_ED_FORM_VOTE == GLP_ED25519_FORM_VOTE && GLP_ED_REC == GLP_ED25519_RECORD_WORDS,
              "glprover.h and ed25519_inputs.cuh name the same codes");

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
    int rc = ensure_sha_tables(c);
    if (rc) return rc;
    GlpPoolBuf recs(c), stat(c);
    if (recs.alloc((size_t)n * GLP_ED_REC * sizeof(u64)) != hipSuccess || stat.alloc((size_t)n * sizeof(int32_t)) != hipSuccess) return GLP_E_HIP;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    hipLaunchKernelGGL(glp_ed25519_witness_kernel<0>, grid, block, 0, c->stream, d_pubs, d_sigs, d_msgs, msg_stride, d_lens, n, c->hash->d_k512, recs.u());
    GlpEdInputsArgs a;
    a.pubs = d_pubs; a.sigs = d_sigs; a.msgs = d_msgs; a.lens = d_lens; a.flags = d_flags; a.dummy = d_dummy; a.recs = recs.u();
    a.k512 = c->hash->d_k512; a.out = d_inputs; a.status = (int32_t*)stat.p; a.n = n; a.out_stride = input_stride; a.msg_stride = msg_stride;
    a.form = layout->form; a.lo = layout->msg_len_min; a.hi = layout->msg_len_max; a.split = layout->split_scalars ? 1u : 0u;
    hipLaunchKernelGGL(glp_ed25519_leaf_inputs_kernel<0>, grid, block, 0, c->stream, a);
    c->ed_input_counts[0] = 2;
    GLP_HIPCHK(c, hipGetLastError());
    GLP_HIPCHK(c, hipMemcpyAsync(h_status, stat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->ed_input_counts[1] = 1;
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    return GLP_OK;
}

extern "C" int glp_ed25519_last_input_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    if (!c || !n_launches || !n_host_syncs) return GLP_E_INVALID;
    *n_launches = c->ed_input_counts[0];
    *n_host_syncs = c->ed_input_counts[1];
    return GLP_OK;
}

extern "C" int glp_ed25519_half_scalars(glp_ctx* c, const uint64_t* d_k, uint64_t n, uint64_t* d_out) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if ((!d_k || !d_out) && n) { glp_set_err(c, "glp_ed25519_half_scalars: null buffer"); return GLP_E_INVALID; }
    if (n == 0) return GLP_OK;
    if (n > (1ull << 30)) { glp_set_err(c, "glp_ed25519_half_scalars: bad size"); return GLP_E_INVALID; }
    hipLaunchKernelGGL(glp_ed25519_half_scalars_kernel<0>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, d_k, n, d_out);
    GLP_HIPCHK(c, hipGetLastError());
    return GLP_OK;
}

// ---- B Tendermint trees per call (tm_batch_kernels.cuh) and the header-chain leaf's input vectors (chain_inputs.cuh) -------------------------
#include "chain_inputs.cuh"
static_assert(GLP_CHAIN_OK == GLP_HEADER_CHAIN_OK && GLP_CHAIN_BAD_LINK == GLP_HEADER_CHAIN_BAD_LINK &&
              GLP_CHAIN_BAD_HEIGHT == GLP_HEADER_CHAIN_BAD_HEIGHT && GLP_CHAIN_BAD_DATA_FIELD == GLP_HEADER_CHAIN_BAD_DATA_FIELD &&
              GLP_CHAIN_FIELDS == sizeof(((glp_header_chain_layout*)0)->field_len) / sizeof(uint32_t),
              "glprover.h and chain_inputs.cuh name the same codes");

// the two launches over a.total_leaves leaves and a.n_trees (> 0) trees none of which has more than max_tree leaves; a.nodes is set here
static int tm_batch_launch(glp_ctx* c, GlpTmBatchArgs& a, u64 max_tree, GlpPoolBuf& nodes, uint32_t* launches) {
    if (a.n_trees > 0x7fffffffull || a.total_leaves > (1ull << 36)) { glp_set_err(c, "glp_tm_merkle_root_batch: too many trees or leaves"); return GLP_E_UNSUPPORTED; }
    int rc = ensure_sha_tables(c);
    if (rc) return rc;
    if (nodes.alloc((size_t)(a.total_leaves ? a.total_leaves : 1) * 32) != hipSuccess) return GLP_E_NOMEM;
    a.nodes = (u32*)nodes.p;
    a.k256 = c->hash->d_k256;
    if (a.total_leaves) {
        hipLaunchKernelGGL(glp_tm_batch_leaf_kernel<0>, dim3((unsigned)((a.total_leaves + 255) / 256)), dim3(256), 0, c->stream, a);
        (*launches)++;
    }
    if (max_tree <= 2 * GLP_TM_BATCH_LANES_SMALL)
        hipLaunchKernelGGL(glp_tm_batch_fold_kernel<GLP_TM_BATCH_LANES_SMALL>, dim3((unsigned)a.n_trees), dim3(GLP_TM_BATCH_LANES_SMALL), 0, c->stream, a);
    else
        hipLaunchKernelGGL(glp_tm_batch_fold_kernel<GLP_TM_BATCH_LANES>, dim3((unsigned)a.n_trees), dim3(GLP_TM_BATCH_LANES), 0, c->stream, a);
    (*launches)++;
    GLP_HIPCHK(c, hipGetLastError());
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
    u64 max_tree = 0;
    for (u64 t = 0; t < n_trees; t++) max_tree = h_tree_first[t + 1] - h_tree_first[t] > max_tree ? h_tree_first[t + 1] - h_tree_first[t] : max_tree;
    // the kernels read the checked words themselves: uploaded here, stream-ordered, into scratch of the ctx
    GlpPoolBuf nodes(c), arrays(c);
    const size_t n_off = (size_t)total_leaves + 1, n_first = (size_t)n_trees + 1;
    if (arrays.alloc((n_off + n_first) * 8) != hipSuccess) return GLP_E_NOMEM;
    GLP_HIPCHK(c, hipMemcpyAsync(arrays.u(), h_leaf_offsets, n_off * 8, hipMemcpyHostToDevice, c->stream));
    GLP_HIPCHK(c, hipMemcpyAsync(arrays.u() + n_off, h_tree_first, n_first * 8, hipMemcpyHostToDevice, c->stream));
    GlpTmBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.data = d_data; a.leaf_off = arrays.u(); a.tree_first = arrays.u() + n_off; a.n_trees = n_trees; a.total_leaves = total_leaves; a.roots = d_roots;
    int rc = tm_batch_launch(c, a, max_tree, nodes, &c->tm_batch_counts[0]);
    if (rc) return rc;
    if (h_roots) {
        GLP_HIPCHK(c, hipMemcpyAsync(h_roots, d_roots, (size_t)n_trees * 32, hipMemcpyDeviceToHost, c->stream));
        c->tm_batch_counts[1] = 1;
        GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GLP_OK;
}

extern "C" int glp_tm_merkle_root_batch_last_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    if (!c || !n_launches || !n_host_syncs) return GLP_E_INVALID;
    *n_launches = c->tm_batch_counts[0];
    *n_host_syncs = c->tm_batch_counts[1];
    return GLP_OK;
}

extern "C" int glp_tm_merkle_root_batch_host(const uint8_t* data, uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* tree_first,
                                             uint64_t total_leaves, uint64_t n_trees, uint8_t* roots) {
    if (n_trees == 0) return GLP_OK;
    if (!leaf_offsets || !tree_first || !roots || (!data && data_len)) return GLP_E_INVALID;
    const int bad = glp_tm_batch_check(leaf_offsets, tree_first, total_leaves, n_trees, data_len);
    if (bad) return bad == 1 ? GLP_E_INVALID : GLP_E_UNSUPPORTED;
    GlpTmBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.data = data; a.leaf_off = leaf_offsets; a.tree_first = tree_first; a.n_trees = n_trees; a.total_leaves = total_leaves; a.roots = roots; a.k256 = K256;
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
    int rc = ensure_sha_tables(c);
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
        if (total_leaves) {
            GlpTmBatchArgs b;
            memset(&b, 0, sizeof(b));
            b.data = d_data; b.leaf_off = arrays.u(); b.tree_first = f->d_tree_first; b.n_trees = n_trees; b.total_leaves = total_leaves;
            b.nodes = f->slab; b.roots = f->roots; b.k256 = a.k256;
            hipLaunchKernelGGL(glp_tm_batch_leaf_kernel<0>, dim3((unsigned)((total_leaves + 255) / 256)), dim3(256), 0, c->stream, b);
            c->tm_forest_counts[0]++;
        }
        for (size_t l = 0; l < n_lvl; l++) {
            a.level = (u32)l;
            a.level_pre = arrays.u() + n_off + l * n_first;
            const u64 items = f->plan.level_pre[l][n_trees];
            hipLaunchKernelGGL(glp_tm_forest_level_kernel<0>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, c->stream, a);
            c->tm_forest_counts[0]++;
        }
        a.level = f->plan.top_level;
        a.level_pre = nullptr;
        if (f->plan.top_width <= 2 * GLP_TM_BATCH_LANES_SMALL)
            hipLaunchKernelGGL(glp_tm_forest_top_kernel<GLP_TM_BATCH_LANES_SMALL>, dim3((unsigned)n_trees), dim3(GLP_TM_BATCH_LANES_SMALL), 0, c->stream, a);
        else
            hipLaunchKernelGGL(glp_tm_forest_top_kernel<GLP_TM_BATCH_LANES>, dim3((unsigned)n_trees), dim3(GLP_TM_BATCH_LANES), 0, c->stream, a);
        c->tm_forest_counts[0]++;
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
    hipLaunchKernelGGL(glp_tm_path_kernel<0>, dim3((unsigned)((n_queries + 255) / 256)), dim3(256), 0, c->stream, a);
    c->tm_forest_counts[0] = 1;
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
    int rc = ensure_sha_tables(c);
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
    hipLaunchKernelGGL(glp_tm_verify_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
    c->tm_forest_counts[0] = 1;
    GLP_HIPCHK(c, hipGetLastError());
    GLP_HIPCHK(c, hipMemcpyAsync(h_status, stat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->tm_forest_counts[1] = 1;
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    return GLP_OK;
}

extern "C" int glp_tm_forest_last_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    if (!c || !n_launches || !n_host_syncs) return GLP_E_INVALID;
    *n_launches = c->tm_forest_counts[0];
    *n_host_syncs = c->tm_forest_counts[1];
    return GLP_OK;
}

extern "C" int glp_tm_forest_proofs_host(const uint8_t* data, uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* tree_first,
                                         uint64_t total_leaves, uint64_t n_trees, const uint64_t* query_tree, const uint64_t* query_leaf,
                                         uint64_t n_queries, uint8_t* roots, uint8_t* aunts, uint32_t aunt_stride, uint32_t* n_aunts,
                                         uint8_t* leaf_hashes) {
    const int bad = glp_tm_forest_proofs_host_impl(data, data_len, leaf_offsets, tree_first, total_leaves, n_trees, query_tree, query_leaf, n_queries,
                                                   roots, aunts, aunt_stride, n_aunts, leaf_hashes, K256);
    return bad == 0 ? GLP_OK : bad == 1 ? GLP_E_INVALID : GLP_E_UNSUPPORTED;
}

extern "C" int glp_tm_verify_inclusion_batch_host(const uint8_t* roots, uint64_t n_roots, const uint32_t* root_of, const uint8_t* data,
                                                  uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* index, const uint64_t* total,
                                                  const uint8_t* aunts, uint32_t aunt_stride, const uint32_t* n_aunts, uint64_t n, int32_t* status) {
    return glp_tm_verify_inclusion_host_impl(roots, n_roots, root_of, data, data_len, leaf_offsets, index, total, aunts, aunt_stride, n_aunts, n,
                                             status, K256) ? GLP_E_INVALID : GLP_OK;
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
    int rc = tm_batch_launch(c, t, GLP_CHAIN_FIELDS, nodes, &c->chain_input_counts[0]);
    if (rc) return rc;
    hipLaunchKernelGGL(glp_header_chain_check_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(glp_header_chain_rows_kernel<0>, dim3((unsigned)n), dim3(64), 0, c->stream, a);
    c->chain_input_counts[0] += 2;
    GLP_HIPCHK(c, hipGetLastError());
    GLP_HIPCHK(c, hipMemcpyAsync(h_status, stat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->chain_input_counts[1] = 1;
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    return GLP_OK;
}

extern "C" int glp_header_chain_last_input_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    if (!c || !n_launches || !n_host_syncs) return GLP_E_INVALID;
    *n_launches = c->chain_input_counts[0];
    *n_host_syncs = c->chain_input_counts[1];
    return GLP_OK;
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
                                                  inputs, input_stride, hashes, status, K256) ? GLP_E_INVALID : GLP_OK;
}
