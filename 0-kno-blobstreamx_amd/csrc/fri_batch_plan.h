// fri_batch_plan.h — the shape rules, launch geometry and launch / synchronise counts of glp_fri_prove_batch (fri.hip), header-only and
// host-only: the product and the CPU emulation (tests/emu_fri_batch) take every grid from the functions below, so the two cannot drift.
//
// One call proves B openings of ONE shape.  Whatever B is, it issues (PoW ending in its first window)
//   launches = 3                                   powers, openings, combine
//            + sum over the L fold layers of (launches of glp_merkle_batch for that layer's tree + 1 fold launch)
//            + (pow_bits ? 1 : 0) + 1              proof of work, the one gather
//   synchronises = 1 (openings) + L (layer caps) + 1 (final codewords) + (pow_bits ? 1 : 0) + 1 (gather)
// with L = (log_n - final_poly_bits) / arity_bits committed layers (0 when log_n <= final_poly_bits); every further PoW window adds one
// launch and one synchronise.  The one-time build of a twiddle table (first use of a length on a ctx) is not part of a call's counts.
//
// Device-side descriptor table of one call (u64 words), written by the host, read by the kernels:
//   off_shape  [n_batches][2]             n_polys, open_mask                     (shared by the instances)
//   off_ptrs   [B][n_batches][3]          d_coeffs, d_lde, d_digests             then [L][2]: layer codeword slab, layer digest slab
//   off_pow    [B * n_points][pow_stride] lo[256][2] = z^j, hi[nhi][2] = z^(256 j)  (host-built, as build_zpowers builds them)
//   off_cmb    [B][cmb_stride]            Y[n_points][2], z[n_points][2], alpha^k [total_polys][2]   (second copy: alpha needs the openings)
// The words from off_ptrs on double as the base-pointer table of the gather.
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/glprover.h"
#include "merkle_plan.h"

#define GLP_FRI_BATCH_EVAL_CHUNK 4096u     // == GLP_EVAL_CHUNK (fri_kernels.cuh; checked in fri_batch_kernels.cuh)
#define GLP_FRI_BATCH_MAX_GRID 0x7fffffffull
#define GLP_GL_P 0xFFFFFFFF00000001ull

struct glp_fri_batch_layer {
    uint32_t log_len;          // the layer's codeword has 2^log_len extension elements
    uint32_t log_leaves;       // its tree: 2^(log_len - arity_bits) leaves of 2 << arity_bits words
    uint32_t cap_h;
    uint64_t digest_stride;    // words of one tree's digest block
    uint32_t merkle_launches;  // of glp_merkle_batch at the default fusion
};

struct glp_fri_batch_plan {
    uint32_t log_n, log_N, n_points, n_batches, arity_bits, L, final_bits, final_log_len, cap0;
    uint32_t total_polys;      // openings per instance: one per (point, polynomial opened there)
    uint32_t n_chunks;         // evaluation chunks per polynomial
    uint64_t pow_stride;       // words of one (instance, point) power table: 512 + 2 * nhi
    uint32_t pow_blocks;       // workgroups per z^j table
    uint64_t eval_blocks;      // workgroups per instance of the openings launch
    uint64_t combine_blocks;   // workgroups per instance of the combine launch
    uint64_t off_shape, off_ptrs, off_pow, off_cmb, cmb_stride, desc_words;
    uint64_t gather_words;     // words gathered per instance
    uint32_t n_launches, n_host_syncs;
    std::vector<glp_fri_batch_layer> layers;
};

// ---- launch geometry (workgroups of 256 lanes, 1-D grids; the instance / table index is blockIdx.x / blocks-per-instance) ------------
static inline uint32_t glp_fri_powers_blocks(uint64_t n) { const uint64_t b = (n + 255) / 256; return (uint32_t)(b > 4096 ? 4096 : b); }
static inline uint32_t glp_fri_eval_chunks(uint64_t n) { return (uint32_t)((n + GLP_FRI_BATCH_EVAL_CHUNK - 1) / GLP_FRI_BATCH_EVAL_CHUNK); }
static inline uint64_t glp_fri_combine_blocks(uint32_t log_N) { return ((1ull << log_N) / 4 + 255) / 256; }
static inline uint64_t glp_fri_fold_layer_blocks(uint32_t log_len, uint32_t arity_bits) { return ((1ull << (log_len - arity_bits)) + 255) / 256; }
static inline uint64_t glp_fri_pow_window(uint32_t pow_bits) {      // the window rule of glp_pow_grind
    uint64_t w = 4ull << pow_bits;
    if (w < (1ull << 16)) w = 1ull << 16;
    if (w > (1ull << 22)) w = 1ull << 22;
    return w;
}
static inline uint64_t glp_fri_gather_blocks(uint64_t n) { return (n + 255) / 256; }

// a * b <= limit without overflow
static inline bool glp_fri_mul_fits(uint64_t a, uint64_t b, uint64_t limit) { return ((unsigned __int128)a * b) <= (unsigned __int128)limit; }

// glp_fri_fold_layer_batch's argument rules: nullptr when acceptable
static inline const char* glp_fri_fold_layer_batch_check(uint64_t in_stride, uint64_t out_stride, uint32_t log_len, uint32_t arity_bits, uint64_t shift,
                                                         uint32_t B) {
    if (arity_bits < 1 || arity_bits > 5 || log_len < arity_bits || log_len > 32 || shift == 0 || shift >= GLP_GL_P) return "bad argument";
    const uint64_t in_words = 2ull << log_len, out_words = 2ull << (log_len - arity_bits);
    if (in_stride < in_words || out_stride < out_words) return "stride < one codeword";
    if ((in_stride | out_stride) & 1ull) return "strides must be even (16-byte accesses)";
    if (!glp_fri_mul_fits(glp_fri_fold_layer_blocks(log_len, arity_bits), B, GLP_FRI_BATCH_MAX_GRID)) return "a launch of more than 2^31 - 1 workgroups";
    // (B - 1) * stride + one codeword, in bytes, must fit 64 bits
    const unsigned __int128 in_fp = (unsigned __int128)(B ? B - 1 : 0) * in_stride + in_words, out_fp = (unsigned __int128)(B ? B - 1 : 0) * out_stride + out_words;
    if ((in_fp >> 61) || (out_fp >> 61)) return "footprint exceeds 2^64 bytes";
    return nullptr;
}

// The plan of one call.  n_polys may be NULL (every batch counted as one polynomial: the launch / synchronise counts do not depend on it).
// Returns nullptr, or what is wrong; *unsupported is set when the shape is valid but beyond the host interpolation (as glp_fri_prove).
static inline const char* glp_fri_batch_plan_make(const glp_fri_config* cfg, const uint32_t* n_polys, const uint32_t* open_masks, uint32_t n_batches,
                                                  uint32_t B, glp_fri_batch_plan& pl, bool* unsupported) {
    if (unsupported) *unsupported = false;
    if (!cfg || !open_masks || n_batches == 0) return "null argument";
    const uint32_t log_n = cfg->log_n, rb = cfg->rate_bits, a = cfg->arity_bits, fb = cfg->final_poly_bits;
    if (log_n < 2 || log_n > 26 || rb < 1 || rb > 6 || a < 1 || a > 5 || fb > log_n || cfg->num_queries == 0 || cfg->num_queries > 256 ||
        cfg->pow_bits > 32 || cfg->cap_height > 12 || cfg->shift == 0 || cfg->shift >= GLP_GL_P || cfg->n_points == 0 || cfg->n_points > 4)
        return "unsupported configuration";
    const uint32_t NP = cfg->n_points;
    for (uint32_t p = 0; p < NP; p++) if (cfg->point_mult[p] == 0 || cfg->point_mult[p] >= GLP_GL_P) return "bad point multiplier";
    pl.log_n = log_n; pl.log_N = log_n + rb; pl.n_points = NP; pl.n_batches = n_batches; pl.arity_bits = a;
    pl.cap0 = cfg->cap_height < pl.log_N ? cfg->cap_height : pl.log_N;
    uint64_t total = 0;
    bool p0 = false;
    for (uint32_t b = 0; b < n_batches; b++) {
        const uint32_t np = n_polys ? n_polys[b] : 1u;
        if (np == 0 || open_masks[b] == 0 || (open_masks[b] >> NP)) return "batch incomplete";
        p0 = p0 || (open_masks[b] & 1u);
        for (uint32_t p = 0; p < NP; p++) if ((open_masks[b] >> p) & 1u) total += np;
    }
    if (!p0) return "no batch is opened at point 0";
    if (total > 0xffffffffull) return "more than 2^32 openings";
    pl.total_polys = (uint32_t)total;
    pl.L = (log_n > fb) ? (log_n - fb) / a : 0;
    pl.final_bits = log_n - a * pl.L;
    pl.final_log_len = pl.final_bits + rb;
    if (pl.final_log_len > 12) { if (unsupported) *unsupported = true; return "final polynomial too large for host interpolation"; }
    const uint64_t n = 1ull << log_n, N = 1ull << pl.log_N;
    pl.n_chunks = glp_fri_eval_chunks(n);
    pl.pow_stride = 512 + 2 * ((n + 255) / 256);
    pl.pow_blocks = glp_fri_powers_blocks(n);
    pl.eval_blocks = total * pl.n_chunks;
    pl.combine_blocks = glp_fri_combine_blocks(pl.log_N);
    // grids: B times the per-instance workgroups
    if (!glp_fri_mul_fits((uint64_t)pl.pow_blocks * NP, B, GLP_FRI_BATCH_MAX_GRID) || !glp_fri_mul_fits(pl.eval_blocks, B, GLP_FRI_BATCH_MAX_GRID) ||
        !glp_fri_mul_fits(pl.combine_blocks, B, GLP_FRI_BATCH_MAX_GRID) || !glp_fri_mul_fits((N + 255) / 256, B, GLP_FRI_BATCH_MAX_GRID) ||
        !glp_fri_mul_fits(glp_fri_pow_window(cfg->pow_bits) / 256, B, GLP_FRI_BATCH_MAX_GRID))
        return "a launch of more than 2^31 - 1 workgroups";
    // layers
    pl.layers.clear();
    pl.n_launches = 3 + (cfg->pow_bits ? 1u : 0u) + 1;
    pl.n_host_syncs = 1 + pl.L + 1 + (cfg->pow_bits ? 1u : 0u) + 1;
    unsigned __int128 slab_words = (unsigned __int128)2 * N;           // codeword slabs + digest slabs, per instance
    uint32_t log_len = pl.log_N;
    pl.gather_words = 0;
    for (uint32_t b = 0; b < n_batches; b++) pl.gather_words += (uint64_t)cfg->num_queries * ((n_polys ? n_polys[b] : 1u) + 4ull * (pl.log_N - pl.cap0));
    for (uint32_t l = 0; l < pl.L; l++) {
        glp_fri_batch_layer ly;
        ly.log_len = log_len;
        ly.log_leaves = log_len - a;
        ly.cap_h = cfg->cap_height < ly.log_leaves ? cfg->cap_height : ly.log_leaves;
        ly.digest_stride = 4 * ((2ull << ly.log_leaves) - (1ull << ly.cap_h));
        std::vector<glp_merkle_step> steps;
        glp_merkle_plan_steps(ly.log_leaves, ly.cap_h, GLP_MERKLE_FUSE_DEFAULT, steps);
        ly.merkle_launches = 1 + (uint32_t)steps.size();
        pl.n_launches += ly.merkle_launches + 1;
        pl.gather_words += (uint64_t)cfg->num_queries * ((2ull << a) + 4ull * (ly.log_leaves - ly.cap_h));
        log_len -= a;
        slab_words += (2ull << log_len) + ly.digest_stride;
        pl.layers.push_back(ly);
    }
    // descriptor table
    pl.off_shape = 0;
    pl.off_ptrs = pl.off_shape + 2ull * n_batches;
    const unsigned __int128 ptr_words = (unsigned __int128)B * n_batches * 3 + 2ull * pl.L;
    const unsigned __int128 pow_words = (unsigned __int128)B * NP * pl.pow_stride;
    pl.cmb_stride = 4ull * NP + 2ull * total;
    const unsigned __int128 desc = (unsigned __int128)pl.off_ptrs + ptr_words + pow_words + (unsigned __int128)B * pl.cmb_stride;
    // everything the call allocates, in bytes: descriptor, z^j tables, partial sums, slabs, gather pairs and words
    const unsigned __int128 bytes = 8 * (desc + (unsigned __int128)B * NP * 2 * n + (unsigned __int128)B * pl.eval_blocks * 2 + (unsigned __int128)B * slab_words +
                                         (unsigned __int128)B * pl.gather_words * 3);
    if (bytes >> 63) return "footprint overflows";
    if (!glp_fri_mul_fits((pl.gather_words + 255) / 256 + 1, B, GLP_FRI_BATCH_MAX_GRID)) return "a launch of more than 2^31 - 1 workgroups";
    pl.off_pow = pl.off_ptrs + (uint64_t)ptr_words;
    pl.off_pow += pl.off_pow & 1ull;                                   // power tables and the combine block are read 16 bytes at a time
    pl.off_cmb = pl.off_pow + (uint64_t)pow_words;
    pl.desc_words = pl.off_cmb + (uint64_t)B * pl.cmb_stride;
    return nullptr;
}
