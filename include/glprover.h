/*
 * glprover.h — C ABI of the MI355X-native Goldilocks prover kernels (libglprover.so).
 *
 * This is the drop-in boundary SURVEY.md §8(b) defines.  The north_star asks for "Rust
 * calling the kernels through a thin extern-"C" FFI"; the reference mount
 * (/root/reference: `.gitignore:1`, `changelog.md:1-2`, nothing else) contains no FFI, no
 * Rust and no interface file, so for every entry point below the "reference interface it
 * replaces" is:  file:line NONE — absent from mount.  The upstream function each one
 * stands in for is given by NAME ONLY, recalled and unverified, so a
 * maintainer knows where the Rust binding of INTEGRATION.md would be called from.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative GLP_E* code
 *     and never aborts; glp_last_error(ctx) gives a ctx-owned message.
 *   - field elements are little-endian uint64, canonical (< p = 2^64 - 2^32 + 1), in and out.
 *   - pointers named d_* are device (HBM) pointers valid on the ctx's GPU; h_* are host.
 *   - one glp_ctx per GPU per process; a ctx is not thread-safe.  Work is enqueued on the
 *     ctx's HIP stream; functions without an _async suffix return after enqueueing and the
 *     results are ordered on that stream (call glp_sync before reading them on the host).
 *   - there is NO CPU fallback: without a usable gfx950 device glp_create fails, and nothing the prover
 *     computes has a host path.  The only host arithmetic in the library is what is host work by nature:
 *     the Fiat-Shamir transcript (a few hundred permutations with a serial dependency) and the VERIFIERS
 *     (glp_*_verify*), which a party without a GPU must be able to run.
 */
#ifndef GLPROVER_H
#define GLPROVER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLP_OK 0
#define GLP_E_INVALID -1     /* bad argument */
#define GLP_E_NODEVICE -2    /* no usable HIP device */
#define GLP_E_HIP -3         /* HIP runtime error (see glp_last_error) */
#define GLP_E_NOMEM -4
#define GLP_E_UNSUPPORTED -5
#define GLP_E_STATE -6       /* e.g. Poseidon constants not set */
#define GLP_E_REJECT -7      /* a verifier rejected the proof (reason: glp_last_error) */

#define GLP_NTT_INVERSE 1u   /* inverse transform, scaled by 1/n */
#define GLP_NTT_BITREV 2u    /* write outputs in bit-reversed index order */

typedef struct glp_ctx glp_ctx;

/* ---- context, memory, stream ------------------------------------------------------ */
int glp_create(glp_ctx** out, int device_id);
void glp_destroy(glp_ctx* ctx);
const char* glp_last_error(const glp_ctx* ctx);
const char* glp_version(void);
/* The two-adic subgroup this BUILD computes in (csrc/gl_field.cuh: GLP_TWO_ADIC_GENERATOR, an element of order 2^32, and GLP_W64_LOG2 with
 * generator^(2^26) = 2^GLP_W64_LOG2): every root of unity of every transform is a power of that generator.  Default 7^((p-1)/2^32), w_64 = 2^39;
 * `make -C csrc altgen` builds lib/libglprover_altgen.so on 7277203076849721926, w_64 = 2^3 (recalled as upstream's choice, unverified).
 * GLP_E_STATE when the compiled pair is inconsistent (glp_create then refuses too).  Either pointer may be NULL. */
int glp_field_params(uint64_t* two_adic_generator, uint32_t* w64_log2);
int glp_alloc(glp_ctx* ctx, void** d_ptr, size_t bytes);
int glp_free(glp_ctx* ctx, void* d_ptr);
int glp_h2d(glp_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);  /* synchronous */
int glp_d2h(glp_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);  /* synchronous */
int glp_sync(glp_ctx* ctx);
/* the prover drivers keep their temporaries in a ctx-owned pool (reused across proofs, no hipFree on
 * the hot path); this returns every cached block to the driver (GLP_POOL_CAP_MB caps the cache) */
int glp_trim_pool(glp_ctx* ctx);
/* A ctx may be driven by a host thread other than its creator (still one thread at a time per ctx); HIP's
 * current device is per thread, so such a thread calls this once before its first call on the ctx.
 * glp_plonk_setup / glp_plonk_prove / glp_fri_prove bind by themselves. */
int glp_bind_thread(glp_ctx* ctx);
/* adopt an external hipStream_t (e.g. torch's current stream); NULL restores the ctx's own.  The ctx's pool and NTT
 * scratch are reused in stream order, so the switch first WAITS for everything enqueued on the stream being left
 * (a host-side synchronise): work on the new stream never overlaps work still using those blocks on the old one. */
int glp_set_stream(glp_ctx* ctx, void* hip_stream);
/* HIP-event timer on the ctx's stream: start, enqueue work, stop -> elapsed milliseconds */
int glp_timer_start(glp_ctx* ctx);
int glp_timer_stop(glp_ctx* ctx, float* ms);

/* ---- field arithmetic (upstream name recalled: GoldilocksField) ------
 * element-wise on device arrays of n canonical elements: out[i] = a[i] (op) b[i].
 * op: 0 add, 1 sub, 2 mul, 3 a[i] * 2^(b[i] mod 192), 4 inverse of a[i] (0 -> 0).
 * ops 5..10 take ARBITRARY 64-bit words and expose the reduction primitives under the products
 * (results canonical): 5 (a*2^64 + b) mod p, 6 the same through the lazy form, 7 a*b for any
 * representatives, 8 (a>>7) + (b>>7)*2^32, 9/10 a + (b mod 2^32)*(2^32-1) lazy/canonical.
 * The prover never calls this; it exposes the exact device arithmetic of the kernels to
 * parity tests and to hosts that need a few field operations on resident data. */
int glp_field_op(glp_ctx* ctx, int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, uint64_t n);

/* ---- NTT / LDE (upstream names recalled: plonky2_field::fft::
 *      fft / ifft / coset_fft, PolynomialCoeffs::lde, fri::oracle::PolynomialBatch) ------ */
/* in place, natural order in and out:  X[k] = sum_j x[j] w_n^{jk},  w_n = 7^((p-1)/n) */
int glp_ntt(glp_ctx* ctx, uint64_t* d_io, uint32_t log_n, uint32_t batch, int inverse);
/* general form: src may equal dst; poly strides in elements (>= n); flags = GLP_NTT_* */
int glp_ntt_ex(glp_ctx* ctx, const uint64_t* d_src, uint64_t* d_dst, uint32_t log_n, uint32_t batch,
               uint64_t src_poly_stride, uint64_t dst_poly_stride, uint32_t flags);
/* coefficients [batch][n] -> evaluations [batch][n << rate_bits] on the coset shift*<w>:
 * zero-pad, scale coefficient j by shift^j, forward NTT.  flags: GLP_NTT_BITREV or 0 */
int glp_lde_coset(glp_ctx* ctx, const uint64_t* d_coeffs, uint64_t* d_out, uint32_t log_n, uint32_t rate_bits,
                  uint32_t batch, uint64_t shift, uint32_t flags);
/* [rows][cols] -> [cols][rows] (polynomial-major <-> leaf-major) */
int glp_transpose(glp_ctx* ctx, const uint64_t* d_in, uint64_t* d_out, uint64_t rows, uint64_t cols);
/* force the pass structure of subsequent NTTs of size 2^log_n ("r:c,r:c,..." log2 radix :
 * log2 columns per pass; NULL/"" = default heuristic).  Tuning/benchmark aid. */
int glp_ntt_set_plan(glp_ctx* ctx, uint32_t log_n, const char* plan);
/* describe the plan that would be used for this size and batch (for logs): NUL-terminated */
int glp_ntt_describe_plan(glp_ctx* ctx, uint32_t log_n, uint32_t batch, uint32_t flags, char* buf, size_t buf_len);
/* per-pass kernel times (ms) of the LAST glp_ntt*_ call when profiling is on; n_out <= 4 */
int glp_set_profiling(glp_ctx* ctx, int on);
int glp_last_pass_ms(glp_ctx* ctx, float* ms, int* n_out);
/* stage timing tree of the LAST glp_plonk_prove / glp_fri_prove while profiling is on (each stage
 * boundary then synchronises the stream): names are ';'-separated, *n_inout = capacity in, count out */
int glp_last_stage_ms(glp_ctx* ctx, char* names, size_t names_len, float* ms, int* n_inout);

/* ---- Poseidon / Merkle (row a4; upstream names recalled: plonky2::hash::poseidon,
 *      hashing::hash_n_to_hash_no_pad, PoseidonHash::two_to_one, merkle_tree::MerkleTree::new) */
/* rc: 360 round constants (30 rounds x 12), mds_circ: 12, mds_diag: 12.  Must be called
 * before any hashing entry point; the library ships no constants. */
int glp_set_poseidon_constants(glp_ctx* ctx, const uint64_t* h_rc, size_t n_rc, const uint64_t* h_mds_circ,
                               const uint64_t* h_mds_diag);
/* n_states independent width-12 permutations, in place, [n_states][12] */
int glp_poseidon_permute(glp_ctx* ctx, uint64_t* d_states, uint64_t n_states);
/* d_leaves: [2^log_leaves][leaf_len] (leaf-major).  d_digests receives every level from
 * the leaf digests down to the cap level: 4 * (2^(log_leaves+1) - 2^cap_h) u64.
 * h_cap (may be NULL) receives the 2^cap_h cap digests (4 u64 each) — synchronous if given. */
int glp_merkle(glp_ctx* ctx, const uint64_t* d_leaves, uint32_t leaf_len, uint32_t log_leaves, uint32_t cap_h,
               uint64_t* d_digests, uint64_t* h_cap);
/* same tree, but leaves given polynomial-major: d_polys [leaf_len][2^log_leaves]
 * (leaf i = column i), so the LDE output is hashed without a transpose pass */
int glp_merkle_from_polys(glp_ctx* ctx, const uint64_t* d_polys, uint64_t poly_stride, uint32_t leaf_len,
                          uint32_t log_leaves, uint32_t cap_h, uint64_t* d_digests, uint64_t* h_cap);
#define GLP_MERKLE_FUSE_DEFAULT 0xFFFFFFFFu
/* B trees of one shape.  Tree b reads d_src + b * src_tree_stride (u64 words): leaves as glp_merkle (poly_major = 0, poly_stride ignored)
 * or as glp_merkle_from_polys (poly_major = 1: [leaf_len][poly_stride]); its digests, in the layout of glp_merkle, go to
 * d_digests + b * digest_tree_stride.  h_caps (may be NULL): [B][4 << cap_h] words, ONE copy, synchronous if given.
 * fuse_max_log: levels of at most 2^fuse_max_log nodes per tree are built by the fused subtree kernel (up to 9 levels per launch),
 * wider ones one launch per level; GLP_MERKLE_FUSE_DEFAULT = the library's measured default; 0 = never fuse.
 * GLP_E_INVALID also for digest_tree_stride < 4 * ((2 << log_leaves) - (1 << cap_h)), a src_tree_stride smaller than one tree's leaves and
 * poly_major with poly_stride < 2^log_leaves; B == 0 is GLP_OK and does nothing.  Words of a digest block past the tree's length are left
 * alone.  GLP_COOP_MAX_NODES is not read.
 * Measured (profiles/merkle_batch.json; 2^19 leaves, cap 4): the default is 15 — 6 launches per CALL where glp_merkle takes 14 launches, a
 * copy and a synchronise per TREE; 12 - 14 % (144-word leaves) and 33 - 37 % (16-word leaves) less time than B = 4 / 8 sequential
 * glp_merkle_from_polys calls.  B = 1 gains nothing (+0.5 % and +0.04 %, inside the baseline's run-to-run spread): one tree should keep
 * calling glp_merkle. */
int glp_merkle_batch(glp_ctx* ctx, const uint64_t* d_src, uint64_t src_tree_stride, int poly_major, uint64_t poly_stride, uint32_t leaf_len,
                     uint32_t log_leaves, uint32_t cap_h, uint32_t B, uint32_t fuse_max_log, uint64_t* d_digests,
                     uint64_t digest_tree_stride, uint64_t* h_caps);
/* the launches glp_merkle_batch issues for that shape (leaf hashing included); host only, no ctx */
int glp_merkle_batch_plan(uint32_t log_leaves, uint32_t cap_h, uint32_t fuse_max_log, uint32_t* n_launches, uint32_t* n_fused);
/* d_vals [B * n_polys][2^log_n]: values in, coefficients out (in place); d_lde [B * n_polys][2^(log_n + rate_bits)], bit-reversed, coset
 * shift 7 — exactly what commit_values / PolynomialBatch.from_values produce per batch; then glp_merkle_batch over the B LDE blocks
 * (poly-major, leaf_len = n_polys) at the default fusion. */
int glp_commit_values_batch(glp_ctx* ctx, uint64_t* d_vals, uint32_t n_polys, uint32_t log_n, uint32_t rate_bits, uint32_t cap_h, uint32_t B,
                            uint64_t* d_lde, uint64_t* d_digests, uint64_t digest_tree_stride, uint64_t* h_caps);

/* ---- FRI (row a8; upstream name recalled: plonky2::fri::prover) -------------------- */
/* arity-2 fold of extension-field evaluations in bit-reversed order over shift*<w_{log_n}>:
 * d_evals [n][2] -> d_out [n/2][2];  h_beta = 2 u64 */
int glp_fri_fold2(glp_ctx* ctx, const uint64_t* d_evals, uint64_t* d_out, uint32_t log_n, uint64_t shift,
                  const uint64_t* h_beta);

/* ---- Fiat-Shamir challenger (row a5; upstream name recalled: plonky2::iop::challenger) ----
 * Poseidon duplex sponge (width 12, rate 8, overwrite mode) run on the HOST with the injected
 * constants: observing invalidates pending outputs; a challenge absorbs whatever is buffered
 * and pops outputs from the end of state[0..8).  Build-defined (transcript order unpinned). */
typedef struct glp_challenger glp_challenger;
int glp_challenger_new(glp_ctx* ctx, glp_challenger** out);
void glp_challenger_free(glp_challenger* ch);
int glp_challenger_observe(glp_challenger* ch, const uint64_t* h_elems, size_t n);
int glp_challenger_challenges(glp_challenger* ch, uint64_t* h_out, size_t n);

/* ---- FRI opening proof (rows a8, a12; upstream names recalled: fri::prover::fri_proof,
 *      PolynomialBatch::prove_openings).  Protocol + byte layout are build-defined: DESIGN.md §3.5 */
/* f_p(z) for n_polys coefficient-form polynomials (z in the quadratic extension, h_z = 2 u64):
 * h_out receives n_polys pairs */
int glp_eval_at_ext(glp_ctx* ctx, const uint64_t* d_coeffs, uint64_t poly_stride, uint32_t log_n, uint32_t n_polys,
                    const uint64_t* h_z, uint64_t* h_out);
/* smallest nonce with the top pow_bits bits of Poseidon(seed[0..4], nonce, 0...)[0] clear */
int glp_pow_grind(glp_ctx* ctx, const uint64_t* h_seed4, uint32_t pow_bits, uint64_t* h_nonce);

typedef struct {
    uint32_t log_n;            /* every committed polynomial has 2^log_n coefficients */
    uint32_t rate_bits;        /* LDE blow-up used when the batches were committed */
    uint32_t cap_height;       /* Merkle cap height of the batches and (clamped) of the fold layers */
    uint32_t arity_bits;       /* fold arity 2^arity_bits per committed layer */
    uint32_t final_poly_bits;  /* stop folding when the degree bound is <= 2^final_poly_bits (+ remainder) */
    uint32_t num_queries;
    uint32_t pow_bits;
    uint64_t shift;            /* coset shift of the LDE domain (7) */
    uint32_t n_points;         /* 1..4 opening points z_p = zeta * point_mult[p] (zeta from the transcript) */
    uint64_t point_mult[4];    /* base-field multipliers; {1} for a single point, {1, w_n} to also open the next row */
} glp_fri_config;
typedef struct {               /* one committed batch, as produced by ifft -> glp_lde_coset(BITREV) -> glp_merkle_from_polys */
    const uint64_t* d_coeffs;  /* [n_polys][2^log_n], dense */
    const uint64_t* d_lde;     /* [n_polys][2^(log_n+rate_bits)], bit-reversed evaluation order */
    const uint64_t* d_digests; /* Merkle digests of that LDE (layout of glp_merkle) */
    const uint64_t* h_cap;     /* its cap: 4 << min(cap_height, log_n+rate_bits) words (host) */
    uint32_t n_polys;
    uint32_t open_mask;        /* bit p set: every polynomial of the batch is opened at point p */
} glp_fri_batch;
/* proves the openings of the batches at the transcript-derived point(s) selected by open_mask.
 * *proof is malloc'd by the library (little-endian u64 words), free with glp_free_host. */
int glp_fri_prove(glp_ctx* ctx, const glp_fri_config* cfg, const glp_fri_batch* batches, uint32_t n_batches,
                  uint8_t** proof, size_t* proof_len);
void glp_free_host(void* p);

/* B opening proofs of ONE shape. batches: [B][n_batches], instance-major. For every batch index, n_polys and open_mask must be equal in
 * all instances; device pointers and caps are per instance (an instance may share a batch — e.g. a preprocessed commitment — with
 * others by pointing at the same memory). proofs[i] / proof_lens[i]: as glp_fri_prove gives for instance i alone, BYTE FOR BYTE.
 * All or nothing: on any error every proofs[i] is NULL, nothing is leaked, glp_last_error names the instance where one is at fault.
 * B == 0 is GLP_OK and does nothing.
 * The B transcripts advance in lock-step on the host; every device step is shared by the whole batch.  Whatever B is, one call issues
 *   launches     = 3 (z^j tables, openings, combine) + sum over the L fold layers of (glp_merkle_batch_plan launches of the layer's
 *                  tree of 2^(log_len - arity_bits) leaves, default fusion, + 1 fold launch) + (pow_bits ? 1 : 0) + 1 (the gather)
 *   synchronises = 1 (openings) + L (layer caps) + 1 (final codewords) + (pow_bits ? 1 : 0) + 1 (the gather)
 * with L = (log_n - final_poly_bits) / arity_bits (0 when log_n <= final_poly_bits), plus one launch and one synchronise for every
 * PoW window after the first.  glp_fri_prove's limits apply; GLP_E_INVALID also for shapes that differ between instances, a launch
 * of more than 2^31 - 1 workgroups and a footprint that overflows.  All temporaries come from the ctx pool and are held until the
 * call returns.  LDE rows are read 16 bytes at a time when every d_lde is 16-byte aligned (8-byte reads otherwise).
 * Measured (profiles/fri_batch.json; the 2^16 x 144 leaf's opening proof, medians of 20 alternating repeats, ms): B sequential glp_fri_prove calls
 * against one call here — B = 1: 2.860 / 2.316, B = 2: 5.711 / 3.284, B = 4: 11.461 / 5.525, B = 8: 23.083 / 10.843, B = 16: 45.965 / 20.489; every B
 * gains by more than the baseline's own spread (max - min 0.04 - 0.40 ms), B = 1 included (-19 %). */
int glp_fri_prove_batch(glp_ctx* ctx, const glp_fri_config* cfg, const glp_fri_batch* batches, uint32_t n_batches, uint32_t B,
                        uint8_t** proofs, size_t* proof_lens);
/* what one glp_fri_prove_batch call issues for that shape when every PoW search ends in its first window; host only, no ctx */
int glp_fri_prove_batch_plan(const glp_fri_config* cfg, const uint32_t* open_masks, uint32_t n_batches,
                             uint32_t* n_launches, uint32_t* n_host_syncs);
/* counts of the LAST glp_fri_prove_batch on this ctx (kernel launches, stream synchronises, PoW windows searched) */
int glp_fri_last_batch_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs, uint32_t* pow_windows);
/* B seeds [B][4] -> B nonces, each exactly what glp_pow_grind returns for that seed (same window rule: the smallest accepted nonce
 * of the first window that has one) */
int glp_pow_grind_batch(glp_ctx* ctx, const uint64_t* h_seeds, uint32_t B, uint32_t pow_bits, uint64_t* h_nonces);
/* one committed fold layer for B codewords: instance b reads d_in + b*in_stride ([2^log_len][2] words), writes d_out + b*out_stride
 * ([2^(log_len-arity_bits)][2]); equals arity_bits successive glp_fri_fold2 calls with beta, beta^2, beta^4.. and shift, shift^2..
 * d_in and d_out are 16-byte aligned and both strides even (16-byte accesses); arity_bits 1..5 <= log_len <= 32. */
int glp_fri_fold_layer_batch(glp_ctx* ctx, const uint64_t* d_in, uint64_t in_stride, uint64_t* d_out, uint64_t out_stride, uint32_t log_len,
                             uint32_t arity_bits, uint64_t shift, const uint64_t* h_betas /*[B][2]*/, uint32_t B);

/* ---- prover for the build-defined circuit (rows a6, a7 + driver; upstream names recalled:
 *      plonk::prover::prove, compute_partial_products_and_z_polys, compute_quotient_polys, gates::{arithmetic_base,
 *      constant, public_input, poseidon}).
 * Circuit: 2^log_n rows, n_wires columns of which the first n_routed take part in the permutation
 * argument (copy constraints through sigma; the others are advice wires).  Per-row constant columns, in this order:
 *   [0] q_arith [1] c0 [2] c1 [3] c2 [4] q_pi [5] q_pos          (GLP_PLONK_NCONST = 6)
 * Gates:
 *   arithmetic / constant   every group of 4 routed wires (x, y, z, w):  q_arith * (c0*x*y + c1*z + c2 - w) = 0
 *   public input            q_pi * wire_0 - PI(x) = 0: set q_pi = 1 on rows 0..n_public-1 — wire 0 of row i is public input i
 *   Poseidon (flag)         a q_pos row carries one permutation with the ctx's constants: wires 0..11 in, 12..23 out, 24 a swap bit s
 *                           (s = 1 exchanges in[0..4) and in[4..8) before the permutation: the Merkle-path step), 25..130 the S-box inputs of
 *                           the later rounds, 131..134 s * (in[4+i] - in[i]) (123 constraints of degree <= 7; fill wires 12..134 with
 *                           glp_poseidon_gate_fill_rows); set q_arith = 0 on such rows
 * d_const_vals: [6][n] row values; d_sigma_vals: [n_routed][n] with sigma_j(row i) = k_{j'} * w_n^{i'} for the cell (j', i')
 * that (j, i) maps to, k_j = 7^j.  rate_bits must be 3: the quotient has degree < 8n (permutation constraint degree 9,
 * Poseidon row degree 8), so 8 chunks on the 8n-point coset is exactly what fits; it is not a tunable. */
#define GLP_PLONK_NCONST 6
#define GLP_CIRCUIT_POSEIDON_GATE 1u
#define GLP_POS_GATE_WIRES 135
/*   SHA-256 rows (flag)     four more constant columns select the row kind — [6] q_she [7] q_sha [8] q_shw [9] q_add, so d_const_vals is
 *                           [GLP_PLONK_NCONST_SHA][n] for such a circuit — and one compression is 64 E rows (e-half of a round: T1 and the new e;
 *                           K_t in the row's c2), 64 A rows (the new a), 48 W rows (message schedule) and 2 ADD rows (the feed-forward; four
 *                           additions mod 2^32 per row, also the 32-bit range check).  Words are routed wires 0..11; wires 12..143 are the
 *                           row's own bit decompositions (fill them with glp_sha_gate_fill_rows); 140 constraints of degree <= 4; layouts
 *                           and equations: csrc/plonk_gates.h */
#define GLP_PLONK_NCONST_SHA 10
#define GLP_CIRCUIT_SHA_GATES 2u
/*   extension rows (flag)   one more constant column, q_ext, LAST (index 6, or 10 with the SHA selectors): on a q_ext row every chunk of 8 routed
 *                           wires (x0, x1, y0, y1, z0, z1, w0, w1) is w = x * y + z in F_p[X]/(X^2 - 7); no further constraints (the two
 *                           values share the chunk's arithmetic-gate slots).  d_const_vals then has glp n_const = 6 + 4 (SHA) + 1 rows */
#define GLP_CIRCUIT_EXT_GATE 4u
#define GLP_SHA_GATE_WIRES 144
#define GLP_SHA_ROW_E 0
#define GLP_SHA_ROW_A 1
#define GLP_SHA_ROW_W 2
#define GLP_SHA_ROW_ADD 3
typedef struct {
    uint32_t log_n;        /* 3..24 */
    uint32_t n_wires;      /* multiple of 8, <= 160 */
    uint32_t n_routed;     /* multiple of 8, 8..n_wires */
    uint32_t n_public;     /* <= 2^log_n */
    uint32_t rate_bits;    /* 3 */
    uint32_t cap_height;   /* <= 12 */
    uint32_t flags;        /* GLP_CIRCUIT_POSEIDON_GATE: needs n_wires >= GLP_POS_GATE_WIRES and n_routed >= 24;
                              GLP_CIRCUIT_SHA_GATES: n_wires >= GLP_SHA_GATE_WIRES, n_routed >= 16, ten constant columns */
} glp_circuit_shape;
typedef struct glp_plonk_circuit glp_plonk_circuit;
int glp_plonk_setup_ex(glp_ctx* ctx, const glp_circuit_shape* shape, const uint64_t* d_const_vals, const uint64_t* d_sigma_vals,
                       glp_plonk_circuit** out);
/* the round-1 form: every wire routed, no public inputs, no Poseidon rows, d_const_vals [3][n] = (q, c0, c1) */
int glp_plonk_setup(glp_ctx* ctx, uint32_t log_n, uint32_t n_wires, const uint64_t* d_const_vals, const uint64_t* d_sigma_vals,
                    uint32_t rate_bits, uint32_t cap_height, glp_plonk_circuit** out);
void glp_plonk_free(glp_plonk_circuit* ck);
/* d_wire_vals: [n_wires][n] witness values; h_public: n_public canonical words (NULL when the circuit has none).
 * Proof (little-endian u64 words): header (tag, log_n, n_wires, n_routed, rate_bits, cap_height, n_public, flags), the
 * public inputs, four caps, then the FRI opening proof (all batches at zeta, the Z batch also at w_n*zeta).  Header, public
 * inputs and the circuit's cap enter the transcript before the wires cap.  Free with glp_free_host. */
int glp_plonk_prove_ex(glp_ctx* ctx, glp_plonk_circuit* ck, const uint64_t* d_wire_vals, const uint64_t* h_public, uint32_t num_queries,
                       uint32_t pow_bits, uint8_t** proof, size_t* proof_len);
int glp_plonk_prove(glp_ctx* ctx, glp_plonk_circuit* ck, const uint64_t* d_wire_vals, uint32_t num_queries, uint32_t pow_bits,
                    uint8_t** proof, size_t* proof_len);
/* B proofs of ONE circuit.  d_wire_vals: B device pointers, each a [n_wires][n] witness (read only; two instances may point at the same
 * matrix); h_public: [B][n_public] canonical words (NULL when the circuit has none).  proofs[i] / proof_lens[i]: as glp_plonk_prove_ex gives
 * for instance i alone, BYTE FOR BYTE.  All or nothing: on any error every proofs[i] is NULL, nothing is leaked from the ctx pool, and
 * glp_last_error names the instance where one is at fault.  B == 0 is GLP_OK and does nothing.  glp_plonk_prove_ex's argument limits
 * apply; GLP_E_UNSUPPORTED for a B whose launches would exceed 2^31 - 1 workgroups; GLP_E_NOMEM when the pool cannot hold the footprint.
 * The B transcripts advance in lock-step on the host; every device step is issued once for the whole batch: one gather of the B wire
 * matrices into a [B*W][n] slab, glp_commit_values_batch (wires), K6 over the batch, glp_commit_values_batch (Z and partial products),
 * the public-input slab (one inverse NTT, one LDE), K7 (and K7s) over the batch, un-bit-reversal / inverse NTT / unshift of the B*2
 * quotients, one LDE, glp_merkle_batch, then the batched opening proof (glp_fri_prove_batch's driver on the B challengers).
 * Whatever B is, the driver's OWN code issues (glp_plonk_last_batch_counts)
 *   launches     = 1 (wire gather) + 4 (K6: chunk quotients, scan reduce, scan blocks, scan apply) + 1 (K7)
 *                  + (SHA rows ? 1 : 0) (K7s) + 1 (un-bit-reversal) + 1 (unshift)          = 8, or 9 with SHA rows
 *   synchronises = 0 — the caps come back with the one synchronise of each of the three commitment calls
 * and 3 + (n_public ? 1 : 0) + 1 host-to-device copies (descriptor table per stage, public inputs, unshift table).  The NTT, LDE and Merkle
 * calls and the opening proof are counted by their own plans (glp_merkle_batch_plan, glp_fri_last_batch_counts).
 * Device footprint, held from the pool until the call returns, in bytes, with n = 2^log_n, N = 8n, W wires, R routed, M = R / 8 and
 * D = 4 * (2N - 2^cap) digest words per tree:
 *   8 * B * ( n * (W + 2M) + N * (W + 2M + 2 + 16) + 3 * D )        coefficients and LDEs of the three batches, their digests
 * plus, transiently, 8 * B * n * (2M + 2) during K6 and 8 * B * (2N + (n_public ? n + N : 0)) during K7, plus the opening proof's own.
 * A 2^16 x 144 leaf (R = 80) holds 0.60 GB of wire LDE and 0.95 GB in all per instance.
 * Measured (profiles/plonk_batch.json; the 2^16 x 144 data-commitment leaf, 28 queries, 16 PoW bits, medians of 12 alternating repeats, ms): B sequential
 * glp_plonk_prove_ex calls against one call here — B = 1: 12.10 / 11.56, B = 2: 24.22 / 19.69, B = 4: 48.43 / 35.56, B = 8: 96.94 / 67.45; every B gains by
 * more than the baseline's own spread (max - min 0.49 - 2.48 ms).  The Map step of 64 such leaves: 575 ms on three ctxs unbatched, 570 ms on one ctx
 * and 499 ms on three ctxs with groups of 8. */
int glp_plonk_prove_batch(glp_ctx* ctx, glp_plonk_circuit* ck, const uint64_t* const* d_wire_vals, const uint64_t* h_public, uint32_t B,
                          uint32_t num_queries, uint32_t pow_bits, uint8_t** proofs, size_t* proof_lens);
/* what the PLONK driver's own code issued in the LAST glp_plonk_prove_batch on this ctx: kernel launches and stream synchronises */
int glp_plonk_last_batch_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs);
/* witness generation for Poseidon rows: for each of the n_rows row indices in d_rows (device, u32), wires 12..23 and 25..134 of that row
 * are computed from its wires 0..11 and its swap bit (wire 24), in place in d_wire_vals [n_wires][2^log_n].  Stream-ordered. */
int glp_poseidon_gate_fill_rows(glp_ctx* ctx, uint64_t* d_wire_vals, uint32_t log_n, uint32_t n_wires, const uint32_t* d_rows,
                                uint32_t n_rows);
/* witness generation for SHA rows: for row d_rows[k] of kind d_kinds[k] (GLP_SHA_ROW_*; both device, u32) the bit wires 12..143 are computed
 * from the routed words in wires 0..11 (inputs AND outputs of the row: the witness program computed the outputs), in place.  Stream-ordered. */
int glp_sha_gate_fill_rows(glp_ctx* ctx, uint64_t* d_wire_vals, uint32_t log_n, uint32_t n_wires, const uint32_t* d_rows,
                           const uint32_t* d_kinds, uint32_t n_rows);

/* Parity hook for rows a6 / a7: the prover's intermediate stages for CALLER-CHOSEN challenges, so the HIP output can be
 * compared directly with an independent restatement (tests/plonk_ref.py) and not only through accepted proofs.
 *   GLP_DEBUG_ZS:       h_challenges = beta[2], gamma[2];           d_out [2*M][n]  Z then the M-1 partial products per
 *                       challenge, values on the trace domain (M = n_routed / 8)
 *   GLP_DEBUG_QUOTIENT: h_challenges = beta[2], gamma[2], alpha[2]; d_out [2][8n]   quotient evaluations on the coset
 *                       7*<w_8n>, bit-reversed index order (before the division into chunks)
 * Synchronous.  The prover itself never calls it. */
#define GLP_DEBUG_ZS 0
#define GLP_DEBUG_QUOTIENT 1
int glp_plonk_debug_stage(glp_ctx* ctx, glp_plonk_circuit* ck, const uint64_t* d_wire_vals, const uint64_t* h_public, int which,
                          const uint64_t* h_challenges, uint64_t* d_out);

/* ---- witness checker: does a wire matrix satisfy the circuit the key commits to, and if not, where (opt-in; the prover never calls it) ----
 * Evaluated on every row i of the trace domain, natural order, with the KEY's constants and sigmas (the constant columns come back from the
 * preprocessed commitment's coefficients by one forward NTT into a transient buffer; nothing is taken from the caller):
 *   GLP_CHECK_GATE  index = the constraint's number in the quotient's alpha order: 1 the public input  q_pi * wire_0 - PI(i)  (PI(i) =
 *                   h_public[i] for i < n_public, else 0); 3+3c, 4+3c the two arithmetic / extension slots of chunk c (q_arith * gate +
 *                   q_ext * e); 2+3M+k Poseidon constraint k times q_pos (M = n_routed / 8; the small-integer-MDS body when the ctx's MDS is
 *                   small, as the prover's quotient kernel chooses); then the 140 selector-weighted SHA slots
 *   GLP_CHECK_COPY  index = routed wire j: cell (j, row) differs from the cell sigma sends it to — the copy constraints tested directly
 * Not evaluated: L_1 (Z - 1) (index 0) and the permutation-chunk constraints (index 2+3c) need Z; the direct copy check stands in their place.
 * sum: the counts.  list (may be NULL when max_list == 0): one entry per failing row and kind, carrying that row's LOWEST failing index,
 * ascending by (row, kind), at most max_list entries (n_listed of them written); the same input always gives the same list.
 * Single form: GLP_OK when every constraint holds, GLP_E_REJECT when not (sum, list and glp_last_error name the first violation).
 * Batch form: B witnesses of one key in the same launches; GLP_OK when it ran, the verdict of instance b in h_status[b] (GLP_OK / GLP_E_REJECT),
 * sums[b], lists[b * max_list ..].  Argument rules as glp_plonk_prove_batch: B == 0 is GLP_OK and does nothing, two instances may point at the
 * same matrix, GLP_E_INVALID for a null argument or a non-canonical public input (glp_last_error names the instance), GLP_E_UNSUPPORTED for
 * B > 65535 (the instance is a grid dimension), GLP_E_STATE for a Poseidon circuit on a ctx without constants.
 * The key's FIRST check decodes its sigma values (k_j' * w_n^i', with the ctx's roots of unity) into cell indices, one u32 per routed cell:
 * 4 * n_routed * n bytes, kept on the key and freed with it; a key that is never checked holds nothing more than before.  GLP_E_INVALID, with
 * the cell named in glp_last_error, when a sigma value is no routed cell of the domain or sigma is no permutation of the routed cells.
 * Whatever B is (glp_plonk_last_check_counts): launches = [first check of a key: 2] + 1 (the NTT call) + 1 (base) + (Poseidon rows ? 1 : 0) +
 * (SHA rows ? 1 : 0) + 1 (copy); synchronises = 1 — the device builds the lists, counts and lists come back with that one synchronise.
 * The count is of the driver's explicit stream synchronises; the device-to-host copies of the counters and lists land in pageable host
 * memory, where the runtime may wait for each copy as it is issued.
 * d_wire_vals must hold canonical words (< p), as for the prover: cells are compared as 64-bit words, so a non-canonical representative
 * of the value its peer holds is reported as a copy mismatch.
 * Cost of a FAILING witness: the list is written by one 256-lane workgroup per instance, which walks the rows from the first failing one in
 * steps of 256 until max_list entries are found or the rows end — at most n / 256 steps (256 at n = 2^16, 65536 at n = 2^24) when fewer than
 * max_list (row, kind) pairs fail; a satisfied witness takes none.  Pass the max_list you will read, not a large one.
 * Transient device memory: 8 * n_const * n + B * (44 * n + 40 * max_list) bytes (+ 4 * n_routed * n during the decode). */
#define GLP_CHECK_GATE 0u
#define GLP_CHECK_COPY 1u
typedef struct {
    uint32_t kind, row, index, n_in_row;      /* n_in_row: failing constraints (GATE) or wires (COPY) in this row */
    uint32_t peer_wire, peer_row;             /* COPY: the cell sigma names; GATE: 0 */
    uint64_t value, peer_value;               /* GATE: value = the term the quotient weights by alpha^index, on this trace row; COPY: the two cell values */
} glp_check_violation;
typedef struct {
    uint64_t n_gate_bad, n_copy_bad;          /* failing (row, constraint) and (row, wire) pairs */
    uint32_t n_gate_rows, n_copy_rows, n_listed;
} glp_check_summary;
int glp_plonk_check_witness(glp_ctx* ctx, glp_plonk_circuit* ck, const uint64_t* d_wire_vals, const uint64_t* h_public, glp_check_summary* sum,
                            glp_check_violation* list, uint32_t max_list);
int glp_plonk_check_witness_batch(glp_ctx* ctx, glp_plonk_circuit* ck, const uint64_t* const* d_wire_vals, const uint64_t* h_public, uint32_t B,
                                  int32_t* h_status, glp_check_summary* sums, glp_check_violation* lists, uint32_t max_list);
/* what the LAST glp_plonk_check_witness[_batch] on this ctx issued: kernel launches (the NTT call counts as one) and stream synchronises */
int glp_plonk_last_check_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs);

/* the circuit's preprocessed commitment (cap of the constants + sigmas batch) = its verifying key:
 * copies min(*n_words, needed) u64 to h_cap and stores the needed count in *n_words */
int glp_plonk_circuit_cap(glp_plonk_circuit* ck, uint64_t* h_cap, size_t* n_words);

/* ---- verification (rows a5, a8, a12 from the consuming side; the Reduce step of row a11 as far as this
 *      build goes; upstream names recalled: plonk::verifier::verify, fri::verifier::verify_fri_proof).
 * Host arithmetic with the ctx's Poseidon constants (a verification is a few thousand permutations with
 * a serial transcript).  proof: 8-byte aligned little-endian u64 words as written by the provers above.
 * Returns GLP_OK when the proof is accepted, GLP_E_REJECT when it is not (glp_last_error says why),
 * other codes for bad arguments.  min_queries / min_pow_bits: the security parameters the caller
 * requires (a proof declaring fewer is rejected). */
int glp_fri_verify(glp_ctx* ctx, const uint8_t* h_proof, size_t proof_len, uint32_t min_queries, uint32_t min_pow_bits);
/* A stand-alone FRI proof says "polynomials of degree < 2^log_n behind THESE caps take THESE values at THESE points"; all of that
 * comes from the proof, so OK/REJECT alone does not tell the caller which statement was proven.  The _ex form also requires a
 * minimum code rate (rate_bits >= min_rate_bits; rate_bits = 0 is rejected by every entry point: at rate 1 any claimed value
 * passes) and returns the statement.  The caller MUST compare it with the one it expects (log_n, the caps, the points, the
 * opened values): caps = words [caps_word_off, + n_batches*cap_words) of the proof, openings = n_openings (a, b) pairs from
 * openings_word_off in (point, batch, polynomial) order; point p is zeta * point_mult[p], zeta derived from the transcript. */
typedef struct {
    uint32_t log_n, rate_bits, cap_height, n_batches, n_points, num_queries, pow_bits, total_polys;
    uint64_t shift;
    uint64_t zeta[2];
    uint64_t point_mult[4];
    size_t caps_word_off, cap_words;
    size_t openings_word_off, n_openings;
    uint32_t n_polys[64], open_mask[64];
} glp_fri_statement;
int glp_fri_verify_ex(glp_ctx* ctx, const uint8_t* h_proof, size_t proof_len, uint32_t min_queries, uint32_t min_pow_bits,
                      uint32_t min_rate_bits, glp_fri_statement* statement /* may be NULL */);
/* h_circuit_cap (from glp_plonk_circuit_cap; may be NULL = do not bind to a circuit) */
int glp_plonk_verify(glp_ctx* ctx, const uint8_t* h_proof, size_t proof_len, const uint64_t* h_circuit_cap, size_t cap_words,
                     uint32_t min_queries, uint32_t min_pow_bits);
/* ... and to a statement: h_public (NULL = do not bind) must equal the proof's public inputs word for word.  A proof is about
 * (circuit, public inputs): a verifier that passes NULL for either accepts proofs of OTHER statements. */
int glp_plonk_verify_ex(glp_ctx* ctx, const uint8_t* h_proof, size_t proof_len, const uint64_t* h_circuit_cap, size_t cap_words,
                        const uint64_t* h_public, size_t n_public, uint32_t min_queries, uint32_t min_pow_bits);
/* ---- batched verification: B proofs per call, the query phase on the device (opt-in; the single verifiers above are unchanged) ----
 * Per proof the HOST runs what is serial: header and range checks, the binding to h_circuit_cap / h_public, the transcript replay, proof of
 * work, the query indices, the alpha powers and opening sums and — after the queries, as the single verifier orders them — the trailing-data
 * check, the shape checks and the PLONK identity at zeta.  The query loop, which is independent per (proof, query), runs on the DEVICE for all
 * proofs of the call at once: one work-item per (proof, query, Merkle tree) — leaf canonicity, leaf hash, path walk, cap compare — and one per
 * (proof, query) — combination at x, the folds, the final polynomial.  Every failure inside the loop has a key (query, step in the loop's
 * order); the lowest key of a proof is the failure the single verifier stops at, so status, reason and query of every verdict EQUAL what
 * glp_plonk_verify_ex / glp_fri_verify_ex give on the same bytes (reason: glp_verify_reason_text(reason) is exactly the text after
 * "proof rejected: ").  A failure the host finds before the loop wins outright; one it finds after the loop counts only when no item failed.
 * Tampered bytes: the items use no offset, length or index that the host phase has not derived from the range-checked header and checked
 * against proof_len; the query index is the transcript's; a query that does not lie wholly inside the proof is settled on the host.
 * A proof whose shape the items do not take (arity_bits > 4, more than 65536 opened values, 2^31 words or more) is verified inside the same
 * call by the single verifier's code: on_device = 0, counted in n_fallback.
 * h_proofs[i]: 8-byte aligned, lens[i] a non-zero multiple of 8; the same pointer may appear twice.  h_public: NULL = do not bind, else
 * [B][n_public] expected public inputs.  h_digests (may be NULL): [B][4], what glp_plonk_proof_digest gives, zero where it would refuse.
 * statements (may be NULL): [B], filled for accepted proofs as glp_fri_verify_ex does, zero otherwise.
 * GLP_OK when the call ran (the verdicts are per proof; glp_last_error names the first refused proof and its reason); B == 0 is GLP_OK and
 * does nothing; GLP_E_INVALID for a null or misaligned argument; GLP_E_STATE without Poseidon constants.
 * Whatever B is (glp_verify_last_batch_counts): launches = 2 (Merkle items, arithmetic items) and synchronises = 1 per chunk, and one chunk
 * holds up to 2^30 Merkle items (B * queries * (batches + layers)): 2 launches and 1 synchronise for every B a host can hold.  No launch and no
 * synchronise when no proof reaches the query phase.  The count is of the driver's explicit stream synchronises.
 * Transient device memory per chunk: 8 * (sum of the words before the end of each recorded proof's last query) + 8 * (sum over proofs of
 * queries + 3 batches + 6 layers + 4 * 4 + 2 * opened values + order entries) + 120 * proofs + 8 * (Merkle items + arithmetic items) + 8 * proofs. */
#define GLP_VR_NONE 0u
#define GLP_VR_TRUNCATED 1u
#define GLP_VR_BAD_TAG 2u
#define GLP_VR_BAD_HEADER 3u
#define GLP_VR_HEADER_RANGE 4u
#define GLP_VR_RATE_ONE 5u
#define GLP_VR_WEAK_PARAMS 6u
#define GLP_VR_LOW_RATE 7u
#define GLP_VR_OPEN_MASKS 8u
#define GLP_VR_POINT_MULT 9u
#define GLP_VR_CAP_HEIGHT 10u
#define GLP_VR_CAP_NONCANONICAL 11u
#define GLP_VR_OPENING_NONCANONICAL 12u
#define GLP_VR_LAYER_CAP_NONCANONICAL 13u
#define GLP_VR_FINAL_NONCANONICAL 14u
#define GLP_VR_POW 15u
#define GLP_VR_QUERY_INDEX 16u
#define GLP_VR_LEAF_NONCANONICAL 17u
#define GLP_VR_MERKLE_PATH 18u
#define GLP_VR_QUERY_AT_POINT 19u
#define GLP_VR_LAYER_LEAF_NONCANONICAL 20u
#define GLP_VR_FOLD 21u
#define GLP_VR_LAYER_MERKLE_PATH 22u
#define GLP_VR_FINAL_POLY 23u
#define GLP_VR_TRAILING 24u
#define GLP_VR_PLONK_HEADER 25u
#define GLP_VR_PUBLIC_NONCANONICAL 26u
#define GLP_VR_PUBLIC_DIFFER 27u
#define GLP_VR_CIRCUIT_DIFFER 28u
#define GLP_VR_FRI_SHAPE 29u
#define GLP_VR_FRI_CAPS 30u
#define GLP_VR_POINTS 31u
#define GLP_VR_IDENTITY 32u
#define GLP_VR_COUNT 33u
typedef struct {
    int32_t status;      /* GLP_OK / GLP_E_REJECT */
    uint32_t reason;     /* GLP_VR_*: index into the single verifier's reason texts */
    uint32_t query;      /* failing query, 0xFFFFFFFF outside the query loop */
    uint32_t on_device;  /* 1: the query phase of this proof ran as items of the batched phase */
} glp_verify_verdict;
int glp_plonk_verify_batch(glp_ctx* ctx, const uint8_t* const* h_proofs, const size_t* lens, uint32_t B, const uint64_t* h_circuit_cap,
                           size_t cap_words, const uint64_t* h_public /* [B][n_public] or NULL */, size_t n_public, uint32_t min_queries,
                           uint32_t min_pow_bits, glp_verify_verdict* h_verdicts, uint64_t* h_digests /* [B][4] or NULL */);
int glp_fri_verify_batch(glp_ctx* ctx, const uint8_t* const* h_proofs, const size_t* lens, uint32_t B, uint32_t min_queries,
                         uint32_t min_pow_bits, uint32_t min_rate_bits, glp_verify_verdict* h_verdicts,
                         glp_fri_statement* statements /* [B] or NULL */);
/* exactly the text after "proof rejected: " of the single verifiers; "" for GLP_VR_NONE or an unknown value */
const char* glp_verify_reason_text(uint32_t reason);
/* what the LAST glp_*_verify_batch on this ctx issued, and how many of its proofs ran their queries as items / in place (any pointer may be NULL) */
int glp_verify_last_batch_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs, uint32_t* n_on_device, uint32_t* n_fallback);
/* The same two calls for a host WITHOUT a GPU: the same host phase, then the same item bodies one after the other on the host (the constants
 * arguments of the host verifiers below).  n_on_device / n_fallback (may be NULL): the counts glp_verify_last_batch_counts would give. */
int glp_plonk_verify_batch_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* const* h_proofs,
                                const size_t* lens, uint32_t B, const uint64_t* h_circuit_cap, size_t cap_words, const uint64_t* h_public,
                                size_t n_public, uint32_t min_queries, uint32_t min_pow_bits, glp_verify_verdict* h_verdicts,
                                uint64_t* h_digests, uint32_t* n_on_device, uint32_t* n_fallback);
int glp_fri_verify_batch_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* const* h_proofs,
                              const size_t* lens, uint32_t B, uint32_t min_queries, uint32_t min_pow_bits, uint32_t min_rate_bits,
                              glp_verify_verdict* h_verdicts, glp_fri_statement* statements, uint32_t* n_on_device, uint32_t* n_fallback);

/* the public inputs a proof carries: copies min(*n_words, n_public) words to h_out (may be NULL with *n_words = 0) and stores
 * n_public in *n_words.  No verification: GLP_E_INVALID when the bytes are not a circuit proof of this format. */
int glp_plonk_proof_public_inputs(const uint8_t* h_proof, size_t proof_len, uint64_t* h_out, size_t* n_words);
/* 4-word Poseidon digest of a circuit proof's statement and commitments: hash_no_pad(header || public inputs || the four caps) —
 * the leaf value of the Reduce step's aggregation tree (0-kno-blobstreamx_amd/recursion.py).  No verification. */
int glp_plonk_proof_digest(glp_ctx* ctx, const uint8_t* h_proof, size_t proof_len, uint64_t* h_out4);
/* Witness evaluator for circuits recorded by the host builder (0-kno-blobstreamx_amd/recursion.py::WitnessProgram): a straight-line program
 * (arithmetic gates, inputs, bit extractions, inverses, Poseidon permutations; encoding in csrc/verify.hip) computes every variable of the circuit
 * from its inputs in one forward pass, then the copy constraints between different variables (eq_pairs, 2 indices each) are checked:
 * GLP_E_REJECT + *first_bad when the witness does not satisfy the circuit.  Host arithmetic, one op after the other (the batched device form:
 * glp_witness_eval_device below). */
int glp_witness_eval(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint64_t* prog, size_t prog_words,
                     const uint64_t* inputs, size_t n_inputs, uint64_t* values, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                     size_t* first_bad);
/* ... on several host threads: seg_bounds = n_seg + 1 ascending word offsets (op boundaries); the ops of [seg_bounds[k], seg_bounds[k+1]) are
 * n_seg mutually independent segments (each reads only what the prefix [0, seg_bounds[0]) or itself wrote — e.g. the verifier sub-circuits of
 * the proofs a recursion node checks), run on up to n_threads threads; the tail after seg_bounds[n_seg] runs last.  The independence claim is
 * checked while running: GLP_E_INVALID when a segment reads another segment's variable.  seg_bounds NULL / n_seg < 2 / n_threads < 2 = serial. */
int glp_witness_eval_mt(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint64_t* prog, size_t prog_words,
                        const uint64_t* inputs, size_t n_inputs, uint64_t* values, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                        size_t* first_bad, const uint64_t* seg_bounds, size_t n_seg, uint32_t n_threads);
/* Witness placement on the device: d_dst[i] = d_index[i] == 0xFFFFFFFF ? 0 : d_src[d_index[i]], i < n (d_index: uint32, every other entry < n_src
 * — checked on the device: an out-of-range entry writes 0 and the call returns GLP_E_INVALID).  With d_index = the circuit's cell -> variable map
 * (resident, built once per circuit) and d_src = the evaluated variables, this lays out the wire matrix without a host-side copy of it. */
int glp_gather_u64(glp_ctx* ctx, uint64_t* d_dst, const uint64_t* d_src, size_t n_src, const uint32_t* d_index, size_t n);
/* Device-side witness evaluation.  A PLAN is the witness program compiled once into a level schedule (level of an op = 1 + the highest level
 * among the producers of its operands; ops without operands are level 0): ops ordered by (level, kind), 32-bit variable indices, the distinct
 * ARITH constant triples in a dictionary.  glp_witness_plan_create does every structural check of glp_witness_eval (indices < n_values, constants
 * < p, shift / bit counts, op lengths, unknown kinds) and also refuses an operand that no earlier op wrote and a variable written twice:
 * GLP_E_INVALID; GLP_E_UNSUPPORTED when n_values or n_inputs >= 2^32 - 1.  No GPU is needed for create / stats / run_host / destroy (as long
 * as the plan was never evaluated on a device). */
typedef struct glp_witness_plan glp_witness_plan;
int glp_witness_plan_create(const uint64_t* prog, size_t prog_words, size_t n_inputs, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                            glp_witness_plan** plan);
void glp_witness_plan_destroy(glp_witness_plan* plan);
/* ops, levels, barrier-separated steps at the kernel's workgroup size (sum over levels of ceil(width / 256)), bytes resident per device.
 * Any output pointer may be NULL. */
int glp_witness_plan_stats(const glp_witness_plan* plan, uint64_t* n_ops, uint64_t* depth, uint64_t* steps, uint64_t* stream_bytes);
/* the REORDERED schedule run serially on the host with the arithmetic of glp_witness_eval: same values, return code and *first_bad.  It exists
 * so that a schedule can be checked without a GPU; glp_witness_eval_mt stays the host product path. */
int glp_witness_plan_run_host(const glp_witness_plan* plan, const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag,
                              const uint64_t* inputs, size_t n_inputs, uint64_t* values, size_t n_values, size_t* first_bad);
/* B instances of the plan on the device, one workgroup per instance, level by level: d_inputs [B][n_inputs] -> d_values [B][value_stride]
 * (value_stride >= n_values; words past n_values are left alone; a variable no op writes is set to 0), the layout glp_gather_u64 places wire cells from.  Stream-ordered on the ctx's
 * stream, which is synchronised before the call returns.  GLP_OK when the batch ran; the verdict of instance b is h_status[b]: GLP_OK,
 * GLP_E_REJECT (h_first_bad[b] = the lowest failing copy-constraint index, or (uint64_t)-1 when a row operand is out of range) or GLP_E_INVALID
 * (an input word >= p) — an instance's verdict does not affect the others.  The plan's schedule is uploaded on first use per DEVICE and owned by
 * the plan: shared by every ctx of that device, freed by glp_witness_plan_destroy (not by glp_destroy). */
int glp_witness_eval_device(glp_ctx* ctx, const glp_witness_plan* plan, const uint64_t* d_inputs, uint64_t* d_values, size_t value_stride,
                            uint32_t B, int32_t* h_status, uint64_t* h_first_bad);
/* A SEGMENTED plan, for a program that is ONE instance of n_seg mutually independent segments (a recursion node: the verifier sub-circuits of
 * its children).  seg_bounds: the n_seg + 1 offsets of glp_witness_eval_mt.  The plan has n_seg + 2 PARTS — the prefix [0, seg_bounds[0]), the
 * segments, the tail — each with a level schedule of its own (a level counts only producers inside the part).  Everything is checked here:
 * GLP_E_INVALID for an offset that is not an op boundary, descending or past the program, and for a segment that reads what another segment
 * wrote, besides what glp_witness_plan_create refuses.  n_seg < 2 (seg_bounds then ignored) is glp_witness_plan_create: one part.
 * glp_witness_eval_device on a segmented plan issues three launches on the ctx's stream — the prefix, all segments at once (a workgroup per
 * (instance, segment) pair), the tail with the copy constraints — with the verdicts of the plain plan; glp_witness_plan_run_host runs the
 * parts in order; glp_witness_plan_stats counts depth and steps over all parts. */
int glp_witness_plan_create_ex(const uint64_t* prog, size_t prog_words, size_t n_inputs, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                               const uint64_t* seg_bounds, size_t n_seg, glp_witness_plan** plan);
/* per part: ops, levels, steps at 256 lanes.  In: *n_parts = the capacity of the arrays (any of them may be NULL); out: the plan's number of
 * parts (1 for a plain plan), of which min(capacity, parts) entries were written. */
int glp_witness_plan_parts(const glp_witness_plan* plan, uint32_t* n_parts, uint64_t* ops, uint64_t* depth, uint64_t* steps);
/* The word checks of a recorded circuit on evaluated instances ON THE DEVICE (d_values as glp_witness_eval_device leaves them): check k < n_var
 * of instance b holds when d_values[b][d_var_idx[k]] == d_var_want[b * n_var + k]; check j < n_bits when the variables
 * d_bit_vars[d_bit_start[j] .. d_bit_start[j + 1]) (0 / 1 values, at most 64 of them), packed little-endian mod 2^64, equal
 * d_bit_want[b * n_bits + j].  h_first_bad_var[b] / h_first_bad_bits[b]: the lowest failing check of each kind, (uint64_t)-1 when none fails.
 * A variable index >= value_stride fails its check.  d_bit_start holds n_bits + 1 ascending offsets into d_bit_vars (the caller's contract).
 * Stream-ordered on the ctx's stream, which is synchronised before the call returns.  ..._host: the same checks on host arrays, no GPU. */
int glp_witness_check_words(glp_ctx* ctx, const uint64_t* d_values, size_t value_stride, uint32_t B, const uint32_t* d_var_idx,
                            const uint64_t* d_var_want, uint32_t n_var, const uint32_t* d_bit_vars, const uint32_t* d_bit_start,
                            const uint64_t* d_bit_want, uint32_t n_bits, uint64_t* h_first_bad_var, uint64_t* h_first_bad_bits);
int glp_witness_check_words_host(const uint64_t* values, size_t value_stride, uint32_t B, const uint32_t* var_idx, const uint64_t* var_want,
                                 uint32_t n_var, const uint32_t* bit_vars, const uint32_t* bit_start, const uint64_t* bit_want, uint32_t n_bits,
                                 uint64_t* first_bad_var, uint64_t* first_bad_bits);
/* Batched witness placement.  A LAYOUT holds the host arrays that say how a recorded circuit's evaluated variables become a wire matrix
 * [n_wires][2^log_n]: cell_index [n_wires * n] (cell -> source word; 0xFFFFFFFF = an unused cell, zero), n_src (the variables plus the fixed
 * values appended behind them: the words of one slab row that cells may name), the Poseidon rows, the SHA rows with their kinds (GLP_SHA_ROW_*)
 * and the variables that are the public inputs.  glp_witness_layout_create is host-only (no ctx, no GPU) and does EVERY range check once:
 * a cell entry is < n_src or the unused marker, a row is < n, a kind is <= 3, n_wires >= GLP_POS_GATE_WIRES when there are Poseidon rows and
 * >= GLP_SHA_GATE_WIRES when there are SHA rows, a public variable is < n_src: GLP_E_INVALID with the reason in err (may be NULL) for a
 * violation, GLP_E_UNSUPPORTED for n_src >= 2^32 - 1.  The placement kernels therefore carry no "bad index" flag and copy nothing back.
 * The arrays are copied.  The device copy is uploaded on the first glp_witness_place_batch per DEVICE and owned by the layout: shared by every
 * ctx of that device, freed by glp_witness_layout_destroy (not by glp_destroy) — destroy it when no call that uses it is running and the
 * streams that ran one have been synchronised. */
typedef struct glp_witness_layout glp_witness_layout;
int glp_witness_layout_create(uint32_t log_n, uint32_t n_wires, const uint32_t* cell_index, size_t n_src, const uint32_t* pos_rows,
                              uint32_t n_pos_rows, const uint32_t* sha_rows, const uint32_t* sha_kinds, uint32_t n_sha_rows,
                              const uint32_t* public_vars, uint32_t n_public, glp_witness_layout** layout, char* err, size_t err_len);
void glp_witness_layout_destroy(glp_witness_layout* layout);
/* what the layout was made with; any output pointer may be NULL */
int glp_witness_layout_info(const glp_witness_layout* layout, uint32_t* log_n, uint32_t* n_wires, uint64_t* n_src, uint32_t* n_pos_rows,
                            uint32_t* n_sha_rows, uint32_t* n_public);
/* B wire matrices from B rows of an evaluated slab (d_values [rows][value_stride] as glp_witness_eval_device leaves it, the fixed values behind
 * the variables of each row; value_stride >= n_src).  Instance i reads slab row h_rows[i] (host, [B]; any order, repeats allowed) and its matrix
 * is written at d_wires + i * wire_stride_words (wire_stride_words >= n_wires * n; words past n_wires * n are left alone): B matrices side by
 * side, the layout glp_plonk_prove_batch's pointers name.  The derived wires of the Poseidon and SHA rows are filled as
 * glp_poseidon_gate_fill_rows / glp_sha_gate_fill_rows fill them (same kernel bodies, same small-MDS choice): every word equals what
 * glp_gather_u64 and the two row fillers give per instance.  h_public ([B][n_public], or NULL): the public values of each instance.
 * Whatever B is, the call issues
 *   launches     = 1 (all B matrices: one work-item per cell, a loop over the instances) + (Poseidon rows ? 1 : 0) + (SHA rows ? 1 : 0)
 *                  + (h_public && n_public ? 1 : 0)                                                   <= 4
 *   synchronises = (h_public && n_public ? 1 : 0), after the one device-to-host copy                     <= 1
 * and one host-to-device copy of the B slab rows (from pinned staging of the ctx: h_rows is done with on return; before it is overwritten the
 * next call waits for the event behind the previous call's copy).  Without h_public the call is stream-ordered and returns at once.
 * glp_witness_last_place_counts reports the two numbers of the LAST call on the ctx.
 * Measured (profiles/reduce_batch.json; 8 data-commitment leaves of 2^16 x 144, resident slab -> resident wires + public values, medians of 5
 * alternating repeats): eight glp_gather_u64 / row filler / public gather sequences 1.83 ms, one call here 0.63 ms.
 * B == 0 is GLP_OK and does nothing.  GLP_E_INVALID for a null argument or a stride below the layout's; GLP_E_STATE when the layout has Poseidon
 * rows and the ctx has no Poseidon constants; GLP_E_UNSUPPORTED for a B whose row launches would exceed 2^31 - 1 workgroups.
 * THE CALLER'S CONTRACT, which the callee cannot check: every h_rows[i] is a row of the slab (< its row count), as value_stride is the caller's
 * for glp_witness_eval_device; and the B destination matrices do not overlap the slab or each other. */
int glp_witness_place_batch(glp_ctx* ctx, const glp_witness_layout* layout, const uint64_t* d_values, size_t value_stride, const uint32_t* h_rows,
                            uint32_t B, uint64_t* d_wires, size_t wire_stride_words, uint64_t* h_public);
int glp_witness_last_place_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs);
/* the Poseidon permutation on the host: n states of 12 canonical words, in place (same constants arguments as the host verifiers) */
int glp_poseidon_permute_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, uint64_t* states, size_t n);
int glp_plonk_proof_digest_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* h_proof,
                                size_t proof_len, uint64_t* h_out4);

/* The same two verifiers for a host WITHOUT a GPU (a light client, CI): no ctx — the Poseidon constants are
 * passed explicitly (the arguments of glp_set_poseidon_constants: 360, 12, 12 words) and err (may be NULL)
 * receives the rejection reason.  GLP_E_INVALID for unusable arguments or non-canonical constants. */
int glp_fri_verify_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* h_proof,
                        size_t proof_len, uint32_t min_queries, uint32_t min_pow_bits, char* err, size_t err_len);
int glp_fri_verify_host_ex(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* h_proof,
                           size_t proof_len, uint32_t min_queries, uint32_t min_pow_bits, uint32_t min_rate_bits,
                           glp_fri_statement* statement, char* err, size_t err_len);
int glp_plonk_verify_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* h_proof,
                          size_t proof_len, const uint64_t* h_circuit_cap, size_t cap_words, uint32_t min_queries,
                          uint32_t min_pow_bits, char* err, size_t err_len);
int glp_plonk_verify_host_ex(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* h_proof,
                             size_t proof_len, const uint64_t* h_circuit_cap, size_t cap_words, const uint64_t* h_public, size_t n_public,
                             uint32_t min_queries, uint32_t min_pow_bits, char* err, size_t err_len);

/* ---- witness generation (rows a9; upstream names recalled: curta SHA-256/SHA-512 chips) */
/* n_msgs messages, each already padded to blocks_per_msg 64-byte blocks, [n_msgs][blocks*64].
 * d_digests: [n_msgs][8] u32 (big-endian words as u32).  d_trace (may be NULL):
 * [n_msgs][blocks][576] u32 = 64 schedule words then 64x8 round states. */
int glp_sha256_trace(glp_ctx* ctx, const uint8_t* d_blocks, uint64_t n_msgs, uint32_t blocks_per_msg,
                     uint32_t* d_digests, uint32_t* d_trace);
/* 128-byte blocks; digests [n_msgs][8] u64; trace [n_msgs][blocks][720] u64 */
int glp_sha512_trace(glp_ctx* ctx, const uint8_t* d_blocks, uint64_t n_msgs, uint32_t blocks_per_msg,
                     uint64_t* d_digests, uint64_t* d_trace);

/* Ed25519 verification witness (row a10; upstream name recalled: curta Ed25519 gadget), RFC 8032
 * cofactorless check [S]B = R + [k]A.  Per signature GLP_ED25519_RECORD_WORDS u64:
 * [0] valid, [1..4] k = SHA512(R||A||M) mod L, then affine Ax, Ay, Rx, Ry, P1x, P1y (= [S]B),
 * P2x, P2y (= [k]A), each 4 little-endian words.  The message bytes of signature i are
 * d_msgs[i*msg_stride .. + d_lens[i]); a row with d_lens[i] > msg_stride is invalid input: its record is all zero
 * (valid = 0) and nothing is read.  Stream-ordered (glp_sync before reading d_out). */
#define GLP_ED25519_RECORD_WORDS 37
int glp_ed25519_witness(glp_ctx* ctx, const uint8_t* d_pubs, const uint8_t* d_sigs, const uint8_t* d_msgs, uint32_t msg_stride,
                        const uint32_t* d_lens, uint64_t n, uint64_t* d_out);

/* The INPUT VECTORS of the signature leaf on the device: row i of d_inputs is what ed25519_circuit.witness_inputs builds for slot i, word for
 * word — the bytes of the statement's free inputs, the 24-bit limbs of x_A, x_R, t = h div L and k = h mod L (h = SHA-512(R || A || M)) and,
 * with split_scalars, the half-size form's hints u[6] v[6] neg q1[7] w[11] q2[7] (u k = -+v mod 8L by Lagrange reduction of a 2-dimensional
 * lattice; u S = q1 L + w; u k -+ v = q2 8L).  d_inputs ([n][input_stride] words, input_stride >= glp_ed25519_leaf_input_words) is what
 * glp_witness_eval_device reads: nothing of a slot visits the host.
 * form: GLP_ED25519_FORM_PLAIN    A[32] R[32] S[32] M[len] | limbs                          (msg_len_min = msg_len_max = len; d_flags, d_dummy NULL)
 *       GLP_ED25519_FORM_FLAGGED  flag key[32] M[len] | R S of the VERIFIED triple | limbs    (msg_len_min = msg_len_max = len)
 *       GLP_ED25519_FORM_VOTE     flag key[32] M zero-padded to msg_len_max, L, one-hot of L - msg_len_min [max - min + 1] | R S | limbs
 * The verified triple of a slot is its own when d_flags[i] != 0 and the caller's dummy triple when it is 0: d_dummy = pub[32] | sig[64] |
 * msg[msg_len_min], a constant of the circuit.  Two stream-ordered launches whatever n is: the kernel of glp_ed25519_witness over the slots'
 * own triples into pool scratch, then the input kernel (one work-item per slot), which takes x_A, x_R, k of a flagged slot from its record and
 * decodes / reduces the dummy's itself for an unflagged one.  ONE synchronise, after the copy of the statuses to h_status[n]:
 *   GLP_ED25519_IN_OK       the row is written
 *   GLP_ED25519_IN_REJECT   the record says invalid (a flagged signature that does not verify, an A or R that does not decode, S >= L)
 *   GLP_ED25519_IN_NO_PAIR  no half-size pair below 2^144 (probability ~2^-36; the Python raises)
 *   GLP_ED25519_IN_INVALID  d_lens[i] outside [msg_len_min, msg_len_max] or above msg_stride
 * A row whose status is not OK is all zero: none is written partially.  glp_ed25519_last_input_counts reports the launches and synchronises
 * of the LAST call on the ctx.  n == 0 is GLP_OK.  GLP_E_INVALID for a null argument, a layout no statement has, or a stride below the row.
 * glp_ed25519_leaf_input_words needs no GPU and no ctx. */
#define GLP_ED25519_FORM_PLAIN 0
#define GLP_ED25519_FORM_FLAGGED 1
#define GLP_ED25519_FORM_VOTE 2
#define GLP_ED25519_IN_OK 0
#define GLP_ED25519_IN_REJECT 1
#define GLP_ED25519_IN_NO_PAIR 2
#define GLP_ED25519_IN_INVALID 3
typedef struct {
    uint32_t form;
    uint32_t msg_len_min, msg_len_max;
    uint32_t split_scalars;
} glp_ed25519_input_layout;
int glp_ed25519_leaf_input_words(const glp_ed25519_input_layout* layout, uint64_t* n_words);
int glp_ed25519_leaf_inputs(glp_ctx* ctx, const glp_ed25519_input_layout* layout, const uint8_t* d_pubs, const uint8_t* d_sigs,
                            const uint8_t* d_msgs, uint32_t msg_stride, const uint32_t* d_lens, const uint8_t* d_flags, const uint8_t* d_dummy,
                            uint64_t n, uint64_t* d_inputs, size_t input_stride, int32_t* h_status);
int glp_ed25519_last_input_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs);
/* The reduction alone: d_k [n][4] little-endian scalars -> d_out [n][8] = u[3] v[3] neg status (OK, NO_PAIR, or INVALID for k >= L; u, v are
 * zero unless OK).  ed25519_circuit.half_size_pair on the device.  One launch, stream-ordered (glp_sync before reading d_out). */
int glp_ed25519_half_scalars(glp_ctx* ctx, const uint64_t* d_k, uint64_t n, uint64_t* d_out);

/* Tendermint "simple" Merkle root (RFC 6962 prefixes) of n leaves of leaf_len (<= 118) bytes each:
 * the validator-set / header hashing of BASELINE configs[0].  Synchronous; h_root32 = 32 bytes. */
int glp_tm_merkle_root(glp_ctx* ctx, const uint8_t* d_leaves, uint32_t leaf_len, uint64_t n, uint8_t* h_root32);
/* the same tree over leaves of different lengths (protobuf-encoded validators, header fields):
 * leaf i = d_data[d_offsets[i] .. d_offsets[i+1]), n + 1 non-decreasing byte offsets (device), the last one <= data_len
 * (checked: GLP_E_INVALID otherwise, nothing is read out of range) */
int glp_tm_merkle_root_var(glp_ctx* ctx, const uint8_t* d_data, uint64_t data_len, const uint64_t* d_offsets, uint64_t n,
                           uint8_t* h_root32);

/* n_trees such trees in ONE stream-ordered call: tree t has the leaves [tree_first[t], tree_first[t + 1]) of one numbering over all trees,
 * leaf i = d_data[leaf_offsets[i] .. leaf_offsets[i + 1]) — the _var form's offsets across all trees.  The trees of a call may differ in leaf
 * count and leaf lengths; a tree without leaves gives what glp_tm_merkle_root_var gives for n = 0 (SHA-256 of nothing).  d_roots [n_trees][32]
 * stays on the device.  Two launches whatever n_trees is (a work-item per leaf for the leaf hashes; a workgroup per tree folding the levels
 * through LDS) and NO synchronise and no copy to the host, unless h_roots is not NULL: then one copy of all n_trees roots and one synchronise.
 * The two arrays are validated ON THE HOST, from the host's copy of them, before anything is launched — h_leaf_offsets [total_leaves + 1]
 * non-decreasing with the last <= data_len, h_tree_first [n_trees + 1] ascending from 0 to total_leaves: GLP_E_INVALID otherwise, and nothing is
 * written.  The call uploads the checked words itself, stream-ordered, into scratch of the ctx, and the kernels read no other offset: there is
 * no device copy for the caller to keep in step.  The two host arrays must stay as they are until the stream has passed the call (h_roots,
 * glp_sync or any later synchronising call).
 * A tree of more than GLP_TM_BATCH_MAX_LEAVES leaves (one workgroup's LDS level: 256 nodes after the first pairing) gives GLP_E_UNSUPPORTED
 * and writes nothing; use glp_tm_merkle_root_var for such a tree.  Validator sets of 100 - 150 and the 14 fields of a header are far below it.
 * n_trees == 0 is GLP_OK.  glp_tm_merkle_root_batch_last_counts: launches and synchronises of the LAST call on the ctx.
 * glp_tm_merkle_root_batch_host: the same trees serially on the host with the kernels' per-item functions; no ctx, no GPU. */
#define GLP_TM_BATCH_MAX_LEAVES 512
int glp_tm_merkle_root_batch(glp_ctx* ctx, const uint8_t* d_data, uint64_t data_len, const uint64_t* h_leaf_offsets, const uint64_t* h_tree_first,
                             uint64_t total_leaves, uint64_t n_trees, uint8_t* d_roots, uint8_t* h_roots);
int glp_tm_merkle_root_batch_last_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs);
int glp_tm_merkle_root_batch_host(const uint8_t* data, uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* tree_first,
                                  uint64_t total_leaves, uint64_t n_trees, uint8_t* roots);

/* INCLUSION PROOFS: the same trees with EVERY LEVEL KEPT on the device, the audit paths of any leaves read out of them, and the batched check
 * of such paths against roots — "this DataRootTuple lies inside the proven data commitment", validator-set membership, "this field belongs to
 * this header hash".  The proof format is BUILD-DEFINED (Tendermint's crypto/merkle.Proof{Total, Index, LeafHash, Aunts} restated from memory,
 * unpinned): the proof of leaf `index` of `total` leaves is its sibling hashes BOTTOM-UP (nearest the leaf first), 32 bytes each; leaf hash
 * SHA256(00 || leaf), inner hash SHA256(01 || l || r); an odd last node of a level is promoted and contributes NO aunt at that level, so the
 * aunt count is fixed by (index, total) and is at most ceil(log2 total): with 5 leaves, leaf 4 has 1 aunt and leaf 0 has 3.
 * glp_tm_forest_create: arguments as glp_tm_merkle_root_batch (arrays validated on the host before anything is launched; on a refusal nothing
 *   is written and no handle is made), with at most GLP_TM_FOREST_MAX_LEAVES leaves per tree (GLP_E_UNSUPPORTED above).  At most
 *   2 + max(0, ceil(log2(largest tree)) - 9) launches — leaf hashes, one launch per level while the widest tree has more than 512 nodes, one
 *   workgroup per tree for the rest — and NO synchronise, unless h_roots [n_trees][32] is not NULL: then one copy and one synchronise.  d_data
 *   and h_leaf_offsets are not needed once the stream has passed the call.  n_trees == 0 is GLP_OK (a forest that admits no query); a tree
 *   without leaves has the root SHA256("") and admits no query.  The forest belongs to ctx: use it on that ctx, destroy it before the ctx.
 * glp_tm_forest_info: trees, leaves, the aunts of leaf 0 of the largest tree (max_aunts), device bytes held; any pointer may be NULL.
 * glp_tm_forest_roots: the device array [n_trees][32], valid until the forest is destroyed.
 * glp_tm_forest_proofs: ONE launch and no synchronise for any number of queries (h_query_tree[q], h_query_leaf[q] = leaf inside that tree),
 *   validated on the host before the launch: tree < n_trees, leaf < that tree's count, aunt_stride >= ceil(log2(count)) of every queried tree —
 *   GLP_E_INVALID otherwise, nothing written.  Both arrays NULL with n_queries == total_leaves: every leaf in numbering order.  Writes
 *   d_aunts [n_queries][aunt_stride][32] (slots past a row's count are written as ZERO), d_n_aunts [n_queries], and d_leaf_hashes
 *   [n_queries][32] unless NULL.  The host arrays must stay until the stream has passed the call.
 * glp_tm_verify_inclusion_batch: n proofs in ONE launch and one synchronise (after the copy to h_status [n]): proof p is leaf BYTES
 *   d_data[h_leaf_offsets[p] .. h_leaf_offsets[p + 1]) — hashed here with the 00 prefix, never a leaf hash taken from the proof — d_index[p],
 *   d_total[p], d_n_aunts[p] and row p of d_aunts, against root h_root_of[p] (NULL: root 0) of d_roots [n_roots][32].  index, total and n_aunts
 *   are untrusted: GLP_TM_INCLUSION_BAD_SHAPE for total == 0, index >= total, n_aunts > aunt_stride or n_aunts not the count (index, total)
 *   fixes (no aunt is read then); else GLP_TM_INCLUSION_BAD_ROOT or GLP_TM_INCLUSION_OK.  The offsets and h_root_of are checked on the host
 *   (GLP_E_INVALID).  n == 0 is GLP_OK.
 * glp_tm_forest_last_counts: launches and synchronises of the LAST of these three calls on the ctx.
 * The _host forms run the same per-item functions serially; no ctx, no GPU.  glp_tm_forest_proofs_host builds the trees and reads the paths in
 * one call (roots [n_trees][32] may be NULL). */
#define GLP_TM_FOREST_MAX_LEAVES (1ull << 24)
#define GLP_TM_INCLUSION_OK 0
#define GLP_TM_INCLUSION_BAD_SHAPE 1
#define GLP_TM_INCLUSION_BAD_ROOT 2
typedef struct glp_tm_forest glp_tm_forest;
int glp_tm_forest_create(glp_ctx* ctx, const uint8_t* d_data, uint64_t data_len, const uint64_t* h_leaf_offsets, const uint64_t* h_tree_first,
                         uint64_t total_leaves, uint64_t n_trees, uint8_t* h_roots, glp_tm_forest** out);
int glp_tm_forest_info(const glp_tm_forest* forest, uint64_t* n_trees, uint64_t* total_leaves, uint32_t* max_aunts, uint64_t* bytes);
int glp_tm_forest_roots(const glp_tm_forest* forest, const uint8_t** d_roots);
int glp_tm_forest_destroy(glp_tm_forest* forest);
int glp_tm_forest_proofs(glp_ctx* ctx, const glp_tm_forest* forest, const uint64_t* h_query_tree, const uint64_t* h_query_leaf, uint64_t n_queries,
                         uint8_t* d_aunts, uint32_t aunt_stride, uint32_t* d_n_aunts, uint8_t* d_leaf_hashes);
int glp_tm_verify_inclusion_batch(glp_ctx* ctx, const uint8_t* d_roots, uint64_t n_roots, const uint32_t* h_root_of, const uint8_t* d_data,
                                  uint64_t data_len, const uint64_t* h_leaf_offsets, const uint64_t* d_index, const uint64_t* d_total,
                                  const uint8_t* d_aunts, uint32_t aunt_stride, const uint32_t* d_n_aunts, uint64_t n, int32_t* h_status);
int glp_tm_forest_last_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs);
int glp_tm_forest_proofs_host(const uint8_t* data, uint64_t data_len, const uint64_t* leaf_offsets, const uint64_t* tree_first,
                              uint64_t total_leaves, uint64_t n_trees, const uint64_t* query_tree, const uint64_t* query_leaf, uint64_t n_queries,
                              uint8_t* roots, uint8_t* aunts, uint32_t aunt_stride, uint32_t* n_aunts, uint8_t* leaf_hashes);
int glp_tm_verify_inclusion_batch_host(const uint8_t* roots, uint64_t n_roots, const uint32_t* root_of, const uint8_t* data, uint64_t data_len,
                                       const uint64_t* leaf_offsets, const uint64_t* index, const uint64_t* total, const uint8_t* aunts,
                                       uint32_t aunt_stride, const uint32_t* n_aunts, uint64_t n, int32_t* status);

/* The INPUT VECTORS of the header-chain leaf on the device: from the raw headers of a chain to the rows glp_witness_eval_device reads.
 * d_headers: n headers, each the concatenation of its 14 field encodings at the layout's lengths (field_len: what the leaf recording fixes;
 * leaf_headers: headers per leaf; n_groups: the varint bytes of a height).  Three steps, at most 4 launches and ONE synchronise (after the
 * copy of the statuses to h_status[n]) whatever n is:
 *   1. the n header hashes: the batched tree kernels over n trees of 14 leaves, read at the layout's offsets (no offset array exists);
 *   2. one work-item per header k tests what the leaf circuit will build instead of reading: field 4 begins 0a 20 || hash of header k - 1
 *      (start_hash32 for k = 0), field 2 is 08 || varint(first_height + k) in exactly n_groups bytes (a non-minimal or over-long varint is not),
 *      field 6 begins 0a 20 -> GLP_HEADER_CHAIN_OK / _BAD_LINK / _BAD_HEIGHT / _BAD_DATA_FIELD, the first that applies in this order;
 *   3. row l of d_inputs ([n / leaf_headers][input_stride] words, input_stride >= glp_header_chain_leaf_input_words) = the 8 big-endian words
 *      of the hash before header l * leaf_headers, the height first_height + l * leaf_headers, then per header: the varint groups (low first),
 *      the 32 data-hash bytes, the bytes of last_block_id behind its hash, the bytes of the eleven other fields — one byte per word.  A leaf
 *      with a header whose status is not OK gets an all-zero row: none is written partially.  Words past the row's width are left alone.
 * d_hashes ([n + 1][32]: start hash, then the hash of every header) may be NULL.  n == 0 is GLP_OK; GLP_E_INVALID for n that is not a multiple
 * of leaf_headers or above 2^30, first_height >= 2^49 (heights are below 2^49: 7 varint bytes), a null argument, a stride below the row, or a
 * layout no leaf statement has (field 4 below 34 bytes, field 6 not 34 bytes, a field above 65536 bytes, n_groups outside 1 .. 7, leaf_headers
 * outside 1 .. 1024: every wave of the row kernel reads its leaf's leaf_headers statuses, which is meant for leaves of a few headers — the
 * statements use 1 to 8).  glp_header_chain_leaf_input_words needs no GPU and no ctx.  glp_header_chain_last_input_counts: launches and
 * synchronises of the LAST call on the ctx.  glp_header_chain_leaf_inputs_host: the same three steps serially on the host with the kernels'
 * per-item functions (hashes [n + 1][32] may be NULL); no ctx, no GPU. */
#define GLP_HEADER_CHAIN_OK 0
#define GLP_HEADER_CHAIN_BAD_LINK 1
#define GLP_HEADER_CHAIN_BAD_HEIGHT 2
#define GLP_HEADER_CHAIN_BAD_DATA_FIELD 3
typedef struct {
    uint32_t field_len[14];
    uint32_t leaf_headers;
    uint32_t n_groups;
} glp_header_chain_layout;
int glp_header_chain_leaf_input_words(const glp_header_chain_layout* layout, uint64_t* n_words);
int glp_header_chain_leaf_inputs(glp_ctx* ctx, const glp_header_chain_layout* layout, const uint8_t* d_headers, const uint8_t* start_hash32,
                                 uint64_t first_height, uint64_t n, uint64_t* d_inputs, size_t input_stride, uint8_t* d_hashes,
                                 int32_t* h_status);
int glp_header_chain_last_input_counts(glp_ctx* ctx, uint32_t* n_launches, uint32_t* n_host_syncs);
int glp_header_chain_leaf_inputs_host(const glp_header_chain_layout* layout, const uint8_t* headers, const uint8_t* start_hash32,
                                      uint64_t first_height, uint64_t n, uint64_t* inputs, size_t input_stride, uint8_t* hashes,
                                      int32_t* status);

/* ---- Multi-GPU exchange (row a11 / SURVEY §8e, §8(b) glp_allgather_proofs; upstream name recalled: plonky2x mapreduce) ----
 * Leaf subproofs shard one per GPU, one process (and one ctx) per GPU.  The exchange is ONE RCCL all-gather of fixed-size
 * blocks over xGMI, on the ctx's stream.  Bootstrap as NCCL does: rank 0 makes the id and hands its GLP_COMM_ID_BYTES bytes
 * to the other ranks out of band (file, socket, environment, MPI, torch.distributed ...); then EVERY rank calls
 * glp_comm_init with the same id (collective).  One communicator per ctx; glp_destroy tears it down.
 * Block format used by the MapReduce host (0-kno-blobstreamx_amd/mapreduce.py::pack_leaves): per leaf a 16-byte header
 * (u64 leaf index, u64 payload length; index 2^64-1 = unused row) then the proof zero-padded to the agreed length. */
#define GLP_COMM_ID_BYTES 128
int glp_comm_unique_id(uint8_t* id_out /* GLP_COMM_ID_BYTES */);
int glp_comm_init(glp_ctx* ctx, const uint8_t* id /* GLP_COMM_ID_BYTES */, int rank, int nranks);
int glp_comm_rank(glp_ctx* ctx, int* rank, int* nranks);
int glp_comm_destroy(glp_ctx* ctx);       /* the communicator is gone afterwards either way; non-OK = it did not go cleanly */
/* Staging for the exchange lives with the communicator (allocated by glp_comm_init for blocks up to 4 MiB), so a collective entry point
 * cannot fail locally before it enters RCCL and strand its peers.  Ranks about to exchange LARGER blocks call glp_comm_reserve first (no
 * collective inside) and agree on the result, e.g. through glp_allreduce_min_u64.  Any non-OK return from glp_allgather_proofs /
 * glp_allreduce_min_u64 means the ranks may be out of step: abort the job on every rank. */
int glp_comm_reserve(glp_ctx* ctx, size_t padded_len);
/* every rank passes padded_len bytes (host); h_all receives nranks * padded_len bytes, rank r's block at r * padded_len */
int glp_allgather_proofs(glp_ctx* ctx, const uint8_t* h_mine, size_t padded_len, uint8_t* h_all);
/* element-wise minimum over the ranks, in place (the Reduce step's verdicts); n <= 4096 words */
int glp_allreduce_min_u64(glp_ctx* ctx, uint64_t* h_io, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* GLPROVER_H */
