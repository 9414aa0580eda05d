// verify.hip — native verifier of the build-defined proofs (DESIGN.md §3.5 FRI opening proof, §3.6
// circuit proof).  SURVEY.md §8a rows a5/a8/a12 seen from the consuming side and the body of the
// MapReduce Reduce step (row a11) as far as this build goes: the gathered leaf proofs are verified
// here, natively, instead of inside a recursive circuit.  Upstream names (recalled, unverified;
// reference file:line NONE — the mount is empty): plonky2::plonk::verifier::verify,
// fri::verifier::verify_fri_proof.
//
// The single verifiers are host C++ (verify_plan.h): a verification is ~5,000 Poseidon permutations and a few hundred
// extension-field operations.  Host on purpose for the TRANSCRIPT and the PLONK identity — a serial dependency
// chain, the same reason the prover's challenger runs on the host.  Not so for the queries: the loop over the queries
// is independent per (proof, query) and is most of the permutations, and the batched entry points at the end of the
// first half of this file (glp_plonk_verify_batch, glp_fri_verify_batch) run it on the device for
// B proofs at once (verify_batch_kernels.cuh), the host keeping the serial part per proof.  Both use the same field
// primitives (gl_field.cuh, portable forms) and the same permutation body (hash_kernels.cuh) with the constants
// injected into the ctx.  tests/fri_verifier.py and tests/plonk_ref.py (Python big-int) stay the independent
// checkers of both the prover and this file.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#include "glp_ctx.h"
#include "hash_state.h"
#include "challenger.h"
#include "plonk_gates.h"
#include "nnf25519.h"
#include "witness_plan.h"
#include "verify_plan.h"
#include "verify_batch_kernels.cuh"

using namespace glp_verify;

namespace {
bool make_hasher(glp_ctx* c, Hasher& h, glp_challenger& ch) {
    if (!c->hash || !c->hash->have_consts) { glp_set_err(c, "Poseidon constants not set (glp_set_poseidon_constants)"); return false; }
    init_hasher(c->hash->h_consts, c->hash->small_mds, h, ch);
    return true;
}
// the single verifiers' reason goes to the ctx's error text, as "proof rejected: <reason>"
int to_ctx(glp_ctx* c, int rc, const char* text) {
    if (rc == GLP_E_REJECT) glp_set_err(c, "%s", text);
    return rc;
}

// ---- the batched verifiers ---------------------------------------------------------------------------------------------------------
typedef GlpPoolBuf DBuf;
#define GLP_VB_CHUNK_ITEMS (1ull << 30)

// the device phase of one chunk's plan: one staging block up (descriptors | tables | items | tree table | keys | proof words), two launches,
// the keys back, one synchronise.  `up` (the staging block) and `keys` belong to the CALLER's frame: the asynchronous copies read and write them,
// and on an error return the caller synchronises the stream before either goes away.
int device_phase(glp_ctx* c, const VerifyPlan& P, const std::vector<const u64*>& words, std::vector<u64>& up, std::vector<unsigned long long>& keys,
                 u32* counts) {
    const size_t nd = P.desc.size();
    keys.assign(nd, GLP_VB_KEY_NONE);
    if (nd == 0 || P.arith.empty()) return GLP_OK;
    std::vector<u64> items;
    std::vector<u32> tree_first;
    flatten_items(P, items, tree_first);
    const size_t n_merkle = items.size(), n_arith = P.arith.size();
    for (auto& it : P.arith) items.push_back((u64)it.desc | ((u64)it.q << 32));
    const size_t w_desc = nd * (sizeof(GlpVerifyDesc) / 8), w_aux = P.aux.size(), w_items = items.size(), w_tree = (tree_first.size() + 1) / 2, w_keys = nd;
    const size_t o_aux = w_desc, o_items = o_aux + w_aux, o_tree = o_items + w_items, o_keys = o_tree + w_tree, o_slab = o_keys + w_keys;
    up.assign(o_slab + P.slab_words, 0);
    memcpy(up.data(), P.desc.data(), w_desc * 8);
    if (w_aux) memcpy(up.data() + o_aux, P.aux.data(), w_aux * 8);
    memcpy(up.data() + o_items, items.data(), w_items * 8);
    memcpy(up.data() + o_tree, tree_first.data(), tree_first.size() * 4);
    for (size_t k = 0; k < nd; k++) up[o_keys + k] = GLP_VB_KEY_NONE;
    for (size_t k = 0; k < nd; k++) {
        const size_t used = (k + 1 < nd ? P.desc[k + 1].base : P.slab_words) - P.desc[k].base;
        memcpy(up.data() + o_slab + P.desc[k].base, words[k], used * 8);
    }
    DBuf d_up(c);
    if (d_up.alloc(up.size() * 8) != hipSuccess) return GLP_E_NOMEM;
    GLP_HIPCHK(c, hipMemcpyAsync(d_up.p, up.data(), up.size() * 8, hipMemcpyHostToDevice, c->stream));
    GlpVerifyArgs a;
    memset(&a, 0, sizeof(a));
    a.desc = reinterpret_cast<const GlpVerifyDesc*>(d_up.u());
    a.aux = d_up.u() + o_aux; a.items = d_up.u() + o_items; a.tree_first = reinterpret_cast<const u32*>(d_up.u() + o_tree);
    a.keys = reinterpret_cast<unsigned long long*>(d_up.u() + o_keys); a.slab = d_up.u() + o_slab;
    a.n_trees = (u32)P.by_tree.size(); a.n_items = n_merkle;
    a.k = glp_dev_consts(c->hash);
    const bool small = c->hash->small_mds && !getenv("GLP_K7_GENERIC_MDS");
    if (n_merkle) {
        const dim3 g((unsigned)((n_merkle + GLP_VB_BLOCK - 1) / GLP_VB_BLOCK)), blk(GLP_VB_BLOCK);
        if (small) hipLaunchKernelGGL(glp_verify_merkle_kernel<true>, g, blk, 0, c->stream, a);
        else hipLaunchKernelGGL(glp_verify_merkle_kernel<false>, g, blk, 0, c->stream, a);
        GLP_HIPCHK(c, hipGetLastError());
        counts[0]++;
    }
    a.items = d_up.u() + o_items + n_merkle; a.n_items = n_arith;
    hipLaunchKernelGGL(glp_verify_arith_kernel<0>, dim3((unsigned)((n_arith + GLP_VB_BLOCK - 1) / GLP_VB_BLOCK)), dim3(GLP_VB_BLOCK), 0, c->stream, a);
    GLP_HIPCHK(c, hipGetLastError());
    counts[0]++;
    GLP_HIPCHK(c, hipMemcpyAsync(keys.data(), a.keys, nd * 8, hipMemcpyDeviceToHost, c->stream));
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    counts[1]++;
    return GLP_OK;
}

// c == nullptr: the ctx-less form (items on the host, constants in h0)
int verify_batch(glp_ctx* c, const Hasher& h0, const BatchArgs& A, u32* out_counts) {
    std::vector<ProofState> S(A.B);
    glp_challenger ch;                           // one transcript object for the call, reset per proof
    ch.consts = h0.consts; ch.small_mds = h0.small_mds;
    u32 counts[4] = {0, 0, 0, 0};
    int rc = GLP_OK;
    for (u32 i0 = 0; i0 < A.B && rc == GLP_OK;) {
        // a chunk: proofs from i0 while their Merkle items stay below the limit of one launch
        VerifyPlan P;
        std::vector<const u64*> words;
        u32 i1 = i0;
        while (i1 < A.B && (i1 == i0 || P.n_merkle() < GLP_VB_CHUNK_ITEMS)) {
            const size_t nd = P.desc.size();
            host_phase(A, h0, ch, i1, i1 + 1, S, P);
            if (P.desc.size() > nd) words.push_back((const u64*)A.proofs[i1]);
            i1++;
        }
        std::vector<unsigned long long> keys(P.desc.size(), GLP_VB_KEY_NONE);
        std::vector<u64> up;                     // the chunk's staging block: lives until the stream has been synchronised
        if (c) {
            rc = device_phase(c, P, words, up, keys, counts);
            if (rc) (void)hipStreamSynchronize(c->stream);     // copies in flight read `up` and write `keys`, both of this frame (not counted: not on the path of a verdict)
        } else
            glp_vb_run_host(P, words.data(), h0.k(), h0.small_mds, keys.data());
        if (rc == GLP_OK) {
            // descriptors are numbered per chunk: settle with the chunk's keys
            settle(A, S, keys.data(), i0, i1, &counts[2], &counts[3]);
        }
        i0 = i1;
    }
    for (int k = 0; k < 4; k++) out_counts[k] = counts[k];
    return rc;
}

int first_refused(const BatchArgs& A) {
    for (u32 i = 0; i < A.B; i++)
        if (A.verdicts[i].status != GLP_OK) return (int)i;
    return -1;
}

int batch_entry(glp_ctx* c, const BatchArgs& A, const char* who) {
    for (int k = 0; k < 4; k++) c->verify_batch_counts[k] = 0;
    if (A.B == 0) return GLP_OK;
    if (const char* bad = batch_args_bad(A)) { glp_set_err(c, "%s: bad argument (%s)", who, bad); return GLP_E_INVALID; }
    Hasher h;
    glp_challenger ch;
    if (!make_hasher(c, h, ch)) return GLP_E_STATE;
    const int rc = verify_batch(c, h, A, c->verify_batch_counts);
    if (rc != GLP_OK) return rc;
    const int bad = first_refused(A);
    if (bad >= 0) {
        const glp_verify_verdict& v = A.verdicts[bad];
        if (v.query != 0xFFFFFFFFu) glp_set_err(c, "%s: proof %d rejected: %s (query %u)", who, bad, glp_vr_text(v.reason), v.query);
        else glp_set_err(c, "%s: proof %d rejected: %s", who, bad, glp_vr_text(v.reason));
    }
    return GLP_OK;
}
}  // namespace

extern "C" int glp_plonk_verify_batch(glp_ctx* c, const uint8_t* const* h_proofs, const size_t* lens, uint32_t B, const uint64_t* h_circuit_cap,
                                      size_t cap_words, const uint64_t* h_public, size_t n_public, uint32_t min_queries, uint32_t min_pow_bits,
                                      glp_verify_verdict* h_verdicts, uint64_t* h_digests) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    const BatchArgs A{true, h_proofs, lens, B, h_circuit_cap, cap_words, h_public, n_public, min_queries, min_pow_bits, 1, h_verdicts, h_digests, nullptr};
    return batch_entry(c, A, "glp_plonk_verify_batch");
}
extern "C" int glp_fri_verify_batch(glp_ctx* c, const uint8_t* const* h_proofs, const size_t* lens, uint32_t B, uint32_t min_queries,
                                    uint32_t min_pow_bits, uint32_t min_rate_bits, glp_verify_verdict* h_verdicts, glp_fri_statement* statements) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    const BatchArgs A{false, h_proofs, lens, B, nullptr, 0, nullptr, 0, min_queries, min_pow_bits, min_rate_bits, h_verdicts, nullptr, statements};
    return batch_entry(c, A, "glp_fri_verify_batch");
}
extern "C" const char* glp_verify_reason_text(uint32_t reason) { return glp_vr_text(reason); }
extern "C" int glp_verify_last_batch_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs, uint32_t* n_on_device, uint32_t* n_fallback) {
    if (!c) return GLP_E_INVALID;
    if (n_launches) *n_launches = c->verify_batch_counts[0];
    if (n_host_syncs) *n_host_syncs = c->verify_batch_counts[1];
    if (n_on_device) *n_on_device = c->verify_batch_counts[2];
    if (n_fallback) *n_fallback = c->verify_batch_counts[3];
    return GLP_OK;
}
static int batch_host_entry(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const BatchArgs& A, uint32_t* n_on_device,
                            uint32_t* n_fallback) {
    if (n_on_device) *n_on_device = 0;
    if (n_fallback) *n_fallback = 0;
    Hasher h;
    glp_challenger ch;
    if (!make_hasher_from(h_rc, h_mds_circ, h_mds_diag, h, ch)) return GLP_E_INVALID;
    if (A.B == 0) return GLP_OK;
    if (batch_args_bad(A)) return GLP_E_INVALID;
    u32 counts[4];
    const int rc = verify_batch(nullptr, h, A, counts);
    if (n_on_device) *n_on_device = counts[2];
    if (n_fallback) *n_fallback = counts[3];
    return rc;
}
extern "C" int glp_plonk_verify_batch_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* const* h_proofs,
                                           const size_t* lens, uint32_t B, const uint64_t* h_circuit_cap, size_t cap_words, const uint64_t* h_public,
                                           size_t n_public, uint32_t min_queries, uint32_t min_pow_bits, glp_verify_verdict* h_verdicts,
                                           uint64_t* h_digests, uint32_t* n_on_device, uint32_t* n_fallback) {
    const BatchArgs A{true, h_proofs, lens, B, h_circuit_cap, cap_words, h_public, n_public, min_queries, min_pow_bits, 1, h_verdicts, h_digests, nullptr};
    return batch_host_entry(h_rc, h_mds_circ, h_mds_diag, A, n_on_device, n_fallback);
}
extern "C" int glp_fri_verify_batch_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* const* h_proofs,
                                         const size_t* lens, uint32_t B, uint32_t min_queries, uint32_t min_pow_bits, uint32_t min_rate_bits,
                                         glp_verify_verdict* h_verdicts, glp_fri_statement* statements, uint32_t* n_on_device, uint32_t* n_fallback) {
    const BatchArgs A{false, h_proofs, lens, B, nullptr, 0, nullptr, 0, min_queries, min_pow_bits, min_rate_bits, h_verdicts, nullptr, statements};
    return batch_host_entry(h_rc, h_mds_circ, h_mds_diag, A, n_on_device, n_fallback);
}

extern "C" int glp_fri_verify_ex(glp_ctx* c, const uint8_t* proof, size_t len, uint32_t min_queries, uint32_t min_pow_bits,
                                 uint32_t min_rate_bits, glp_fri_statement* statement) {
    if (!c) return GLP_E_INVALID;
    if (!proof_args_ok(proof, len)) { glp_set_err(c, "glp_fri_verify: bad argument (proof must be 8-byte aligned words)"); return GLP_E_INVALID; }
    Hasher h;
    glp_challenger ch;
    if (!make_hasher(c, h, ch)) return GLP_E_STATE;
    char text[160];
    Reject rj{text, sizeof(text)};
    return to_ctx(c, fri_verify_entry(rj, h, ch, proof, len, min_queries, min_pow_bits, min_rate_bits, statement), text);
}
extern "C" int glp_fri_verify(glp_ctx* c, const uint8_t* proof, size_t len, uint32_t min_queries, uint32_t min_pow_bits) {
    return glp_fri_verify_ex(c, proof, len, min_queries, min_pow_bits, 1, nullptr);
}

extern "C" int glp_plonk_verify_ex(glp_ctx* c, const uint8_t* proof, size_t len, const uint64_t* h_circuit_cap, size_t cap_words,
                                   const uint64_t* h_public, size_t n_public, uint32_t min_queries, uint32_t min_pow_bits) {
    if (!c) return GLP_E_INVALID;
    if (!proof_args_ok(proof, len)) { glp_set_err(c, "glp_plonk_verify: bad argument (proof must be 8-byte aligned words)"); return GLP_E_INVALID; }
    Hasher h;
    glp_challenger ch;
    if (!make_hasher(c, h, ch)) return GLP_E_STATE;
    char text[160];
    Reject rj{text, sizeof(text)};
    return to_ctx(c, plonk_verify_entry(rj, h, ch, proof, len, h_circuit_cap, cap_words, h_public, n_public, min_queries, min_pow_bits), text);
}
extern "C" int glp_plonk_verify(glp_ctx* c, const uint8_t* proof, size_t len, const uint64_t* h_circuit_cap, size_t cap_words,
                                uint32_t min_queries, uint32_t min_pow_bits) {
    return glp_plonk_verify_ex(c, proof, len, h_circuit_cap, cap_words, nullptr, 0, min_queries, min_pow_bits);
}
extern "C" int glp_plonk_proof_digest(glp_ctx* c, const uint8_t* proof, size_t len, uint64_t* h_out4) {
    if (!c) return GLP_E_INVALID;
    if (!proof_args_ok(proof, len) || !h_out4) { glp_set_err(c, "glp_plonk_proof_digest: bad argument"); return GLP_E_INVALID; }
    Hasher h;
    glp_challenger ch;
    if (!make_hasher(c, h, ch)) return GLP_E_STATE;
    const int rc = proof_digest(h, proof, len, h_out4);
    if (rc) glp_set_err(c, "glp_plonk_proof_digest: not a circuit proof of this format");
    return rc;
}
extern "C" int glp_plonk_proof_digest_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* proof, size_t len,
                                           uint64_t* h_out4) {
    Hasher h;
    glp_challenger ch;
    if (!proof_args_ok(proof, len) || !h_out4 || !make_hasher_from(h_rc, h_mds_circ, h_mds_diag, h, ch)) return GLP_E_INVALID;
    return proof_digest(h, proof, len, h_out4);
}

// the permutation on the host (n states of 12 words, in place): what the circuit builder and a light client hash with
extern "C" int glp_poseidon_permute_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, uint64_t* states, size_t n) {
    Hasher h;
    glp_challenger ch;
    if ((!states && n) || !make_hasher_from(h_rc, h_mds_circ, h_mds_diag, h, ch)) return GLP_E_INVALID;
    for (size_t i = 0; i < n; i++) {
        u64 st[12];
        for (int k = 0; k < 12; k++) { if (states[12 * i + k] >= GL_P) return GLP_E_INVALID; st[k] = states[12 * i + k]; }
        h.permute(st);
        for (int k = 0; k < 12; k++) states[12 * i + k] = st[k];
    }
    return GLP_OK;
}

// ---- witness evaluator for circuits recorded by the host builder (recursion.py::WitnessProgram) -------------------------------------
// A recorded circuit is a straight-line program over its variables: arithmetic gates, free inputs, bit extractions, inverses, Poseidon
// permutations — each op defines NEW variables from earlier ones, so one forward pass computes the whole witness.  This file walks the ops
// one after the other on the host (segments on several threads: glp_witness_eval_mt).  The dependency chain is far shorter than the program —
// a signature leaf is 1.2 M ops in 8 k dependency levels — which is what the batched device evaluator uses (witness_plan.h compiles the level
// schedule, witness_kernels.cuh runs it: glp_witness_eval_device); both decode with one table of op lengths (GLP_WIT_OP_LEN).  Program words (u64):
//   0 ARITH  w x y z c0 c1 c2   w = c0*x*y + c1*z + c2        1 INPUT w i          w = inputs[i]
//   2 BIT    w x k              w = bit k of canonical x        3 INV   w x          w = 1/x (0 -> 0)
//   4 EINV   w0 w1 x0 x1        (w0,w1) = 1/(x0 + x1 X)          5 ZERO  w            w = 0
//   6 POSEIDON o0..o11 i0..i11  outputs = permutation(inputs)
//   7 SHA_E T1 e_new e f g h d w K    8 SHA_A a_new a b c T1    9 SHA_W w_new w16 w15 w7 w2    10 ADD32 s x y      (the SHA rows of plonk_gates.h;
//   11 BITS w x shift bits   w = (x >> shift) mod 2^bits     12 POSEIDON_SWAP o0..o11 i0..i11 s   the Poseidon row with its swap bit
//   13 EXTMULADD w0 w1 x0 x1 y0 y1 z0 z1   w = x * y + z in the quadratic extension (the extension-arithmetic row)
//   14 NNF_MUL first a0..a10 b0..b10   variables first..first+43 = remainder, quotient and column carries of a product in the NON-NATIVE field
//      F_q, q = 2^255 - 19, on 24-bit limbs (nnf25519.h): witness values only, the circuit constrains them with arithmetic gates and range checks
//     an input that is not a 32-bit word -> GLP_E_REJECT with *first_bad = (size_t)-1: no witness satisfies the row)
// eq_pairs: 2*n_eq variable indices that must hold equal values (the circuit's copy constraints between DIFFERENT variables): the first
// violated pair is reported through *first_bad and the call returns GLP_E_REJECT — the witness does not satisfy the circuit (e.g. the
// verifier circuit was fed a proof that does not verify).
// One range [pc, end) of a witness program.  OWNED: the range is a parallel segment with id `me` — it may read only variables written by the
// prefix (owner 0) or by itself, and write only variables nobody has written, so concurrent segments cannot race; the owner table makes a
// wrong independence claim an error instead of a wrong witness.
template <bool OWNED>
static int witness_run(const Hasher& h, const u64* prog, size_t pc, size_t end, const u64* inputs, size_t n_inputs, u64* values, size_t n_values,
                       uint16_t* owner, uint16_t me) {
    auto ok = [&](u64 v) { return v < n_values; };
    auto rd = [&](u64 v) {
        if constexpr (OWNED) { const uint16_t o = __atomic_load_n(&owner[v], __ATOMIC_RELAXED); return o == 0 || o == me; }
        return true;
    };
    auto wr = [&](u64 v) {
        if constexpr (OWNED) {
            uint16_t expected = 0xFFFF;                      // claim the variable: two segments racing for it cannot both succeed
            if (!__atomic_compare_exchange_n(&owner[v], &expected, me, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED) && expected != me) return false;
        } else if (owner) owner[v] = me;
        return true;
    };
    while (pc < end) {
        const u64 op = prog[pc];
        const u64* a = prog + pc + 1;
        switch (op) {
            case 0: {
                if (pc + GLP_WIT_OP_LEN[0] > end || !ok(a[0]) || !ok(a[1]) || !ok(a[2]) || !ok(a[3]) || a[4] >= GL_P || a[5] >= GL_P || a[6] >= GL_P) return GLP_E_INVALID;
                if (!rd(a[1]) || !rd(a[2]) || !rd(a[3]) || !wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = gl_add(gl_add(gl_mul(a[4], gl_mul(values[a[1]], values[a[2]])), gl_mul(a[5], values[a[3]])), a[6]);
                pc += GLP_WIT_OP_LEN[0];
                break;
            }
            case 1:
                if (pc + GLP_WIT_OP_LEN[1] > end || !ok(a[0]) || a[1] >= n_inputs || inputs[a[1]] >= GL_P || !wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = inputs[a[1]];
                pc += GLP_WIT_OP_LEN[1];
                break;
            case 2:
                if (pc + GLP_WIT_OP_LEN[2] > end || !ok(a[0]) || !ok(a[1]) || a[2] >= 64 || !rd(a[1]) || !wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = (values[a[1]] >> a[2]) & 1ull;
                pc += GLP_WIT_OP_LEN[2];
                break;
            case 3:
                if (pc + GLP_WIT_OP_LEN[3] > end || !ok(a[0]) || !ok(a[1]) || !rd(a[1]) || !wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = values[a[1]] ? gl_inv(values[a[1]]) : 0;
                pc += GLP_WIT_OP_LEN[3];
                break;
            case 4: {
                if (pc + GLP_WIT_OP_LEN[4] > end || !ok(a[0]) || !ok(a[1]) || !ok(a[2]) || !ok(a[3]) || !rd(a[2]) || !rd(a[3]) || !wr(a[0]) || !wr(a[1])) return GLP_E_INVALID;
                const gl_ext2 x{values[a[2]], values[a[3]]};
                const gl_ext2 r = (x.a || x.b) ? ext_inv(x) : gl_ext2{0, 0};
                values[a[0]] = r.a; values[a[1]] = r.b;
                pc += GLP_WIT_OP_LEN[4];
                break;
            }
            case 5:
                if (pc + GLP_WIT_OP_LEN[5] > end || !ok(a[0]) || !wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = 0;
                pc += GLP_WIT_OP_LEN[5];
                break;
            case 6: {
                if (pc + GLP_WIT_OP_LEN[6] > end) return GLP_E_INVALID;
                u64 st[12];
                for (int i = 0; i < 12; i++) { if (!ok(a[i]) || !ok(a[12 + i]) || !rd(a[12 + i])) return GLP_E_INVALID; st[i] = values[a[12 + i]]; }
                h.permute(st);
                for (int i = 0; i < 12; i++) { if (!wr(a[i])) return GLP_E_INVALID; values[a[i]] = st[i]; }
                pc += GLP_WIT_OP_LEN[6];
                break;
            }
            // SHA-256 rows (plonk_gates.h): every input must be a 32-bit word (T1: < 2^35) — anything else cannot satisfy the row
            case 7: {   // SHA_E  T1 e_new | e f g h d w | K
                if (pc + GLP_WIT_OP_LEN[7] > end || a[8] > 0xFFFFFFFFull) return GLP_E_INVALID;
                for (int i = 0; i < 8; i++) if (!ok(a[i])) return GLP_E_INVALID;
                for (int i = 2; i < 8; i++) if (!rd(a[i])) return GLP_E_INVALID;
                u64 v[6];
                for (int i = 0; i < 6; i++) { v[i] = values[a[2 + i]]; if (v[i] >> 32) return GLP_E_REJECT; }
                if (!wr(a[0]) || !wr(a[1])) return GLP_E_INVALID;
                const u64 t1 = v[3] + glp_sha_S1(v[0]) + glp_sha_ch(v[0], v[1], v[2]) + a[8] + v[5];
                values[a[0]] = t1;
                values[a[1]] = (v[4] + t1) & 0xFFFFFFFFull;
                pc += GLP_WIT_OP_LEN[7];
                break;
            }
            case 8: {   // SHA_A  a_new | a b c T1
                if (pc + GLP_WIT_OP_LEN[8] > end) return GLP_E_INVALID;
                for (int i = 0; i < 5; i++) if (!ok(a[i])) return GLP_E_INVALID;
                for (int i = 1; i < 5; i++) if (!rd(a[i])) return GLP_E_INVALID;
                const u64 va = values[a[1]], vb = values[a[2]], vc = values[a[3]], t1 = values[a[4]];
                if ((va | vb | vc) >> 32 || t1 >> 35) return GLP_E_REJECT;
                if (!wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = (t1 + glp_sha_S0(va) + glp_sha_maj(va, vb, vc)) & 0xFFFFFFFFull;
                pc += GLP_WIT_OP_LEN[8];
                break;
            }
            case 9: {   // SHA_W  w_new | w16 w15 w7 w2
                if (pc + GLP_WIT_OP_LEN[9] > end) return GLP_E_INVALID;
                for (int i = 0; i < 5; i++) if (!ok(a[i])) return GLP_E_INVALID;
                for (int i = 1; i < 5; i++) if (!rd(a[i])) return GLP_E_INVALID;
                const u64 w16 = values[a[1]], w15 = values[a[2]], w7 = values[a[3]], w2 = values[a[4]];
                if ((w16 | w15 | w7 | w2) >> 32) return GLP_E_REJECT;
                if (!wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = (w16 + glp_sha_s0(w15) + w7 + glp_sha_s1(w2)) & 0xFFFFFFFFull;
                pc += GLP_WIT_OP_LEN[9];
                break;
            }
            case 10: {  // ADD32  s | x y
                if (pc + GLP_WIT_OP_LEN[10] > end || !ok(a[0]) || !ok(a[1]) || !ok(a[2]) || !rd(a[1]) || !rd(a[2])) return GLP_E_INVALID;
                const u64 x = values[a[1]], y = values[a[2]];
                if ((x | y) >> 32) return GLP_E_REJECT;
                if (!wr(a[0])) return GLP_E_INVALID;
                values[a[0]] = (x + y) & 0xFFFFFFFFull;
                pc += GLP_WIT_OP_LEN[10];
                break;
            }
            case 12: {  // POSEIDON_SWAP o0..o11 | i0..i11 | s:  the permutation of the input with its first two 4-word blocks exchanged when s = 1
                if (pc + GLP_WIT_OP_LEN[12] > end || !ok(a[24]) || !rd(a[24])) return GLP_E_INVALID;
                u64 st[12];
                for (int i = 0; i < 12; i++) { if (!ok(a[i]) || !ok(a[12 + i]) || !rd(a[12 + i])) return GLP_E_INVALID; st[i] = values[a[12 + i]]; }
                const u64 sw = values[a[24]];
                if (sw > 1) return GLP_E_REJECT;                       // not a bit: the row's booleanity constraint cannot hold
                if (sw) for (int i = 0; i < 4; i++) { const u64 t = st[i]; st[i] = st[4 + i]; st[4 + i] = t; }
                h.permute(st);
                for (int i = 0; i < 12; i++) { if (!wr(a[i])) return GLP_E_INVALID; values[a[i]] = st[i]; }
                pc += GLP_WIT_OP_LEN[12];
                break;
            }
            case 13: {  // EXTMULADD  w0 w1 | x0 x1 y0 y1 z0 z1:  w = x * y + z in F_p[X]/(X^2 - 7)
                if (pc + GLP_WIT_OP_LEN[13] > end) return GLP_E_INVALID;
                for (int i = 0; i < 8; i++) if (!ok(a[i])) return GLP_E_INVALID;
                for (int i = 2; i < 8; i++) if (!rd(a[i])) return GLP_E_INVALID;
                const gl_ext2 x{values[a[2]], values[a[3]]}, y{values[a[4]], values[a[5]]}, z{values[a[6]], values[a[7]]};
                const gl_ext2 w = gl_ext_add(gl_ext_mul(x, y), z);
                if (!wr(a[0]) || !wr(a[1])) return GLP_E_INVALID;
                values[a[0]] = w.a; values[a[1]] = w.b;
                pc += GLP_WIT_OP_LEN[13];
                break;
            }
            case 14: {  // NNF_MUL  first | a0..a10 | b0..b10:  the 44 hint values of a product in F_q, q = 2^255 - 19 (nnf25519.h): r, k, carries
                if (pc + GLP_WIT_OP_LEN[14] > end || a[0] >= n_values || a[0] + GLP_NNF_OUT > n_values) return GLP_E_INVALID;
                u64 va[GLP_NNF_LIMBS], vb[GLP_NNF_LIMBS], out[GLP_NNF_OUT];
                for (int i = 0; i < GLP_NNF_LIMBS; i++) {
                    const u64 ia = a[1 + i], ib = a[1 + GLP_NNF_LIMBS + i];
                    if (!ok(ia) || !ok(ib) || !rd(ia) || !rd(ib)) return GLP_E_INVALID;
                    va[i] = values[ia]; vb[i] = values[ib];
                }
                if (!glp_nnf::mul_hints(va, vb, out)) return GLP_E_REJECT;         // an operand limb out of range: no witness satisfies the product rows
                for (int i = 0; i < GLP_NNF_OUT; i++) { if (!wr(a[0] + i)) return GLP_E_INVALID; values[a[0] + i] = out[i]; }
                pc += GLP_WIT_OP_LEN[14];
                break;
            }
            case 11: {  // BITS  w | x shift bits:  w = (x >> shift) mod 2^bits
                if (pc + GLP_WIT_OP_LEN[11] > end || !ok(a[0]) || !ok(a[1]) || a[2] >= 64 || a[3] == 0 || a[3] > 64 || !rd(a[1]) || !wr(a[0])) return GLP_E_INVALID;
                const u64 sh = values[a[1]] >> a[2];
                values[a[0]] = a[3] >= 64 ? sh : (sh & ((1ull << a[3]) - 1));
                pc += GLP_WIT_OP_LEN[11];
                break;
            }
            default: return GLP_E_INVALID;
        }
    }
    return GLP_OK;
}

// seg_bounds (n_seg + 1 ascending word offsets on op boundaries, or NULL): the ops of [seg_bounds[k], seg_bounds[k+1]) are n_seg mutually
// independent segments — each reads only what the prefix [0, seg_bounds[0]) or itself wrote — evaluated on up to n_threads host threads; the
// tail [seg_bounds[n_seg], prog_words) runs after them.  The independence claim is CHECKED while running (GLP_E_INVALID when it is false).
extern "C" int glp_witness_eval_mt(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint64_t* prog, size_t prog_words,
                                   const uint64_t* inputs, size_t n_inputs, uint64_t* values, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                                   size_t* first_bad, const uint64_t* seg_bounds, size_t n_seg, uint32_t n_threads) {
    Hasher h;
    glp_challenger ch;
    if (!prog || !values || (!inputs && n_inputs) || (!eq_pairs && n_eq) || !make_hasher_from(h_rc, h_mds_circ, h_mds_diag, h, ch)) return GLP_E_INVALID;
    if (first_bad) *first_bad = (size_t)-1;
    if (!seg_bounds || n_seg < 2 || n_threads < 2) {
        const int rc = witness_run<false>(h, prog, 0, prog_words, inputs, n_inputs, values, n_values, nullptr, 0);
        if (rc != GLP_OK) return rc;
    } else {
        if (n_seg >= 0xFFFE) return GLP_E_INVALID;
        for (size_t k = 0; k <= n_seg; k++)
            if (seg_bounds[k] > prog_words || (k && seg_bounds[k] < seg_bounds[k - 1])) return GLP_E_INVALID;
        std::vector<uint16_t> owner(n_values, (uint16_t)0xFFFF);
        int rc = witness_run<false>(h, prog, 0, (size_t)seg_bounds[0], inputs, n_inputs, values, n_values, owner.data(), 0);
        if (rc != GLP_OK) return rc;
        std::atomic<size_t> next{0};
        std::atomic<int> status{GLP_OK};
        auto worker = [&]() {
            for (;;) {
                const size_t k = next.fetch_add(1);
                if (k >= n_seg || status.load() != GLP_OK) return;
                const int r = witness_run<true>(h, prog, (size_t)seg_bounds[k], (size_t)seg_bounds[k + 1], inputs, n_inputs, values, n_values, owner.data(),
                                                (uint16_t)(k + 1));
                if (r != GLP_OK) status.store(r);
            }
        };
        const size_t nt = n_threads < n_seg ? n_threads : n_seg;
        std::vector<std::thread> pool;
        try {
            for (size_t t = 1; t < nt; t++) pool.emplace_back(worker);
        } catch (...) {
            // the host refused another thread: the ones that started (and this one) share the segments — no exception crosses the C ABI
        }
        worker();
        for (auto& t : pool) t.join();
        if (status.load() != GLP_OK) return status.load();
        rc = witness_run<false>(h, prog, (size_t)seg_bounds[n_seg], prog_words, inputs, n_inputs, values, n_values, nullptr, 0);
        if (rc != GLP_OK) return rc;
    }
    auto ok = [&](u64 v) { return v < n_values; };
    for (size_t k = 0; k < n_eq; k++) {
        if (!ok(eq_pairs[2 * k]) || !ok(eq_pairs[2 * k + 1])) return GLP_E_INVALID;
        if (values[eq_pairs[2 * k]] != values[eq_pairs[2 * k + 1]]) { if (first_bad) *first_bad = k; return GLP_E_REJECT; }
    }
    return GLP_OK;
}
extern "C" int glp_witness_eval(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint64_t* prog, size_t prog_words,
                                const uint64_t* inputs, size_t n_inputs, uint64_t* values, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                                size_t* first_bad) {
    return glp_witness_eval_mt(h_rc, h_mds_circ, h_mds_diag, prog, prog_words, inputs, n_inputs, values, n_values, eq_pairs, n_eq, first_bad, nullptr, 0, 1);
}

extern "C" int glp_plonk_proof_public_inputs(const uint8_t* proof, size_t len, uint64_t* h_out, size_t* n_words) {
    if (!proof_args_ok(proof, len) || !n_words || (!h_out && *n_words)) return GLP_E_INVALID;
    const u64* w = (const u64*)proof;
    if (len / 8 < 8 || w[0] != PLONK_TAG || w[6] > (1ull << 24) || 8 + w[6] > len / 8) return GLP_E_INVALID;
    const size_t k = *n_words < w[6] ? *n_words : (size_t)w[6];
    if (k) memcpy(h_out, w + 8, k * 8);
    *n_words = (size_t)w[6];
    return GLP_OK;
}

// The same verifiers for a host WITHOUT a GPU (a light client, CI): no ctx, the Poseidon constants are passed
// explicitly (360 + 12 + 12 words, the arguments of glp_set_poseidon_constants); err (may be NULL) receives the reason.
extern "C" int glp_fri_verify_host_ex(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* proof,
                                      size_t len, uint32_t min_queries, uint32_t min_pow_bits, uint32_t min_rate_bits,
                                      glp_fri_statement* statement, char* err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    Hasher h;
    glp_challenger ch;
    if (!proof_args_ok(proof, len) || !make_hasher_from(h_rc, h_mds_circ, h_mds_diag, h, ch)) return GLP_E_INVALID;
    Reject rj{err, err_len};
    return fri_verify_entry(rj, h, ch, proof, len, min_queries, min_pow_bits, min_rate_bits, statement);
}
extern "C" int glp_fri_verify_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* proof, size_t len,
                                   uint32_t min_queries, uint32_t min_pow_bits, char* err, size_t err_len) {
    return glp_fri_verify_host_ex(h_rc, h_mds_circ, h_mds_diag, proof, len, min_queries, min_pow_bits, 1, nullptr, err, err_len);
}
extern "C" int glp_plonk_verify_host_ex(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* proof, size_t len,
                                        const uint64_t* h_circuit_cap, size_t cap_words, const uint64_t* h_public, size_t n_public,
                                        uint32_t min_queries, uint32_t min_pow_bits, char* err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    Hasher h;
    glp_challenger ch;
    if (!proof_args_ok(proof, len) || !make_hasher_from(h_rc, h_mds_circ, h_mds_diag, h, ch)) return GLP_E_INVALID;
    Reject rj{err, err_len};
    return plonk_verify_entry(rj, h, ch, proof, len, h_circuit_cap, cap_words, h_public, n_public, min_queries, min_pow_bits);
}
extern "C" int glp_plonk_verify_host(const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag, const uint8_t* proof, size_t len,
                                     const uint64_t* h_circuit_cap, size_t cap_words, uint32_t min_queries, uint32_t min_pow_bits, char* err,
                                     size_t err_len) {
    return glp_plonk_verify_host_ex(h_rc, h_mds_circ, h_mds_diag, proof, len, h_circuit_cap, cap_words, nullptr, 0, min_queries, min_pow_bits, err, err_len);
}
