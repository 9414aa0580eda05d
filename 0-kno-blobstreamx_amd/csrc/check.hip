// check.hip — glp_plonk_check_witness / glp_plonk_check_witness_batch: does a wire matrix satisfy the circuit the key commits to, and if not,
// where.  The gate constraints of plonk_gates.h on the n trace rows and the copy constraints cell by cell (kernels: check_kernels.cuh), with the
// key's OWN data: the constant columns come back from the preprocessed commitment's coefficients by one forward NTT into a transient buffer,
// sigma from the key's sigma values, decoded once per key into cell indices (check_plan.h) and kept on the key.
//
// One call, whatever B is: [first call of a key: 2 decode launches] + 1 NTT call + base + (Poseidon) + (SHA) + copy launches, then ONE stream
// synchronise; the counters, and the lists the device built, come back with it.  Nothing of the prover is touched: opt-in throughout.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "glp_ctx.h"
#include "plonk_circuit.h"
#include "hash_state.h"
#include "check_kernels.cuh"

int glp_ntt_table(glp_ctx* c, int log_N, int inv, const u64** lo, const u64** hi);

namespace {
typedef GlpPoolBuf DBuf;
static_assert(sizeof(GlpCheckInst) == 16 && sizeof(GlpCheckAcc) == 40 && sizeof(glp_check_violation) == 40, "the staging block is laid out in words");
#define POOL_ALLOC(buf, bytes) do { if ((buf).alloc(bytes) != hipSuccess) return GLP_E_NOMEM; } while (0)

// host memory that the call's asynchronous copies read or write: it lives in the entry point's frame, which synchronises before it returns
struct CheckHost {
    std::vector<u64> up;                       // [B] GlpCheckInst | [B] GlpCheckAcc | [B][n_public] public inputs
    std::vector<u64> sig;                      // kn[R] | kinv[R] | status[2]
    std::vector<GlpCheckAcc> acc;              // [B] back from the device
    std::vector<glp_check_violation> lists;    // [B][max_list] back from the device
    unsigned long long status[2] = {~0ull, ~0ull};
};

// the key's sigma values -> cell indices in `idx`, a block of this CALL (2 launches); the verdict (H.status) is read after the call's synchronise,
// and only a table that decoded as a permutation is adopted by the key: whatever fails on the way, the key never holds a table that is not filled
int decode_sigma(glp_ctx* c, glp_plonk_circuit* ck, CheckHost& H, DBuf& idx, DBuf& d_sig, DBuf& hits, u32* counts) {
    const u32 log_n = ck->log_n, R = ck->R;
    const u64 n = 1ull << log_n, cells = (u64)R * n;
    POOL_ALLOC(idx, cells * 4);
    POOL_ALLOC(hits, cells * 4);
    POOL_ALLOC(d_sig, (size_t)(2 * R + 2) * 8);
    H.sig.resize(2 * R + 2);
    glp_sigma_fill_tables(log_n, R, H.sig.data(), H.sig.data() + R);
    H.sig[2 * R] = H.sig[2 * R + 1] = ~0ull;
    GLP_HIPCHK(c, hipMemcpyAsync(d_sig.p, H.sig.data(), H.sig.size() * 8, hipMemcpyHostToDevice, c->stream));
    GLP_HIPCHK(c, hipMemsetAsync(hits.p, 0, cells * 4, c->stream));
    GlpSigmaDecodeArgs da;
    memset(&da, 0, sizeof(da));
    int rc = glp_ntt_table(c, (int)log_n, 0, &da.w_lo, &da.w_hi);
    if (rc) return rc;
    rc = glp_ntt_table(c, (int)log_n, 1, &da.T.winv_lo, &da.T.winv_hi);
    if (rc) return rc;
    da.sigma_vals = ck->sigma_vals.u(); da.ks = ck->ks.u();
    da.T.kn = d_sig.u(); da.T.kinv = d_sig.u() + R; da.T.log_n = log_n; da.T.R = R;
    da.idx = (u32*)idx.p; da.hits = (u32*)hits.p; da.status = (unsigned long long*)(d_sig.u() + 2 * R);
    const unsigned blocks = (unsigned)((cells + 255) / 256);
    hipLaunchKernelGGL(glp_sigma_decode_kernel<0>, dim3(blocks), dim3(256), 0, c->stream, da);
    GLP_HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(glp_sigma_bijective_kernel<0>, dim3(blocks), dim3(256), 0, c->stream, (const u32*)hits.p, cells, da.status);
    GLP_HIPCHK(c, hipGetLastError());
    counts[0] += 2;
    GLP_HIPCHK(c, hipMemcpyAsync(H.status, da.status, 16, hipMemcpyDeviceToHost, c->stream));
    return GLP_OK;
}

int check_impl(glp_ctx* c, glp_plonk_circuit* ck, const uint64_t* const* d_wire_vals, const uint64_t* h_public, u32 B, u32 max_list, CheckHost& H,
               DBuf& fresh_idx, u32* counts) {
    const u32 log_n = ck->log_n, R = ck->R, NP = ck->n_public;
    const u64 n = 1ull << log_n;
    const u32 n_const = (u32)glp_plonk_n_const(ck->flags), M = R / GLP_PLONK_CHUNK;
    int rc;
    DBuf d_sig(c), hits(c);
    if (!ck->sigma_idx.p) {
        rc = decode_sigma(c, ck, H, fresh_idx, d_sig, hits, counts);
        if (rc) return rc;
    }
    const u32* sigma_idx = (const u32*)(ck->sigma_idx.p ? ck->sigma_idx.p : fresh_idx.p);
    // the constant columns on the trace domain, from the key: coefficients (rows 0 .. n_const-1 of the preprocessed batch) -> values
    DBuf cv(c);
    POOL_ALLOC(cv, (size_t)n_const * n * 8);
    GLP_HIPCHK(c, hipMemcpyAsync(cv.p, ck->pre.coeffs.p, (size_t)n_const * n * 8, hipMemcpyDeviceToDevice, c->stream));
    rc = glp_ntt(c, cv.u(), log_n, n_const, 0);
    if (rc) return rc;
    counts[0]++;
    // instance table, accumulators and public inputs: one staging block, one copy
    const size_t w_inst = (size_t)B * 2, w_acc = (size_t)B * 5, w_pub = (size_t)B * NP;
    H.up.assign(w_inst + w_acc + w_pub, 0);
    DBuf d_up(c), rows(c), d_lists(c);
    POOL_ALLOC(d_up, H.up.size() * 8);
    POOL_ALLOC(rows, (size_t)B * n * GLP_CHECK_ROW_BYTES);
    if (max_list) POOL_ALLOC(d_lists, (size_t)B * max_list * sizeof(glp_check_violation));
    GlpCheckInst* inst = reinterpret_cast<GlpCheckInst*>(H.up.data());
    GlpCheckAcc* acc0 = reinterpret_cast<GlpCheckAcc*>(H.up.data() + w_inst);
    const u64* d_pub = d_up.u() + w_inst + w_acc;
    for (u32 b = 0; b < B; b++) {
        inst[b].wires = d_wire_vals[b];
        inst[b].pub = NP ? d_pub + (size_t)b * NP : nullptr;
        acc0[b].first_key = GLP_CHECK_KEY_NONE;
    }
    if (NP) memcpy(H.up.data() + w_inst + w_acc, h_public, w_pub * 8);
    GLP_HIPCHK(c, hipMemcpyAsync(d_up.p, H.up.data(), H.up.size() * 8, hipMemcpyHostToDevice, c->stream));

    GlpCheckArgs a;
    memset(&a, 0, sizeof(a));
    a.consts = cv.u(); a.sigma_idx = sigma_idx; a.pos_consts = c->hash ? c->hash->d_consts : nullptr;
    a.insts = reinterpret_cast<const GlpCheckInst*>(d_up.p);
    a.acc = reinterpret_cast<GlpCheckAcc*>(d_up.u() + w_inst);
    a.rows = (unsigned char*)rows.p;
    a.lists = (glp_check_violation*)d_lists.p;
    a.log_n = log_n; a.W = ck->W; a.R = R; a.n_public = NP;
    a.q_ext_col = (ck->flags & GLP_CIRCUIT_EXT_GATE) ? n_const - 1 : GLP_CHECK_NONE;
    a.first_pos = 2 + 3 * M;
    a.first_sha = 2 + 3 * M + ((ck->flags & GLP_CIRCUIT_POSEIDON_GATE) ? GLP_POS_GATE_CONSTRAINTS : 0);
    a.max_list = max_list;
    const dim3 g((unsigned)((n + GLP_CHECK_BLOCK - 1) / GLP_CHECK_BLOCK), B), blk(GLP_CHECK_BLOCK);
    hipLaunchKernelGGL(glp_check_base_kernel<0>, g, blk, 0, c->stream, a);
    GLP_HIPCHK(c, hipGetLastError());
    counts[0]++;
    if (ck->flags & GLP_CIRCUIT_POSEIDON_GATE) {
        if (c->hash->small_mds && !getenv("GLP_K7_GENERIC_MDS")) hipLaunchKernelGGL(glp_check_poseidon_kernel<true>, g, blk, 0, c->stream, a);
        else hipLaunchKernelGGL(glp_check_poseidon_kernel<false>, g, blk, 0, c->stream, a);
        GLP_HIPCHK(c, hipGetLastError());
        counts[0]++;
    }
    if (ck->flags & GLP_CIRCUIT_SHA_GATES) {
        hipLaunchKernelGGL(glp_check_sha_kernel<0>, g, blk, 0, c->stream, a);
        GLP_HIPCHK(c, hipGetLastError());
        counts[0]++;
    }
    hipLaunchKernelGGL(glp_check_copy_kernel<0>, g, blk, 0, c->stream, a);
    GLP_HIPCHK(c, hipGetLastError());
    counts[0]++;
    H.acc.resize(B);
    GLP_HIPCHK(c, hipMemcpyAsync(H.acc.data(), a.acc, (size_t)B * sizeof(GlpCheckAcc), hipMemcpyDeviceToHost, c->stream));
    if (max_list) {
        H.lists.resize((size_t)B * max_list);
        GLP_HIPCHK(c, hipMemcpyAsync(H.lists.data(), d_lists.p, H.lists.size() * sizeof(glp_check_violation), hipMemcpyDeviceToHost, c->stream));
    }
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    counts[1]++;
    return GLP_OK;
}

// shared by both entry points; h_status / sums / lists as the batch form takes them
int check_entry(glp_ctx* c, glp_plonk_circuit* ck, const uint64_t* const* d_wire_vals, const uint64_t* h_public, u32 B, int32_t* h_status,
                glp_check_summary* sums, glp_check_violation* lists, u32 max_list, const char* who, bool single) {
    c->check_counts[0] = c->check_counts[1] = 0;
    if (B == 0) return GLP_OK;
    if (!ck || !d_wire_vals || !h_status || !sums || (!lists && max_list) || (ck->n_public && !h_public)) {
        glp_set_err(c, "%s: bad argument", who);
        return GLP_E_INVALID;
    }
    for (u32 b = 0; b < B; b++) {
        if (!d_wire_vals[b]) { glp_set_err(c, "%s: instance %u: null wire matrix", who, b); return GLP_E_INVALID; }
        for (u32 k = 0; k < ck->n_public; k++)
            if (h_public[(size_t)b * ck->n_public + k] >= GL_P) {
                glp_set_err(c, "%s: instance %u: public input %u not canonical", who, b, k);
                return GLP_E_INVALID;
            }
    }
    if ((ck->flags & GLP_CIRCUIT_POSEIDON_GATE) && (!c->hash || !c->hash->have_consts)) { glp_set_err(c, "Poseidon constants not set"); return GLP_E_STATE; }
    if (B > 65535u || (u64)B * max_list > 0x7fffffffull) {
        glp_set_err(c, "%s: B = %u (the instance is a grid dimension: at most 65535) or B * max_list is more than one call takes", who, B);
        return GLP_E_UNSUPPORTED;
    }
    CheckHost H;
    DBuf fresh_idx(c);                          // this call's decode of sigma, when the key has none yet
    u32 counts[2] = {0, 0};
    int rc = check_impl(c, ck, d_wire_vals, h_public, B, max_list, H, fresh_idx, counts);
    c->check_counts[0] = counts[0]; c->check_counts[1] = counts[1];
    if (rc) {
        hipStreamSynchronize(c->stream);        // copies still in flight read and write H (not counted: not on the path of a verdict)
        return rc;                              // fresh_idx goes back to the pool: the key is as it was
    }
    if (fresh_idx.p && (H.status[0] != ~0ull || H.status[1] != ~0ull)) {
        const bool off = H.status[0] != ~0ull;
        const u64 cell = off ? H.status[0] : H.status[1];
        // a key that does not decode keeps no table (fresh_idx goes back to the pool): the next call says the same
        if (off)
            glp_set_err(c, "%s: the key's sigma at cell (wire %u, row %u) is no routed cell of the trace domain", who, (u32)(cell >> ck->log_n),
                        (u32)(cell & ((1ull << ck->log_n) - 1)));
        else
            glp_set_err(c, "%s: the key's sigma is no permutation of the routed cells: cell (wire %u, row %u) is not the image of exactly one cell", who,
                        (u32)(cell >> ck->log_n), (u32)(cell & ((1ull << ck->log_n) - 1)));
        return GLP_E_INVALID;
    }
    if (fresh_idx.p) ck->sigma_idx.adopt(fresh_idx.release());      // decoded, a permutation of the routed cells: the key keeps it
    for (u32 b = 0; b < B; b++) {
        const GlpCheckAcc& A = H.acc[b];
        glp_check_summary& s = sums[b];
        s.n_gate_bad = A.n_gate_bad; s.n_copy_bad = A.n_copy_bad; s.n_gate_rows = A.n_gate_rows; s.n_copy_rows = A.n_copy_rows;
        const u64 entries = (u64)A.n_gate_rows + A.n_copy_rows;
        s.n_listed = (u32)(entries < max_list ? entries : max_list);
        for (u32 k = 0; k < s.n_listed; k++) lists[(size_t)b * max_list + k] = H.lists[(size_t)b * max_list + k];
        const bool bad = A.n_gate_bad != 0 || A.n_copy_bad != 0;
        h_status[b] = bad ? GLP_E_REJECT : GLP_OK;
        if (bad && single) {
            const u32 row = glp_check_key_row(A.first_key), kind = glp_check_key_kind(A.first_key), index = glp_check_key_index(A.first_key);
            if (kind == GLP_CHECK_GATE)
                glp_set_err(c, "%s: witness not satisfied: row %u, gate constraint %u (%llu failing gate constraints in %u rows, %llu copy mismatches in %u rows)",
                            who, row, index, (unsigned long long)A.n_gate_bad, A.n_gate_rows, (unsigned long long)A.n_copy_bad, A.n_copy_rows);
            else
                glp_set_err(c, "%s: witness not satisfied: row %u, copy constraint of wire %u (%llu failing gate constraints in %u rows, %llu copy mismatches in %u rows)",
                            who, row, index, (unsigned long long)A.n_gate_bad, A.n_gate_rows, (unsigned long long)A.n_copy_bad, A.n_copy_rows);
        }
    }
    return GLP_OK;
}
}  // namespace

extern "C" int glp_plonk_check_witness(glp_ctx* c, glp_plonk_circuit* ck, const uint64_t* d_wire_vals, const uint64_t* h_public, glp_check_summary* sum,
                                       glp_check_violation* list, uint32_t max_list) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    int32_t status = GLP_OK;
    const uint64_t* one[1] = {d_wire_vals};
    if (!d_wire_vals) { c->check_counts[0] = c->check_counts[1] = 0; glp_set_err(c, "glp_plonk_check_witness: bad argument"); return GLP_E_INVALID; }
    const int rc = check_entry(c, ck, one, h_public, 1, &status, sum, list, max_list, "glp_plonk_check_witness", true);
    return rc ? rc : status;
}

extern "C" int glp_plonk_check_witness_batch(glp_ctx* c, glp_plonk_circuit* ck, const uint64_t* const* d_wire_vals, const uint64_t* h_public, uint32_t B,
                                             int32_t* h_status, glp_check_summary* sums, glp_check_violation* lists, uint32_t max_list) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    return check_entry(c, ck, d_wire_vals, h_public, B, h_status, sums, lists, max_list, "glp_plonk_check_witness_batch", false);
}

extern "C" int glp_plonk_last_check_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    if (!c) return GLP_E_INVALID;
    if (n_launches) *n_launches = c->check_counts[0];
    if (n_host_syncs) *n_host_syncs = c->check_counts[1];
    return GLP_OK;
}
