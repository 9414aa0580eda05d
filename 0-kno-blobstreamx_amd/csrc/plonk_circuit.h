// plonk_circuit.h — the circuit key behind glp_plonk_circuit (internal to libglprover.so): what glp_plonk_setup_ex keeps on the device and what
// the drivers that work on a key read — the prover (plonk.hip) and the witness checker (check.hip).
#pragma once
#include <vector>
#include "glp_ctx.h"

struct GlpCommit {              // one PolynomialBatch kept on the device
    GlpPoolBuf coeffs, lde, dig;
    std::vector<u64> cap;
    u32 n_polys = 0;
    explicit GlpCommit(glp_ctx* c) : coeffs(c), lde(c), dig(c) {}
};

struct glp_plonk_circuit {       // must be freed (glp_plonk_free) before its ctx is destroyed
    u32 log_n, W, R, n_public, flags, rate_bits, cap_h;
    u64 shift;
    GlpPoolBuf sigma_vals;      // [R][n] values on the trace domain (K6 input)
    GlpPoolBuf ks, inv_xm1;
    std::vector<u64> h_ks;
    GlpCommit pre;              // constants + sigmas
    // the witness checker's decoded sigma (check.hip): [R][n] u32, cell j*n + i -> the cell sigma sends it to.  4 * R * n bytes, allocated and
    // filled by the key's FIRST glp_plonk_check_witness[_batch] (empty until then: a key that is never checked holds nothing more), freed with the key
    GlpPoolBuf sigma_idx;
    explicit glp_plonk_circuit(glp_ctx* c) : sigma_vals(c), ks(c), inv_xm1(c), pre(c), sigma_idx(c) {}
};
