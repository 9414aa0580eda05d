// tests/emu_witness/emu_witness.cpp — TEST INFRASTRUCTURE.  The witness-evaluation kernel body (csrc/witness_kernels.cuh) and the plan compiler
// (csrc/witness_plan.h) on the CPU through ../emu/hip_emu.h: every work-item a real thread, __syncthreads() a barrier, so that the level
// schedule, the lane assignment of a level's runs and the barrier placement are checked before the kernel touches a GPU.  The field arithmetic
// compiles in its DEVICE form (GLP_EMU: 32-bit partial products), as in the other emulated kernels.  Never part of the product.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/witness_kernels.cuh"

// B instances through the emulated kernel on `grid` workgroups of `block` lanes.  consts384 = rc[360] | circ[12] | diag[12]; small = the fast MDS
// path.  status[B] / first_bad[B] are the kernel's raw outputs; *rc_create is glp_wit_compile's verdict (nothing runs unless it is GLP_OK).
extern "C" int emu_witness_eval(const uint64_t* prog, size_t prog_words, size_t n_inputs, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                                const uint64_t* consts384, int small, const uint64_t* inputs, uint64_t* values, size_t value_stride, uint32_t B,
                                unsigned grid, unsigned block, int32_t* status, uint64_t* first_bad) {
    glp_wit_compiled c;
    const int rc = glp_wit_compile(prog, prog_words, n_inputs, n_values, eq_pairs, n_eq, c);
    if (rc != GLP_OK) return rc;
    if (value_stride < n_values || block == 0 || grid == 0) return GLP_E_INVALID;
    const glp_wit_view v = c.view();
    const GlpPoseidonConsts pk{consts384, consts384 + 360, consts384 + 372, nullptr, nullptr};
    std::vector<int> st(B, 77);
    std::vector<unsigned long long> fb(B, 77);
    int* stp = st.data();
    unsigned long long* fbp = fb.data();
    if (small)
        glp_emu_launch(grid, block, 0, [&] { glp_witness_eval_kernel<true>(v, inputs, values, (u64)value_stride, B, stp, fbp, pk); });
    else
        glp_emu_launch(grid, block, 0, [&] { glp_witness_eval_kernel<false>(v, inputs, values, (u64)value_stride, B, stp, fbp, pk); });
    for (uint32_t b = 0; b < B; b++) { status[b] = st[b]; first_bad[b] = fb[b]; }
    return GLP_OK;
}
