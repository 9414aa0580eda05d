// tests/emu_witness_seg/emu_witness_seg.cpp — TEST INFRASTRUCTURE.  The segmented witness evaluation (csrc/witness_kernels.cuh:
// glp_witness_eval_part_kernel in the three launches glp_witness_eval_device issues, and glp_witness_check_words_kernel) and the segmented plan
// compiler (csrc/witness_plan.h) on the CPU through ../emu/hip_emu.h: every work-item a real thread, __syncthreads() a barrier, one workgroup
// after the other — so the launches' order is the only ordering between the parts, as on the stream.  Never part of the product.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/witness_kernels.cuh"

// B instances through prefix | segments | tail.  seg_grid: workgroups of the segment launch (fewer than B * n_seg: the pair loop strides);
// the prefix and tail launches take `grid` workgroups.  consts384 = rc[360] | circ[12] | diag[12].  status[B] / first_bad[B]: the kernels' raw outputs.
// Returns glp_wit_compile_ex's verdict (nothing runs unless it is GLP_OK); GLP_E_STATE when the plan is not segmented.
extern "C" int emu_witness_eval_seg(const uint64_t* prog, size_t prog_words, size_t n_inputs, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                                    const uint64_t* seg_bounds, size_t n_seg, const uint64_t* consts384, int small, const uint64_t* inputs,
                                    uint64_t* values, size_t value_stride, uint32_t B, unsigned grid, unsigned seg_grid, unsigned block, int32_t* status,
                                    uint64_t* first_bad) {
    glp_wit_compiled c;
    const int rc = glp_wit_compile_ex(prog, prog_words, n_inputs, n_values, eq_pairs, n_eq, seg_bounds, n_seg, c);
    if (rc != GLP_OK) return rc;
    if (value_stride < n_values || block == 0 || grid == 0 || seg_grid == 0) return GLP_E_INVALID;
    if (c.parts.size() < 2) return GLP_E_STATE;
    const glp_wit_view v = c.view();
    const u32* pl = c.part_level.data();
    const u32 n_parts = (u32)c.parts.size();
    const GlpPoseidonConsts pk{consts384, consts384 + 360, consts384 + 372, nullptr, nullptr};
    std::vector<int> st(B, 77);
    std::vector<unsigned long long> fb(B, 77);
    int* stp = st.data();
    unsigned long long* fbp = fb.data();
    const struct { u32 lo, n; unsigned grid; int first, last; } launch[3] = {{0, 1, grid, 1, 0}, {1, n_parts - 2, seg_grid, 0, 0}, {n_parts - 1, 1, grid, 0, 1}};
    for (const auto& L : launch) {
        if (small)
            glp_emu_launch(L.grid, block, 0, [&] {
                glp_witness_eval_part_kernel<true>(v, pl, L.lo, L.n, L.first, L.last, inputs, values, (u64)value_stride, B, stp, fbp, pk);
            });
        else
            glp_emu_launch(L.grid, block, 0, [&] {
                glp_witness_eval_part_kernel<false>(v, pl, L.lo, L.n, L.first, L.last, inputs, values, (u64)value_stride, B, stp, fbp, pk);
            });
    }
    for (uint32_t b = 0; b < B; b++) { status[b] = st[b]; first_bad[b] = fb[b]; }
    return GLP_OK;
}

// the word-check kernel on host arrays: first_bad_var[B] / first_bad_bits[B] as glp_witness_check_words reports them
extern "C" int emu_witness_check_words(const uint64_t* values, size_t value_stride, uint32_t B, const uint32_t* var_idx, const uint64_t* var_want,
                                       uint32_t n_var, const uint32_t* bit_vars, const uint32_t* bit_start, const uint64_t* bit_want, uint32_t n_bits,
                                       unsigned grid, unsigned block, uint64_t* first_bad_var, uint64_t* first_bad_bits) {
    if (grid == 0 || block == 0) return GLP_E_INVALID;
    std::vector<unsigned long long> bad(2 * (size_t)B, ~0ull);
    unsigned long long* bp = bad.data();
    const glp_wit_words t{var_idx, bit_vars, bit_start, n_var, n_bits};
    glp_emu_launch(grid, block, 0, [&] { glp_witness_check_words_kernel(t, values, (u64)value_stride, B, var_want, bit_want, bp, bp + B); });
    for (uint32_t b = 0; b < B; b++) { first_bad_var[b] = bad[b]; first_bad_bits[b] = bad[B + b]; }
    return GLP_OK;
}
