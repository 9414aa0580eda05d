// witness_kernels.cuh — batched device-side witness evaluation of a level schedule (witness_plan.h).
//
// One workgroup per instance at a time, grid-stride over the B instances.  For each level the workgroup's lanes take the level's ops, then
// __syncthreads(): the next level reads what this one wrote (global memory, same workgroup: the barrier's workgroup-scope fence is all the
// ordering there is — no cross-workgroup communication, no flags, no cooperative launch).  Values are instance-major,
// d_values[b * value_stride + var]: the layout glp_gather_u64 places wire cells from.
//
// The runs of a level (one per op kind present) share the lanes: run j starts at the lane after run j - 1's last op, so a level of 5 ARITH and
// 7 BIT ops uses 12 lanes in one pass rather than two passes of a few lanes, while heavy kinds (POSEIDON, NNF_MUL, INV) sit in lanes — for wide
// levels whole wavefronts — of their own.
//
// Refusals that depend on VALUES (witness_run's GLP_E_REJECT rows, an input word >= p) flag the instance and write 0; the kernel never stops
// early and never indexes memory with a computed value.  Structural checks were all done by glp_wit_compile.
#pragma once
#include "witness_plan.h"

#if defined(GLP_EMU)
#include <mutex>
inline std::mutex& glp_wit_emu_mutex() { static std::mutex m; return m; }
inline void glp_wit_flag(int* status, int code) {
    std::lock_guard<std::mutex> g(glp_wit_emu_mutex());
    if (code == GLP_E_INVALID || *status == GLP_OK) *status = code;
}
inline void glp_wit_min(unsigned long long* p, unsigned long long x) { glp_emu_atomic_min(p, x); }
#else
// GLP_E_INVALID (a malformed input) wins over GLP_E_REJECT whatever the order the lanes arrive in
__device__ __forceinline__ void glp_wit_flag(int* status, int code) {
    if (code == GLP_E_INVALID) atomicExch(status, code);
    else atomicCAS(status, GLP_OK, code);
}
__device__ __forceinline__ void glp_wit_min(unsigned long long* p, unsigned long long x) { atomicMin(p, x); }
#endif

// status[b]: GLP_OK or the refusal of an op.  first_bad[b]: the lowest failing copy-constraint index, ~0 when none fails (meaningful when
// status[b] is GLP_OK: the host orders it the same way, ops first, then the pairs).
template <bool SMALL>
__global__ void __launch_bounds__(GLP_WIT_WG) glp_witness_eval_kernel(glp_wit_view p, const u64* __restrict__ d_inputs, u64* d_values, u64 value_stride,
                                                                      u32 B, int* status, unsigned long long* first_bad, GlpPoseidonConsts pk) {
    const u32 tid = threadIdx.x, wg = blockDim.x;
    for (u32 b = blockIdx.x; b < B; b += gridDim.x) {
        u64* v = d_values + (u64)b * value_stride;
        const u64* in = d_inputs + (u64)b * p.n_inputs;
        if (tid == 0) { status[b] = GLP_OK; first_bad[b] = ~0ull; }
        for (u32 k = tid; k < p.n_zero; k += wg) v[p.zero[k]] = 0;
        __syncthreads();
        // the descriptors of level l + 1 (uniform loads, independent of any value) are fetched while level l computes: per level the dependent
        // chain is record -> operands -> store, not level table -> run -> record -> operands -> store.  Every level holds at least one op.
        u32 r0 = p.depth ? p.level_run[0] : 0, r1 = p.depth ? p.level_run[1] : 0;
        glp_wit_run first = p.depth ? p.runs[r0] : glp_wit_run{0, 0, 0};
        for (u32 l = 0; l < p.depth; l++) {
            u32 r2 = r1;
            glp_wit_run next_first = first;
            if (l + 1 < p.depth) { r2 = p.level_run[l + 2]; next_first = p.runs[r1]; }
            u32 base = 0;                                      // lane (mod wg) of the run's first op
            for (u32 r = r0; r < r1; r++) {
                const glp_wit_run run = r == r0 ? first : p.runs[r];
                const u32 len = glp_wit_rec_len(run.kind);
                for (u32 k = tid >= base ? tid - base : tid + wg - base; k < run.count; k += wg) {
                    const int rc = glp_wit_exec<SMALL>(run.kind, p.stream + run.off + (size_t)k * len, p.dict, in, v, pk);
                    if (rc != GLP_OK) glp_wit_flag(&status[b], rc);
                }
                base = (base + run.count) % wg;
            }
            __syncthreads();
            r0 = r1; r1 = r2; first = next_first;
        }
        for (u32 k = tid; k < p.n_eq; k += wg)
            if (v[p.eq[2 * k]] != v[p.eq[2 * k + 1]]) glp_wit_min(&first_bad[b], k);
    }
}
