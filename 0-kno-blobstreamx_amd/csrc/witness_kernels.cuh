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
// A recursion node — ONE instance of fan-in independent verifier segments — gets a workgroup per segment instead
// (glp_witness_eval_part_kernel, three stream-ordered launches), and the word checks of a node's children run in glp_witness_check_words_kernel.
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

// The levels [l0, l1) of the schedule on one instance, by the whole workgroup; a barrier after each level.
// The descriptors of level l + 1 (uniform loads, independent of any value) are fetched while level l computes: per level the dependent
// chain is record -> operands -> store, not level table -> run -> record -> operands -> store.  Every level holds at least one op.
template <bool SMALL>
__device__ __forceinline__ void glp_wit_walk_levels(const glp_wit_view& p, u32 l0, u32 l1, const u64* __restrict__ in, u64* v, int* status_b,
                                                    const GlpPoseidonConsts& pk) {
    const u32 tid = threadIdx.x, wg = blockDim.x;
    u32 r0 = l0 < l1 ? p.level_run[l0] : 0, r1 = l0 < l1 ? p.level_run[l0 + 1] : 0;
    glp_wit_run first = l0 < l1 ? p.runs[r0] : glp_wit_run{0, 0, 0};
    for (u32 l = l0; l < l1; l++) {
        u32 r2 = r1;
        glp_wit_run next_first = first;
        if (l + 1 < l1) { r2 = p.level_run[l + 2]; next_first = p.runs[r1]; }
        u32 base = 0;                                      // lane (mod wg) of the run's first op
        for (u32 r = r0; r < r1; r++) {
            const glp_wit_run run = r == r0 ? first : p.runs[r];
            const u32 len = glp_wit_rec_len(run.kind);
            for (u32 k = tid >= base ? tid - base : tid + wg - base; k < run.count; k += wg) {
                const int rc = glp_wit_exec<SMALL>(run.kind, p.stream + run.off + (size_t)k * len, p.dict, in, v, pk);
                if (rc != GLP_OK) glp_wit_flag(status_b, rc);
            }
            base = (base + run.count) % wg;
        }
        __syncthreads();
        r0 = r1; r1 = r2; first = next_first;
    }
}

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
        glp_wit_walk_levels<SMALL>(p, 0, p.depth, in, v, &status[b], pk);
        for (u32 k = tid; k < p.n_eq; k += wg)
            if (v[p.eq[2 * k]] != v[p.eq[2 * k + 1]]) glp_wit_min(&first_bad[b], k);
    }
}

// A SEGMENTED plan (witness_plan.h, PARTS): one launch runs the parts [part_lo, part_lo + n_parts) of every instance, a workgroup per
// (instance, part) pair at a time, grid-stride over the B * n_parts pairs.  Parts of one launch must be mutually independent (the segments, or a
// single part); the order BETWEEN launches is the stream's — nothing here waits for another workgroup.  glp_witness_eval_device issues
//   1. the prefix (first = 1: the launch that zeroes the unwritten variables and initialises status / first_bad),
//   2. all segments at once,
//   3. the tail (last = 1: the copy constraints).
// status / first_bad keep the meaning they have above across the three launches: the atomics are device-scope and launch 1 is the only writer of
// the initial values.
template <bool SMALL>
__global__ void __launch_bounds__(GLP_WIT_WG) glp_witness_eval_part_kernel(glp_wit_view p, const u32* __restrict__ part_level, u32 part_lo, u32 n_parts,
                                                                           int first, int last, const u64* __restrict__ d_inputs, u64* d_values,
                                                                           u64 value_stride, u32 B, int* status, unsigned long long* first_bad,
                                                                           GlpPoseidonConsts pk) {
    const u32 tid = threadIdx.x, wg = blockDim.x;
    const u64 pairs = (u64)B * n_parts;
    for (u64 w = blockIdx.x; w < pairs; w += gridDim.x) {
        const u32 b = (u32)(w / n_parts), s = part_lo + (u32)(w % n_parts);
        u64* v = d_values + (u64)b * value_stride;
        const u64* in = d_inputs + (u64)b * p.n_inputs;
        if (first) {
            if (tid == 0) { status[b] = GLP_OK; first_bad[b] = ~0ull; }
            for (u32 k = tid; k < p.n_zero; k += wg) v[p.zero[k]] = 0;
            __syncthreads();
        }
        glp_wit_walk_levels<SMALL>(p, part_level[s], part_level[s + 1], in, v, &status[b], pk);
        if (last)
            for (u32 k = tid; k < p.n_eq; k += wg)
                if (v[p.eq[2 * k]] != v[p.eq[2 * k + 1]]) glp_wit_min(&first_bad[b], k);
    }
}

// One work-item per (instance, check): the lowest failing check of each kind per instance (first_bad_* start at ~0, set by the caller).
// want: [B][n_var] then [B][n_bits] words.
__global__ void __launch_bounds__(256) glp_witness_check_words_kernel(glp_wit_words t, const u64* __restrict__ d_values, u64 value_stride, u32 B,
                                                                      const u64* __restrict__ var_want, const u64* __restrict__ bit_want,
                                                                      unsigned long long* first_bad_var, unsigned long long* first_bad_bits) {
    const u32 n_checks = t.n_var + t.n_bits;
    const u64 total = (u64)B * n_checks;
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (u64)gridDim.x * blockDim.x) {
        const u32 b = (u32)(w / n_checks), k = (u32)(w % n_checks);
        if (!glp_wit_word_ok(t, d_values + (u64)b * value_stride, value_stride, var_want + (u64)b * t.n_var, bit_want + (u64)b * t.n_bits, k)) {
            if (k < t.n_var) glp_wit_min(&first_bad_var[b], k);
            else glp_wit_min(&first_bad_bits[b], k - t.n_var);
        }
    }
}
