// place_batch_kernels.cuh — witness placement: the single-instance kernel of glp_gather_u64 (glprover.hip) and the kernels of
// glp_witness_place_batch (witness.hip), which turn B rows of an evaluated slab into B wire matrices [W][n] side by side.
//
//   glp_witness_place_kernel                  dst[i] = src[index[i]] for ONE instance, with its out-of-range flag (glp_gather_u64)
//   glp_witness_place_batch_kernel            the B matrices from one cell -> variable map: ONE work-item per cell, a loop over the instances
//   glp_poseidon_gate_fill_batch_kernel<S>    the Poseidon rows of all B matrices (glp_poseidon_gate_fill_kernel<S> per instance)
//   glp_sha_gate_fill_batch_kernel            the SHA rows of all B matrices (glp_sha_gate_fill_kernel per instance)
//   glp_witness_public_batch_kernel           the B * n_public public values
//
// Placement is cell-major, not the instance-major grid of plonk_batch_kernels.cuh: every instance reads the SAME index entry for a cell, so a
// work-item loads its 4-byte entry once and then does B 8-byte loads and B coalesced stores with the entry in a register.  The index stream — a third
// of the bytes a single placement reads — crosses the memory system once per call instead of once per instance.  The slab row of each instance
// comes from a device table of B entries; its reads are wave-uniform (scalar loads).
// The row fillers ARE instance-major (inst = blockIdx.x / blocks_per_instance, 64 lanes): the lanes of a wavefront take consecutive rows of one
// instance, so the column stores stay coalesced exactly as in the single kernels; the bodies are those of plonk_kernels.cuh word for word.
// The indices were all checked on the host when the layout was made (glp_witness_layout_create): no flag, nothing to copy back.
// Plain HIP C++ without AMD builtins: tests/emu_place_batch runs these bodies on the CPU.
#pragma once
#include "plonk_kernels.cuh"

// witness placement: wire cell i takes the variable its index entry names (0xFFFFFFFF = an unused cell, zero)
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_witness_place_kernel(u64* __restrict__ dst, const u64* __restrict__ src, u64 n_src, const u32* __restrict__ index,
                                                                u64 n, u32* __restrict__ bad) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 k = index[i];
        u64 v = 0;
        if (k != 0xFFFFFFFFu) {
            if (k < n_src) v = src[k];
#if defined(GLP_EMU)
            else __atomic_fetch_or(bad, 1u, __ATOMIC_RELAXED);
#else
            else atomicOr(bad, 1u);
#endif
        }
        dst[i] = v;
    }
}

// dst[b * wire_stride + i] = src[slab_row[b] * value_stride + index[i]] (0 for an unused cell), b < B, i < n_cells
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_witness_place_batch_kernel(u64* __restrict__ dst, u64 wire_stride, const u64* __restrict__ src, u64 value_stride,
                                                                      const u32* __restrict__ slab_row, u32 B, const u32* __restrict__ index, u64 n_cells) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (u64)gridDim.x * blockDim.x) {
        const u32 k = index[i];
        for (u32 b = 0; b < B; b++) {                    // one loop for used and unused cells: 12 VGPRs, as the single kernel (two loops: 14)
            u64 v = 0;
            if (k != 0xFFFFFFFFu) v = src[(u64)slab_row[b] * value_stride + k];
            dst[(u64)b * wire_stride + i] = v;
        }
    }
}

// out[b * n_public + j] = src[slab_row[b] * value_stride + public_vars[j]]
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_witness_public_batch_kernel(u64* __restrict__ out, const u64* __restrict__ src, u64 value_stride,
                                                                       const u32* __restrict__ slab_row, u32 B, const u32* __restrict__ public_vars,
                                                                       u32 n_public) {
    const u64 total = (u64)B * n_public;
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (u64)gridDim.x * blockDim.x) {
        const u32 b = (u32)(g / n_public), j = (u32)(g - (u64)b * n_public);
        out[g] = src[(u64)slab_row[b] * value_stride + public_vars[j]];
    }
}

// ---- Poseidon rows of B matrices: instance inst's matrix starts at wires + inst * wire_stride (glp_poseidon_gate_fill_kernel's body) ----
template <int SMALL_MDS = 0>
__global__ void __launch_bounds__(64) glp_poseidon_gate_fill_batch_kernel(u64* __restrict__ wires_all, u64 wire_stride, u64 n, const u32* __restrict__ rows,
                                                                         u32 n_rows, u32 blocks_per_instance, const u64* __restrict__ consts) {
    const u32 inst = blockIdx.x / blocks_per_instance;
    const u32 k = (blockIdx.x - inst * blocks_per_instance) * blockDim.x + threadIdx.x;
    if (k >= n_rows) return;
    const u64 row = rows[k];
    if (row >= n) return;
    u64* __restrict__ wires = wires_all + (u64)inst * wire_stride;
    u64 in[12], out[GLP_POS_GATE_WIRES - 12];
    for (int j = 0; j < 12; j++) in[j] = wires[(u64)j * n + row];
    const u64 swap = wires[(u64)GLP_POS_SWAP_WIRE * n + row];
    if constexpr (SMALL_MDS != 0) glp_poseidon_gate_fill_fast<true>(in, swap, consts, consts + 360, consts + 372, out);
    else glp_poseidon_gate_fill(in, swap, consts, consts + 360, consts + 372, out);
    for (int j = 0; j < GLP_POS_GATE_WIRES - 12; j++) wires[(u64)(12 + j) * n + row] = out[j];
}

// ---- SHA rows of B matrices (glp_sha_gate_fill_kernel's body) ----
template <int UNUSED = 0>
__global__ void __launch_bounds__(64) glp_sha_gate_fill_batch_kernel(u64* __restrict__ wires_all, u64 wire_stride, u64 n, const u32* __restrict__ rows,
                                                                    const u32* __restrict__ kinds, u32 n_rows, u32 blocks_per_instance) {
    const u32 inst = blockIdx.x / blocks_per_instance;
    const u32 k = (blockIdx.x - inst * blocks_per_instance) * blockDim.x + threadIdx.x;
    if (k >= n_rows) return;
    const u64 row = rows[k];
    if (row >= n || kinds[k] > 3) return;
    u64* __restrict__ wires = wires_all + (u64)inst * wire_stride;
    u64 r[12], bits[132];
    for (int j = 0; j < 12; j++) r[j] = wires[(u64)j * n + row];
    glp_sha_gate_fill((int)kinds[k], r, bits);
    for (int j = 0; j < 132; j++) wires[(u64)(12 + j) * n + row] = bits[j];
}
