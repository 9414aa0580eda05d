// check_kernels.cuh — the kernels of glp_plonk_check_witness[_batch] (check.hip): the gate constraints of plonk_gates.h evaluated where they
// are meant to vanish, on the n trace rows in natural order, and the copy constraints tested directly, cell against the cell sigma names.
//
// One work-item per trace row, 256 per workgroup, grid = (ceil(n / 256), B): the instance is blockIdx.y, its wire matrix and public inputs
// come from a device table (GlpCheckInst[B]), everything else is shared by the B instances.  Wires are read as wires[j * n + i]: consecutive
// lanes read consecutive words.  The work is split the way the prover splits K7 / K7s, for the same register reasons:
//   glp_check_base_kernel          public input (index 1) and, per chunk c, the two arithmetic / extension slots (3+3c, 4+3c)
//   glp_check_poseidon_kernel<S>   the 123 Poseidon constraints times q_pos (2+3M+k); a row with q_pos == 0 evaluates nothing
//   glp_check_sha_kernel           the 140 selector-weighted SHA slots (first_sha + k); a row with all four selectors zero evaluates nothing
//   glp_check_copy_kernel          wire(j, i) == wire(sigma(j, i)) for every routed cell; its last workgroup per instance writes the list
// Each row writes, per kind, its lowest failing index, the value there and its count of failing constraints (GlpCheckRows); per workgroup the
// counts and the lowest (row, kind, index) key are reduced through LDS and, only when the workgroup saw a failure, combined into GlpCheckAcc
// with atomicAdd / atomicMin on global memory — a satisfied witness issues no atomic but one ticket per workgroup of the copy kernel.
// The list (one entry per failing row and kind, ascending by (row, kind), at most max_list) is built on the device by the workgroup of the
// copy kernel that draws the last ticket of its instance: it walks the per-row arrays from the first failing row in steps of 256 rows, an
// exclusive scan through LDS giving every entry its slot — the same input gives the same list whatever order the workgroups ran in.
//
// glp_sigma_decode_kernel / glp_sigma_bijective_kernel: the once-per-key decode of the key's sigma values into cell indices (check_plan.h).
// Plain HIP C++ without AMD builtins: tests/emu_check runs these bodies on the CPU.
#pragma once
#include "../../include/glprover.h"
#include "check_plan.h"
#include "plonk_kernels.cuh"

#if defined(GLP_EMU)
#define GLP_CHECK_ADD64(p, v) __atomic_fetch_add((p), (unsigned long long)(v), __ATOMIC_RELAXED)
#define GLP_CHECK_ADD32(p, v) __atomic_fetch_add((p), (u32)(v), __ATOMIC_RELAXED)
#define GLP_CHECK_MIN64(p, v) glp_emu_atomic_min((p), (unsigned long long)(v))
#define GLP_CHECK_FENCE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#else
#define GLP_CHECK_ADD64(p, v) atomicAdd((p), (unsigned long long)(v))
#define GLP_CHECK_ADD32(p, v) atomicAdd((p), (u32)(v))
#define GLP_CHECK_MIN64(p, v) atomicMin((p), (unsigned long long)(v))
#define GLP_CHECK_FENCE() __threadfence()
#endif

#define GLP_CHECK_BLOCK 256
#define GLP_CHECK_NONE 0xFFFFFFFFu

struct GlpCheckInst {
    const u64* wires;              // [W][n] the caller's witness on the trace domain (read only)
    const u64* pub;                // [n_public] on the device, null when the circuit has none
};
// per instance, zeroed (first_key: all ones) before the first launch of a call
struct GlpCheckAcc {
    unsigned long long n_gate_bad, n_copy_bad;     // failing (row, constraint) and (row, wire) pairs
    unsigned long long first_key;                  // lowest glp_check_key of a violation
    u32 n_gate_rows, n_copy_rows;
    u32 ticket, pad;
};
// the per-row arrays of one instance inside the call's row buffer: 44 bytes per row
struct GlpCheckRows {
    u64 *gate_val, *copy_val, *copy_pval;
    u32 *gate_first, *gate_cnt, *copy_first, *copy_cnt, *copy_peer;
};
#define GLP_CHECK_ROW_BYTES 44ull
GL_HD GlpCheckRows glp_check_rows(unsigned char* base, u64 n, u32 inst) {
    unsigned char* p = base + (u64)inst * n * GLP_CHECK_ROW_BYTES;
    GlpCheckRows r;
    r.gate_val = reinterpret_cast<u64*>(p); r.copy_val = r.gate_val + n; r.copy_pval = r.copy_val + n;
    r.gate_first = reinterpret_cast<u32*>(r.copy_pval + n); r.gate_cnt = r.gate_first + n; r.copy_first = r.gate_cnt + n;
    r.copy_cnt = r.copy_first + n; r.copy_peer = r.copy_cnt + n;
    return r;
}

struct GlpCheckArgs {
    const u64* consts;             // [n_const][n] the key's constant columns on the trace domain (natural order)
    const u32* sigma_idx;          // [R][n] decoded sigma
    const u64* pos_consts;         // rc[360], circ[12], diag[12] on the device (Poseidon circuits)
    const GlpCheckInst* insts;     // [B]
    GlpCheckAcc* acc;              // [B]
    unsigned char* rows;           // [B] GlpCheckRows blocks
    glp_check_violation* lists;    // [B][max_list] on the device (null when max_list == 0)
    u32 log_n, W, R, n_public;
    u32 q_ext_col;                 // the q_ext constant column, GLP_CHECK_NONE when the circuit has no extension rows
    u32 first_pos, first_sha;      // constraint number of the first Poseidon / SHA constraint
    u32 max_list;
};

// what a row found for one kind: lowest failing index, the value there, how many failed
struct GlpCheckRowAcc {
    u32 first = GLP_CHECK_NONE, cnt = 0;
    u64 val = 0;
    GL_HD void see(u32 index, u64 v) {
        if (v != 0) {
            if (cnt == 0) { first = index; val = v; }
            cnt++;
        }
    }
};

// workgroup totals of (failing pairs, failing rows) and the lowest key -> the instance's accumulators; every work-item of the workgroup calls
template <int GATE>
__device__ inline void glp_check_reduce(GlpCheckAcc* acc, u32 cnt, u32 rows, u64 key) {
    __shared__ u32 s_cnt[GLP_CHECK_BLOCK];
    __shared__ u32 s_rows[GLP_CHECK_BLOCK];
    __shared__ u64 s_key[GLP_CHECK_BLOCK];
    const u32 t = threadIdx.x;
    s_cnt[t] = cnt; s_rows[t] = rows; s_key[t] = key;
    __syncthreads();
    for (u32 s = GLP_CHECK_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_cnt[t] += s_cnt[t + s];
            s_rows[t] += s_rows[t + s];
            if (s_key[t + s] < s_key[t]) s_key[t] = s_key[t + s];
        }
        __syncthreads();
    }
    if (t == 0 && s_cnt[0] != 0) {
        if (GATE) { GLP_CHECK_ADD64(&acc->n_gate_bad, s_cnt[0]); if (s_rows[0]) GLP_CHECK_ADD32(&acc->n_gate_rows, s_rows[0]); }
        else { GLP_CHECK_ADD64(&acc->n_copy_bad, s_cnt[0]); if (s_rows[0]) GLP_CHECK_ADD32(&acc->n_copy_rows, s_rows[0]); }
        GLP_CHECK_MIN64(&acc->first_key, s_key[0]);
    }
    __syncthreads();               // the arrays are reused by the next call in this workgroup
}

// ---- public input, arithmetic and extension slots: writes every row's gate entry (the later gate kernels add to it) ----------------------
template <int UNUSED = 0>
__global__ void __launch_bounds__(GLP_CHECK_BLOCK) glp_check_base_kernel(GlpCheckArgs a) {
    const u64 n = 1ull << a.log_n;
    const u32 inst = blockIdx.y;
    const u64 i = (u64)blockIdx.x * GLP_CHECK_BLOCK + threadIdx.x;
    GlpCheckRowAcc ra;
    if (i < n) {
        const GlpCheckInst d = a.insts[inst];
        const u64* wires = d.wires;
        const u32 M = a.R / GLP_PLONK_CHUNK;
        const u64 q = a.consts[i], c0 = a.consts[n + i], c1 = a.consts[2 * n + i], c2 = a.consts[3 * n + i], q_pi = a.consts[4 * n + i];
        const bool ext = a.q_ext_col != GLP_CHECK_NONE;
        const u64 qx = ext ? a.consts[(u64)a.q_ext_col * n + i] : 0ull;
        const u64 pi = (i < a.n_public) ? d.pub[i] : 0ull;
        ra.see(1, gl_sub(gl_mul(q_pi, wires[i]), pi));
        for (u32 c = 0; c < M; c++) {
            u64 w[GLP_PLONK_CHUNK];
            glp_static_for<0, GLP_PLONK_CHUNK>([&](auto j_) {
                constexpr int jj = decltype(j_)::value;
                w[jj] = wires[((u64)c * GLP_PLONK_CHUNK + jj) * n + i];
            });
            // exactly as K7 forms the two slots of the chunk
            u64 g0 = gl_mul(q, glp_arith_gate<GlpGateBase>(c0, c1, c2, w[0], w[1], w[2], w[3]));
            u64 g1 = gl_mul(q, glp_arith_gate<GlpGateBase>(c0, c1, c2, w[4], w[5], w[6], w[7]));
            if (ext) {
                u64 e0, e1;
                glp_ext_gate<GlpGateBase>(w, e0, e1);
                g0 = gl_add(g0, gl_mul(qx, e0));
                g1 = gl_add(g1, gl_mul(qx, e1));
            }
            ra.see(3 + 3 * c, g0);
            ra.see(4 + 3 * c, g1);
        }
        const GlpCheckRows r = glp_check_rows(a.rows, n, inst);
        r.gate_first[i] = ra.first;
        r.gate_cnt[i] = ra.cnt;
        if (ra.cnt) r.gate_val[i] = ra.val;
    }
    glp_check_reduce<1>(a.acc + inst, ra.cnt, ra.cnt ? 1u : 0u, ra.cnt ? glp_check_key((u32)i, GLP_CHECK_GATE, ra.first) : GLP_CHECK_KEY_NONE);
}

// a later gate kernel's findings into the row's entry (the base kernel wrote it; its indices are lower than this block's)
GL_HD u32 glp_check_merge_gate(const GlpCheckRows& r, u64 i, const GlpCheckRowAcc& ra) {
    if (ra.cnt == 0) return 0;
    const u32 before = r.gate_cnt[i];
    if (before == 0) { r.gate_first[i] = ra.first; r.gate_val[i] = ra.val; }
    r.gate_cnt[i] = before + ra.cnt;
    return before == 0 ? 1u : 0u;           // 1: a row that had not failed yet
}

// ---- Poseidon rows: the 123 constraints times q_pos; SMALL = the small-integer-MDS body (the switch K7 makes) -----------------------------
template <bool SMALL>
__global__ void __launch_bounds__(GLP_CHECK_BLOCK) glp_check_poseidon_kernel(GlpCheckArgs a) {
    const u64 n = 1ull << a.log_n;
    const u32 inst = blockIdx.y;
    const u64 i = (u64)blockIdx.x * GLP_CHECK_BLOCK + threadIdx.x;
    GlpCheckRowAcc ra;
    u32 new_row = 0;
    if (i < n) {
        const u64 q_pos = a.consts[5 * n + i];
        if (q_pos != 0) {
            const u64* wires = a.insts[inst].wires;
            u32 k = a.first_pos;
            auto wire = [&](int j) -> u64 { return wires[(u64)j * n + i]; };
            auto emit = [&](u64 con) {
                if (con != 0) ra.see(k, gl_mul(q_pos, con));       // no zero divisors: the term is non-zero exactly when the constraint is
                k++;
            };
            if constexpr (SMALL) glp_poseidon_gate_constraints_fast<true>(wire, a.pos_consts, a.pos_consts + 360, a.pos_consts + 372, emit);
            else glp_poseidon_gate_constraints<GlpGateBase>(wire, a.pos_consts, a.pos_consts + 360, a.pos_consts + 372, emit);
            new_row = glp_check_merge_gate(glp_check_rows(a.rows, n, inst), i, ra);
        }
    }
    glp_check_reduce<1>(a.acc + inst, ra.cnt, new_row, ra.cnt ? glp_check_key((u32)i, GLP_CHECK_GATE, ra.first) : GLP_CHECK_KEY_NONE);
}

// ---- SHA rows: the 140 selector-weighted slots ---------------------------------------------------------------------------------------------
template <int UNUSED = 0>
__global__ void __launch_bounds__(GLP_CHECK_BLOCK) glp_check_sha_kernel(GlpCheckArgs a) {
    const u64 n = 1ull << a.log_n;
    const u32 inst = blockIdx.y;
    const u64 i = (u64)blockIdx.x * GLP_CHECK_BLOCK + threadIdx.x;
    GlpCheckRowAcc ra;
    u32 new_row = 0;
    if (i < n) {
        const u64 q[4] = {a.consts[6 * n + i], a.consts[7 * n + i], a.consts[8 * n + i], a.consts[9 * n + i]};
        if ((q[0] | q[1] | q[2] | q[3]) != 0) {
            const u64* wires = a.insts[inst].wires;
            const u64 c2 = a.consts[3 * n + i];
            u32 k = a.first_sha;
            glp_sha_gate_constraints<GlpGateBase>([&](int j) -> u64 { return wires[(u64)j * n + i]; }, q, c2, [&](u64 con) { ra.see(k, con); k++; });
            new_row = glp_check_merge_gate(glp_check_rows(a.rows, n, inst), i, ra);
        }
    }
    glp_check_reduce<1>(a.acc + inst, ra.cnt, new_row, ra.cnt ? glp_check_key((u32)i, GLP_CHECK_GATE, ra.first) : GLP_CHECK_KEY_NONE);
}

// ---- the list of one instance, by one workgroup, after every row entry of the instance is written and visible ----------------------------
__device__ inline void glp_check_build_list(const GlpCheckArgs& a, u32 inst, u64 first_key) {
    __shared__ u32 s_scan[GLP_CHECK_BLOCK];
    const u64 n = 1ull << a.log_n;
    const GlpCheckRows r = glp_check_rows(a.rows, n, inst);
    glp_check_violation* list = a.lists + (u64)inst * a.max_list;
    const u32 t = threadIdx.x;
    u32 slot0 = 0;                                                                  // workgroup-uniform
    for (u64 row0 = (u64)glp_check_key_row(first_key) & ~(u64)(GLP_CHECK_BLOCK - 1); row0 < n && slot0 < a.max_list; row0 += GLP_CHECK_BLOCK) {
        const u64 i = row0 + t;
        const u32 g = (i < n && r.gate_cnt[i] != 0) ? 1u : 0u, cp = (i < n && r.copy_cnt[i] != 0) ? 1u : 0u;
        s_scan[t] = g + cp;
        __syncthreads();
        for (u32 off = 1; off < GLP_CHECK_BLOCK; off <<= 1) {                       // inclusive scan (Hillis-Steele)
            const u32 add = (t >= off) ? s_scan[t - off] : 0u;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        u32 slot = slot0 + s_scan[t] - (g + cp);
        const u32 total = s_scan[GLP_CHECK_BLOCK - 1];
        if (g && slot < a.max_list) {
            glp_check_violation v;
            v.kind = GLP_CHECK_GATE; v.row = (u32)i; v.index = r.gate_first[i]; v.n_in_row = r.gate_cnt[i];
            v.peer_wire = 0; v.peer_row = 0; v.value = r.gate_val[i]; v.peer_value = 0;
            list[slot] = v;
        }
        slot += g;
        if (cp && slot < a.max_list) {
            const u32 peer = r.copy_peer[i];
            glp_check_violation v;
            v.kind = GLP_CHECK_COPY; v.row = (u32)i; v.index = r.copy_first[i]; v.n_in_row = r.copy_cnt[i];
            v.peer_wire = peer >> a.log_n; v.peer_row = peer & (u32)(n - 1); v.value = r.copy_val[i]; v.peer_value = r.copy_pval[i];
            list[slot] = v;
        }
        __syncthreads();                                                            // s_scan is rewritten by the next step
        slot0 += total;
    }
}

// ---- copy constraints, directly; then the list ------------------------------------------------------------------------------------------------
template <int UNUSED = 0>
__global__ void __launch_bounds__(GLP_CHECK_BLOCK) glp_check_copy_kernel(GlpCheckArgs a) {
    __shared__ u32 s_last;
    __shared__ unsigned long long s_key;
    const u64 n = 1ull << a.log_n;
    const u32 inst = blockIdx.y;
    const u64 i = (u64)blockIdx.x * GLP_CHECK_BLOCK + threadIdx.x;
    GlpCheckRowAcc ra;
    if (i < n) {
        const u64* wires = a.insts[inst].wires;
        u32 peer = 0;
        u64 pval = 0;
        for (u32 j = 0; j < a.R; j++) {
            const u64 p = (u64)j * n + i;
            const u32 t = a.sigma_idx[p];                                           // < R * n: the decode admits nothing else
            if (t == (u32)p) continue;
            const u64 v = wires[p], pv = wires[t];
            if (v != pv) {
                if (ra.cnt == 0) { ra.first = j; ra.val = v; peer = t; pval = pv; }
                ra.cnt++;
            }
        }
        const GlpCheckRows r = glp_check_rows(a.rows, n, inst);
        r.copy_first[i] = ra.first;
        r.copy_cnt[i] = ra.cnt;
        if (ra.cnt) { r.copy_val[i] = ra.val; r.copy_pval[i] = pval; r.copy_peer[i] = peer; }
    }
    GlpCheckAcc* acc = a.acc + inst;
    glp_check_reduce<0>(acc, ra.cnt, ra.cnt ? 1u : 0u, ra.cnt ? glp_check_key((u32)i, GLP_CHECK_COPY, ra.first) : GLP_CHECK_KEY_NONE);
    if (a.max_list == 0) return;                                                    // uniform: no list wanted
    // the workgroup that draws the instance's last ticket writes its list: every other workgroup's row entries and accumulator updates are
    // released (device-scope fence) before its ticket, and acquired here after the last one
    GLP_CHECK_FENCE();
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 ticket = GLP_CHECK_ADD32(&acc->ticket, 1u);
        s_last = (ticket == gridDim.x - 1) ? 1u : 0u;
        s_key = GLP_CHECK_KEY_NONE;
        if (s_last) {
            GLP_CHECK_FENCE();
            s_key = GLP_CHECK_ADD64(&acc->first_key, 0ull);                         // an atomic read: what the atomicMins left
        }
    }
    __syncthreads();
    if (!s_last || s_key == GLP_CHECK_KEY_NONE) return;                             // uniform
    GLP_CHECK_FENCE();
    glp_check_build_list(a, inst, s_key);
}

// ---- sigma values -> cell indices, once per key ------------------------------------------------------------------------------------------------
// status[0]: lowest cell whose value is no routed cell of the domain; status[1]: lowest cell that is not the image of exactly one cell
// (both preset to all ones).  A cell that does not decode is stored as its own index, so that the table never holds an index out of range.
struct GlpSigmaDecodeArgs {
    const u64* sigma_vals;         // [R][n]
    const u64* ks;                 // [R]
    const u64* w_lo; const u64* w_hi;    // forward root table of size n
    GlpSigmaTables T;              // device pointers
    u32* idx;                      // [R][n] out
    u32* hits;                     // [R][n] zeroed
    unsigned long long* status;    // [2]
};
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_sigma_decode_kernel(GlpSigmaDecodeArgs a) {
    const u64 n = 1ull << a.T.log_n;
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= (u64)a.T.R * n) return;
    const u64 i = p & (n - 1);
    const u32 j = (u32)(p >> a.T.log_n);
    const u64 v = a.sigma_vals[p];
    u64 x = a.w_lo[i & 4095u];
    if (a.w_hi) x = gl_mul(x, a.w_hi[i >> 12]);
    u32 t;
    if (v == gl_mul(a.ks[j], x)) t = (u32)p;                                        // sigma(p) = p: most cells of a sparse routing
    else t = glp_sigma_decode(v, a.T);
    if (t == GLP_SIGMA_BAD) {
        GLP_CHECK_MIN64(&a.status[0], p);
        t = (u32)p;
    }
    a.idx[p] = t;
    GLP_CHECK_ADD32(&a.hits[t], 1u);
}
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_sigma_bijective_kernel(const u32* __restrict__ hits, u64 cells, unsigned long long* status) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= cells) return;
    if (hits[p] != 1u) GLP_CHECK_MIN64(&status[1], p);
}
