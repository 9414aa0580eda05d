// plonk_batch_kernels.cuh — the kernels of glp_plonk_prove_batch (plonk.hip): B witnesses of ONE circuit share every launch.
// 1-D grids throughout: a launch has B * blocks_per_instance workgroups of 256 lanes and the instance index is
// blockIdx.x / blocks_per_instance, so everything read from the descriptor table is wave-uniform (scalar loads).
//
// Shared by the B instances (kernel arguments, as in plonk_kernels.cuh): the circuit's constant and sigma LDEs, ks, inv_xm1, zh_inv,
// n_inv, the root tables, the Poseidon constants.  Per instance (GlpPlonkInst, one table [B] on the device, uploaded once per stage):
// the wire values and LDE, the Z LDE, the public-input LDE, beta, gamma, the alpha-power table and the outputs.
//
//   glp_plonk_gather_wires_batch_kernel   the B wire matrices of the caller into one [B*W][n] slab
//   glp_perm_quotients_batch_kernel       K6a: the chunk quotients qv [B][NCHAL][M][n] and row ratios rr [B][NCHAL][n]
//   glp_quotient_batch_kernel<POS, SMALL> K7: the quotient evaluations [B][NCHAL][N]
//   glp_quotient_sha_batch_kernel         K7s: the SHA-row block, added to what K7 wrote
// K6b needs no batched form: glp_scan_reduce_kernel / glp_scan_blocks_kernel / glp_scan_apply_kernel index by challenge, and over dense
// [B*NCHAL]-major qv / rr / block products and a [B*NCHAL*M][n] output they do the batch when launched with B*NCHAL challenges.
// The bodies are those of plonk_kernels.cuh word for word (same device functions, same order of operations), so every word equals
// what the single-instance kernels produce.  Plain HIP C++ without AMD builtins: tests/emu_plonk_batch runs these bodies on the CPU.
#pragma once
#include "plonk_kernels.cuh"

struct GlpPlonkInst {
    const u64* wire_vals;          // [W][n] the caller's witness on the trace domain (read only)
    const u64* wires_lde;          // [W][N]
    const u64* zs_lde;             // [NCHAL*M][N]
    const u64* pi_lde;             // [N], null when the circuit has no public inputs
    const u64* alpha_pow;          // [NCHAL][n_con]
    u64* qv;                       // [NCHAL][M][n]
    u64* rr;                       // [NCHAL][n]
    u64* out;                      // [NCHAL][N]
    u64 beta[GLP_PLONK_NCHAL], gamma[GLP_PLONK_NCHAL];
};

// dst[inst][k] = insts[inst].wire_vals[k], k < words (= W * n): the B matrices side by side
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_plonk_gather_wires_batch_kernel(const GlpPlonkInst* __restrict__ insts, u64 words, u32 blocks_per_instance,
                                                                           u64* __restrict__ dst) {
    const u32 inst = blockIdx.x / blocks_per_instance, lb = blockIdx.x - inst * blocks_per_instance;
    const u64* __restrict__ src = insts[inst].wire_vals;
    u64* __restrict__ out = dst + (u64)inst * words;
    for (u64 k = (u64)lb * 256 + threadIdx.x; k < words; k += (u64)blocks_per_instance * 256) out[k] = src[k];
}

// ---- K6a for B instances (glp_perm_quotients_kernel).  a: sigmas, ks, log_n, W (= routed), w_lo, w_hi; the rest of it is not read ----
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_perm_quotients_batch_kernel(GlpPermArgs a, const GlpPlonkInst* __restrict__ insts, u32 blocks_per_instance) {
    const u32 inst = blockIdx.x / blocks_per_instance;
    const GlpPlonkInst& d = insts[inst];
    const u64 n = 1ull << a.log_n;
    const u64 i = (u64)(blockIdx.x - inst * blocks_per_instance) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64* wires = d.wire_vals;
    u64* qv = d.qv;
    const u32 M = a.W / GLP_PLONK_CHUNK;
    u64 x = a.w_lo[i & 4095u];
    if (a.w_hi) x = gl_mul(x, a.w_hi[i >> 12]);
    for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) {
        const u64 beta = d.beta[t], gamma = d.gamma[t];
        const u64 bx = gl_mul(beta, x);
        auto chunk = [&](u32 c, u64& num, u64& den) {
            num = 1; den = 1;
            glp_static_for<0, GLP_PLONK_CHUNK>([&](auto j_) {
                constexpr int jj = decltype(j_)::value;
                const u32 j = c * GLP_PLONK_CHUNK + jj;
                const u64 wg = gl_add(wires[(u64)j * n + i], gamma);
                num = gl_mul(num, gl_add(wg, gl_mul(bx, a.ks[j])));
                den = gl_mul(den, gl_add(wg, gl_mul(beta, a.sigmas[(u64)j * n + i])));
            });
        };
        u64 run = 1;                                   // prefix products of the denominators
        for (u32 c = 0; c < M; c++) {
            u64 num, den;
            chunk(c, num, den);
            run = gl_mul(run, den);
            qv[((u64)t * M + c) * n + i] = run;
        }
        u64 inv = gl_inv(run);
        u64 ratio = 1;
        for (u32 c = M; c-- > 0;) {
            u64 num, den;
            chunk(c, num, den);
            const u64 before = c ? qv[((u64)t * M + c - 1) * n + i] : 1ull;
            const u64 q = gl_mul(num, gl_mul(inv, before));   // num_c / den_c
            inv = gl_mul(inv, den);
            qv[((u64)t * M + c) * n + i] = q;
            ratio = gl_mul(ratio, q);
        }
        d.rr[(u64)t * n + i] = ratio;
    }
}

// ---- K7 for B instances (glp_quotient_kernel).  a: everything shared; its wires, zs, pi, beta, gamma, alpha_pow and out are not read ----
template <bool POS, bool SMALL_MDS = false>
__global__ void __launch_bounds__(256) glp_quotient_batch_kernel(GlpQuotientArgs a, const GlpPlonkInst* __restrict__ insts, u32 blocks_per_instance) {
    const u32 inst = blockIdx.x / blocks_per_instance;
    const GlpPlonkInst& d = insts[inst];
    const u32 log_N = a.log_n + a.rate_bits;
    const u64 N = 1ull << log_N;
    const u64 i = (u64)(blockIdx.x - inst * blocks_per_instance) * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const u64* wires = d.wires_lde;
    const u64* zs = d.zs_lde;
    const u64* pi = d.pi_lde;
    const u64* alpha_pow = d.alpha_pow;
    const u32 M = a.R / GLP_PLONK_CHUNK;
    u64 e = 0;                                   // natural index of this point
    for (u32 b = 0; b < log_N; b++) e |= ((i >> b) & 1ull) << (log_N - 1 - b);
    u64 x = a.w_lo[e & 4095u];
    if (a.w_hi) x = gl_mul(x, a.w_hi[e >> 12]);
    x = gl_mul(x, a.shift);
    const u64 en = (e + (1ull << a.rate_bits)) & (N - 1);
    u64 inext = 0;
    for (u32 b = 0; b < log_N; b++) inext |= ((en >> b) & 1ull) << (log_N - 1 - b);
    const u64 zhi = a.zh_inv[e & ((1ull << a.rate_bits) - 1)];
    const u64 l1_over_zh = gl_mul(a.n_inv, a.inv_xm1[i]);
    const u64 q = a.consts[i], c0 = a.consts[N + i], c1 = a.consts[2 * N + i], c2 = a.consts[3 * N + i], q_pi = a.consts[4 * N + i];
    const u64 qx = a.q_ext ? a.q_ext[i] : 0ull;
    u64 acc[GLP_PLONK_NCHAL], prev[GLP_PLONK_NCHAL], bx[GLP_PLONK_NCHAL];
    const u64 pi_con = gl_sub(gl_mul(q_pi, wires[i]), pi ? pi[i] : 0ull);
    for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) {
        const u64 z = zs[((u64)t * M) * N + i];
        acc[t] = gl_mul(alpha_pow[(u64)t * a.n_con + 1], pi_con);
        prev[t] = z;
        bx[t] = gl_mul(d.beta[t], x);
    }
    for (u32 c = 0; c < M; c++) {
        u64 w[GLP_PLONK_CHUNK], sg[GLP_PLONK_CHUNK], kk[GLP_PLONK_CHUNK];
        glp_static_for<0, GLP_PLONK_CHUNK>([&](auto j_) {
            constexpr int jj = decltype(j_)::value;
            const u64 j = (u64)c * GLP_PLONK_CHUNK + jj;
            w[jj] = wires[j * N + i];
            sg[jj] = a.sigmas[j * N + i];
            kk[jj] = a.ks[j];
        });
        u64 g0 = gl_mul(q, glp_arith_gate<GlpGateBase>(c0, c1, c2, w[0], w[1], w[2], w[3]));
        u64 g1 = gl_mul(q, glp_arith_gate<GlpGateBase>(c0, c1, c2, w[4], w[5], w[6], w[7]));
        if (a.q_ext) {                           // wave-uniform
            u64 e0, e1;
            glp_ext_gate<GlpGateBase>(w, e0, e1);
            g0 = gl_add(g0, gl_mul(qx, e0));
            g1 = gl_add(g1, gl_mul(qx, e1));
        }
        for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) {
            u64 num = 1, den = 1;
            glp_static_for<0, GLP_PLONK_CHUNK>([&](auto j_) {
                constexpr int jj = decltype(j_)::value;
                const u64 wg = gl_add(w[jj], d.gamma[t]);
                num = gl_mul(num, gl_add(wg, gl_mul(bx[t], kk[jj])));
                den = gl_mul(den, gl_add(wg, gl_mul(d.beta[t], sg[jj])));
            });
            const u64 next = (c + 1 < M) ? zs[((u64)t * M + 1 + c) * N + i] : zs[((u64)t * M) * N + inext];
            const u64 perm = gl_sub(gl_mul(prev[t], num), gl_mul(next, den));
            const u64* ap = alpha_pow + (u64)t * a.n_con + 2 + 3 * c;
            acc[t] = gl_add(acc[t], gl_mul(ap[0], perm));
            acc[t] = gl_add(acc[t], gl_mul(ap[1], g0));
            acc[t] = gl_add(acc[t], gl_mul(ap[2], g1));
            prev[t] = next;
        }
    }
    if constexpr (POS) {
        const u64 q_pos = a.consts[5 * N + i];
        u64 pacc[GLP_PLONK_NCHAL];
        for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) pacc[t] = 0;
        u32 k = 0;
        const u64* ap0 = alpha_pow + 2 + 3 * M;
        auto wire = [&](int j) -> u64 { return wires[(u64)j * N + i]; };
        auto emit = [&](u64 con) {
            for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) pacc[t] = gl_add(pacc[t], gl_mul(ap0[(u64)t * a.n_con + k], con));
            k++;
        };
        if constexpr (SMALL_MDS) glp_poseidon_gate_constraints_fast<true>(wire, a.pos_consts, a.pos_consts + 360, a.pos_consts + 372, emit);
        else glp_poseidon_gate_constraints<GlpGateBase>(wire, a.pos_consts, a.pos_consts + 360, a.pos_consts + 372, emit);
        for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) acc[t] = gl_add(acc[t], gl_mul(q_pos, pacc[t]));
    }
    for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) {
        const u64 z = zs[((u64)t * M) * N + i];
        d.out[(u64)t * N + i] = gl_add(gl_mul(acc[t], zhi), gl_mul(l1_over_zh, gl_sub(z, 1)));   // alpha^0 = 1
    }
}

// ---- K7s for B instances (glp_quotient_sha_kernel): added to what the K7 launch wrote ----
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_quotient_sha_batch_kernel(GlpQuotientArgs a, const GlpPlonkInst* __restrict__ insts, u32 blocks_per_instance,
                                                                     u32 first_con) {
    const u32 inst = blockIdx.x / blocks_per_instance;
    const GlpPlonkInst& d = insts[inst];
    const u32 log_N = a.log_n + a.rate_bits;
    const u64 N = 1ull << log_N;
    const u64 i = (u64)(blockIdx.x - inst * blocks_per_instance) * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const u64* wires = d.wires_lde;
    u64* out = d.out;
    u64 e = 0;
    for (u32 b = 0; b < log_N; b++) e |= ((i >> b) & 1ull) << (log_N - 1 - b);
    const u64 zhi = a.zh_inv[e & ((1ull << a.rate_bits) - 1)];
    const u64 q[4] = {a.consts[6 * N + i], a.consts[7 * N + i], a.consts[8 * N + i], a.consts[9 * N + i]};
    const u64 c2 = a.consts[3 * N + i];
    u64 acc[GLP_PLONK_NCHAL];
    for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) acc[t] = 0;
    u32 k = 0;
    const u64* ap0 = d.alpha_pow + first_con;
    glp_sha_gate_constraints<GlpGateBase>([&](int j) -> u64 { return wires[(u64)j * N + i]; }, q, c2, [&](u64 con) {
        for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) acc[t] = gl_add(acc[t], gl_mul(ap0[(u64)t * a.n_con + k], con));
        k++;
    });
    for (u32 t = 0; t < GLP_PLONK_NCHAL; t++) out[(u64)t * N + i] = gl_add(out[(u64)t * N + i], gl_mul(acc[t], zhi));
}
