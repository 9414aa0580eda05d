// check_plan.h — the arithmetic of the witness checker that host code and kernels share (check.hip, check_kernels.cuh; host tests call it
// through tests/emu_check): decoding one sigma value into the cell it names, the host-built tables the decode reads, and the packed
// (row, kind, index) key of a violation.
//
// The key stores sigma as field values  sigma(j, i) = k_{j'} * w_n^{i'}  (k_j = 7^j, w_n the ctx's primitive n-th root of unity — the two-adic
// generator is a build parameter, gl_field.cuh).  Decoding v:
//   v^n = k_{j'}^n * (w_n^{i'})^n = k_{j'}^n          selects j' from the table kn[j] = k_j^n, j < R (distinct: 7 generates the whole group, so
//                                                     7^(j n) = 7^(j' n) needs (j - j') n = 0 mod p - 1, impossible for 0 < |j - j'| n < p - 1)
//   u = v / k_{j'} lies in the order-n subgroup       its discrete logarithm i' bit by bit, lowest first: with the bits below b cleared,
//                                                     u^(n / 2^(b+1)) is -1 when bit b is set (then u *= w_n^(-2^b)) and 1 when it is clear
// A v whose n-th power is not in the table (0, a point of another coset, a coset j' >= R) is no routed cell: GLP_SIGMA_BAD.
// Cell indices are j * n + i < 160 * 2^24 < 2^32: one u32 per routed cell.
#pragma once
#include "gl_field.cuh"

#define GLP_SIGMA_BAD 0xFFFFFFFFu
#define GLP_CHECK_TW_SPLIT 12          // the ctx's root tables are two-level: w^e = lo[e & 4095] * hi[e >> 12] (ntt_plan.h)

struct GlpSigmaTables {
    const u64* kn;        // [R] k_j^n
    const u64* kinv;      // [R] 1 / k_j
    const u64* winv_lo;   // the ctx's INVERSE root table of size n: w_n^-e = winv_lo[e & 4095] * winv_hi[e >> 12] (winv_hi null for n <= 4096)
    const u64* winv_hi;
    u32 log_n, R;
};

GL_HD u32 glp_sigma_decode(u64 v, const GlpSigmaTables& T) {
    u64 vn = v;
    for (u32 s = 0; s < T.log_n; s++) vn = gl_mul(vn, vn);
    u32 jp = GLP_SIGMA_BAD;
    for (u32 j = 0; j < T.R; j++) if (T.kn[j] == vn) { jp = j; break; }
    if (jp == GLP_SIGMA_BAD) return GLP_SIGMA_BAD;
    u64 u = gl_mul(v, T.kinv[jp]);
    u32 ip = 0;
    for (u32 b = 0; b < T.log_n; b++) {
        u64 e = u;
        for (u32 s = b + 1; s < T.log_n; s++) e = gl_mul(e, e);
        if (e == 1) continue;
        if (e != GL_P - 1) return GLP_SIGMA_BAD;          // cannot happen once v^n matched: u^n = 1
        ip |= 1u << b;
        const u64 wi = b < GLP_CHECK_TW_SPLIT ? T.winv_lo[1u << b] : T.winv_hi[1u << (b - GLP_CHECK_TW_SPLIT)];
        u = gl_mul(u, wi);
    }
    if (u != 1) return GLP_SIGMA_BAD;
    return (jp << T.log_n) | ip;
}

// host: kn[j] = k_j^n and kinv[j] = 1 / k_j for k_j = 7^j, j < R
static inline void glp_sigma_fill_tables(u32 log_n, u32 R, u64* kn, u64* kinv) {
    const u64 seven_inv = gl_inv(7);
    u64 k = 1, ki = 1;
    for (u32 j = 0; j < R; j++) {
        u64 t = k;
        for (u32 s = 0; s < log_n; s++) t = gl_mul(t, t);
        kn[j] = t; kinv[j] = ki;
        k = gl_mul(k, 7); ki = gl_mul(ki, seven_inv);
    }
}

// a violation's sort key: ascending = by row, then kind (gate before copy), then index.  row < 2^24, index < 2^19.
#define GLP_CHECK_KEY_NONE 0xFFFFFFFFFFFFFFFFull
GL_HD u64 glp_check_key(u32 row, u32 kind, u32 index) { return ((u64)row << 20) | ((u64)kind << 19) | index; }
GL_HD u32 glp_check_key_row(u64 key) { return (u32)(key >> 20); }
GL_HD u32 glp_check_key_kind(u64 key) { return (u32)(key >> 19) & 1u; }
GL_HD u32 glp_check_key_index(u64 key) { return (u32)key & 0x7FFFFu; }
