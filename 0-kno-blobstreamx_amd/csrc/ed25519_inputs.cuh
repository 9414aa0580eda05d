// ed25519_inputs.cuh — the INPUT VECTORS of the signature leaf on the device: what ed25519_circuit.witness_inputs builds with Python integers
// (the limbs of x_A, x_R, t = h div L, k, and the half-size form's hints u, v, sign, q1, w, q2), word for word, one work-item per slot.
//
//   * glp_w8 / glp_s8      512-bit magnitudes (8 u64 words, little-endian) and sign-magnitude integers: add, subtract, compare, bit length,
//                          a product truncated to 512 bits, and a shift-subtract division whose step count is the bit-length difference of its
//                          operands.  Every word loop has a compile-time trip count and is unrolled: no register array is indexed dynamically
//                          (a variable shift is a barrel of three conditional word moves and one bit shift).
//   * glp_half_size_pair   ed25519_circuit.half_size_pair: Lagrange reduction of the lattice {(t, r): r = t k mod 8L}, the same swap, rounding,
//                          exit, candidate order and tie-break as the Python.  Every intermediate stays below 2^512 (the norms are at most
//                          (8L)^2 + 1 < 2^511); the factors of every product are vector coordinates, sums of two of them, or the rounded
//                          quotient mu, all below 2^258: the products read five words of each factor.
//   * glp_divmod_l         quotient and remainder of a 512-bit value by L (beside glp_mod_l, which stays as it is).
//   * glp_ed25519_leaf_inputs_kernel / glp_ed25519_half_scalars_kernel   the two kernels of glp_ed25519_leaf_inputs / glp_ed25519_half_scalars.
// Plain HIP C++ (tests/emu_ed25519_inputs runs these bodies on the CPU, under ASan + UBSan as a stand-alone program).
#pragma once
#include "ed25519_kernels.cuh"

#define GLP_ED_IN_OK 0
#define GLP_ED_IN_REJECT 1
#define GLP_ED_IN_NO_PAIR 2
#define GLP_ED_IN_INVALID 3
#define GLP_ED_FORM_PLAIN 0      // (a) A, R, S, message, limbs
#define GLP_ED_FORM_FLAGGED 1    // (b) flag, key, message | R, S of the verified triple (its A is the key or a constant of the circuit), limbs
#define GLP_ED_FORM_VOTE 2       // (c) flag, key, message padded to max_len, L, one-hot of L - min_len | as (b)
#define GLP_ED_LIMBS 11          // 24-bit limbs of a field element / of t, k, w
#define GLP_ED_TAIL_WORDS 38     // u[6] v[6] neg q1[7] w[11] q2[7]
#define GLP_ED_HALF_BITS 144
#define GLP_ED_REDUCE_CAP 600    // iterations of the reduction: the norm falls strictly, 38-71 for random k, 255 division steps in all for k = 1

#define GLP_UNROLL _Pragma("unroll")

struct glp_w8 { u64 w[8]; };
struct glp_s8 { glp_w8 m; u32 neg; };      // sign and magnitude; zero has neg = 0

GL_HD glp_w8 glp_w8_zero() { glp_w8 r; GLP_UNROLL for (int i = 0; i < 8; i++) r.w[i] = 0; return r; }
GL_HD glp_w8 glp_w8_small(u64 x) { glp_w8 r = glp_w8_zero(); r.w[0] = x; return r; }
GL_HD glp_w8 glp_w8_from4(const u64 (&x)[4]) { glp_w8 r = glp_w8_zero(); GLP_UNROLL for (int i = 0; i < 4; i++) r.w[i] = x[i]; return r; }
GL_HD glp_w8 glp_w8_ell() {
    glp_w8 r = glp_w8_zero();
    r.w[0] = 0x5812631a5cf5d3edull; r.w[1] = 0x14def9dea2f79cd6ull; r.w[3] = 0x1000000000000000ull;
    return r;
}
GL_HD bool glp_w8_is_zero(const glp_w8& a) { u64 t = 0; GLP_UNROLL for (int i = 0; i < 8; i++) t |= a.w[i]; return t == 0; }
// r = a + b mod 2^512; the carry out
GL_HD u64 glp_w8_add(glp_w8& r, const glp_w8& a, const glp_w8& b) {
    u64 c = 0;
    GLP_UNROLL for (int i = 0; i < 8; i++) {
        const u64 s = a.w[i] + b.w[i];
        const u64 c1 = s < a.w[i];
        const u64 s2 = s + c;
        c = c1 | (u64)(s2 < s);
        r.w[i] = s2;
    }
    return c;
}
// r = a - b mod 2^512; the borrow out (1 when a < b)
GL_HD u64 glp_w8_sub(glp_w8& r, const glp_w8& a, const glp_w8& b) {
    u64 br = 0;
    GLP_UNROLL for (int i = 0; i < 8; i++) {
        const u64 d1 = a.w[i] - b.w[i];
        const u64 b1 = a.w[i] < b.w[i];
        const u64 d2 = d1 - br;
        br = b1 | (u64)(d1 < br);
        r.w[i] = d2;
    }
    return br;
}
// -1, 0, 1
GL_HD int glp_w8_cmp(const glp_w8& a, const glp_w8& b) {
    int r = 0;
    GLP_UNROLL for (int i = 0; i < 8; i++) r = a.w[i] > b.w[i] ? 1 : (a.w[i] < b.w[i] ? -1 : r);
    return r;
}
GL_HD int glp_w8_bitlen(const glp_w8& a) {
    int n = 0;
    GLP_UNROLL for (int i = 0; i < 8; i++) if (a.w[i]) n = 64 * i + 64 - __builtin_clzll(a.w[i]);
    return n;
}
GL_HD glp_w8 glp_w8_shl1(const glp_w8& a) {
    glp_w8 r;
    GLP_UNROLL for (int i = 7; i > 0; i--) r.w[i] = (a.w[i] << 1) | (a.w[i - 1] >> 63);
    r.w[0] = a.w[0] << 1;
    return r;
}
GL_HD glp_w8 glp_w8_shr1(const glp_w8& a) {
    glp_w8 r;
    GLP_UNROLL for (int i = 0; i < 7; i++) r.w[i] = (a.w[i] >> 1) | (a.w[i + 1] << 63);
    r.w[7] = a.w[7] >> 1;
    return r;
}
// a << sh, sh < 512, bits past 2^512 dropped.  Word moves by 4, 2, 1 under the bits of sh / 64, then one shift below 64 (none at all when
// sh is a multiple of 64: x >> 64 is not a shift C++ defines)
GL_HD glp_w8 glp_w8_shl(const glp_w8& a, u32 sh) {
    glp_w8 r = a;
    if (sh & 256) { GLP_UNROLL for (int i = 7; i >= 4; i--) r.w[i] = r.w[i - 4]; GLP_UNROLL for (int i = 0; i < 4; i++) r.w[i] = 0; }
    if (sh & 128) { GLP_UNROLL for (int i = 7; i >= 2; i--) r.w[i] = r.w[i - 2]; r.w[0] = r.w[1] = 0; }
    if (sh & 64) { GLP_UNROLL for (int i = 7; i >= 1; i--) r.w[i] = r.w[i - 1]; r.w[0] = 0; }
    const u32 bs = sh & 63;
    if (bs) {
        GLP_UNROLL for (int i = 7; i >= 1; i--) r.w[i] = (r.w[i] << bs) | (r.w[i - 1] >> (64 - bs));
        r.w[0] <<= bs;
    }
    return r;
}
// the low 512 bits of a * b, reading words [0, NA) of a and [0, NB) of b (the caller knows the rest is zero)
template <int NA, int NB>
GL_HD glp_w8 glp_w8_mul(const glp_w8& a, const glp_w8& b) {
    glp_w8 r;
    u64 c0 = 0, c1 = 0, c2 = 0;
    GLP_UNROLL for (int col = 0; col < 8; col++) {
        GLP_UNROLL for (int i = 0; i < NA; i++) {
            const int j = col - i;
            if (j >= 0 && j < NB) {
                const unsigned __int128 p = (unsigned __int128)a.w[i] * b.w[j];
                const u64 lo = (u64)p, hi = (u64)(p >> 64);
                c0 += lo;
                const u64 t = hi + (u64)(c0 < lo);          // hi <= 2^64 - 2
                c1 += t;
                c2 += (u64)(c1 < t);
            }
        }
        r.w[col] = c0; c0 = c1; c1 = c2; c2 = 0;
    }
    return r;
}
// q = n div d, r = n mod d (d > 0; d = 0 gives q = 0, r = n).  Restoring shift-subtract: bitlen(n) - bitlen(d) + 1 steps
GL_HD void glp_w8_divmod(const glp_w8& n, const glp_w8& d, glp_w8& q, glp_w8& r) {
    q = glp_w8_zero();
    r = n;
    const int bn = glp_w8_bitlen(n), bd = glp_w8_bitlen(d);
    if (bd == 0 || bn < bd) return;
    glp_w8 t = glp_w8_shl(d, (u32)(bn - bd));
    for (int s = bn - bd; s >= 0; s--) {
        q = glp_w8_shl1(q);
        glp_w8 diff;
        if (!glp_w8_sub(diff, r, t)) { r = diff; q.w[0] |= 1; }
        t = glp_w8_shr1(t);
    }
}

GL_HD glp_s8 glp_s8_make(const glp_w8& m, u32 neg) { glp_s8 r; r.m = m; r.neg = glp_w8_is_zero(m) ? 0u : neg; return r; }
GL_HD glp_s8 glp_s8_neg(const glp_s8& a) { return glp_s8_make(a.m, a.neg ^ 1u); }
GL_HD glp_s8 glp_s8_add(const glp_s8& a, const glp_s8& b) {
    glp_w8 m;
    if (a.neg == b.neg) { glp_w8_add(m, a.m, b.m); return glp_s8_make(m, a.neg); }
    if (!glp_w8_sub(m, a.m, b.m)) return glp_s8_make(m, a.neg);
    glp_w8_sub(m, b.m, a.m);
    return glp_s8_make(m, b.neg);
}
GL_HD glp_s8 glp_s8_sub(const glp_s8& a, const glp_s8& b) { return glp_s8_add(a, glp_s8_neg(b)); }
template <int NA, int NB>
GL_HD glp_s8 glp_s8_mul(const glp_s8& a, const glp_s8& b) { return glp_s8_make(glp_w8_mul<NA, NB>(a.m, b.m), a.neg ^ b.neg); }
// floor(n / d), d > 0: Python's // for a negative numerator
GL_HD glp_s8 glp_s8_floordiv(const glp_s8& n, const glp_w8& d) {
    glp_w8 q, r;
    glp_w8_divmod(n.m, d, q, r);
    if (n.neg && !glp_w8_is_zero(r)) glp_w8_add(q, q, glp_w8_small(1));
    return glp_s8_make(q, n.neg);
}

// quotient (up to 260 bits) and remainder of a 512-bit value by L
GL_HD void glp_divmod_l(const glp_w8& x, glp_w8& q, u64 (&r)[4]) {
    glp_w8 rem;
    glp_w8_divmod(x, glp_w8_ell(), q, rem);
    GLP_UNROLL for (int i = 0; i < 4; i++) r[i] = rem.w[i];
}

struct glp_vec2 { glp_s8 t, r; };
GL_HD glp_w8 glp_vec2_norm(const glp_vec2& v) {
    glp_w8 n;
    glp_w8_add(n, glp_w8_mul<5, 5>(v.t.m, v.t.m), glp_w8_mul<5, 5>(v.r.m, v.r.m));
    return n;
}
GL_HD glp_w8 glp_s8_absmax(const glp_vec2& v) { return glp_w8_cmp(v.t.m, v.r.m) >= 0 ? v.t.m : v.r.m; }

// ed25519_circuit.half_size_pair: u odd, 0 < u, 0 <= v, both below 2^144, u k = (neg ? -v : v) (mod 8L).  Returns GLP_ED_IN_OK, NO_PAIR
// (the Python raises) or INVALID (k >= L)
GL_HD int glp_half_size_pair(const u64 (&k)[4], u64 (&u)[3], u64 (&v)[3], u32& neg) {
    GLP_UNROLL for (int i = 0; i < 3; i++) { u[i] = 0; v[i] = 0; }
    neg = 0;
    if (!glp_scalar_lt_l(k)) return GLP_ED_IN_INVALID;
    glp_vec2 b1, b2;
    b1.t = glp_s8_make(glp_w8_small(1), 0); b1.r = glp_s8_make(glp_w8_from4(k), 0);
    b2.t = glp_s8_make(glp_w8_zero(), 0);   b2.r = glp_s8_make(glp_w8_shl(glp_w8_ell(), 3), 0);
    glp_w8 n1 = glp_vec2_norm(b1);
    {
        const glp_w8 n2 = glp_vec2_norm(b2);
        if (glp_w8_cmp(n1, n2) > 0) { const glp_vec2 s = b1; b1 = b2; b2 = s; n1 = n2; }
    }
    for (int it = 0;; it++) {
        if (it >= GLP_ED_REDUCE_CAP || glp_w8_is_zero(n1)) return GLP_ED_IN_NO_PAIR;
        // mu = floor((<b1, b2> + |b1|^2 // 2) / |b1|^2): the nearest integer of <b1, b2> / <b1, b1>
        const glp_s8 dot = glp_s8_add(glp_s8_mul<5, 5>(b1.t, b2.t), glp_s8_mul<5, 5>(b1.r, b2.r));
        const glp_s8 mu = glp_s8_floordiv(glp_s8_add(dot, glp_s8_make(glp_w8_shr1(n1), 0)), n1);
        b2.t = glp_s8_sub(b2.t, glp_s8_mul<5, 5>(mu, b1.t));
        b2.r = glp_s8_sub(b2.r, glp_s8_mul<5, 5>(mu, b1.r));
        const glp_w8 n2 = glp_vec2_norm(b2);
        if (glp_w8_cmp(n2, n1) >= 0) break;
        const glp_vec2 s = b1; b1 = b2; b2 = s; n1 = n2;
    }
    // b1, b2, b1 + b2, b1 - b2 in that order; those with an odd first coordinate; the FIRST minimum of max(|t|, |r|)
    glp_vec2 best = b1, cand = b1;
    glp_w8 best_m = glp_w8_zero();
    bool have = false;
    GLP_UNROLL for (int c = 0; c < 4; c++) {
        if (c == 1) cand = b2;
        if (c == 2) { cand.t = glp_s8_add(b1.t, b2.t); cand.r = glp_s8_add(b1.r, b2.r); }
        if (c == 3) { cand.t = glp_s8_sub(b1.t, b2.t); cand.r = glp_s8_sub(b1.r, b2.r); }
        if (cand.t.m.w[0] & 1) {
            const glp_w8 m = glp_s8_absmax(cand);
            if (!have || glp_w8_cmp(m, best_m) < 0) { best = cand; best_m = m; have = true; }
        }
    }
    if (!have) return GLP_ED_IN_NO_PAIR;
    if (best.r.neg) { best.t = glp_s8_neg(best.t); best.r = glp_s8_neg(best.r); }
    u64 high = (best.t.m.w[2] >> 16) | (best.r.m.w[2] >> 16);
    GLP_UNROLL for (int i = 3; i < 8; i++) high |= best.t.m.w[i] | best.r.m.w[i];
    if (high) return GLP_ED_IN_NO_PAIR;
    GLP_UNROLL for (int i = 0; i < 3; i++) { u[i] = best.t.m.w[i]; v[i] = best.r.m.w[i]; }
    neg = best.t.neg;
    return GLP_ED_IN_OK;
}

// ks [n][4] -> out [n][8]: u[3] v[3] neg status
template <int UNUSED = 0>
__global__ void __launch_bounds__(64) glp_ed25519_half_scalars_kernel(const u64* __restrict__ ks, u64 n, u64* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 k[4], u[3], v[3];
    u32 neg;
    GLP_UNROLL for (int j = 0; j < 4; j++) k[j] = ks[i * 4 + j];
    const int st = glp_half_size_pair(k, u, v, neg);
    u64* o = out + i * 8;
    GLP_UNROLL for (int j = 0; j < 3; j++) { o[j] = u[j]; o[3 + j] = v[j]; }
    o[6] = neg;
    o[7] = (u64)st;
}

// N 24-bit limbs of v, least significant first (limbs_of)
template <int N>
GL_HD void glp_put_limbs24(const glp_w8& v, u64* __restrict__ out) {
    GLP_UNROLL for (int i = 0; i < N; i++) {
        const int bit = 24 * i, w = bit >> 6, s = bit & 63;
        u64 x = v.w[w] >> s;
        if (s > 40 && w + 1 < 8) x |= v.w[w + 1] << (64 - s);
        out[i] = x & 0xFFFFFFull;
    }
}

// words of one row; 0 for a layout no statement has
GL_HD u64 glp_ed25519_input_words(u32 form, u32 lo, u32 hi, u32 split) {
    if (form > GLP_ED_FORM_VOTE || lo > hi || hi > (1u << 16) || (form != GLP_ED_FORM_VOTE && lo != hi)) return 0;
    u64 head = 0;
    if (form == GLP_ED_FORM_PLAIN) head = 96 + (u64)hi;
    else if (form == GLP_ED_FORM_FLAGGED) head = 1 + 32 + (u64)hi + 64;
    else head = 1 + 32 + (u64)hi + 1 + (u64)(hi - lo + 1) + 64;
    return head + 4 * GLP_ED_LIMBS + (split ? GLP_ED_TAIL_WORDS : 0);
}

struct GlpEdInputsArgs {
    const uint8_t* pubs;      // [n][32]
    const uint8_t* sigs;      // [n][64]
    const uint8_t* msgs;      // [n][msg_stride]
    const u32* lens;          // [n]
    const uint8_t* flags;     // [n], forms (b), (c)
    const uint8_t* dummy;     // pub32 | sig64 | msg[lo], forms (b), (c)
    const u64* recs;          // [n][GLP_ED_REC]: the witness kernel's records of the slots' OWN triples
    const u64* k512;
    u64* out;                 // [n][out_stride]
    int32_t* status;          // [n]
    u64 n, out_stride;
    u32 msg_stride, form, lo, hi, split;
};

// Row i of out = witness_inputs(slot i) (ed25519_circuit.py), status[i] says whether it is.  A row that is not OK is all zero.
// A flagged slot takes x_A, x_R and k from its record (REJECT when the record says invalid); an unflagged slot verifies the caller's constant
// dummy triple, whose A and R are decoded and whose k is reduced here (REJECT when they do not decode: the circuit would refuse it anyway).
template <int UNUSED = 0>
__global__ void __launch_bounds__(64) glp_ed25519_leaf_inputs_kernel(const GlpEdInputsArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    u64* __restrict__ row = a.out + i * a.out_stride;
    const u64 width = glp_ed25519_input_words(a.form, a.lo, a.hi, a.split);
    const u32 len = a.lens[i];
    int st = (len < a.lo || len > a.hi || len > a.msg_stride) ? GLP_ED_IN_INVALID : GLP_ED_IN_OK;
    const u32 flag = a.form == GLP_ED_FORM_PLAIN ? 1u : (a.flags[i] ? 1u : 0u);
    const uint8_t* pub = a.pubs + i * 32;
    const uint8_t* msg = a.msgs + i * (u64)a.msg_stride;
    const uint8_t* vp = flag ? pub : a.dummy;                        // the VERIFIED triple
    const uint8_t* vs = flag ? a.sigs + i * 64 : a.dummy + 32;
    const uint8_t* vm = flag ? msg : a.dummy + 96;
    const u32 vlen = flag ? len : a.lo;
    u64 kk[4] = {0, 0, 0, 0}, xa[4] = {0, 0, 0, 0}, xr[4] = {0, 0, 0, 0};
    if (st == GLP_ED_IN_OK) {
        if (flag) {
            const u64* rec = a.recs + i * GLP_ED_REC;
            if (!rec[0]) st = GLP_ED_IN_REJECT;
            GLP_UNROLL for (int j = 0; j < 4; j++) { kk[j] = rec[1 + j]; xa[j] = rec[5 + j]; xr[j] = rec[13 + j]; }
        } else {
            u64 Aenc[4], Renc[4];
            GLP_UNROLL for (int j = 0; j < 4; j++) { Aenc[j] = glp_load_le64(vp + 8 * j); Renc[j] = glp_load_le64(vs + 8 * j); }
            glp_fe Ax, Ay, Rx, Ry;
            if (glp_ed_decode(Aenc, Ax, Ay) && glp_ed_decode(Renc, Rx, Ry)) { glp_fe_pack(Ax, xa); glp_fe_pack(Rx, xr); }
            else st = GLP_ED_IN_REJECT;
        }
    }
    glp_w8 t = glp_w8_zero();
    if (st == GLP_ED_IN_OK) {
        u64 hh[8];
        glp_sha512_stream([&](u64 pos) -> u64 { return pos < 32 ? vs[pos] : (pos < 64 ? vp[pos - 32] : vm[pos - 64]); }, 64 + (u64)vlen, a.k512, hh);
        glp_w8 h;                                  // the digest bytes as a little-endian integer
        GLP_UNROLL for (int j = 0; j < 8; j++) {
            u64 x = hh[j], r = 0;
            GLP_UNROLL for (int b = 0; b < 8; b++) { r = (r << 8) | (x & 0xff); x >>= 8; }
            h.w[j] = r;
        }
        if (flag) {                                // t = (h - k) div L with the record's k
            glp_w8 hk;
            u64 rem[4];
            if (glp_w8_sub(hk, h, glp_w8_from4(kk))) st = GLP_ED_IN_REJECT;
            glp_divmod_l(hk, t, rem);
        } else {
            glp_divmod_l(h, t, kk);
        }
    }
    u64 u[3] = {0, 0, 0}, v[3] = {0, 0, 0};
    u32 neg = 0;
    glp_w8 q1 = glp_w8_zero(), q2 = glp_w8_zero(), w = glp_w8_zero();
    if (st == GLP_ED_IN_OK && a.split) {
        st = glp_half_size_pair(kk, u, v, neg);
        if (st == GLP_ED_IN_INVALID) st = GLP_ED_IN_REJECT;          // a k that is not reduced: no honest record has one
        if (st == GLP_ED_IN_OK) {
            glp_w8 uw = glp_w8_zero(), vw = glp_w8_zero(), S = glp_w8_zero(), rem;
            GLP_UNROLL for (int j = 0; j < 3; j++) { uw.w[j] = u[j]; vw.w[j] = v[j]; }
            GLP_UNROLL for (int j = 0; j < 4; j++) S.w[j] = glp_load_le64(vs + 32 + 8 * j);
            glp_w8_divmod(glp_w8_mul<3, 4>(uw, S), glp_w8_ell(), q1, w);                      // u S = q1 L + w
            glp_w8 num;                                                                       // u k -+ v = q2 * 8L, exactly
            const glp_w8 uk = glp_w8_mul<3, 4>(uw, glp_w8_from4(kk));
            if (neg) glp_w8_add(num, uk, vw); else glp_w8_sub(num, uk, vw);
            glp_w8_divmod(num, glp_w8_shl(glp_w8_ell(), 3), q2, rem);
        }
    }
    a.status[i] = st;
    if (st != GLP_ED_IN_OK) {
        for (u64 j = 0; j < width; j++) row[j] = 0;
        return;
    }
    u64 o = 0;
    if (a.form != GLP_ED_FORM_PLAIN) {
        row[o++] = flag;
        for (int j = 0; j < 32; j++) row[o++] = pub[j];
        for (u32 j = 0; j < a.hi; j++) row[o++] = j < len ? msg[j] : 0;         // (b): len = hi
        if (a.form == GLP_ED_FORM_VOTE) {
            row[o++] = len;
            for (u32 j = a.lo; j <= a.hi; j++) row[o++] = j == len ? 1 : 0;
        }
    } else {
        for (int j = 0; j < 32; j++) row[o++] = vp[j];
    }
    for (int j = 0; j < 64; j++) row[o++] = vs[j];
    if (a.form == GLP_ED_FORM_PLAIN) for (u32 j = 0; j < len; j++) row[o++] = msg[j];
    glp_put_limbs24<GLP_ED_LIMBS>(glp_w8_from4(xa), row + o); o += GLP_ED_LIMBS;
    glp_put_limbs24<GLP_ED_LIMBS>(glp_w8_from4(xr), row + o); o += GLP_ED_LIMBS;
    glp_put_limbs24<GLP_ED_LIMBS>(t, row + o); o += GLP_ED_LIMBS;
    glp_put_limbs24<GLP_ED_LIMBS>(glp_w8_from4(kk), row + o); o += GLP_ED_LIMBS;
    if (a.split) {
        glp_w8 uw = glp_w8_zero(), vw = glp_w8_zero();
        GLP_UNROLL for (int j = 0; j < 3; j++) { uw.w[j] = u[j]; vw.w[j] = v[j]; }
        glp_put_limbs24<6>(uw, row + o); o += 6;
        glp_put_limbs24<6>(vw, row + o); o += 6;
        row[o++] = neg;
        glp_put_limbs24<7>(q1, row + o); o += 7;
        glp_put_limbs24<GLP_ED_LIMBS>(w, row + o); o += GLP_ED_LIMBS;
        glp_put_limbs24<7>(q2, row + o); o += 7;
    }
}

// The launches of the calls, written once for the driver (tm.hip, l = GlpLaunch, device pointers) and the CPU emulation (l = GlpEmuLaunch, host
// pointers): one work-item per slot, 64 per workgroup
template <class L>
static inline void glp_ed25519_witness_launch(L& l, const uint8_t* pubs, const uint8_t* sigs, const uint8_t* msgs, u32 msg_stride, const u32* lens,
                                              u64 n, const u64* k512, u64* out) {
    l.launch(glp_ed25519_witness_kernel<0>, (n + 63) / 64, 64, pubs, sigs, msgs, msg_stride, lens, n, k512, out);
}
template <class L> static inline void glp_ed25519_half_scalars_launch(L& l, const u64* ks, u64 n, u64* out) {
    l.launch(glp_ed25519_half_scalars_kernel<0>, (n + 63) / 64, 64, ks, n, out);
}
// the witness kernel over the slots' own triples into recs (= a.recs, writable), then the input kernel
template <class L> static inline void glp_ed25519_leaf_inputs_launches(L& l, const GlpEdInputsArgs& a, u64* recs) {
    glp_ed25519_witness_launch(l, a.pubs, a.sigs, a.msgs, a.msg_stride, a.lens, a.n, a.k512, recs);
    l.launch(glp_ed25519_leaf_inputs_kernel<0>, (a.n + 63) / 64, 64, a);
}
