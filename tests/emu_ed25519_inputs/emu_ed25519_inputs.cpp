// tests/emu_ed25519_inputs/emu_ed25519_inputs.cpp — TEST INFRASTRUCTURE.  The kernels of glp_ed25519_leaf_inputs and glp_ed25519_half_scalars
// (csrc/ed25519_inputs.cuh) on the CPU, unchanged, through the launch sequences the driver (csrc/tm.hip) runs (glp_ed25519_leaf_inputs_launches,
// glp_ed25519_half_scalars_launch of that header), issued by GlpEmuLaunch of ../emu/hip_emu.h: the witness kernel over the slots' own triples,
// then the input kernel.  Neither kernel has a barrier, so the work-items run one after the other.  Never part of the
// product.  With -DGLP_EMU_ED_INPUTS_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that runs
// the reduction and both divisions over edge values and a few thousand random ones and checks their defining identities with a separate
// base-2^32 big-integer reference.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/ed25519_inputs.cuh"

extern "C" u64 emu_leaf_input_words(u32 form, u32 lo, u32 hi, u32 split) { return glp_ed25519_input_words(form, lo, hi, split); }

extern "C" int emu_half_scalars(const u64* ks, u64 n, u64* out) {
    GlpEmuLaunch l;
    glp_ed25519_half_scalars_launch(l, ks, n, out);
    return 0;
}

// x [8] -> q [8], r [4]
extern "C" int emu_divmod_l(const u64* x, u64* q, u64* r) {
    glp_w8 xv, qv;
    u64 rv[4];
    for (int i = 0; i < 8; i++) xv.w[i] = x[i];
    glp_divmod_l(xv, qv, rv);
    for (int i = 0; i < 8; i++) q[i] = qv.w[i];
    for (int i = 0; i < 4; i++) r[i] = rv[i];
    return 0;
}

#ifndef GLP_EMU_ED_INPUTS_MAIN      // the stand-alone program runs the reduction and the divisions only: it does not instantiate the two big kernels
// the launches of glp_ed25519_leaf_inputs: out [n][out_stride], status [n]
extern "C" int emu_leaf_inputs(u32 form, u32 lo, u32 hi, u32 split, const uint8_t* pubs, const uint8_t* sigs, const uint8_t* msgs, u32 msg_stride,
                               const u32* lens, const uint8_t* flags, const uint8_t* dummy, u64 n, const u64* k512, u64* out, u64 out_stride,
                               int32_t* status) {
    const u64 width = glp_ed25519_input_words(form, lo, hi, split);
    if (!width || out_stride < width || !msg_stride) return -1;
    std::vector<u64> recs((size_t)n * GLP_ED_REC);              // exact size: ASan sees any overrun
    GlpEdInputsArgs a;
    a.pubs = pubs; a.sigs = sigs; a.msgs = msgs; a.lens = lens; a.flags = flags; a.dummy = dummy; a.recs = recs.data(); a.k512 = k512;
    a.out = out; a.status = status; a.n = n; a.out_stride = out_stride; a.msg_stride = msg_stride; a.form = form; a.lo = lo; a.hi = hi;
    a.split = split;
    GlpEmuLaunch l;
    glp_ed25519_leaf_inputs_launches(l, a, recs.data());
    return 0;
}
#endif

#ifdef GLP_EMU_ED_INPUTS_MAIN
#include <cstdio>
// ---- a separate reference: little-endian base-2^32 digits, schoolbook, bit-serial remainder ----
typedef std::vector<uint32_t> Big;
static void trim(Big& a) { while (!a.empty() && a.back() == 0) a.pop_back(); }
static Big big_of(const u64* w, int n) { Big r; for (int i = 0; i < n; i++) { r.push_back((uint32_t)w[i]); r.push_back((uint32_t)(w[i] >> 32)); } trim(r); return r; }
static int big_cmp(const Big& a, const Big& b) {
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    for (size_t i = a.size(); i-- > 0;) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
static Big big_add(const Big& a, const Big& b) {
    Big r; uint64_t c = 0;
    for (size_t i = 0; i < a.size() || i < b.size() || c; i++) { c += (i < a.size() ? a[i] : 0ull) + (i < b.size() ? b[i] : 0ull); r.push_back((uint32_t)c); c >>= 32; }
    trim(r); return r;
}
static Big big_sub(const Big& a, const Big& b) {     // a >= b
    Big r; int64_t c = 0;
    for (size_t i = 0; i < a.size(); i++) { int64_t d = (int64_t)a[i] - (i < b.size() ? (int64_t)b[i] : 0) + c; c = d < 0 ? -1 : 0; r.push_back((uint32_t)(d + (d < 0 ? (1ll << 32) : 0))); }
    trim(r); return r;
}
static Big big_mul(const Big& a, const Big& b) {
    Big r(a.size() + b.size() + 1, 0);
    for (size_t i = 0; i < a.size(); i++) {
        uint64_t c = 0;
        for (size_t j = 0; j < b.size() || c; j++) { c += r[i + j] + (uint64_t)a[i] * (j < b.size() ? b[j] : 0u); r[i + j] = (uint32_t)c; c >>= 32; }
    }
    trim(r); return r;
}
static Big big_mod(const Big& a, const Big& m) {
    Big r;
    for (size_t i = a.size() * 32; i-- > 0;) {
        uint32_t c = (a[i / 32] >> (i % 32)) & 1;
        for (auto& d : r) { const uint32_t n = d >> 31; d = (d << 1) | c; c = n; }
        if (c) r.push_back(c);
        if (big_cmp(r, m) >= 0) r = big_sub(r, m);
    }
    return r;
}
static u64 next_word(u64& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    u64 z = st ^ (st >> 29);
    z *= 0xBF58476D1CE4E5B9ull;
    return z ^ (z >> 32);
}
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static const u64 ELLW[4] = {0x5812631a5cf5d3edull, 0x14def9dea2f79cd6ull, 0, 0x1000000000000000ull};

// the reduction of one k against its defining identities; *status_out = what the kernel said
static int check_pair(const u64 (&k)[4], int* status_out) {
    u64 out[8];
    emu_half_scalars(k, 1, out);
    *status_out = (int)out[7];
    const Big L = big_of(ELLW, 4), kb = big_of(k, 4);
    REQUIRE((big_cmp(kb, L) >= 0) == (out[7] == GLP_ED_IN_INVALID));
    if (out[7] != GLP_ED_IN_OK) { for (int i = 0; i < 7; i++) REQUIRE(out[i] == 0); return 0; }
    REQUIRE(out[0] & 1);                                                        // u odd
    REQUIRE((out[2] >> 16) == 0 && (out[5] >> 16) == 0 && out[6] <= 1);         // u, v < 2^144
    const u64 eight[1] = {8};
    const Big L8 = big_mul(L, big_of(eight, 1)), uk = big_mul(big_of(out, 3), kb), v = big_of(out + 3, 3);
    REQUIRE(out[6] || big_cmp(uk, v) >= 0);
    REQUIRE(big_mod(out[6] ? big_add(uk, v) : big_sub(uk, v), L8).empty());     // u k -+ v = 0 (mod 8L)
    return 0;
}
// q L + r reproduces x, r < L
static int check_div(const u64 (&x)[8]) {
    u64 q[8], r[4];
    emu_divmod_l(x, q, r);
    const Big L = big_of(ELLW, 4);
    REQUIRE(big_cmp(big_of(r, 4), L) < 0);
    REQUIRE(big_cmp(big_add(big_mul(big_of(q, 8), L), big_of(r, 4)), big_of(x, 8)) == 0);
    // glp_mod_l, which stays as it is, agrees
    u64 r2[4];
    glp_mod_l(x, r2);
    for (int i = 0; i < 4; i++) REQUIRE(r[i] == r2[i]);
    return 0;
}

int main() {
    u64 st = 20261020;
    int status = 0;
    // ---- the reduction: 0, 1, 2, 3, 2^126, 2^127 + 1, 2^200, L - 3, L - 2, L - 1, (L + 1) / 2, L, 2^256 - 1, then random k below L ----
    const u64 edges[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, 0, 0, 0}, {3, 0, 0, 0}, {0, 1ull << 62, 0, 0}, {1, 1ull << 63, 0, 0}, {0, 0, 0, 1ull << 8},
                            {ELLW[0] - 3, ELLW[1], 0, ELLW[3]}, {ELLW[0] - 2, ELLW[1], 0, ELLW[3]}, {ELLW[0] - 1, ELLW[1], 0, ELLW[3]},
                            {(ELLW[0] + 1) / 2 | (ELLW[1] << 63), ELLW[1] >> 1, 0, ELLW[3] >> 1},
                            {ELLW[0], ELLW[1], 0, ELLW[3]}, {~0ull, ~0ull, ~0ull, ~0ull}};
    // what ed25519_circuit.half_size_pair does with each: the four scalars next to L have no pair below 2^144 (u k = -+v needs u or v ~ L)
    const int want[] = {0, 0, 0, 0, 0, 0, 0, GLP_ED_IN_NO_PAIR, GLP_ED_IN_NO_PAIR, GLP_ED_IN_NO_PAIR, GLP_ED_IN_NO_PAIR, GLP_ED_IN_INVALID, GLP_ED_IN_INVALID};
    for (size_t e = 0; e < sizeof(edges) / sizeof(edges[0]); e++) {
        if (check_pair(edges[e], &status)) return 1;
        if (status != want[e]) std::printf("edge %zu: status %d, expected %d\n", e, status, want[e]);
        REQUIRE(status == want[e]);
    }
    for (int it = 0; it < 3000; it++) {
        u64 k[4] = {next_word(st), next_word(st), next_word(st), next_word(st) >> 4};
        if (it % 7 == 0) { k[3] = 0; k[2] >>= (it % 64); }          // short scalars too
        if (!glp_scalar_lt_l(k)) k[3] >>= 1;
        if (check_pair(k, &status)) return 1;
        REQUIRE(status == GLP_ED_IN_OK);
    }
    // ---- the division by L: zero, below L, L - 1, L, L + 1, 2^256, 2^512 - 1, single bits at word edges (shifts by 0 and 64), random ----
    {
        u64 x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (check_div(x)) return 1;
        for (int d = -1; d <= 1; d++) {
            u64 y[8] = {ELLW[0] + (u64)d, ELLW[1], 0, ELLW[3], 0, 0, 0, 0};
            if (check_div(y)) return 1;
        }
        for (int b = 0; b < 512; b += (b % 64 == 63 || b % 64 == 0) ? 1 : 31) {
            u64 y[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            y[b >> 6] = 1ull << (b & 63);
            if (check_div(y)) return 1;
        }
        u64 ones[8];
        for (auto& w : ones) w = ~0ull;
        if (check_div(ones)) return 1;
        for (int it = 0; it < 3000; it++) {
            u64 y[8];
            for (auto& w : y) w = next_word(st);
            for (int i = 7; i > 7 - it % 8; i--) y[i] = 0;
            if (check_div(y)) return 1;
        }
    }
    // ---- the general division against the exact one: (a * 8L) / 8L = a, remainder 0 (the q2 form), and shifts by every amount ----
    for (int it = 0; it < 600; it++) {
        glp_w8 a = glp_w8_zero(), q, r;
        a.w[0] = next_word(st); a.w[1] = next_word(st); a.w[2] = next_word(st) >> (it % 64);
        const glp_w8 L8 = glp_w8_shl(glp_w8_ell(), 3);
        glp_w8_divmod(glp_w8_mul<3, 4>(a, L8), L8, q, r);
        REQUIRE(glp_w8_is_zero(r) && glp_w8_cmp(q, a) == 0);
        const u32 sh = (u32)it % 512;
        const glp_w8 s = glp_w8_shl(glp_w8_small(1), sh);
        REQUIRE(glp_w8_bitlen(s) == (int)sh + 1 && s.w[sh >> 6] == 1ull << (sh & 63));
    }
    std::printf("emu_ed25519_inputs_san ok\n");
    return 0;
}
#endif
