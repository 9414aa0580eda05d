// tests/emu_plonk_batch/emu_plonk_batch.cpp — TEST INFRASTRUCTURE.  The kernels of glp_plonk_prove_batch (csrc/plonk_batch_kernels.cuh) on the
// CPU, unchanged, launched through ../emu/hip_emu.h with the grids the driver uses (256 lanes, B * blocks_per_instance workgroups), beside the
// single-instance bodies of csrc/plonk_kernels.cuh they must equal word for word.  Never part of the product.
// With -DGLP_EMU_PLONK_BATCH_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that compares
// batched against single on small shapes.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/plonk_batch_kernels.cuh"
#include "../../0-kno-blobstreamx_amd/csrc/ntt_plan.h"

namespace {
struct Table {
    std::vector<u64> lo, hi;
    bool has_hi;
    explicit Table(u32 log_N) : lo(glp_table_lo_len(log_N)), hi(glp_table_hi_len(log_N) ? glp_table_hi_len(log_N) : 1) {
        glp_fill_table(log_N, 0, lo.data(), hi.data());
        has_hi = glp_table_hi_len(log_N) != 0;
    }
    const u64* hip() const { return has_hi ? hi.data() : nullptr; }
};
std::vector<u64> coset_ks(u32 R) {
    std::vector<u64> ks(R);
    u64 t = 1;
    for (u32 j = 0; j < R; j++) { ks[j] = t; t = gl_mul(t, 7); }
    return ks;
}
u32 n_constraints(u32 R, u32 flags) {
    return 2 + 3 * (R / GLP_PLONK_CHUNK) + ((flags & GLP_CIRCUIT_POSEIDON_GATE) ? GLP_POS_GATE_CONSTRAINTS : 0) +
           ((flags & GLP_CIRCUIT_SHA_GATES) ? GLP_SHA_GATE_CONSTRAINTS : 0);
}
void alpha_powers(const u64* alpha, u32 n_con, u64* out) {
    for (int t = 0; t < GLP_PLONK_NCHAL; t++) { u64 x = 1; for (u32 k = 0; k < n_con; k++) { out[(size_t)t * n_con + k] = x; x = gl_mul(x, alpha[t]); } }
}
// what every instance of a K7 launch shares (quotient_evals in plonk.hip)
struct K7Shared {
    Table tab;
    std::vector<u64> ks, inv;
    GlpQuotientArgs qa;
    K7Shared(const u64* consts, const u64* sigmas, u32 log_n, u32 rb, u32 W, u32 R, u32 flags, const u64* pos_consts) : tab(log_n + rb), ks(coset_ks(R)) {
        const u32 log_N = log_n + rb;
        const u64 n = 1ull << log_n, N = 1ull << log_N;
        inv.resize(N);
        const u64* lo = tab.lo.data(); const u64* hi = tab.hip(); u64* ip = inv.data();
        glp_emu_launch((unsigned)((N / 4 + 255) / 256), 256, 0, [&] { glp_inv_xm1_kernel<0>(ip, log_N, 7, lo, hi); });
        memset(&qa, 0, sizeof(qa));
        qa.consts = consts; qa.sigmas = sigmas; qa.ks = ks.data();
        qa.q_ext = (flags & GLP_CIRCUIT_EXT_GATE) ? consts + (u64)(glp_plonk_n_const(flags) - 1) * N : nullptr;
        qa.log_n = log_n; qa.rate_bits = rb; qa.W = W; qa.R = R; qa.n_con = n_constraints(R, flags);
        qa.pos_consts = pos_consts; qa.w_lo = lo; qa.w_hi = hi; qa.shift = 7;
        const u64 sn = gl_pow(7, n), wr = gl_root_of_unity(rb);
        for (u32 k = 0; k < (1u << rb); k++) qa.zh_inv[k] = gl_inv(gl_sub(gl_mul(sn, gl_pow(wr, k)), 1));
        qa.n_inv = gl_inv(n % GL_P); qa.inv_xm1 = inv.data();
    }
};
}  // namespace

// ---- the wire gather ---------------------------------------------------------------------------------------------------------------------
extern "C" int emu_gather_wires_batch(const u64* const* wires, u64 words, u32 B, u32 bpi, u64* dst) {
    std::vector<GlpPlonkInst> insts(B);
    memset(insts.data(), 0, B * sizeof(GlpPlonkInst));
    for (u32 i = 0; i < B; i++) insts[i].wire_vals = wires[i];
    const GlpPlonkInst* ip = insts.data();
    glp_emu_launch(bpi * B, 256, 0, [&] { glp_plonk_gather_wires_batch_kernel<0>(ip, words, bpi, dst); });
    return 0;
}

// ---- K6a -----------------------------------------------------------------------------------------------------------------------------------
// wires: B host pointers ([R][n] each); betas, gammas: [B][NCHAL]; instance i writes qv_out + i * qv_stride ([NCHAL][M][n]) and
// rr_out + i * rr_stride ([NCHAL][n])
extern "C" int emu_perm_quotients_batch(const u64* const* wires, const u64* sigmas, u32 log_n, u32 R, u32 B, const u64* betas, const u64* gammas,
                                        u64* qv_out, u64 qv_stride, u64* rr_out, u64 rr_stride) {
    const u64 n = 1ull << log_n;
    Table tab(log_n);
    const std::vector<u64> ks = coset_ks(R);
    std::vector<GlpPlonkInst> insts(B);
    memset(insts.data(), 0, B * sizeof(GlpPlonkInst));
    for (u32 i = 0; i < B; i++) {
        insts[i].wire_vals = wires[i]; insts[i].qv = qv_out + (u64)i * qv_stride; insts[i].rr = rr_out + (u64)i * rr_stride;
        for (int t = 0; t < GLP_PLONK_NCHAL; t++) { insts[i].beta[t] = betas[i * GLP_PLONK_NCHAL + t]; insts[i].gamma[t] = gammas[i * GLP_PLONK_NCHAL + t]; }
    }
    GlpPermArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.sigmas = sigmas; pa.ks = ks.data(); pa.log_n = log_n; pa.W = R; pa.w_lo = tab.lo.data(); pa.w_hi = tab.hip();
    const u32 bpi = (u32)((n + 255) / 256);
    const GlpPlonkInst* ip = insts.data();
    glp_emu_launch(bpi * B, 256, 0, [&] { glp_perm_quotients_batch_kernel<0>(pa, ip, bpi); });
    return 0;
}
extern "C" int emu_perm_quotients_single(const u64* wires, const u64* sigmas, u32 log_n, u32 R, const u64* beta, const u64* gamma, u64* qv, u64* rr) {
    const u64 n = 1ull << log_n;
    Table tab(log_n);
    const std::vector<u64> ks = coset_ks(R);
    GlpPermArgs pa;
    pa.wires = wires; pa.sigmas = sigmas; pa.ks = ks.data(); pa.log_n = log_n; pa.W = R;
    for (int t = 0; t < GLP_PLONK_NCHAL; t++) { pa.beta[t] = beta[t]; pa.gamma[t] = gamma[t]; }
    pa.w_lo = tab.lo.data(); pa.w_hi = tab.hip(); pa.qv = qv; pa.rr = rr;
    glp_emu_launch((unsigned)((n + 255) / 256), 256, 0, [&] { glp_perm_quotients_kernel<0>(pa); });
    return 0;
}

// ---- K6b: the three scan kernels, unchanged, over `rows` challenges (rows = NCHAL: one proof; rows = B * NCHAL: the batch) ----------------
// rr [rows][n], qv [rows][M][n] -> zs [rows * M][n].  2-D grids: blockIdx.y by an outer loop.
extern "C" int emu_scan(const u64* rr, const u64* qv, u32 log_n, u32 M, u32 rows, u64* zs) {
    const u64 n = 1ull << log_n;
    const u32 nb = (u32)((n + GLP_SCAN_BLOCK - 1) / GLP_SCAN_BLOCK);
    std::vector<u64> bprod((size_t)rows * nb);
    u64* bp = bprod.data();
    for (u32 y = 0; y < rows; y++)
        glp_emu_launch(nb, 256, 0, [&] { blockIdx.y = y; gridDim.y = rows; glp_scan_reduce_kernel<0>(rr, n, bp); });
    glp_emu_launch(rows, GLP_SCAN_TOP, 0, [&] { blockIdx.y = 0; gridDim.y = 1; glp_scan_blocks_kernel<0>(bp, nb); });
    for (u32 y = 0; y < rows; y++)
        glp_emu_launch(nb, 256, 0, [&] { blockIdx.y = y; gridDim.y = rows; glp_scan_apply_kernel<0>(rr, qv, n, M, bp, zs); });
    return 0;
}

// ---- K7 (+ K7s with GLP_CIRCUIT_SHA_GATES) -------------------------------------------------------------------------------------------------
// consts [n_const][N], sigmas [R][N] shared; wires / zs / pi: B host pointers ([W][N], [NCHAL*M][N], [N]; pi may be NULL = no public inputs);
// betas, gammas, alphas: [B][NCHAL]; small_mds: the <true, true> instantiation for Poseidon rows, else the generic one.  Instance i writes
// out + i * out_stride ([NCHAL][N]).
extern "C" int emu_quotient_batch(const u64* consts, const u64* sigmas, const u64* const* wires, const u64* const* zs, const u64* const* pi, u32 log_n,
                                  u32 rb, u32 W, u32 R, u32 flags, int small_mds, const u64* pos_consts, const u64* betas, const u64* gammas,
                                  const u64* alphas, u32 B, u64* out, u64 out_stride) {
    K7Shared sh(consts, sigmas, log_n, rb, W, R, flags, pos_consts);
    const u32 n_con = sh.qa.n_con;
    const u64 N = 1ull << (log_n + rb);
    std::vector<u64> apow((size_t)B * GLP_PLONK_NCHAL * n_con);
    std::vector<GlpPlonkInst> insts(B);
    memset(insts.data(), 0, B * sizeof(GlpPlonkInst));
    for (u32 i = 0; i < B; i++) {
        alpha_powers(alphas + i * GLP_PLONK_NCHAL, n_con, &apow[(size_t)i * GLP_PLONK_NCHAL * n_con]);
        insts[i].wires_lde = wires[i]; insts[i].zs_lde = zs[i]; insts[i].pi_lde = pi ? pi[i] : nullptr;
        insts[i].alpha_pow = &apow[(size_t)i * GLP_PLONK_NCHAL * n_con]; insts[i].out = out + (u64)i * out_stride;
        for (int t = 0; t < GLP_PLONK_NCHAL; t++) { insts[i].beta[t] = betas[i * GLP_PLONK_NCHAL + t]; insts[i].gamma[t] = gammas[i * GLP_PLONK_NCHAL + t]; }
    }
    const u32 bpi = (u32)((N + 255) / 256);
    const GlpPlonkInst* ip = insts.data();
    const GlpQuotientArgs& qa = sh.qa;
    if ((flags & GLP_CIRCUIT_POSEIDON_GATE) && small_mds) glp_emu_launch(bpi * B, 256, 0, [&] { glp_quotient_batch_kernel<true, true>(qa, ip, bpi); });
    else if (flags & GLP_CIRCUIT_POSEIDON_GATE) glp_emu_launch(bpi * B, 256, 0, [&] { glp_quotient_batch_kernel<true>(qa, ip, bpi); });
    else glp_emu_launch(bpi * B, 256, 0, [&] { glp_quotient_batch_kernel<false>(qa, ip, bpi); });
    if (flags & GLP_CIRCUIT_SHA_GATES)
        glp_emu_launch(bpi * B, 256, 0, [&] { glp_quotient_sha_batch_kernel<0>(qa, ip, bpi, n_con - GLP_SHA_GATE_CONSTRAINTS); });
    return 0;
}
extern "C" int emu_quotient_single(const u64* consts, const u64* sigmas, const u64* wires, const u64* zs, const u64* pi, u32 log_n, u32 rb, u32 W, u32 R,
                                   u32 flags, int small_mds, const u64* pos_consts, const u64* beta, const u64* gamma, const u64* alpha, u64* out) {
    K7Shared sh(consts, sigmas, log_n, rb, W, R, flags, pos_consts);
    GlpQuotientArgs qa = sh.qa;
    const u32 n_con = qa.n_con;
    const u64 N = 1ull << (log_n + rb);
    std::vector<u64> apow((size_t)GLP_PLONK_NCHAL * n_con);
    alpha_powers(alpha, n_con, apow.data());
    qa.wires = wires; qa.zs = zs; qa.pi = pi; qa.alpha_pow = apow.data(); qa.out = out;
    for (int t = 0; t < GLP_PLONK_NCHAL; t++) { qa.beta[t] = beta[t]; qa.gamma[t] = gamma[t]; }
    const unsigned g = (unsigned)((N + 255) / 256);
    if ((flags & GLP_CIRCUIT_POSEIDON_GATE) && small_mds) glp_emu_launch(g, 256, 0, [&] { glp_quotient_kernel<true, true>(qa); });
    else if (flags & GLP_CIRCUIT_POSEIDON_GATE) glp_emu_launch(g, 256, 0, [&] { glp_quotient_kernel<true>(qa); });
    else glp_emu_launch(g, 256, 0, [&] { glp_quotient_kernel<false>(qa); });
    if (flags & GLP_CIRCUIT_SHA_GATES) glp_emu_launch(g, 256, 0, [&] { glp_quotient_sha_kernel<0>(qa, n_con - GLP_SHA_GATE_CONSTRAINTS); });
    return 0;
}

#ifdef GLP_EMU_PLONK_BATCH_MAIN
#include <cstdio>
static u64 next_word(u64& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    u64 z = st ^ (st >> 29);
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 32;
    return z % GL_P;
}
static std::vector<u64> rand_words(u64& st, size_t n) { std::vector<u64> v(n); for (u64& w : v) w = next_word(st); return v; }

int main() {
    u64 st = 2027;
    int bad = 0;
    const u64 FILL = 0x5e5e5e5e5e5e5e5eull;
    auto check = [&](bool ok, const char* what, u32 x, u32 y) { if (!ok) { printf("DIFF %s (%u, %u)\n", what, x, y); bad++; } };
    auto all_fill = [&](const u64* p, size_t k) { for (size_t j = 0; j < k; j++) if (p[j] != FILL) return false; return true; };

    // the wire gather: B = 3, a length that is no multiple of the block, fewer blocks than needed for one pass
    {
        const u32 B = 3; const u64 words = 1000;
        std::vector<std::vector<u64>> w; std::vector<const u64*> ptrs;
        for (u32 i = 0; i < B; i++) w.push_back(rand_words(st, words));
        for (auto& v : w) ptrs.push_back(v.data());
        std::vector<u64> dst(B * words + 5, FILL);
        emu_gather_wires_batch(ptrs.data(), words, B, 2, dst.data());
        for (u32 i = 0; i < B; i++) check(!memcmp(&dst[i * words], w[i].data(), words * 8), "gather", i, 0);
        check(all_fill(&dst[B * words], 5), "gather tail", 0, 0);
    }
    // K6a + the scan over B * NCHAL rows: (log_n, R); 2^11 = two scan blocks
    const u32 k6[][2] = {{3, 8}, {5, 136}, {11, 16}};
    for (auto& s : k6) {
        const u32 log_n = s[0], R = s[1], M = R / 8, B = 3;
        const u64 n = 1ull << log_n, qvw = (u64)GLP_PLONK_NCHAL * M * n, rrw = (u64)GLP_PLONK_NCHAL * n;
        const std::vector<u64> sig = rand_words(st, R * n), be = rand_words(st, B * 2), ga = rand_words(st, B * 2);
        std::vector<std::vector<u64>> w; std::vector<const u64*> ptrs;
        for (u32 i = 0; i < B; i++) w.push_back(rand_words(st, R * n));
        for (auto& v : w) ptrs.push_back(v.data());
        std::vector<u64> qv(B * (qvw + 3), FILL), rr(B * (rrw + 3), FILL);
        emu_perm_quotients_batch(ptrs.data(), sig.data(), log_n, R, B, be.data(), ga.data(), qv.data(), qvw + 3, rr.data(), rrw + 3);
        std::vector<u64> qd(B * qvw), rd(B * rrw), zs(B * qvw);
        for (u32 i = 0; i < B; i++) {
            std::vector<u64> q1(qvw), r1(rrw);
            emu_perm_quotients_single(w[i].data(), sig.data(), log_n, R, &be[2 * i], &ga[2 * i], q1.data(), r1.data());
            check(!memcmp(q1.data(), &qv[i * (qvw + 3)], qvw * 8), "K6a qv", log_n, i);
            check(!memcmp(r1.data(), &rr[i * (rrw + 3)], rrw * 8), "K6a rr", log_n, i);
            check(all_fill(&qv[i * (qvw + 3) + qvw], 3) && all_fill(&rr[i * (rrw + 3) + rrw], 3), "K6a gaps", log_n, i);
            memcpy(&qd[i * qvw], q1.data(), qvw * 8); memcpy(&rd[i * rrw], r1.data(), rrw * 8);
        }
        emu_scan(rd.data(), qd.data(), log_n, M, B * GLP_PLONK_NCHAL, zs.data());
        for (u32 i = 0; i < B; i++) {
            std::vector<u64> z1(qvw);
            emu_scan(&rd[i * rrw], &qd[i * qvw], log_n, M, GLP_PLONK_NCHAL, z1.data());
            check(!memcmp(z1.data(), &zs[i * qvw], qvw * 8), "scan", log_n, i);
        }
    }
    // K7 / K7s: every flag combination the driver selects between, both MDS kinds, with and without public inputs, at 2^3 rows
    std::vector<u64> pos_small = rand_words(st, 384), pos_big = rand_words(st, 384);
    for (int i = 0; i < 12; i++) { pos_small[360 + i] = 1 + (u64)i; pos_small[372 + i] = 2 + (u64)i; }
    const u32 P = GLP_CIRCUIT_POSEIDON_GATE, S = GLP_CIRCUIT_SHA_GATES, E = GLP_CIRCUIT_EXT_GATE;
    const u32 k7[][4] = {{3, 8, 8, 0}, {3, 160, 136, 0}, {3, 136, 80, P}, {3, 160, 16, S}, {3, 144, 80, S | P}, {3, 144, 80, E | P | S}, {7, 16, 16, 0}};
    for (auto& s : k7)
        for (int small = 0; small <= ((s[3] & P) ? 1 : 0); small++)
            for (int with_pi = 0; with_pi <= 1; with_pi++) {
                const u32 log_n = s[0], W = s[1], R = s[2], flags = s[3], rb = 3, M = R / 8, B = with_pi ? 3 : 1;
                const u64 N = 1ull << (log_n + rb), ow = (u64)GLP_PLONK_NCHAL * N;
                const std::vector<u64> co = rand_words(st, glp_plonk_n_const(flags) * N), sig = rand_words(st, R * N);
                const std::vector<u64> be = rand_words(st, B * 2), ga = rand_words(st, B * 2), al = rand_words(st, B * 2);
                std::vector<std::vector<u64>> w, z, p; std::vector<const u64*> wp, zp, pp;
                for (u32 i = 0; i < B; i++) { w.push_back(rand_words(st, W * N)); z.push_back(rand_words(st, 2 * M * N)); p.push_back(rand_words(st, N)); }
                for (u32 i = 0; i < B; i++) { wp.push_back(w[i].data()); zp.push_back(z[i].data()); pp.push_back(p[i].data()); }
                const u64* pc = small ? pos_small.data() : pos_big.data();
                std::vector<u64> out(B * (ow + 3), FILL);
                emu_quotient_batch(co.data(), sig.data(), wp.data(), zp.data(), with_pi ? pp.data() : nullptr, log_n, rb, W, R, flags, small, pc, be.data(),
                                   ga.data(), al.data(), B, out.data(), ow + 3);
                for (u32 i = 0; i < B; i++) {
                    std::vector<u64> o1(ow);
                    emu_quotient_single(co.data(), sig.data(), wp[i], zp[i], with_pi ? pp[i] : nullptr, log_n, rb, W, R, flags, small, pc, &be[2 * i], &ga[2 * i],
                                        &al[2 * i], o1.data());
                    check(!memcmp(o1.data(), &out[i * (ow + 3)], ow * 8), "K7", flags * 4 + small * 2 + with_pi, i);
                    check(all_fill(&out[i * (ow + 3) + ow], 3), "K7 gap", flags, i);
                }
            }
    if (bad) { printf("%d differences\n", bad); return 1; }
    printf("emu_plonk_batch: batched == single on every shape\n");
    return 0;
}
#endif
