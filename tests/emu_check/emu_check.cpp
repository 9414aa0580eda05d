// tests/emu_check/emu_check.cpp — TEST INFRASTRUCTURE.  The kernels of glp_plonk_check_witness[_batch] (csrc/check_kernels.cuh) on the CPU,
// unchanged, launched through ../emu/hip_emu.h with the grids the driver uses (256 lanes, ceil(n / 256) x B workgroups, the instance in
// blockIdx.y; the decode kernels over the routed cells), and the host decode function of csrc/check_plan.h.  Every work-item of a check
// kernel is a real thread (the kernels reduce through LDS between barriers); workgroups run one after the other, so the workgroup that draws
// the last ticket — the one that builds the list — is the last one launched.  Never part of the product.
// With -DGLP_EMU_CHECK_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that runs all five
// kernels on small shapes and compares counts and lists with a serial recount.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/check_kernels.cuh"
#include "../../0-kno-blobstreamx_amd/csrc/ntt_plan.h"

namespace {
template <typename F>
void launch_2d(unsigned gx, unsigned gy, F body) {
    gridDim.y = gy;
    for (unsigned y = 0; y < gy; y++) glp_emu_launch(gx, GLP_CHECK_BLOCK, 0, [&] { blockIdx.y = y; body(); });
}
struct SigmaHost {
    std::vector<u64> kn, kinv, wlo, whi, ilo, ihi;
    GlpSigmaTables T;
    SigmaHost(u32 log_n, u32 R) : kn(R), kinv(R), wlo(glp_table_lo_len((int)log_n)), whi(glp_table_hi_len((int)log_n) + 1), ilo(wlo.size()), ihi(whi.size()) {
        glp_sigma_fill_tables(log_n, R, kn.data(), kinv.data());
        glp_fill_table((int)log_n, 0, wlo.data(), whi.data());
        glp_fill_table((int)log_n, 1, ilo.data(), ihi.data());
        T.kn = kn.data(); T.kinv = kinv.data(); T.winv_lo = ilo.data(); T.winv_hi = log_n > GLP_CHECK_TW_SPLIT ? ihi.data() : nullptr;
        T.log_n = log_n; T.R = R;
    }
};
}  // namespace

// the host decode function on count values: out[k] = the cell index, or GLP_SIGMA_BAD
extern "C" int emu_sigma_decode_host(const u64* vals, u64 count, u32 log_n, u32 R, u32* out) {
    SigmaHost S(log_n, R);
    for (u64 k = 0; k < count; k++) out[k] = glp_sigma_decode(vals[k], S.T);
    return 0;
}

// the two decode kernels with the driver's grids: idx [R][n], status[2] (both all ones = the key decodes and is a permutation)
extern "C" int emu_sigma_decode(const u64* sigma_vals, u32 log_n, u32 R, u32* idx, unsigned long long* status) {
    SigmaHost S(log_n, R);
    const u64 n = 1ull << log_n, cells = (u64)R * n;
    std::vector<u64> ks(R);
    { u64 t = 1; for (u32 j = 0; j < R; j++) { ks[j] = t; t = gl_mul(t, 7); } }
    std::vector<u32> hits(cells, 0);
    status[0] = status[1] = ~0ull;
    GlpSigmaDecodeArgs da;
    da.sigma_vals = sigma_vals; da.ks = ks.data(); da.w_lo = S.wlo.data(); da.w_hi = log_n > GLP_CHECK_TW_SPLIT ? S.whi.data() : nullptr;
    da.T = S.T; da.idx = idx; da.hits = hits.data(); da.status = status;
    const unsigned blocks = (unsigned)((cells + 255) / 256);
    glp_emu_launch_seq(blocks, 256, [&] { glp_sigma_decode_kernel<0>(da); });
    glp_emu_launch_seq(blocks, 256, [&] { glp_sigma_bijective_kernel<0>(hits.data(), cells, status); });
    return 0;
}

// the four check kernels as check.hip launches them.  consts [n_const][n] trace values, sigma_idx [R][n], wires: B pointers, pubs [B][n_public];
// acc_out [B][5] words (n_gate_bad, n_copy_bad, first_key, n_gate_rows | n_copy_rows << 32, ticket), lists_out [B][max_list]
extern "C" int emu_check(const u64* consts, const u32* sigma_idx, const u64* pos_consts, int small_mds, const u64* const* wires, const u64* pubs, u32 B,
                         u32 log_n, u32 W, u32 R, u32 n_public, u32 flags, u32 max_list, u64* acc_out, glp_check_violation* lists_out) {
    const u64 n = 1ull << log_n;
    const u32 n_const = (u32)glp_plonk_n_const(flags), M = R / GLP_PLONK_CHUNK;
    std::vector<GlpCheckInst> inst(B);
    std::vector<GlpCheckAcc> acc(B);
    for (u32 b = 0; b < B; b++) {
        inst[b].wires = wires[b]; inst[b].pub = n_public ? pubs + (size_t)b * n_public : nullptr;
        memset(&acc[b], 0, sizeof(GlpCheckAcc));
        acc[b].first_key = GLP_CHECK_KEY_NONE;
    }
    std::vector<unsigned char> rows((size_t)B * n * GLP_CHECK_ROW_BYTES + 8);          // exact size (+ the alignment slack): ASan sees any overrun
    unsigned char* rows_al = rows.data() + ((8 - ((uintptr_t)rows.data() & 7)) & 7);
    GlpCheckArgs a;
    memset(&a, 0, sizeof(a));
    a.consts = consts; a.sigma_idx = sigma_idx; a.pos_consts = pos_consts; a.insts = inst.data(); a.acc = acc.data(); a.rows = rows_al;
    a.lists = lists_out; a.log_n = log_n; a.W = W; a.R = R; a.n_public = n_public;
    a.q_ext_col = (flags & GLP_CIRCUIT_EXT_GATE) ? n_const - 1 : GLP_CHECK_NONE;
    a.first_pos = 2 + 3 * M;
    a.first_sha = 2 + 3 * M + ((flags & GLP_CIRCUIT_POSEIDON_GATE) ? GLP_POS_GATE_CONSTRAINTS : 0);
    a.max_list = max_list;
    const unsigned gx = (unsigned)((n + GLP_CHECK_BLOCK - 1) / GLP_CHECK_BLOCK);
    launch_2d(gx, B, [&] { glp_check_base_kernel<0>(a); });
    if (flags & GLP_CIRCUIT_POSEIDON_GATE) {
        if (small_mds) launch_2d(gx, B, [&] { glp_check_poseidon_kernel<true>(a); });
        else launch_2d(gx, B, [&] { glp_check_poseidon_kernel<false>(a); });
    }
    if (flags & GLP_CIRCUIT_SHA_GATES) launch_2d(gx, B, [&] { glp_check_sha_kernel<0>(a); });
    launch_2d(gx, B, [&] { glp_check_copy_kernel<0>(a); });
    for (u32 b = 0; b < B; b++) {
        u64* o = acc_out + (size_t)b * 5;
        o[0] = acc[b].n_gate_bad; o[1] = acc[b].n_copy_bad; o[2] = acc[b].first_key;
        o[3] = (u64)acc[b].n_gate_rows | ((u64)acc[b].n_copy_rows << 32); o[4] = acc[b].ticket;
    }
    return 0;
}

#ifdef GLP_EMU_CHECK_MAIN
#include <cstdio>
static u64 next_word(u64& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    u64 z = st ^ (st >> 29);
    z *= 0xBF58476D1CE4E5B9ull;
    return (z ^ (z >> 32)) % GL_P;
}
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main() {
    u64 st = 20261020;
    // ---- decode: a random permutation of the routed cells of a 2^4 x 8 and (beyond the 4096-entry first-level table) a 2^13 x 8 domain ----
    for (u32 log_n : {4u, 13u}) {
        const u32 R = 8;
        const u64 n = 1ull << log_n, cells = (u64)R * n;
        std::vector<u32> perm(cells);
        for (u64 p = 0; p < cells; p++) perm[p] = (u32)p;
        for (u64 p = cells - 1; p > 0; p--) {
            if (next_word(st) & 1) continue;                      // half the cells stay fixed points: the fast path
            const u64 q = next_word(st) % (p + 1);
            std::swap(perm[p], perm[q]);
        }
        const u64 w = gl_root_of_unity(log_n);
        std::vector<u64> wp(n), ks(R), sig(cells);
        wp[0] = 1; for (u64 i = 1; i < n; i++) wp[i] = gl_mul(wp[i - 1], w);
        ks[0] = 1; for (u32 j = 1; j < R; j++) ks[j] = gl_mul(ks[j - 1], 7);
        for (u64 p = 0; p < cells; p++) sig[p] = gl_mul(ks[perm[p] >> log_n], wp[perm[p] & (n - 1)]);
        std::vector<u32> idx(cells), hidx(cells);
        unsigned long long status[2];
        emu_sigma_decode(sig.data(), log_n, R, idx.data(), status);
        REQUIRE(status[0] == ~0ull && status[1] == ~0ull);
        emu_sigma_decode_host(sig.data(), cells, log_n, R, hidx.data());
        for (u64 p = 0; p < cells; p++) REQUIRE(idx[p] == perm[p] && hidx[p] == perm[p]);
        // a value on a coset that is not routed, a zero, and two cells sent to one target
        std::vector<u64> bad = sig;
        bad[5] = gl_mul(gl_pow(7, R), wp[3]);
        bad[n + 1] = 0;
        emu_sigma_decode(bad.data(), log_n, R, idx.data(), status);
        REQUIRE(status[0] == 5);
        for (u64 p = 0; p < cells; p++) REQUIRE(idx[p] < cells);
        bad = sig;
        bad[7] = sig[9];
        emu_sigma_decode(bad.data(), log_n, R, idx.data(), status);
        REQUIRE(status[0] == ~0ull && status[1] != ~0ull);
    }
    // ---- the four check kernels, B = 2, on a circuit with every row kind and RANDOM wires (nearly every constraint fails): counts and the
    // lists against a serial recount with the same gate bodies; then a circuit without constraints, which every witness satisfies ----
    const u32 log_n = 9, W = 144, R = 24, B = 2, NP = 3, flags = GLP_CIRCUIT_POSEIDON_GATE | GLP_CIRCUIT_SHA_GATES | GLP_CIRCUIT_EXT_GATE;
    const u64 n = 1ull << log_n;
    const u32 n_const = (u32)glp_plonk_n_const(flags), M = R / 8, max_list = 37;
    std::vector<u64> consts((size_t)n_const * n, 0), pc(384);
    for (auto& v : pc) v = next_word(st);
    for (int k = 360; k < 384; k++) pc[k] &= 0xFFFFF;                                    // a small-integer MDS
    for (u64 i = 0; i < n; i++) {
        const u64 kind = i % 7;                                                        // 0..2 arithmetic, 3 Poseidon, 4 SHA (kind by row), 5 extension, 6 nothing
        if (kind < 3) consts[i] = 1;
        for (int k = 1; k < 4; k++) consts[k * n + i] = next_word(st);
        if (i < NP) consts[4 * n + i] = 1;
        if (kind == 3) consts[5 * n + i] = 1;
        if (kind == 4) consts[(6 + (i / 7) % 4) * n + i] = 1;
        if (kind == 5) consts[10 * n + i] = 1;
    }
    std::vector<u32> sidx((size_t)R * n);
    for (u64 p = 0; p < (u64)R * n; p++) sidx[p] = (u32)p;
    for (u64 p = 0; p + 1 < (u64)R * n; p += 5) std::swap(sidx[p], sidx[p + 1]);
    std::vector<std::vector<u64>> wm(B, std::vector<u64>((size_t)W * n));
    for (auto& m : wm) for (auto& v : m) v = next_word(st) & 3;                        // few distinct values: some copies and some gates hold
    std::vector<u64> pubs((size_t)B * NP);
    for (auto& v : pubs) v = next_word(st) & 3;
    const u64* wp2[B] = {wm[0].data(), wm[1].data()};
    for (int small = 0; small < 2; small++) {
        std::vector<u64> acc((size_t)B * 5);
        std::vector<glp_check_violation> lists((size_t)B * max_list);
        emu_check(consts.data(), sidx.data(), pc.data(), small, wp2, pubs.data(), B, log_n, W, R, NP, flags, max_list, acc.data(), lists.data());
        for (u32 b = 0; b < B; b++) {
            // serial recount of the copy constraints and of the base gate slots (the Poseidon / SHA blocks: the counts must at least cover them)
            u64 copy_bad = 0, copy_rows = 0, base_bad = 0;
            std::vector<int> row_has_copy(n, 0), row_base(n, 0);
            const u64* w = wm[b].data();
            for (u64 i = 0; i < n; i++) {
                for (u32 j = 0; j < R; j++) if (w[(u64)j * n + i] != w[sidx[(u64)j * n + i]]) { copy_bad++; row_has_copy[i] = 1; }
                copy_rows += row_has_copy[i];
                const u64 q = consts[i], c0 = consts[n + i], c1 = consts[2 * n + i], c2 = consts[3 * n + i], qx = consts[10 * n + i];
                if (gl_sub(gl_mul(consts[4 * n + i], w[i]), i < NP ? pubs[(size_t)b * NP + i] : 0)) { base_bad++; row_base[i] = 1; }
                for (u32 c = 0; c < M; c++) {
                    u64 x[8], e0, e1;
                    for (int k = 0; k < 8; k++) x[k] = w[((u64)c * 8 + k) * n + i];
                    glp_ext_gate<GlpGateBase>(x, e0, e1);
                    const u64 g0 = gl_add(gl_mul(q, glp_arith_gate<GlpGateBase>(c0, c1, c2, x[0], x[1], x[2], x[3])), gl_mul(qx, e0));
                    const u64 g1 = gl_add(gl_mul(q, glp_arith_gate<GlpGateBase>(c0, c1, c2, x[4], x[5], x[6], x[7])), gl_mul(qx, e1));
                    if (g0) { base_bad++; row_base[i] = 1; }
                    if (g1) { base_bad++; row_base[i] = 1; }
                }
            }
            const u64* o = acc.data() + (size_t)b * 5;
            REQUIRE(o[1] == copy_bad && (o[3] >> 32) == copy_rows && o[0] >= base_bad && o[4] == (n + 255) / 256);
            const u64 entries = (o[3] & 0xFFFFFFFFu) + (o[3] >> 32);
            REQUIRE(entries >= max_list);
            const glp_check_violation* L = lists.data() + (size_t)b * max_list;
            REQUIRE(glp_check_key(L[0].row, L[0].kind, L[0].index) == o[2]);
            for (u32 k = 0; k < max_list; k++) {
                if (k) REQUIRE(L[k - 1].row < L[k].row || (L[k - 1].row == L[k].row && L[k - 1].kind < L[k].kind));
                if (L[k].kind == GLP_CHECK_COPY) {
                    REQUIRE(row_has_copy[L[k].row] && L[k].value == w[(u64)L[k].index * n + L[k].row] &&
                            L[k].peer_value == w[((u64)L[k].peer_wire << log_n) + L[k].peer_row] && L[k].value != L[k].peer_value);
                } else if (L[k].index < 2 + 3 * M) REQUIRE(row_base[L[k].row]);
            }
        }
    }
    {
        std::vector<u64> zero((size_t)n_const * n, 0), acc((size_t)B * 5);
        std::vector<u32> ident((size_t)R * n);
        for (u64 p = 0; p < (u64)R * n; p++) ident[p] = (u32)p;
        std::vector<glp_check_violation> lists((size_t)B * max_list);
        emu_check(zero.data(), ident.data(), pc.data(), 1, wp2, nullptr, B, log_n, W, R, 0, flags, max_list, acc.data(), lists.data());
        for (u32 b = 0; b < B; b++) REQUIRE(acc[b * 5] == 0 && acc[b * 5 + 1] == 0 && acc[b * 5 + 2] == GLP_CHECK_KEY_NONE && acc[b * 5 + 3] == 0);
    }
    std::printf("emu_check_san ok\n");
    return 0;
}
#endif
