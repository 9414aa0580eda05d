// tests/emu_fri_batch/emu_fri_batch.cpp — TEST INFRASTRUCTURE.  The kernels of glp_fri_prove_batch (csrc/fri_batch_kernels.cuh) on the CPU,
// unchanged, launched through ../emu/hip_emu.h with the grids of the product's own plan (csrc/fri_batch_plan.h), beside the single-instance
// bodies of csrc/fri_kernels.cuh and csrc/hash_kernels.cuh they must equal word for word.  Never part of the product.
// With -DGLP_EMU_FRI_BATCH_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that compares
// batched against single on small shapes.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/fri_batch_kernels.cuh"
#include "../../0-kno-blobstreamx_amd/csrc/fri_batch_plan.h"
#include "../../0-kno-blobstreamx_amd/csrc/ntt_plan.h"
#include "../../0-kno-blobstreamx_amd/csrc/poseidon_precomp.h"

namespace {
struct Table {
    std::vector<u64> lo, hi;
    Table(u32 log_N, int inv) : lo(glp_table_lo_len(log_N)), hi(glp_table_hi_len(log_N) ? glp_table_hi_len(log_N) : 1) {
        glp_fill_table(log_N, inv, lo.data(), hi.data());
        has_hi = glp_table_hi_len(log_N) != 0;
    }
    bool has_hi;
    const u64* hip() const { return has_hi ? hi.data() : nullptr; }
};

void power_tables(gl_ext2 z, u64 n, u64* lo, u64* hi) {     // as build_zpowers (fri.hip)
    const u64 nhi = (n + 255) / 256;
    gl_ext2 t{1, 0};
    for (int j = 0; j < 256; j++) { lo[2 * j] = t.a; lo[2 * j + 1] = t.b; t = gl_ext_mul(t, z); }
    const gl_ext2 z256 = t;
    t = gl_ext2{1, 0};
    for (u64 j = 0; j < nhi; j++) { hi[2 * j] = t.a; hi[2 * j + 1] = t.b; t = gl_ext_mul(t, z256); }
}

GlpPoseidonConsts consts_of(const u64* consts384, int small, std::vector<u32>& cf, std::vector<u64>& cs) {
    GlpPoseidonConsts k{consts384, consts384 + 360, consts384 + 372, nullptr, nullptr};
    if (small == 2 && glp_poseidon_group_tables(consts384, cf, cs)) { k.pg_coef = cf.data(); k.pg_cst = cs.data(); }
    return k;
}

// the descriptor table of one emulated call: shape, pointers, and room for the power tables and the combine blocks
struct Desc {
    glp_fri_batch_plan pl;
    std::vector<u64> w;
    int make(u32 log_n, u32 rate_bits, u32 n_points, const u32* n_polys, const u32* masks, u32 n_batches, u32 B) {
        glp_fri_config cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.log_n = log_n; cfg.rate_bits = rate_bits; cfg.cap_height = 0; cfg.arity_bits = 1; cfg.final_poly_bits = log_n < 5 ? log_n : 5;
        cfg.num_queries = 1; cfg.pow_bits = 0; cfg.shift = 7; cfg.n_points = n_points;
        for (u32 p = 0; p < 4; p++) cfg.point_mult[p] = 1;
        if (glp_fri_batch_plan_make(&cfg, n_polys, masks, n_batches, B, pl, nullptr)) return -1;
        w.assign(pl.desc_words, 0);
        for (u32 b = 0; b < n_batches; b++) { w[pl.off_shape + 2 * b] = n_polys[b]; w[pl.off_shape + 2 * b + 1] = masks[b]; }
        return 0;
    }
};
}  // namespace

// ---- powers + openings -------------------------------------------------------------------------------------------------------------------
// coeffs: [B][n_batches] host pointers ([n_polys[b]][2^log_n] each); z: [B][n_points][2].  zp_out: [B][n_points][n][2]; part_out:
// [B][blocks per instance][2] in (point, opened batch, polynomial, chunk) order.  Returns the blocks per instance, or -1.
extern "C" long emu_powers_eval_batch(const u64* const* coeffs, u32 log_n, const u32* n_polys, const u32* masks, u32 n_batches, u32 n_points, u32 B,
                                      const u64* z, u64* zp_out, u64* part_out) {
    Desc d;
    if (d.make(log_n, 1, n_points, n_polys, masks, n_batches, B)) return -1;
    const glp_fri_batch_plan& pl = d.pl;
    const u64 n = 1ull << log_n;
    for (u32 i = 0; i < B; i++) {
        for (u32 b = 0; b < n_batches; b++) d.w[pl.off_ptrs + 3 * ((size_t)i * n_batches + b)] = (u64)(uintptr_t)coeffs[(size_t)i * n_batches + b];
        for (u32 p = 0; p < n_points; p++) {
            u64* lo = &d.w[pl.off_pow + ((size_t)i * n_points + p) * pl.pow_stride];
            power_tables(gl_ext2{z[2 * ((size_t)i * n_points + p)], z[2 * ((size_t)i * n_points + p) + 1]}, n, lo, lo + 512);
        }
    }
    glp_emu_launch(pl.pow_blocks * n_points * B, 256, 0, [&] { glp_ext_powers_batch_kernel<0>(zp_out, n, d.w.data() + pl.off_pow, pl.pow_stride, pl.pow_blocks); });
    glp_emu_launch((unsigned)(pl.eval_blocks * B), 256, 0, [&] {
        glp_eval_ext_batch_kernel<0>(d.w.data(), pl.off_shape, pl.off_ptrs, n_batches, n_points, n, pl.n_chunks, (u32)pl.eval_blocks, zp_out, part_out);
    });
    return (long)pl.eval_blocks;
}
// the single bodies: one point, one batch.  zp_out [n][2], part_out [n_polys][n_chunks][2]
extern "C" int emu_powers_eval_single(const u64* coeffs, u32 log_n, u32 n_polys, const u64* z, u64* zp_out, u64* part_out) {
    const u64 n = 1ull << log_n, nhi = (n + 255) / 256;
    std::vector<u64> lo(512), hi(2 * nhi);
    power_tables(gl_ext2{z[0], z[1]}, n, lo.data(), hi.data());
    u64 blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    glp_emu_launch((unsigned)blocks, 256, 0, [&] { glp_ext_powers_kernel<0>(zp_out, n, lo.data(), hi.data()); });
    const u32 n_chunks = (u32)((n + GLP_EVAL_CHUNK - 1) / GLP_EVAL_CHUNK);
    glp_emu_launch(n_polys * n_chunks, 256, 0, [&] { glp_eval_ext_kernel<0>(coeffs, n, n, n_chunks, zp_out, part_out); });
    return 0;
}

// ---- combine -----------------------------------------------------------------------------------------------------------------------------
// ldes: [B][n_batches] host pointers ([n_polys[b]][2^log_N]); cmb: [B][4 * n_points + 2 * total] = Y[n_points][2], z[n_points][2], alpha^k
// in (point, opened batch, polynomial) order; out: [B][out_stride] words.  v16: the 16-byte row loads.
extern "C" int emu_combine_batch(const u64* const* ldes, u32 log_n, u32 rate_bits, const u32* n_polys, const u32* masks, u32 n_batches, u32 n_points,
                                 u32 B, const u64* cmb, u64 shift, int v16, u64* out, u64 out_stride) {
    Desc d;
    if (d.make(log_n, rate_bits, n_points, n_polys, masks, n_batches, B)) return -1;
    const glp_fri_batch_plan& pl = d.pl;
    for (u32 i = 0; i < B; i++) {
        for (u32 b = 0; b < n_batches; b++) d.w[pl.off_ptrs + 3 * ((size_t)i * n_batches + b) + 1] = (u64)(uintptr_t)ldes[(size_t)i * n_batches + b];
        memcpy(&d.w[pl.off_cmb + (size_t)i * pl.cmb_stride], cmb + (size_t)i * pl.cmb_stride, pl.cmb_stride * 8);
    }
    Table tw(pl.log_N, 0);
    GlpCombineBatchArgs a;
    a.desc = d.w.data(); a.off_shape = pl.off_shape; a.off_ptrs = pl.off_ptrs; a.off_cmb = pl.off_cmb; a.cmb_stride = pl.cmb_stride;
    a.n_batches = n_batches; a.n_points = n_points; a.log_N = pl.log_N; a.blocks_per_instance = (u32)pl.combine_blocks;
    a.out = out; a.out_stride = out_stride; a.shift = shift; a.w_lo = tw.lo.data(); a.w_hi = tw.hip();
    if (v16) glp_emu_launch((unsigned)(pl.combine_blocks * B), 256, 0, [&] { glp_fri_combine_batch_kernel<true>(a); });
    else glp_emu_launch((unsigned)(pl.combine_blocks * B), 256, 0, [&] { glp_fri_combine_batch_kernel<false>(a); });
    return 0;
}
// one instance through the existing sequence: per point one glp_fri_combine_kernel launch per opened batch into an accumulator, the later
// points' accumulators added to the first (the prover's glp_field_op add).  cmb as above for this instance; out [N][2]
extern "C" int emu_combine_single(const u64* const* ldes, u32 log_N, const u32* n_polys, const u32* masks, u32 n_batches, u32 n_points,
                                  const u64* cmb, u64 shift, u64* out) {
    const u64 N = 1ull << log_N;
    Table tw(log_N, 0);
    std::vector<u64> tmp(2 * N);
    const u64* ap = cmb + 4 * n_points;
    for (u32 p = 0; p < n_points; p++) {
        u32 nb_here = 0, last_b = 0;
        for (u32 b = 0; b < n_batches; b++) if ((masks[b] >> p) & 1u) { nb_here++; last_b = b; }
        if (!nb_here) continue;
        u64* target = p == 0 ? out : tmp.data();
        bool first = true;
        for (u32 b = 0; b < n_batches; b++) {
            if (!((masks[b] >> p) & 1u)) continue;
            GlpCombineArgs ca;
            ca.lde = ldes[b]; ca.poly_stride = N; ca.n_polys = n_polys[b]; ca.alpha_pow = ap; ca.acc = target; ca.log_N = log_N;
            ca.first = first; ca.finish = b == last_b;
            ca.Y = gl_ext2{cmb[2 * p], cmb[2 * p + 1]}; ca.z = gl_ext2{cmb[2 * (n_points + p)], cmb[2 * (n_points + p) + 1]};
            ca.shift = shift; ca.w_lo = tw.lo.data(); ca.w_hi = tw.hip();
            glp_emu_launch((unsigned)((N / 4 + 255) / 256), 256, 0, [&] { glp_fri_combine_kernel<0>(ca); });
            ap += 2 * (size_t)n_polys[b];
            first = false;
        }
        if (p > 0) for (u64 k = 0; k < 2 * N; k++) out[k] = gl_add(out[k], tmp[k]);
    }
    return 0;
}

// ---- fold layer --------------------------------------------------------------------------------------------------------------------------
extern "C" int emu_fold_layer_batch(const u64* in, u64 in_stride, u64* out, u64 out_stride, u32 log_len, u32 arity_bits, u64 shift, const u64* betas,
                                    u32 B) {
    if (B == 0) return 0;
    if (glp_fri_fold_layer_batch_check(in_stride, out_stride, log_len, arity_bits, shift, B)) return -1;
    Table tw(log_len, 1);
    GlpFoldLayerBatchArgs fa;
    fa.in = in; fa.in_stride = in_stride; fa.out = out; fa.out_stride = out_stride; fa.log_len = log_len;
    fa.blocks_per_instance = (u32)glp_fri_fold_layer_blocks(log_len, arity_bits);
    fa.betas = betas; fa.iw_lo = tw.lo.data(); fa.iw_hi = tw.hip();
    glp_fold_layer_consts(arity_bits, shift, fa);
    const unsigned g = fa.blocks_per_instance * B;
    switch (arity_bits) {
        case 1: glp_emu_launch(g, 256, 0, [&] { glp_fri_fold_layer_batch_kernel<1>(fa); }); break;
        case 2: glp_emu_launch(g, 256, 0, [&] { glp_fri_fold_layer_batch_kernel<2>(fa); }); break;
        case 3: glp_emu_launch(g, 256, 0, [&] { glp_fri_fold_layer_batch_kernel<3>(fa); }); break;
        case 4: glp_emu_launch(g, 256, 0, [&] { glp_fri_fold_layer_batch_kernel<4>(fa); }); break;
        default: glp_emu_launch(g, 256, 0, [&] { glp_fri_fold_layer_batch_kernel<5>(fa); }); break;
    }
    return 0;
}
// arity_bits successive glp_fri_fold2_kernel launches with beta, beta^2, .. and shift, shift^2, .. (the prover's loop); out [2^(log_len-a)][2]
extern "C" int emu_fold2_chain(const u64* in, u64* out, u32 log_len, u32 arity_bits, u64 shift, const u64* beta2) {
    std::vector<u64> cur(in, in + (2ull << log_len)), nxt;
    gl_ext2 beta{beta2[0], beta2[1]};
    for (u32 f = 0; f < arity_bits; f++, log_len--) {
        Table tw(log_len, 1);
        const u64 half = 1ull << (log_len - 1);
        nxt.assign(2 * half, 0);
        const u64 half_inv = gl_inv(2), cc = gl_inv(gl_mul(2, shift));
        glp_emu_launch((unsigned)((half + 255) / 256), 256, 0, [&] { glp_fri_fold2_kernel<0>(cur.data(), nxt.data(), log_len, half_inv, cc, beta, tw.lo.data(), tw.hip()); });
        cur.swap(nxt);
        beta = gl_ext_mul(beta, beta);
        shift = gl_mul(shift, shift);
    }
    memcpy(out, cur.data(), cur.size() * 8);
    return 0;
}

// ---- proof of work -----------------------------------------------------------------------------------------------------------------------
// one launch of the batched kernel over [base, base + count) for the listed instances; found [B] is updated in place.  count need not be a
// multiple of 256 (the window is cut where the caller likes)
extern "C" int emu_pow_batch(const u64* seeds, const u32* active, u32 n_active, u64 base, u64 count, u32 pow_bits, unsigned long long* found,
                             const u64* consts384, int small) {
    std::vector<u32> cf; std::vector<u64> cs;
    const GlpPoseidonConsts k = consts_of(consts384, small, cf, cs);
    const u32 bpi = (u32)((count + 255) / 256);
    if (small) glp_emu_launch(bpi * n_active, 256, 0, [&] { glp_pow_batch_kernel<true>(seeds, active, bpi, base, count, pow_bits, found, k); });
    else glp_emu_launch(bpi * n_active, 256, 0, [&] { glp_pow_batch_kernel<false>(seeds, active, bpi, base, count, pow_bits, found, k); });
    return 0;
}
extern "C" int emu_pow_single(const u64* seed, u64 base, u64 count, u32 pow_bits, unsigned long long* found, const u64* consts384, int small) {
    std::vector<u32> cf; std::vector<u64> cs;
    const GlpPoseidonConsts k = consts_of(consts384, small, cf, cs);
    const unsigned g = (unsigned)((count + 255) / 256);
    if (small) glp_emu_launch(g, 256, 0, [&] { glp_pow_kernel<true>(seed, base, count, pow_bits, found, k); });
    else glp_emu_launch(g, 256, 0, [&] { glp_pow_kernel<false>(seed, base, count, pow_bits, found, k); });
    return 0;
}

// ---- gathers -----------------------------------------------------------------------------------------------------------------------------
extern "C" int emu_gather_multi(const u64* const* bases, const u64* pairs, u64 n, u64* out) {
    glp_emu_launch((unsigned)glp_fri_gather_blocks(n), 256, 0, [&] { glp_gather_multi_kernel<0>((const u64*)bases, pairs, n, out); });
    return 0;
}
extern "C" int emu_gather_single(const u64* src, const u64* offs, u64 n, u64* out) {
    glp_emu_launch((unsigned)((n + 255) / 256), 256, 0, [&] { glp_gather_kernel<0>(src, offs, n, out); });
    return 0;
}

#ifdef GLP_EMU_FRI_BATCH_MAIN
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
    u64 st = 2026;
    int bad = 0;
    auto check = [&](bool ok, const char* what, u32 x, u32 y) { if (!ok) { printf("DIFF %s (%u, %u)\n", what, x, y); bad++; } };
    const u64 FILL = 0x5e5e5e5e5e5e5e5eull;

    // powers + openings: two batches (2 and 1 polynomials), masks 1 and 3, two points, B = 2; a partial chunk, then more than one chunk
    for (u32 log_n : {3u, 8u, 13u}) {
        const u32 B = 2, NP = 2, nb = 2, np[2] = {2, 1}, masks[2] = {1, 3};
        const u64 n = 1ull << log_n;
        std::vector<std::vector<u64>> co;
        std::vector<const u64*> ptrs;
        for (u32 i = 0; i < B; i++) for (u32 b = 0; b < nb; b++) co.push_back(rand_words(st, np[b] * n));
        for (auto& v : co) ptrs.push_back(v.data());
        const std::vector<u64> z = rand_words(st, 2 * B * NP);
        const u32 nch = glp_fri_eval_chunks(n), total = 2 + 1 + 1;
        std::vector<u64> zp(2 * n * B * NP), part((size_t)2 * B * total * nch);
        const long bpi = emu_powers_eval_batch(ptrs.data(), log_n, np, masks, nb, NP, B, z.data(), zp.data(), part.data());
        check(bpi == (long)total * nch, "eval blocks", log_n, 0);
        for (u32 i = 0; i < B; i++) {
            size_t k = 0;
            for (u32 p = 0; p < NP; p++)
                for (u32 b = 0; b < nb; b++) {
                    if (!((masks[b] >> p) & 1u)) continue;
                    std::vector<u64> zp1(2 * n), part1((size_t)2 * np[b] * nch);
                    emu_powers_eval_single(ptrs[i * nb + b], log_n, np[b], &z[2 * (i * NP + p)], zp1.data(), part1.data());
                    check(!memcmp(zp1.data(), &zp[2 * n * (i * NP + p)], 16 * n), "powers", log_n, i);
                    check(!memcmp(part1.data(), &part[2 * ((size_t)i * total * nch + k)], part1.size() * 8), "openings", log_n, i);
                    k += (size_t)np[b] * nch;
                }
        }
    }

    // combine: 2 points, 3 batches, masks 1, 3, 1; B = 2; both load widths; a gap between the instances' codewords must survive
    for (u32 log_N : {6u, 13u}) {
        const u32 B = 2, NP = 2, nb = 3, np[3] = {3, 2, 1}, masks[3] = {1, 3, 1}, rb = 1, total = 3 + 2 + 1 + 2;
        const u64 N = 1ull << log_N, stride = 2 * N + 6;
        std::vector<std::vector<u64>> lde;
        std::vector<const u64*> ptrs;
        for (u32 i = 0; i < B; i++) for (u32 b = 0; b < nb; b++) lde.push_back(rand_words(st, np[b] * N));
        for (auto& v : lde) ptrs.push_back(v.data());
        const std::vector<u64> cmb = rand_words(st, (size_t)B * (4 * NP + 2 * total));
        for (int v16 = 0; v16 <= 1; v16++) {
            std::vector<u64> out(stride * B, FILL);
            check(emu_combine_batch(ptrs.data(), log_N - rb, rb, np, masks, nb, NP, B, cmb.data(), 7, v16, out.data(), stride) == 0, "combine refused", log_N, v16);
            for (u32 i = 0; i < B; i++) {
                std::vector<u64> ref(2 * N);
                emu_combine_single(&ptrs[i * nb], log_N, np, masks, nb, NP, &cmb[(size_t)i * (4 * NP + 2 * total)], 7, ref.data());
                check(!memcmp(ref.data(), &out[i * stride], 16 * N), "combine", log_N, i);
                for (u64 w = 2 * N; w < stride; w++) check(out[i * stride + w] == FILL, "combine gap", log_N, i);
            }
        }
    }

    // fold layers (the shapes of tests/test_gpu_fri_batch.py), strides larger than dense
    const u32 folds[][2] = {{1, 1}, {4, 4}, {5, 5}, {7, 3}, {12, 4}, {13, 4}, {14, 2}};
    for (auto& f : folds)
        for (u32 B : {1u, 3u}) {
            const u32 log_len = f[0], a = f[1];
            const u64 in_w = 2ull << log_len, out_w = in_w >> a, in_stride = in_w + 4, out_stride = out_w + 2;
            const std::vector<u64> in = rand_words(st, in_stride * B), betas = rand_words(st, 2 * B);
            std::vector<u64> out(out_stride * B, FILL);
            check(emu_fold_layer_batch(in.data(), in_stride, out.data(), out_stride, log_len, a, 7, betas.data(), B) == 0, "fold refused", log_len, a);
            for (u32 i = 0; i < B; i++) {
                std::vector<u64> ref(out_w);
                emu_fold2_chain(&in[i * in_stride], ref.data(), log_len, a, 7, &betas[2 * i]);
                check(!memcmp(ref.data(), &out[i * out_stride], out_w * 8), "fold layer", log_len, a);
                for (u64 w = out_w; w < out_stride; w++) check(out[i * out_stride + w] == FILL, "fold gap", log_len, a);
            }
        }

    // proof of work: two seeds at 6 bits, a window of 512 nonces cut into two halves, the second half without the instance that has a nonce
    for (int small = 0; small <= 2; small += 2) {
        std::vector<u64> c384 = rand_words(st, 384);
        if (small) for (int i = 360; i < 384; i++) c384[i] = 1 + c384[i] % 40;
        const std::vector<u64> seeds = rand_words(st, 8);
        unsigned long long found[2] = {~0ull, ~0ull}, ref[2];
        const u32 both[2] = {0, 1};
        emu_pow_batch(seeds.data(), both, 2, 0, 256, 6, found, c384.data(), small);
        for (u32 i = 0; i < 2; i++) { ref[i] = ~0ull; emu_pow_single(&seeds[4 * i], 0, 256, 6, &ref[i], c384.data(), small); check(ref[i] == found[i], "pow first half", i, small); }
        // second half for instance 1 alone, whatever it found: instance 0's word must stay as it is
        const u32 one[1] = {1};
        const unsigned long long keep0 = found[0];
        unsigned long long f1 = ~0ull, r1 = ~0ull;
        found[1] = ~0ull;
        emu_pow_batch(seeds.data(), one, 1, 256, 200, 6, found, c384.data(), small);
        f1 = found[1];
        emu_pow_single(&seeds[4], 256, 200, 6, &r1, c384.data(), small);
        check(f1 == r1 && found[0] == keep0, "pow second half", 1, small);
    }

    // multi-gather: three sources
    {
        std::vector<std::vector<u64>> src = {rand_words(st, 100), rand_words(st, 37), rand_words(st, 1000)};
        const u64* bases[3] = {src[0].data(), src[1].data(), src[2].data()};
        const u64 n = 700;
        std::vector<u64> pairs(2 * n), out(n);
        for (u64 k = 0; k < n; k++) { pairs[2 * k] = next_word(st) % 3; pairs[2 * k + 1] = next_word(st) % src[pairs[2 * k]].size(); }
        emu_gather_multi(bases, pairs.data(), n, out.data());
        for (u64 k = 0; k < n; k++) check(out[k] == src[pairs[2 * k]][pairs[2 * k + 1]], "gather", (u32)k, 0);
    }
    printf(bad ? "emu_fri_batch_san: %d differences\n" : "emu_fri_batch_san: batched == single on every shape\n", bad);
    return bad ? 1 : 0;
}
#endif
