// tests/emu_place_batch/emu_place_batch.cpp — TEST INFRASTRUCTURE.  The kernels of glp_witness_place_batch (csrc/place_batch_kernels.cuh) on the
// CPU, unchanged, with the grids the driver uses (witness.hip), beside the single-instance bodies they must equal word for word:
// glp_witness_place_kernel (glp_gather_u64) and glp_poseidon_gate_fill_kernel<0> / <1> / glp_sha_gate_fill_kernel (csrc/plonk_kernels.cuh).
// Never part of the product.  None of these kernels has a barrier or a shuffle, so the work-items of a launch run one after the other on the
// calling thread (glp_emu_launch_seq) instead of one std::thread each: a 2^9 x 144 placement is 73 728 work-items per launch.
// With -DGLP_EMU_PLACE_BATCH_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined: `make sanitized`) that compares
// batched against single on small shapes.
#include "../emu/hip_emu.h"
#include <vector>
#include "../../0-kno-blobstreamx_amd/csrc/place_batch_kernels.cuh"

namespace {
unsigned capped(u64 items, unsigned per_block, unsigned cap) {
    const u64 want = (items + per_block - 1) / per_block;
    return (unsigned)(want < cap ? want : cap);
}
}  // namespace

// ---- placement: the driver's grids (256 lanes, min(ceil(cells / 256), 4096) workgroups, both entry points) --------------------------------
extern "C" int emu_place_batch(u64* dst, u64 wire_stride, const u64* src, u64 value_stride, const u32* slab_row, u32 B, const u32* index, u64 n_cells) {
    glp_emu_launch_seq(capped(n_cells, 256, 4096), 256, [&] { glp_witness_place_batch_kernel<0>(dst, wire_stride, src, value_stride, slab_row, B, index, n_cells); });
    return 0;
}
extern "C" int emu_place_single(u64* dst, const u64* src, u64 n_src, const u32* index, u64 n_cells, u32* bad) {
    glp_emu_launch_seq(capped(n_cells, 256, 4096), 256, [&] { glp_witness_place_kernel<0>(dst, src, n_src, index, n_cells, bad); });
    return 0;
}
extern "C" int emu_public_batch(u64* out, const u64* src, u64 value_stride, const u32* slab_row, u32 B, const u32* public_vars, u32 n_public) {
    glp_emu_launch_seq(capped((u64)B * n_public, 256, 4096), 256, [&] { glp_witness_public_batch_kernel<0>(out, src, value_stride, slab_row, B, public_vars, n_public); });
    return 0;
}

// ---- row fillers: 64 lanes, B * ceil(n_rows / 64) workgroups against ceil(n_rows / 64) per instance ------------------------------------------
extern "C" int emu_pos_fill_batch(u64* wires, u64 wire_stride, u32 log_n, const u32* rows, u32 n_rows, u32 B, const u64* consts, int small_mds) {
    const u32 bpi = (n_rows + 63) / 64;
    const u64 n = 1ull << log_n;
    if (small_mds) glp_emu_launch_seq(B * bpi, 64, [&] { glp_poseidon_gate_fill_batch_kernel<1>(wires, wire_stride, n, rows, n_rows, bpi, consts); });
    else glp_emu_launch_seq(B * bpi, 64, [&] { glp_poseidon_gate_fill_batch_kernel<0>(wires, wire_stride, n, rows, n_rows, bpi, consts); });
    return 0;
}
extern "C" int emu_pos_fill_single(u64* wires, u32 log_n, const u32* rows, u32 n_rows, const u64* consts, int small_mds) {
    const u64 n = 1ull << log_n;
    if (small_mds) glp_emu_launch_seq((n_rows + 63) / 64, 64, [&] { glp_poseidon_gate_fill_kernel<1>(wires, n, rows, n_rows, consts); });
    else glp_emu_launch_seq((n_rows + 63) / 64, 64, [&] { glp_poseidon_gate_fill_kernel<0>(wires, n, rows, n_rows, consts); });
    return 0;
}
extern "C" int emu_sha_fill_batch(u64* wires, u64 wire_stride, u32 log_n, const u32* rows, const u32* kinds, u32 n_rows, u32 B) {
    const u32 bpi = (n_rows + 63) / 64;
    glp_emu_launch_seq(B * bpi, 64, [&] { glp_sha_gate_fill_batch_kernel<0>(wires, wire_stride, 1ull << log_n, rows, kinds, n_rows, bpi); });
    return 0;
}
extern "C" int emu_sha_fill_single(u64* wires, u32 log_n, const u32* rows, const u32* kinds, u32 n_rows) {
    glp_emu_launch_seq((n_rows + 63) / 64, 64, [&] { glp_sha_gate_fill_kernel<0>(wires, 1ull << log_n, rows, kinds, n_rows); });
    return 0;
}

#ifdef GLP_EMU_PLACE_BATCH_MAIN
#include <cstdio>
static u64 next_raw(u64& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    u64 z = st ^ (st >> 29);
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 32;
    return z;
}
static u64 next_word(u64& st) { return next_raw(st) % GL_P; }

int main() {
    u64 st = 2029;
    int bad = 0;
    const u64 FILL = 0x5e5e5e5e5e5e5e5eull;
    auto check = [&](bool ok, const char* what, u32 x, u32 y) { if (!ok) { printf("DIFF %s (%u, %u)\n", what, x, y); bad++; } };
    std::vector<u64> pos_small(384), pos_big(384);
    for (u64& w : pos_small) w = next_word(st);
    for (u64& w : pos_big) w = next_word(st);
    for (int i = 0; i < 12; i++) { pos_small[360 + i] = 1 + (u64)i; pos_small[372 + i] = 2 + (u64)i; }
    // (log_n, W, Poseidon rows?, SHA rows?): row counts that are no multiple of 64 at 2^9, strides with gaps, slab rows [2, 0, 2]
    const u32 shapes[][4] = {{3, 136, 1, 0}, {3, 144, 0, 1}, {3, 144, 1, 1}, {9, 136, 1, 0}, {9, 144, 1, 1}};
    for (auto& s : shapes)
        for (u32 B : {1u, 3u}) {
            const u32 log_n = s[0], W = s[1], slab_rows = 3, GAPW = 5, GAPV = 7;
            const u64 n = 1ull << log_n, cells = (u64)W * n, n_src = cells / 3 + 11, vstride = n_src + GAPV, wstride = cells + GAPW;
            const u32 row_of[3] = {2, 0, 2};
            const u32 n_pos = s[2] ? (u32)(n * 3 / 8 + 1) : 0, n_sha = s[3] ? (u32)(n / 2 - 1) : 0;
            std::vector<u32> pos_rows(n_pos), sha_rows(n_sha), kinds(n_sha), index(cells);
            for (u32 k = 0; k < n_pos; k++) pos_rows[k] = k;
            for (u32 k = 0; k < n_sha; k++) { sha_rows[k] = n_pos + k; kinds[k] = k & 3; }
            std::vector<u64> slab(slab_rows * vstride, FILL);
            for (u32 r = 0; r < slab_rows; r++)
                for (u64 k = 0; k < n_src; k++) slab[r * vstride + k] = next_word(st);
            for (u64 i = 0; i < cells; i++) index[i] = next_raw(st) % 5 == 0 ? 0xFFFFFFFFu : (u32)(next_raw(st) % n_src);
            // what the row fillers read must be in range: SHA words are 32-bit, the swap bit is 0 / 1
            for (u32 r = 0; r < slab_rows; r++) {
                slab[r * vstride + 0] = r & 1; slab[r * vstride + 1] = 0x89abcdefull ^ r; slab[r * vstride + 2] = 0x01234567ull + r;
            }
            for (u32 k = 0; k < n_pos; k++) index[(u64)GLP_POS_SWAP_WIRE * n + pos_rows[k]] = 0;
            for (u32 k = 0; k < n_sha; k++) for (u32 j = 0; j < 12; j++) index[(u64)j * n + sha_rows[k]] = 1 + ((k + j) & 1);
            std::vector<u64> got(B * wstride, FILL);
            emu_place_batch(got.data(), wstride, slab.data(), vstride, row_of, B, index.data(), cells);
            for (int small = 0; small <= 1 && n_pos; small++) {
                std::vector<u64> g2 = got;
                const u64* pc = small ? pos_small.data() : pos_big.data();
                emu_pos_fill_batch(g2.data(), wstride, log_n, pos_rows.data(), n_pos, B, pc, small);
                for (u32 i = 0; i < B; i++) {
                    std::vector<u64> one(cells, FILL);
                    u32 flag = 0;
                    emu_place_single(one.data(), &slab[row_of[i] * vstride], n_src, index.data(), cells, &flag);
                    emu_pos_fill_single(one.data(), log_n, pos_rows.data(), n_pos, pc, small);
                    check(!flag && !memcmp(one.data(), &g2[i * wstride], cells * 8), "place + Poseidon rows", log_n * 1000 + W, i * 2 + small);
                }
            }
            if (n_sha) emu_sha_fill_batch(got.data(), wstride, log_n, sha_rows.data(), kinds.data(), n_sha, B);
            for (u32 i = 0; i < B; i++) {
                std::vector<u64> one(cells, FILL);
                u32 flag = 0;
                emu_place_single(one.data(), &slab[row_of[i] * vstride], n_src, index.data(), cells, &flag);
                if (n_sha) emu_sha_fill_single(one.data(), log_n, sha_rows.data(), kinds.data(), n_sha);
                check(!flag && !memcmp(one.data(), &got[i * wstride], cells * 8), "place + SHA rows", log_n * 1000 + W, i);
                for (u32 g = 0; g < GAPW; g++) check(got[i * wstride + cells + g] == FILL, "wire gap", log_n, i);
            }
            for (u32 r = 0; r < slab_rows; r++)
                for (u32 g = 0; g < GAPV; g++) check(slab[r * vstride + n_src + g] == FILL, "value gap", log_n, r);
            // the public values
            const u32 n_pub = 12;
            std::vector<u32> pv(n_pub);
            for (u32 j = 0; j < n_pub; j++) pv[j] = (u32)(next_raw(st) % n_src);
            std::vector<u64> pub(B * n_pub + 2, FILL);
            emu_public_batch(pub.data(), slab.data(), vstride, row_of, B, pv.data(), n_pub);
            for (u32 i = 0; i < B; i++)
                for (u32 j = 0; j < n_pub; j++) check(pub[i * n_pub + j] == slab[row_of[i] * vstride + pv[j]], "public", i, j);
            check(pub[B * n_pub] == FILL && pub[B * n_pub + 1] == FILL, "public tail", log_n, B);
        }
    if (bad) { printf("%d differences\n", bad); return 1; }
    printf("emu_place_batch: batched == single on every shape\n");
    return 0;
}
#endif
