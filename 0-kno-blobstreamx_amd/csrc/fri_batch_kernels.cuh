// fri_batch_kernels.cuh — the kernels of glp_fri_prove_batch (fri.hip): B opening proofs of one shape share every launch.
// 1-D grids throughout: a launch has B * blocks_per_instance workgroups of 256 lanes and the instance (or table) index is
// blockIdx.x / blocks_per_instance (geometry: fri_batch_plan.h).  Per-instance data (pointers, power tables, alpha powers, Y_p, z_p) is
// read from the call's descriptor table, whose layout fri_batch_plan.h documents.
//
//   glp_ext_powers_batch_kernel     z^j tables for every (instance, point)
//   glp_eval_ext_batch_kernel       partial sums of f(z) for every (instance, point, opened batch, polynomial, chunk)
//   glp_fri_combine_batch_kernel    sum over the points p of (sum_k alpha^k f_k(x) - Y_p) / (x - z_p), one store per element
//   glp_fri_fold_layer_batch_kernel one committed fold layer (arity 2^A) in registers
//   glp_pow_batch_kernel            one proof-of-work window for the instances still searching
//   glp_gather_multi_kernel         out[k] = base[src[k]][off[k]]
// All arithmetic is exact and canonical, so every word equals what the single-instance kernels of fri_kernels.cuh produce.
// Plain HIP C++ without AMD builtins: tests/emu_fri_batch runs these bodies on the CPU.
#pragma once
#include "fri_kernels.cuh"

static_assert(GLP_EVAL_CHUNK == 4096u, "fri_batch_plan.h: GLP_FRI_BATCH_EVAL_CHUNK");

// 16-byte global accesses (global_load_dwordx4 / global_store_dwordx4); the address must be 16-byte aligned
struct __attribute__((aligned(16), may_alias)) glp_u64x2 { u64 x, y; };
GL_HD glp_u64x2 glp_ld16(const u64* p) { return *reinterpret_cast<const glp_u64x2*>(p); }
GL_HD void glp_st16(u64* p, u64 x, u64 y) { *reinterpret_cast<glp_u64x2*>(p) = glp_u64x2{x, y}; }
GL_HD const u64* glp_desc_ptr(u64 word) { return reinterpret_cast<const u64*>(word); }

// zp[t][j] = z_t^j, j < n, for table t = blockIdx.x / blocks_per_table; tabs + t * tab_stride: lo[256][2] then hi[*][2] (glp_ext_powers_kernel)
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_ext_powers_batch_kernel(u64* __restrict__ zp, u64 n, const u64* __restrict__ tabs, u64 tab_stride,
                                                                   u32 blocks_per_table) {
    const u32 t = blockIdx.x / blocks_per_table, lb = blockIdx.x - t * blocks_per_table;
    const u64* __restrict__ lo = tabs + (u64)t * tab_stride;
    const u64* __restrict__ hi = lo + 512;
    u64* __restrict__ out = zp + (u64)t * 2 * n;
    for (u64 j = (u64)lb * 256 + threadIdx.x; j < n; j += (u64)blocks_per_table * 256) {
        const u64 l = j & 255u, h = j >> 8;
        const glp_u64x2 a = glp_ld16(lo + 2 * l), b = glp_ld16(hi + 2 * h);
        const gl_ext2 v = gl_ext_mul(gl_ext2{a.x, a.y}, gl_ext2{b.x, b.y});
        glp_st16(out + 2 * j, v.a, v.b);
    }
}

// partial[blockIdx.x] = one chunk's sum of coeffs[j] * z^j (glp_eval_ext_kernel).  The blocks of one instance run over
// (point, batch opened there, polynomial, chunk) in that order — the order of the proof's openings.
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_eval_ext_batch_kernel(const u64* __restrict__ desc, u64 off_shape, u64 off_ptrs, u32 n_batches, u32 n_points,
                                                                 u64 n, u32 n_chunks, u32 blocks_per_instance, const u64* __restrict__ zp,
                                                                 u64* __restrict__ partial) {
    __shared__ u64 ra[256], rb[256];
    const u32 inst = blockIdx.x / blocks_per_instance;
    u32 r = blockIdx.x - inst * blocks_per_instance;
    u32 pt = 0, bt = 0, poly = 0, c = 0;
    bool found = false;
    for (u32 p = 0; p < n_points; p++)
        for (u32 b = 0; b < n_batches; b++) {
            if (found || !((desc[off_shape + 2 * b + 1] >> p) & 1ull)) continue;
            const u32 cnt = (u32)desc[off_shape + 2 * b] * n_chunks;
            if (r < cnt) { found = true; pt = p; bt = b; poly = r / n_chunks; c = r - poly * n_chunks; }
            else r -= cnt;
        }
    const u64* __restrict__ coeffs = glp_desc_ptr(desc[off_ptrs + 3 * ((u64)inst * n_batches + bt)]) + (u64)poly * n;
    const u64* __restrict__ zt = zp + ((u64)inst * n_points + pt) * 2 * n;
    const u64 j0 = (u64)c * GLP_EVAL_CHUNK;
    u64 sa = 0, sb = 0;
    for (u32 t = threadIdx.x; t < GLP_EVAL_CHUNK; t += 256) {
        const u64 j = j0 + t;
        if (j < n) {
            const u64 cf = coeffs[j];
            const glp_u64x2 z = glp_ld16(zt + 2 * j);
            sa = gl_add(sa, gl_mul(cf, z.x));
            sb = gl_add(sb, gl_mul(cf, z.y));
        }
    }
    ra[threadIdx.x] = sa;
    rb[threadIdx.x] = sb;
    __syncthreads();
    for (u32 s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            ra[threadIdx.x] = gl_add(ra[threadIdx.x], ra[threadIdx.x + s]);
            rb[threadIdx.x] = gl_add(rb[threadIdx.x], rb[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) glp_st16(partial + 2 * (u64)blockIdx.x, ra[0], rb[0]);
}

// The whole combined codeword of every instance in one launch.  A work-item owns 4 consecutive points x_i of one instance (so the 4
// extension inversions of an opening point share one field inversion, as in glp_fri_combine_kernel).  For each opening point p it sums
// alpha^k * lde_k(x_i) over the batches opened there — the four sums live in registers, no read-modify-write of the codeword between
// batches —, finishes (s - Y_p) / (x_i - z_p), adds the per-point quotients and stores each element once.
// V16: every d_lde is 16-byte aligned, so a row's 4 words are two 16-byte loads; otherwise four 8-byte loads.
struct GlpCombineBatchArgs {
    const u64* desc; u64 off_shape, off_ptrs, off_cmb, cmb_stride;
    u32 n_batches, n_points, log_N, blocks_per_instance;
    u64* out; u64 out_stride;               // instance b's codeword [N][2] at out + b * out_stride (16-byte aligned, stride even)
    u64 shift;
    const u64* w_lo; const u64* w_hi;       // forward two-level table of w_N
};
template <bool V16>
__global__ void __launch_bounds__(256) glp_fri_combine_batch_kernel(GlpCombineBatchArgs a) {
    const u64 N = 1ull << a.log_N;
    const u32 inst = blockIdx.x / a.blocks_per_instance;
    const u64 i0 = ((u64)(blockIdx.x - inst * a.blocks_per_instance) * 256 + threadIdx.x) * 4;
    if (i0 >= N) return;
    const u64* __restrict__ shape = a.desc + a.off_shape;
    const u64* __restrict__ ptrs = a.desc + a.off_ptrs + 3 * (u64)inst * a.n_batches;
    const u64* __restrict__ cmb = a.desc + a.off_cmb + (u64)inst * a.cmb_stride;      // Y[n_points][2], z[n_points][2], alpha^k
    const u64* __restrict__ ap = cmb + 4 * (u64)a.n_points;
    u64 x[4];
    glp_static_for<0, 4>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
        const u64 i = i0 + k;
        u64 e = 0;                             // bit reversal over log_N bits (portable form)
        for (u32 b = 0; b < a.log_N; b++) e |= ((i >> b) & 1ull) << (a.log_N - 1 - b);
        u64 v = a.w_lo[e & 4095u];
        if (a.w_hi) v = gl_mul(v, a.w_hi[e >> 12]);
        x[k] = gl_mul(v, a.shift);
    });
    gl_ext2 acc[4];
    glp_static_for<0, 4>([&](auto k_) { constexpr int k = decltype(k_)::value; acc[k] = gl_ext2{0, 0}; });
    for (u32 p = 0; p < a.n_points; p++) {
        gl_ext2 s[4];
        glp_static_for<0, 4>([&](auto k_) { constexpr int k = decltype(k_)::value; s[k] = gl_ext2{0, 0}; });
        bool any = false;
        for (u32 b = 0; b < a.n_batches; b++) {
            if (!((shape[2 * b + 1] >> p) & 1ull)) continue;
            any = true;
            const u32 np = (u32)shape[2 * b];
            const u64* __restrict__ row = glp_desc_ptr(ptrs[3 * b + 1]) + i0;
            for (u32 q = 0; q < np; q++, row += N, ap += 2) {
                const u64 aa = ap[0], ab = ap[1];
                u64 v[4];
                if (V16) {
                    const glp_u64x2 v01 = glp_ld16(row), v23 = glp_ld16(row + 2);
                    v[0] = v01.x; v[1] = v01.y; v[2] = v23.x; v[3] = v23.y;
                } else {
                    glp_static_for<0, 4>([&](auto k_) { constexpr int k = decltype(k_)::value; v[k] = row[k]; });
                }
                glp_static_for<0, 4>([&](auto k_) {
                    constexpr int k = decltype(k_)::value;
                    s[k].a = gl_add(s[k].a, gl_mul(v[k], aa));
                    s[k].b = gl_add(s[k].b, gl_mul(v[k], ab));
                });
            }
        }
        if (!any) continue;
        const gl_ext2 Y{cmb[2 * p], cmb[2 * p + 1]}, z{cmb[2 * (a.n_points + p)], cmb[2 * (a.n_points + p) + 1]};
        gl_ext2 d[4];
        u64 nrm[4];
        glp_static_for<0, 4>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            d[k] = gl_ext2{gl_sub(x[k], z.a), gl_neg(z.b)};              // x - z
            const u64 bb = gl_mul(d[k].b, d[k].b);
            const u64 b7 = gl_add(gl_add(gl_add(bb, bb), gl_add(bb, bb)), gl_add(gl_add(bb, bb), bb));
            nrm[k] = gl_sub(gl_mul(d[k].a, d[k].a), b7);                 // norm, nonzero unless x == z
        });
        const u64 p01 = gl_mul(nrm[0], nrm[1]), p012 = gl_mul(p01, nrm[2]), p0123 = gl_mul(p012, nrm[3]);
        u64 inv = gl_inv(p0123);
        u64 ni[4];
        ni[3] = gl_mul(inv, p012); inv = gl_mul(inv, nrm[3]);
        ni[2] = gl_mul(inv, p01); inv = gl_mul(inv, nrm[2]);
        ni[1] = gl_mul(inv, nrm[0]);
        ni[0] = gl_mul(inv, nrm[1]);
        glp_static_for<0, 4>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            const gl_ext2 dinv{gl_mul(d[k].a, ni[k]), gl_mul(gl_neg(d[k].b), ni[k])};
            acc[k] = gl_ext_add(acc[k], gl_ext_mul(gl_ext_sub(s[k], Y), dinv));
        });
    }
    u64* __restrict__ out = a.out + (u64)inst * a.out_stride + 2 * i0;
    glp_static_for<0, 4>([&](auto k_) { constexpr int k = decltype(k_)::value; glp_st16(out + 2 * k, acc[k].a, acc[k].b); });
}

// One committed fold layer of arity 2^A for B codewords: work-item j of instance b loads the 2^A consecutive extension elements of layer
// leaf j (bit-reversed order: they are the coset that folds to output j), folds A times in registers with beta, beta^2, beta^4, .. and
// stores one element — what A successive glp_fri_fold2_kernel launches compute through A - 1 intermediate buffers.
// Pair i = j * 2^(A-1) + t of the first step has 1/x_i = w_L^-rev(i) / shift with rev(i) = rev(t) << (L - A) | rev(j) (L = log_len), i.e.
// (w_L^-rev(j)) * tw[t], tw[t] = w_(2^A)^-rev(t) / shift: one table read per work-item (inverse table of w at 2^log_len) and the 2^(A-1)
// host-built constants tw.  The folded point of pair t is x_t^2 and pair t of the next step holds the folded pairs 2t and 2t + 1 (points
// +-x_2t^2), so the deeper steps take 1/x from (1/x_2t)^2.
struct GlpFoldLayerBatchArgs {
    const u64* in; u64 in_stride; u64* out; u64 out_stride;     // words; 16-byte aligned, strides even
    u32 log_len, blocks_per_instance;
    const u64* betas;                       // device [B][2]
    u64 half_inv;                           // 1/2
    u64 tw[16];
    const u64* iw_lo; const u64* iw_hi;     // two-level inverse table of w at 2^log_len
};
// host: half_inv and tw[t] = w_(2^a)^-rev(t) / shift, t < 2^(a-1) (rev over a - 1 bits), for the layer whose domain is shift * <w>
static inline void glp_fold_layer_consts(u32 a, u64 shift, GlpFoldLayerBatchArgs& fa) {
    const u64 wi = gl_inv(gl_root_of_unity(a)), si = gl_inv(shift);
    for (u32 t = 0; t < 16; t++) fa.tw[t] = 0;
    for (u32 t = 0; t < (1u << (a - 1)); t++) {
        u32 r = 0;
        for (u32 b = 0; b + 1 < a; b++) r |= ((t >> b) & 1u) << (a - 2 - b);
        fa.tw[t] = gl_mul(gl_pow(wi, r), si);
    }
    fa.half_inv = gl_inv(2);
}
template <int A>
__global__ void __launch_bounds__(256) glp_fri_fold_layer_batch_kernel(GlpFoldLayerBatchArgs a) {
    constexpr int W = 1 << A;
    const u32 lo_bits = a.log_len - A;
    const u32 inst = blockIdx.x / a.blocks_per_instance;
    const u64 j = (u64)(blockIdx.x - inst * a.blocks_per_instance) * 256 + threadIdx.x;
    if (j >= (1ull << lo_bits)) return;
    const u64* __restrict__ src = a.in + (u64)inst * a.in_stride + j * (2 * W);
    gl_ext2 v[W];
    glp_static_for<0, W>([&](auto t_) {
        constexpr int t = decltype(t_)::value;
        const glp_u64x2 w = glp_ld16(src + 2 * t);
        v[t] = gl_ext2{w.x, w.y};
    });
    u64 e = 0;                                 // bit reversal of j over log_len - A bits (portable form)
    for (u32 b = 0; b < lo_bits; b++) e |= ((j >> b) & 1ull) << (lo_bits - 1 - b);
    u64 base = a.iw_lo[e & 4095u];
    if (a.iw_hi) base = gl_mul(base, a.iw_hi[e >> 12]);
    u64 ix[W / 2 > 0 ? W / 2 : 1];
    glp_static_for<0, W / 2>([&](auto t_) { constexpr int t = decltype(t_)::value; ix[t] = gl_mul(base, a.tw[t]); });
    gl_ext2 beta{a.betas[2 * (u64)inst], a.betas[2 * (u64)inst + 1]};
    glp_static_for<0, A>([&](auto f_) {
        constexpr int f = decltype(f_)::value;
        constexpr int half = W >> (f + 1);
        glp_static_for<0, half>([&](auto t_) {
            constexpr int t = decltype(t_)::value;
            const gl_ext2 f0 = v[2 * t], f1 = v[2 * t + 1];
            const gl_ext2 sum = gl_ext_scale(gl_ext_add(f0, f1), a.half_inv);
            const gl_ext2 dif = gl_ext_scale(gl_ext_sub(f0, f1), gl_mul(ix[t], a.half_inv));      // (f(x) - f(-x)) / (2x)
            v[t] = gl_ext_add(sum, gl_ext_mul(beta, dif));
        });
        glp_static_for<0, half / 2>([&](auto t_) { constexpr int t = decltype(t_)::value; ix[t] = gl_sqr(ix[2 * t]); });
        beta = gl_ext_mul(beta, beta);
    });
    glp_st16(a.out + (u64)inst * a.out_stride + 2 * j, v[0].a, v[0].b);
}

// One window [base, base + count) of the proof-of-work search for the instances listed in active[0 .. gridDim.x / blocks_per_instance):
// instance i = active[..] hashes seeds[4 i ..] and keeps the smallest accepted nonce of the window in found[i] (glp_pow_kernel's rule;
// found[i] is ~0 until instance i has a nonce, and an instance that has one is no longer listed).
template <bool SMALL>
__global__ void __launch_bounds__(256) glp_pow_batch_kernel(const u64* __restrict__ seeds, const u32* __restrict__ active, u32 blocks_per_instance,
                                                            u64 base, u64 count, u32 pow_bits, unsigned long long* found, GlpPoseidonConsts k) {
    const u32 slot = blockIdx.x / blocks_per_instance;
    const u64 t = (u64)(blockIdx.x - slot * blocks_per_instance) * 256 + threadIdx.x;
    if (t >= count) return;
    const u32 inst = active[slot];
    const u64 nonce = base + t;
    u64 s[12];
    glp_static_for<0, 4>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = seeds[4 * (u64)inst + j]; });
    s[4] = nonce % GL_P;
    glp_static_for<5, 12>([&](auto j_) { constexpr int j = decltype(j_)::value; s[j] = 0; });
    glp_poseidon_permute<SMALL>(s, k);
    if ((s[0] >> (64 - pow_bits)) == 0) {
#if defined(GLP_EMU)
        glp_emu_atomic_min(found + inst, (unsigned long long)nonce);
#else
        atomicMin(found + inst, (unsigned long long)nonce);
#endif
    }
}

// out[k] = base[src[k]][off[k]]: pairs[2k] = src (index into the table of base pointers), pairs[2k + 1] = off (words)
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) glp_gather_multi_kernel(const u64* __restrict__ bases, const u64* __restrict__ pairs, u64 n,
                                                               u64* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const glp_u64x2 so = glp_ld16(pairs + 2 * i);
    out[i] = glp_desc_ptr(bases[so.x])[so.y];
}
