// verify_batch_kernels.cuh — the query phase of glp_plonk_verify_batch / glp_fri_verify_batch (verify.hip): what the
// single verifier's loop `for q < nq` does, as two kinds of work item over the plan of verify_plan.h.
//
//   Merkle item (proof, query, tree)   tree < nb: a batch tree, else layer tree (tree - nb).  Leaf canonicity, hash_or_noop (the leaf itself
//                                      up to 4 words, else the overwrite sponge with a last block shorter than 8 words), the path walk to the
//                                      cap entry, the 4-word compare.  Items are ordered tree-major, (proof, query) minor: the lanes of a
//                                      wavefront walk the same tree of consecutive queries, so the trip counts of the sponge and of the path
//                                      loop are wave-uniform for same-shape proofs.
//   arithmetic item (proof, query)     x from the index, the alpha-power combination over all opened polynomials, "query point equals an
//                                      opening point", per layer "continues the fold" and the 2^a-point fold, the final polynomial at x^(2^(aL)).
//                                      The 2^a <= 16 extension values of a layer leaf live in registers: every index into them is a
//                                      compile-time constant (static loops and selects), none is computed at run time.
// A failing item does atomicMin of its key (query << 16 | step) on its proof's slot; the lowest key is the verdict.  Non-canonical leaf words
// are reported by the Merkle item; the arithmetic item may compute on them, its result then loses against the lower key.
// Every offset comes from the descriptor and its tables, which the host phase computed from the range-checked header and checked against the
// proof's length; the proof's own words are used as field data only.
// Plain HIP C++ without AMD builtins, vector stores only: tests/emu_verify_batch runs these bodies on the CPU.
#pragma once
#include "verify_plan.h"

#if defined(GLP_EMU)
#define GLP_VB_MIN64(p, v) glp_emu_atomic_min((p), (unsigned long long)(v))
#else
#define GLP_VB_MIN64(p, v) atomicMin((p), (unsigned long long)(v))
#endif

// the bodies of the static loops must end up inside the item: a lambda left as a call keeps the values it captures in memory (scratch)
#define GLP_VB_INL __attribute__((always_inline))

struct GlpVerifyArgs {
    const u64* slab;                 // the proofs' words, one after the other
    const u64* aux;                  // their tables
    const GlpVerifyDesc* desc;
    const u64* items;                // desc | query << 32 (Merkle items: tree in tree_of below)
    const u32* tree_first;           // [n_trees + 1] first Merkle item of every tree
    unsigned long long* keys;        // [n_desc], all ones before the first launch
    u32 n_trees;
    u64 n_items;
    GlpPoseidonConsts k;
};

// hash_or_noop: digest of `len` words at e
template <bool SMALL>
GL_HD void glp_vb_leaf_digest(const u64* e, u32 len, const GlpPoseidonConsts& k, u64 (&out)[4]) {
    if (len <= 4) {
        glp_static_for<0, 4>([&](auto i_) GLP_VB_INL { constexpr int i = decltype(i_)::value; out[i] = (u32)i < len ? e[i] : 0; });
        return;
    }
    u64 s[12];
    glp_static_for<0, 12>([&](auto i_) GLP_VB_INL { constexpr int i = decltype(i_)::value; s[i] = 0; });
    for (u32 off = 0; off < len; off += 8) {
        const u32 m = len - off;                                     // a last block shorter than 8 words overwrites its first m words only
        glp_static_for<0, 8>([&](auto i_) GLP_VB_INL { constexpr int i = decltype(i_)::value; if ((u32)i < m) s[i] = e[off + i]; });
        glp_poseidon_permute<SMALL>(s, k);
    }
    glp_static_for<0, 4>([&](auto i_) GLP_VB_INL { constexpr int i = decltype(i_)::value; out[i] = s[i]; });
}

// one Merkle item: 0 when the tree's checks hold for this query, else the failing step
template <bool SMALL>
GL_HD u32 glp_vb_merkle_item(const u64* proof, const u64* aux, const GlpVerifyDesc& d, u32 q, u32 tree, const GlpPoseidonConsts& k, bool& bad) {
    const u64 idx = aux[d.o_idx + q];
    const u64* qbase = proof + d.q0 + (u64)q * d.qwords;
    const u64 *leaf, *cap;
    u32 len, plen, step_noncanon, step_path;
    u64 index, cap_len;
    if (tree < d.nb) {
        const u64* t = aux + d.o_batch + GLP_VB_BATCH_WORDS * tree;
        len = (u32)t[0]; leaf = qbase + t[1]; cap = proof + t[2];
        plen = d.log_N - d.cap0; index = idx; cap_len = 1ull << d.cap0;
        step_noncanon = glp_vstep_batch(tree, 1); step_path = glp_vstep_batch(tree, 2);
    } else {
        const u32 l = tree - d.nb;
        const u64* t = aux + d.o_layer + GLP_VB_LAYER_WORDS * l;
        const u32 caph = (u32)t[2], ll = (u32)t[3];
        len = 2u << d.a; leaf = qbase + t[0]; cap = proof + t[1];
        plen = ll - d.a - caph; index = (idx >> (d.a * l)) >> d.a; cap_len = 1ull << caph;
        step_noncanon = glp_vstep_layer(d.nb, l, 1); step_path = glp_vstep_layer(d.nb, l, 3);
    }
    const u64* path = leaf + len;
    bad = true;
    for (u32 j = 0; j < len; j++)
        if (leaf[j] >= GL_P) return step_noncanon;
    u64 cur[4];
    glp_vb_leaf_digest<SMALL>(leaf, len, k, cur);
    for (u32 lvl = 0; lvl < plen; lvl++) {
        const u64* sib = path + 4 * lvl;
        const bool right = ((index >> lvl) & 1ull) != 0;             // this node is the right child: the sibling goes first
        u64 s[12];
        glp_static_for<0, 4>([&](auto i_) GLP_VB_INL {
            constexpr int i = decltype(i_)::value;
            const u64 sv = sib[i];
            s[i] = right ? sv : cur[i];
            s[4 + i] = right ? cur[i] : sv;
            s[8 + i] = 0;
        });
        glp_poseidon_permute<SMALL>(s, k);
        glp_static_for<0, 4>([&](auto i_) GLP_VB_INL { constexpr int i = decltype(i_)::value; cur[i] = s[i]; });
    }
    const u64 ci = index >> plen;
    if (ci >= cap_len) return step_path;
    bool same = true;
    glp_static_for<0, 4>([&](auto i_) GLP_VB_INL { constexpr int i = decltype(i_)::value; same = same && cur[i] == cap[4 * ci + i]; });
    if (!same) return step_path;
    bad = false;
    return 0;
}

// one arithmetic item: `bad` and the failing step, as above
GL_HD u32 glp_vb_arith_item(const u64* proof, const u64* aux, const GlpVerifyDesc& d, u32 q, bool& bad) {
    const u64 idx = aux[d.o_idx + q];
    const u64* qbase = proof + d.q0 + (u64)q * d.qwords;
    const u64 inv2 = gl_inv(2);
    const u32 a = d.a;
    bad = true;
    const u64 x = gl_mul(d.shift, gl_pow(d.w_N, glp_bitrev(idx, d.log_N)));
    // sum_k alpha^k * leaf value k, per opening point
    gl_ext2 acc0{0, 0}, acc1{0, 0}, acc2{0, 0}, acc3{0, 0};
    {
        const u64* ap = aux + d.o_apow;
        for (u32 e = 0; e < d.n_order; e++) {
            const u64 pb = aux[d.o_order + e];
            const u32 p = (u32)pb, b = (u32)(pb >> 32);
            const u64* t = aux + d.o_batch + GLP_VB_BATCH_WORDS * b;
            const u32 np = (u32)t[0];
            const u64* leaf = qbase + t[1];
            gl_ext2 s{0, 0};
            for (u32 j = 0; j < np; j++, ap += 2) s = gl_ext_add(s, gl_ext_scale(gl_ext2{ap[0], ap[1]}, leaf[j]));
            acc0 = p == 0 ? gl_ext_add(acc0, s) : acc0;
            acc1 = p == 1 ? gl_ext_add(acc1, s) : acc1;
            acc2 = p == 2 ? gl_ext_add(acc2, s) : acc2;
            acc3 = p == 3 ? gl_ext_add(acc3, s) : acc3;
        }
    }
    gl_ext2 cur{0, 0};
    {
        const gl_ext2 accs[4] = {acc0, acc1, acc2, acc3};
        bool at_point = false;
        glp_static_for<0, 4>([&](auto p_) GLP_VB_INL {
            constexpr int p = decltype(p_)::value;
            if ((u32)p < d.n_pts && ((d.pt_used >> p) & 1u) && !at_point) {
                const gl_ext2 pt{aux[d.o_pts + 2 * p], aux[d.o_pts + 2 * p + 1]}, Y{aux[d.o_ys + 2 * p], aux[d.o_ys + 2 * p + 1]};
                const gl_ext2 den = gl_ext_sub(gl_ext2{x, 0}, pt);
                if (den.a == 0 && den.b == 0) at_point = true;
                else cur = gl_ext_add(cur, gl_ext_mul(gl_ext_sub(accs[p], Y), glp_ext_inv(den)));
            }
        });
        if (at_point) return glp_vstep_point(d.nb);
    }
    u64 sh = d.shift;
    const u32 cnt = 1u << a;
    for (u32 l = 0; l < d.L; l++) {
        const u64* t = aux + d.o_layer + GLP_VB_LAYER_WORDS * l;
        const u64* leaf = qbase + t[0];
        const u32 ll = (u32)t[3];
        gl_ext2 vals[16];
        glp_static_for<0, 16>([&](auto j_) GLP_VB_INL {
            constexpr int j = decltype(j_)::value;
            vals[j] = (u32)j < cnt ? gl_ext2{leaf[2 * j], leaf[2 * j + 1]} : gl_ext2{0, 0};
        });
        const u64 p_l = idx >> (a * l);
        const u64 leaf_idx = p_l >> a;
        const u32 sel = (u32)(p_l & (cnt - 1));
        const gl_ext2 mine{leaf[2 * sel], leaf[2 * sel + 1]};          // the value at this query's position: read from the proof, not from vals
        if (!glp_ext_eq(mine, cur)) return glp_vstep_layer(d.nb, l, 2);
        gl_ext2 beta{t[4], t[5]};
        u64 base = leaf_idx << a;
        u32 cl = ll;
        glp_static_for<0, 4>([&](auto s_) GLP_VB_INL {
            constexpr int s = decltype(s_)::value;
            if ((u32)s < a) {
                const u64 wl = gl_root_of_unity(cl);
                const u32 half = cnt >> (s + 1);
                glp_static_for<0, (8 >> s)>([&](auto i_) GLP_VB_INL {
                    constexpr int i = decltype(i_)::value;
                    if ((u32)i < half) {
                        const u64 xi = gl_mul(sh, gl_pow(wl, glp_bitrev(base + 2 * i, cl)));
                        const gl_ext2 f0 = vals[2 * i], f1 = vals[2 * i + 1];
                        const gl_ext2 sm = gl_ext_scale(gl_ext_add(f0, f1), inv2);
                        const gl_ext2 dd = gl_ext_scale(gl_ext_sub(f0, f1), gl_mul(inv2, gl_inv(xi)));
                        vals[i] = gl_ext_add(sm, gl_ext_mul(beta, dd));      // in place: entry i is read by pair i only
                    }
                });
                base >>= 1;
                cl -= 1;
                beta = gl_ext_mul(beta, beta);
                sh = gl_mul(sh, sh);
            }
        });
        cur = vals[0];
    }
    const u32 fl = d.log_N - a * d.L;
    const u64 xf = gl_mul(sh, gl_pow(gl_root_of_unity(fl), glp_bitrev(idx >> (a * d.L), fl)));
    const u64* fin = proof + d.fin_off;
    gl_ext2 ev{0, 0};
    for (u32 j = 1u << d.final_bits; j-- > 0;) ev = gl_ext_add(gl_ext_scale(ev, xf), gl_ext2{fin[2 * j], fin[2 * j + 1]});
    if (!glp_ext_eq(ev, cur)) return glp_vstep_final(d.nb, d.L);
    bad = false;
    return 0;
}

#if defined(__HIPCC__) || defined(GLP_EMU)
// the tree of Merkle item i: the last t with tree_first[t] <= i (n_trees <= 96: a linear walk over a table every lane reads alike)
GL_HD u32 glp_vb_tree_of(const u32* tree_first, u32 n_trees, u64 i) {
    u32 t = 0;
    while (t + 1 < n_trees && (u64)tree_first[t + 1] <= i) t++;
    return t;
}

template <bool SMALL>
__global__ void __launch_bounds__(GLP_VB_BLOCK) glp_verify_merkle_kernel(GlpVerifyArgs a) {
    const u64 i = (u64)blockIdx.x * GLP_VB_BLOCK + threadIdx.x;
    if (i >= a.n_items) return;
    const u64 it = a.items[i];
    const GlpVerifyDesc d = a.desc[(u32)it];
    const u32 q = (u32)(it >> 32);
    bool bad;
    const u32 step = glp_vb_merkle_item<SMALL>(a.slab + d.base, a.aux + d.aux, d, q, glp_vb_tree_of(a.tree_first, a.n_trees, i), a.k, bad);
    if (bad) GLP_VB_MIN64(&a.keys[d.key_slot], glp_vkey(q, step));
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(GLP_VB_BLOCK) glp_verify_arith_kernel(GlpVerifyArgs a) {
    const u64 i = (u64)blockIdx.x * GLP_VB_BLOCK + threadIdx.x;
    if (i >= a.n_items) return;
    const u64 it = a.items[i];
    const GlpVerifyDesc d = a.desc[(u32)it];
    const u32 q = (u32)(it >> 32);
    bool bad;
    const u32 step = glp_vb_arith_item(a.slab + d.base, a.aux + d.aux, d, q, bad);
    if (bad) GLP_VB_MIN64(&a.keys[d.key_slot], glp_vkey(q, step));
}
#endif

// the same items one after the other on the host (glp_*_verify_batch_host): keys[n_desc], all ones on entry; proofs[i] = the words of desc i
static inline void glp_vb_run_host(const glp_verify::VerifyPlan& P, const u64* const* proofs, const GlpPoseidonConsts& k, bool small_mds,
                                   unsigned long long* keys) {
    for (u32 t = 0; t < P.by_tree.size(); t++)
        for (const auto& it : P.by_tree[t]) {
            const GlpVerifyDesc& d = P.desc[it.desc];
            bool bad;
            const u32 step = small_mds ? glp_vb_merkle_item<true>(proofs[it.desc], P.aux.data() + d.aux, d, it.q, t, k, bad)
                                       : glp_vb_merkle_item<false>(proofs[it.desc], P.aux.data() + d.aux, d, it.q, t, k, bad);
            if (bad && glp_vkey(it.q, step) < keys[d.key_slot]) keys[d.key_slot] = glp_vkey(it.q, step);
        }
    for (const auto& it : P.arith) {
        const GlpVerifyDesc& d = P.desc[it.desc];
        bool bad;
        const u32 step = glp_vb_arith_item(proofs[it.desc], P.aux.data() + d.aux, d, it.q, bad);
        if (bad && glp_vkey(it.q, step) < keys[d.key_slot]) keys[d.key_slot] = glp_vkey(it.q, step);
    }
}
