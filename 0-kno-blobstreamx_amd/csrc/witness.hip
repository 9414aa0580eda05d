// witness.hip — the compiled witness plan (witness_plan.h) behind the C ABI, and its batched evaluation on the device (witness_kernels.cuh).
//
// OWNERSHIP of the device copy: the PLAN owns it.  The stream is uploaded once per DEVICE on the first glp_witness_eval_device there (every ctx
// on that device — the map provers of one GPU — shares the copy) and freed by glp_witness_plan_destroy; destroying a ctx does not touch it.
// glp_witness_eval_device synchronises its stream before it returns, so a plan may be destroyed as soon as no call is running.
#include <hip/hip_runtime.h>
#include <mutex>
#include <new>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "glp_ctx.h"
#include "hash_state.h"
#include "witness_kernels.cuh"
#include "place_batch_kernels.cuh"

struct glp_witness_plan {
    glp_wit_compiled c;
    struct Resident { u32* stream; glp_wit_run* runs; u32* level_run; u64* dict; u32* eq; u32* zero; u32* part_level; };
    std::map<int, Resident> dev;          // device id -> resident copy
    std::mutex mu;
};

extern "C" int glp_witness_plan_create_ex(const uint64_t* prog, size_t prog_words, size_t n_inputs, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                                          const uint64_t* seg_bounds, size_t n_seg, glp_witness_plan** plan) {
    if (!plan) return GLP_E_INVALID;
    *plan = nullptr;
    glp_witness_plan* p = new (std::nothrow) glp_witness_plan();
    if (!p) return GLP_E_NOMEM;
    int rc;
    try {
        rc = glp_wit_compile_ex(prog, prog_words, n_inputs, n_values, eq_pairs, n_eq, seg_bounds, n_seg, p->c);
    } catch (const std::bad_alloc&) {
        rc = GLP_E_NOMEM;
    }
    if (rc != GLP_OK) { delete p; return rc; }
    *plan = p;
    return GLP_OK;
}

extern "C" int glp_witness_plan_create(const uint64_t* prog, size_t prog_words, size_t n_inputs, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                                       glp_witness_plan** plan) {
    return glp_witness_plan_create_ex(prog, prog_words, n_inputs, n_values, eq_pairs, n_eq, nullptr, 0, plan);
}

extern "C" void glp_witness_plan_destroy(glp_witness_plan* p) {
    if (!p) return;
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : p->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        hipFree(kv.second.stream); hipFree(kv.second.runs); hipFree(kv.second.level_run); hipFree(kv.second.dict); hipFree(kv.second.eq); hipFree(kv.second.zero);
        hipFree(kv.second.part_level);
    }
    if (have_cur && !p->dev.empty()) hipSetDevice(cur);
    delete p;
}

extern "C" int glp_witness_plan_stats(const glp_witness_plan* p, uint64_t* n_ops, uint64_t* depth, uint64_t* steps, uint64_t* stream_bytes) {
    if (!p) return GLP_E_INVALID;
    if (n_ops) *n_ops = p->c.n_ops;
    if (depth) *depth = p->c.depth;
    if (steps) *steps = p->c.steps;
    if (stream_bytes) *stream_bytes = p->c.stream_bytes();
    return GLP_OK;
}

extern "C" int glp_witness_plan_parts(const glp_witness_plan* p, uint32_t* n_parts, uint64_t* ops, uint64_t* depth, uint64_t* steps) {
    if (!p || !n_parts) return GLP_E_INVALID;
    const uint32_t cap = *n_parts, n = (uint32_t)p->c.parts.size();
    *n_parts = n;
    for (uint32_t s = 0; s < n && s < cap; s++) {
        if (ops) ops[s] = p->c.parts[s].n_ops;
        if (depth) depth[s] = p->c.parts[s].depth;
        if (steps) steps[s] = p->c.parts[s].steps;
    }
    return GLP_OK;
}

extern "C" int glp_witness_plan_run_host(const glp_witness_plan* p, const uint64_t* h_rc, const uint64_t* h_mds_circ, const uint64_t* h_mds_diag,
                                         const uint64_t* inputs, size_t n_inputs, uint64_t* values, size_t n_values, size_t* first_bad) {
    if (!p || !h_rc || !h_mds_circ || !h_mds_diag || !values || (!inputs && n_inputs) || n_inputs != p->c.n_inputs || n_values != p->c.n_values)
        return GLP_E_INVALID;
    // the validity rules of glp_set_poseidon_constants / the host verifiers: canonical words; the fast MDS path for small entries
    u64 all[384];
    unsigned __int128 sum = 0;
    u64 maxdiag = 0;
    bool small = true;
    for (int i = 0; i < 360; i++) { if (h_rc[i] >= GL_P) return GLP_E_INVALID; all[i] = h_rc[i]; }
    for (int i = 0; i < 12; i++) {
        if (h_mds_circ[i] >= GL_P || h_mds_diag[i] >= GL_P) return GLP_E_INVALID;
        all[360 + i] = h_mds_circ[i]; all[372 + i] = h_mds_diag[i];
        sum += h_mds_circ[i];
        if (h_mds_diag[i] > maxdiag) maxdiag = h_mds_diag[i];
        if (h_mds_circ[i] >> 24 || h_mds_diag[i] >> 24) small = false;
    }
    if (sum + maxdiag >= ((unsigned __int128)1 << 24)) small = false;
    const GlpPoseidonConsts pk{all, all + 360, all + 372, nullptr, nullptr};
    const glp_wit_view v = p->c.view();
    return small ? glp_wit_run_host<true>(v, pk, inputs, values, first_bad) : glp_wit_run_host<false>(v, pk, inputs, values, first_bad);
}

template <typename T>
static hipError_t upload_vec(const std::vector<T>& h, T** d) {
    hipError_t e = hipMalloc((void**)d, h.size() * sizeof(T) + 16);
    if (e != hipSuccess) return e;
    return h.empty() ? hipSuccess : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

extern "C" int glp_witness_eval_device(glp_ctx* c, const glp_witness_plan* plan_c, const uint64_t* d_inputs, uint64_t* d_values, size_t value_stride,
                                       uint32_t B, int32_t* h_status, uint64_t* h_first_bad) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    glp_witness_plan* plan = const_cast<glp_witness_plan*>(plan_c);
    if (!plan || !h_status || !h_first_bad || (B && (!d_values || (!d_inputs && plan->c.n_inputs))) || value_stride < plan->c.n_values) {
        glp_set_err(c, "glp_witness_eval_device: bad argument (value_stride must be >= the plan's n_values)");
        return GLP_E_INVALID;
    }
    glp_hash_state* h = glp_hash_get(c);
    if (!h->have_consts) { glp_set_err(c, "glp_witness_eval_device: Poseidon constants not set"); return GLP_E_STATE; }
    if (B == 0) return GLP_OK;
    glp_witness_plan::Resident res;
    {
        std::lock_guard<std::mutex> g(plan->mu);
        auto it = plan->dev.find(c->device);
        if (it == plan->dev.end()) {
            glp_witness_plan::Resident r{};
            hipError_t e = upload_vec(plan->c.stream, &r.stream);            // blocking copies: resident before any stream can use it
            if (e == hipSuccess) e = upload_vec(plan->c.runs, &r.runs);
            if (e == hipSuccess) e = upload_vec(plan->c.level_run, &r.level_run);
            if (e == hipSuccess) e = upload_vec(plan->c.dict, &r.dict);
            if (e == hipSuccess) e = upload_vec(plan->c.eq, &r.eq);
            if (e == hipSuccess) e = upload_vec(plan->c.zero, &r.zero);
            if (e == hipSuccess) e = upload_vec(plan->c.part_level, &r.part_level);
            if (e != hipSuccess) {
                hipFree(r.stream); hipFree(r.runs); hipFree(r.level_run); hipFree(r.dict); hipFree(r.eq); hipFree(r.zero); hipFree(r.part_level);
                glp_set_err(c, "glp_witness_eval_device: uploading the plan: %s", hipGetErrorString(e));
                return e == hipErrorOutOfMemory ? GLP_E_NOMEM : GLP_E_HIP;
            }
            it = plan->dev.emplace(c->device, r).first;
        }
        res = it->second;
    }
    glp_wit_view v = plan->c.view();
    v.stream = res.stream; v.runs = res.runs; v.level_run = res.level_run; v.dict = res.dict; v.eq = res.eq; v.zero = res.zero;
    // per-instance verdicts: [B] first_bad (u64) then [B] status (i32)
    GlpPoolBuf out(c);
    if (out.alloc((size_t)B * 12 + 16) != hipSuccess) return GLP_E_NOMEM;
    unsigned long long* d_bad = (unsigned long long*)out.p;
    int* d_status = (int*)(d_bad + B);
    int cus = 0;
    GLP_HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const u32 grid = B < (u32)(cus > 0 ? cus : 1) ? B : (u32)(cus > 0 ? cus : 1);     // one resident workgroup per CU; more instances: grid-stride
    const GlpPoseidonConsts pk = glp_dev_consts(h);
    const u32 n_parts = (u32)plan->c.parts.size();
    if (n_parts > 1) {
        // prefix | all segments | tail + copy constraints: three launches, ordered by the stream alone
        const u32 n_seg = n_parts - 2;
        const u64 seg_pairs = (u64)B * n_seg, seg_cap = 4ull * (u32)(cus > 0 ? cus : 1);
        const u32 seg_grid = (u32)(seg_pairs < seg_cap ? seg_pairs : seg_cap);
        const struct { u32 lo, n, grid; int first, last; } launch[3] = {{0, 1, grid, 1, 0}, {1, n_seg, seg_grid, 0, 0}, {n_parts - 1, 1, grid, 0, 1}};
        for (const auto& L : launch) {
            if (h->small_mds)
                hipLaunchKernelGGL(glp_witness_eval_part_kernel<true>, dim3(L.grid), dim3(GLP_WIT_WG), 0, c->stream, v, res.part_level, L.lo, L.n, L.first,
                                   L.last, d_inputs, d_values, (u64)value_stride, B, d_status, d_bad, pk);
            else
                hipLaunchKernelGGL(glp_witness_eval_part_kernel<false>, dim3(L.grid), dim3(GLP_WIT_WG), 0, c->stream, v, res.part_level, L.lo, L.n, L.first,
                                   L.last, d_inputs, d_values, (u64)value_stride, B, d_status, d_bad, pk);
            GLP_HIPCHK(c, hipGetLastError());
        }
    } else if (h->small_mds)
        hipLaunchKernelGGL(glp_witness_eval_kernel<true>, dim3(grid), dim3(GLP_WIT_WG), 0, c->stream, v, d_inputs, d_values, (u64)value_stride, B, d_status,
                           d_bad, pk);
    else
        hipLaunchKernelGGL(glp_witness_eval_kernel<false>, dim3(grid), dim3(GLP_WIT_WG), 0, c->stream, v, d_inputs, d_values, (u64)value_stride, B, d_status,
                           d_bad, pk);
    GLP_HIPCHK(c, hipGetLastError());
    std::vector<unsigned char> host((size_t)B * 12);
    GLP_HIPCHK(c, hipMemcpyAsync(host.data(), out.p, host.size(), hipMemcpyDeviceToHost, c->stream));
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long* hb = (const unsigned long long*)host.data();
    const int* hs = (const int*)(hb + B);
    for (u32 b = 0; b < B; b++) {
        // the host's order: a refused op first (no pair index), then the lowest failing copy constraint
        if (hs[b] != GLP_OK) { h_status[b] = hs[b]; h_first_bad[b] = ~0ull; }
        else if (hb[b] != ~0ull) { h_status[b] = GLP_E_REJECT; h_first_bad[b] = hb[b]; }
        else { h_status[b] = GLP_OK; h_first_bad[b] = ~0ull; }
    }
    return GLP_OK;
}

extern "C" int glp_witness_check_words_host(const uint64_t* values, size_t value_stride, uint32_t B, const uint32_t* var_idx, const uint64_t* var_want,
                                            uint32_t n_var, const uint32_t* bit_vars, const uint32_t* bit_start, const uint64_t* bit_want, uint32_t n_bits,
                                            uint64_t* first_bad_var, uint64_t* first_bad_bits) {
    if (!first_bad_var || !first_bad_bits || (B && !values) || (n_var && (!var_idx || (B && !var_want))) ||
        (n_bits && (!bit_vars || !bit_start || (B && !bit_want))) || (u64)n_var + n_bits > 0xFFFFFFFFull)
        return GLP_E_INVALID;
    for (u32 j = 0; j < n_bits; j++) if (bit_start[j] > bit_start[j + 1]) return GLP_E_INVALID;
    glp_wit_check_words_host(glp_wit_words{var_idx, bit_vars, bit_start, n_var, n_bits}, values, value_stride, B, var_want, bit_want, first_bad_var,
                             first_bad_bits);
    return GLP_OK;
}

extern "C" int glp_witness_check_words(glp_ctx* c, const uint64_t* d_values, size_t value_stride, uint32_t B, const uint32_t* d_var_idx,
                                       const uint64_t* d_var_want, uint32_t n_var, const uint32_t* d_bit_vars, const uint32_t* d_bit_start,
                                       const uint64_t* d_bit_want, uint32_t n_bits, uint64_t* h_first_bad_var, uint64_t* h_first_bad_bits) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    if (!h_first_bad_var || !h_first_bad_bits || (B && !d_values) || (n_var && (!d_var_idx || !d_var_want)) ||
        (n_bits && (!d_bit_vars || !d_bit_start || !d_bit_want)) || (u64)n_var + n_bits > 0xFFFFFFFFull) {
        glp_set_err(c, "glp_witness_check_words: bad argument");
        return GLP_E_INVALID;
    }
    for (u32 b = 0; b < B; b++) h_first_bad_var[b] = h_first_bad_bits[b] = ~0ull;
    const u64 total = (u64)B * ((u64)n_var + n_bits);
    if (total == 0) return GLP_OK;
    GlpPoolBuf out(c);
    if (out.alloc((size_t)B * 16) != hipSuccess) return GLP_E_NOMEM;
    unsigned long long* d_bad = (unsigned long long*)out.p;
    GLP_HIPCHK(c, hipMemsetAsync(d_bad, 0xFF, (size_t)B * 16, c->stream));
    const u64 blocks = (total + 255) / 256;
    const u32 grid = (u32)(blocks < 4096 ? blocks : 4096);
    hipLaunchKernelGGL(glp_witness_check_words_kernel, dim3(grid), dim3(256), 0, c->stream, glp_wit_words{d_var_idx, d_bit_vars, d_bit_start, n_var, n_bits},
                       d_values, (u64)value_stride, B, d_var_want, d_bit_want, d_bad, d_bad + B);
    GLP_HIPCHK(c, hipGetLastError());
    std::vector<unsigned long long> host((size_t)B * 2);
    GLP_HIPCHK(c, hipMemcpyAsync(host.data(), d_bad, host.size() * 8, hipMemcpyDeviceToHost, c->stream));
    GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
    for (u32 b = 0; b < B; b++) { h_first_bad_var[b] = host[b]; h_first_bad_bits[b] = host[B + b]; }
    return GLP_OK;
}

// ---- batched witness placement ------------------------------------------------------------------------------------------------------------
// The LAYOUT of a recorded circuit: how the evaluated variables (and the fixed values behind them) become a wire matrix.  Host arrays, every
// index checked once in glp_witness_layout_create — the kernels of place_batch_kernels.cuh carry no flag.  OWNERSHIP of the device copy as for
// the plan above: uploaded on the first glp_witness_place_batch per DEVICE, shared by the ctxs of that device, freed by
// glp_witness_layout_destroy.
struct glp_witness_layout {
    u32 log_n = 0, W = 0;
    u64 n_src = 0;
    std::vector<u32> cell, pos_rows, sha_rows, sha_kinds, public_vars;
    struct Resident { u32* cell; u32* pos_rows; u32* sha_rows; u32* sha_kinds; u32* public_vars; };
    std::map<int, Resident> dev;
    std::mutex mu;
};

static int layout_refuse(char* err, size_t err_len, const char* fmt, ...) {
    if (err && err_len) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, err_len, fmt, ap);
        va_end(ap);
    }
    return GLP_E_INVALID;
}

extern "C" int glp_witness_layout_create(uint32_t log_n, uint32_t n_wires, const uint32_t* cell_index, size_t n_src, const uint32_t* pos_rows,
                                         uint32_t n_pos_rows, const uint32_t* sha_rows, const uint32_t* sha_kinds, uint32_t n_sha_rows,
                                         const uint32_t* public_vars, uint32_t n_public, glp_witness_layout** layout, char* err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    if (!layout) return GLP_E_INVALID;
    *layout = nullptr;
    if (log_n > 24 || n_wires == 0 || n_wires > 4096 || !cell_index || (!pos_rows && n_pos_rows) || ((!sha_rows || !sha_kinds) && n_sha_rows) ||
        (!public_vars && n_public))
        return layout_refuse(err, err_len, "glp_witness_layout_create: bad argument (log_n <= 24, 1 <= n_wires <= 4096, no null array with a non-zero count)");
    if ((u64)n_src >= 0xFFFFFFFFull) {
        layout_refuse(err, err_len, "glp_witness_layout_create: n_src = %zu does not fit the 32-bit cell index", n_src);
        return GLP_E_UNSUPPORTED;
    }
    const u64 n = 1ull << log_n, cells = (u64)n_wires * n;
    if (n_pos_rows && n_wires < GLP_POS_GATE_WIRES)
        return layout_refuse(err, err_len, "glp_witness_layout_create: %u wires, a Poseidon row needs %d", n_wires, (int)GLP_POS_GATE_WIRES);
    if (n_sha_rows && n_wires < GLP_SHA_GATE_WIRES)
        return layout_refuse(err, err_len, "glp_witness_layout_create: %u wires, a SHA row needs %d", n_wires, (int)GLP_SHA_GATE_WIRES);
    for (u64 i = 0; i < cells; i++)
        if (cell_index[i] != 0xFFFFFFFFu && cell_index[i] >= n_src)
            return layout_refuse(err, err_len, "glp_witness_layout_create: cell %llu (wire %llu, row %llu) names source %u of %zu", (unsigned long long)i,
                                 (unsigned long long)(i >> log_n), (unsigned long long)(i & (n - 1)), cell_index[i], n_src);
    for (u32 k = 0; k < n_pos_rows; k++)
        if (pos_rows[k] >= n) return layout_refuse(err, err_len, "glp_witness_layout_create: Poseidon row entry %u is row %u of %llu", k, pos_rows[k], (unsigned long long)n);
    for (u32 k = 0; k < n_sha_rows; k++) {
        if (sha_rows[k] >= n) return layout_refuse(err, err_len, "glp_witness_layout_create: SHA row entry %u is row %u of %llu", k, sha_rows[k], (unsigned long long)n);
        if (sha_kinds[k] > 3) return layout_refuse(err, err_len, "glp_witness_layout_create: SHA row entry %u has kind %u (0..3)", k, sha_kinds[k]);
    }
    for (u32 k = 0; k < n_public; k++)
        if (public_vars[k] >= n_src) return layout_refuse(err, err_len, "glp_witness_layout_create: public input %u names source %u of %zu", k, public_vars[k], n_src);
    glp_witness_layout* L = new (std::nothrow) glp_witness_layout();
    if (!L) return GLP_E_NOMEM;
    try {
        L->log_n = log_n; L->W = n_wires; L->n_src = n_src;
        L->cell.assign(cell_index, cell_index + cells);
        L->pos_rows.assign(pos_rows, pos_rows + n_pos_rows);
        L->sha_rows.assign(sha_rows, sha_rows + n_sha_rows);
        L->sha_kinds.assign(sha_kinds, sha_kinds + n_sha_rows);
        L->public_vars.assign(public_vars, public_vars + n_public);
    } catch (const std::bad_alloc&) {
        delete L;
        return GLP_E_NOMEM;
    }
    *layout = L;
    return GLP_OK;
}

extern "C" void glp_witness_layout_destroy(glp_witness_layout* L) {
    if (!L) return;
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : L->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        hipFree(kv.second.cell); hipFree(kv.second.pos_rows); hipFree(kv.second.sha_rows); hipFree(kv.second.sha_kinds); hipFree(kv.second.public_vars);
    }
    if (have_cur && !L->dev.empty()) hipSetDevice(cur);
    delete L;
}

extern "C" int glp_witness_layout_info(const glp_witness_layout* L, uint32_t* log_n, uint32_t* n_wires, uint64_t* n_src, uint32_t* n_pos_rows,
                                       uint32_t* n_sha_rows, uint32_t* n_public) {
    if (!L) return GLP_E_INVALID;
    if (log_n) *log_n = L->log_n;
    if (n_wires) *n_wires = L->W;
    if (n_src) *n_src = L->n_src;
    if (n_pos_rows) *n_pos_rows = (u32)L->pos_rows.size();
    if (n_sha_rows) *n_sha_rows = (u32)L->sha_rows.size();
    if (n_public) *n_public = (u32)L->public_vars.size();
    return GLP_OK;
}

extern "C" int glp_witness_last_place_counts(glp_ctx* c, uint32_t* n_launches, uint32_t* n_host_syncs) {
    if (!c) return GLP_E_INVALID;
    if (n_launches) *n_launches = c->place_counts[0];
    if (n_host_syncs) *n_host_syncs = c->place_counts[1];
    return GLP_OK;
}

constexpr u64 PLACE_MAX_BLOCKS = 0x7fffffffull;

extern "C" int glp_witness_place_batch(glp_ctx* c, const glp_witness_layout* layout_c, const uint64_t* d_values, size_t value_stride,
                                       const uint32_t* h_rows, uint32_t B, uint64_t* d_wires, size_t wire_stride_words, uint64_t* h_public) {
    if (!c) return GLP_E_INVALID;
    GLP_BIND(c);
    c->place_counts[0] = c->place_counts[1] = 0;
    if (B == 0) return GLP_OK;
    glp_witness_layout* L = const_cast<glp_witness_layout*>(layout_c);
    if (!L || !d_values || !h_rows || !d_wires) { glp_set_err(c, "glp_witness_place_batch: bad argument"); return GLP_E_INVALID; }
    const u64 n = 1ull << L->log_n, cells = (u64)L->W * n;
    if (value_stride < L->n_src || wire_stride_words < cells) {
        glp_set_err(c, "glp_witness_place_batch: value_stride must be >= the layout's n_src (%llu) and wire_stride_words >= n_wires * n (%llu)",
                    (unsigned long long)L->n_src, (unsigned long long)cells);
        return GLP_E_INVALID;
    }
    const u32 n_pos = (u32)L->pos_rows.size(), n_sha = (u32)L->sha_rows.size(), n_pub = (u32)L->public_vars.size();
    const u32 bpi_pos = (n_pos + 63) / 64, bpi_sha = (n_sha + 63) / 64;
    if ((u64)B * bpi_pos > PLACE_MAX_BLOCKS || (u64)B * bpi_sha > PLACE_MAX_BLOCKS) {
        glp_set_err(c, "glp_witness_place_batch: B = %u is more than one call takes at this size (a launch of more than 2^31 - 1 workgroups)", B);
        return GLP_E_UNSUPPORTED;
    }
    glp_hash_state* h = nullptr;
    if (n_pos) {
        h = glp_hash_get(c);
        if (!h->have_consts) { glp_set_err(c, "glp_witness_place_batch: Poseidon constants not set"); return GLP_E_STATE; }
    }
    glp_witness_layout::Resident res;
    {
        std::lock_guard<std::mutex> g(L->mu);
        auto it = L->dev.find(c->device);
        if (it == L->dev.end()) {
            glp_witness_layout::Resident r{};
            hipError_t e = upload_vec(L->cell, &r.cell);                       // blocking copies: resident before any stream can use it
            if (e == hipSuccess) e = upload_vec(L->pos_rows, &r.pos_rows);
            if (e == hipSuccess) e = upload_vec(L->sha_rows, &r.sha_rows);
            if (e == hipSuccess) e = upload_vec(L->sha_kinds, &r.sha_kinds);
            if (e == hipSuccess) e = upload_vec(L->public_vars, &r.public_vars);
            if (e != hipSuccess) {
                hipFree(r.cell); hipFree(r.pos_rows); hipFree(r.sha_rows); hipFree(r.sha_kinds); hipFree(r.public_vars);
                glp_set_err(c, "glp_witness_place_batch: uploading the layout: %s", hipGetErrorString(e));
                return e == hipErrorOutOfMemory ? GLP_E_NOMEM : GLP_E_HIP;
            }
            it = L->dev.emplace(c->device, r).first;
        }
        res = it->second;
    }
    // the slab-row table: through pinned staging of the ctx, so that the copy is asynchronous and the caller's h_rows is done with on return
    if (!c->place_ev) GLP_HIPCHK(c, hipEventCreateWithFlags(&c->place_ev, hipEventDisableTiming));
    else GLP_HIPCHK(c, hipEventSynchronize(c->place_ev));                     // the previous call's 4 * B-byte copy: long done unless calls follow back to back
    if (c->place_rows_cap < B) {
        if (c->place_rows_host) { hipHostFree(c->place_rows_host); c->place_rows_host = nullptr; c->place_rows_cap = 0; }
        const size_t cap = B < 64 ? 64 : (size_t)B;
        if (hipHostMalloc((void**)&c->place_rows_host, cap * 4, hipHostMallocDefault) != hipSuccess) {
            c->place_rows_host = nullptr;
            glp_set_err(c, "glp_witness_place_batch: no pinned staging for %u slab rows", B);
            return GLP_E_NOMEM;
        }
        c->place_rows_cap = cap;
    }
    memcpy(c->place_rows_host, h_rows, (size_t)B * 4);
    const bool want_public = h_public && n_pub;
    const size_t pub_bytes = want_public ? (size_t)B * n_pub * 8 : 0;
    GlpPoolBuf tmp(c);                                                          // [B * n_public] public values, then [B] slab rows
    if (tmp.alloc(pub_bytes + (size_t)B * 4 + 16) != hipSuccess) return GLP_E_NOMEM;
    u64* d_pub = tmp.u();
    u32* d_rows = (u32*)((unsigned char*)tmp.p + pub_bytes);
    GLP_HIPCHK(c, hipMemcpyAsync(d_rows, c->place_rows_host, (size_t)B * 4, hipMemcpyHostToDevice, c->stream));
    GLP_HIPCHK(c, hipEventRecord(c->place_ev, c->stream));
    u32 launches = 0;
    {
        const u64 want = (cells + 255) / 256;
        const u32 grid = (u32)(want < 4096 ? want : 4096);
        hipLaunchKernelGGL(glp_witness_place_batch_kernel<0>, dim3(grid), dim3(256), 0, c->stream, d_wires, (u64)wire_stride_words, d_values, (u64)value_stride,
                           d_rows, B, res.cell, cells);
        GLP_HIPCHK(c, hipGetLastError());
        launches++;
    }
    if (n_pos) {
        if (h->small_mds && !getenv("GLP_K7_GENERIC_MDS"))                      // the choice glp_poseidon_gate_fill_rows makes
            hipLaunchKernelGGL(glp_poseidon_gate_fill_batch_kernel<1>, dim3(B * bpi_pos), dim3(64), 0, c->stream, d_wires, (u64)wire_stride_words, n,
                               res.pos_rows, n_pos, bpi_pos, h->d_consts);
        else
            hipLaunchKernelGGL(glp_poseidon_gate_fill_batch_kernel<0>, dim3(B * bpi_pos), dim3(64), 0, c->stream, d_wires, (u64)wire_stride_words, n,
                               res.pos_rows, n_pos, bpi_pos, h->d_consts);
        GLP_HIPCHK(c, hipGetLastError());
        launches++;
    }
    if (n_sha) {
        hipLaunchKernelGGL(glp_sha_gate_fill_batch_kernel<0>, dim3(B * bpi_sha), dim3(64), 0, c->stream, d_wires, (u64)wire_stride_words, n, res.sha_rows,
                           res.sha_kinds, n_sha, bpi_sha);
        GLP_HIPCHK(c, hipGetLastError());
        launches++;
    }
    c->place_counts[0] = launches;
    if (want_public) {
        const u64 want = ((u64)B * n_pub + 255) / 256;
        const u32 grid = (u32)(want < 4096 ? want : 4096);
        hipLaunchKernelGGL(glp_witness_public_batch_kernel<0>, dim3(grid), dim3(256), 0, c->stream, d_pub, d_values, (u64)value_stride, d_rows, B,
                           res.public_vars, n_pub);
        GLP_HIPCHK(c, hipGetLastError());
        c->place_counts[0] = ++launches;
        GLP_HIPCHK(c, hipMemcpyAsync(h_public, d_pub, pub_bytes, hipMemcpyDeviceToHost, c->stream));
        GLP_HIPCHK(c, hipStreamSynchronize(c->stream));
        c->place_counts[1] = 1;
    }
    return GLP_OK;
}
