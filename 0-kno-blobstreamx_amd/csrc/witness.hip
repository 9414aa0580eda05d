// witness.hip — the compiled witness plan (witness_plan.h) behind the C ABI, and its batched evaluation on the device (witness_kernels.cuh).
//
// OWNERSHIP of the device copy: the PLAN owns it.  The stream is uploaded once per DEVICE on the first glp_witness_eval_device there (every ctx
// on that device — the map provers of one GPU — shares the copy) and freed by glp_witness_plan_destroy; destroying a ctx does not touch it.
// glp_witness_eval_device synchronises its stream before it returns, so a plan may be destroyed as soon as no call is running.
#include <hip/hip_runtime.h>
#include <mutex>
#include <new>
#include "glp_ctx.h"
#include "hash_state.h"
#include "witness_kernels.cuh"

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
