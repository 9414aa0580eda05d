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
    struct Resident { u32* stream; glp_wit_run* runs; u32* level_run; u64* dict; u32* eq; u32* zero; };
    std::map<int, Resident> dev;          // device id -> resident copy
    std::mutex mu;
};

extern "C" int glp_witness_plan_create(const uint64_t* prog, size_t prog_words, size_t n_inputs, size_t n_values, const uint64_t* eq_pairs, size_t n_eq,
                                       glp_witness_plan** plan) {
    if (!plan) return GLP_E_INVALID;
    *plan = nullptr;
    glp_witness_plan* p = new (std::nothrow) glp_witness_plan();
    if (!p) return GLP_E_NOMEM;
    int rc;
    try {
        rc = glp_wit_compile(prog, prog_words, n_inputs, n_values, eq_pairs, n_eq, p->c);
    } catch (const std::bad_alloc&) {
        rc = GLP_E_NOMEM;
    }
    if (rc != GLP_OK) { delete p; return rc; }
    *plan = p;
    return GLP_OK;
}

extern "C" void glp_witness_plan_destroy(glp_witness_plan* p) {
    if (!p) return;
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : p->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        hipFree(kv.second.stream); hipFree(kv.second.runs); hipFree(kv.second.level_run); hipFree(kv.second.dict); hipFree(kv.second.eq); hipFree(kv.second.zero);
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
            if (e != hipSuccess) {
                hipFree(r.stream); hipFree(r.runs); hipFree(r.level_run); hipFree(r.dict); hipFree(r.eq); hipFree(r.zero);
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
    if (h->small_mds)
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
