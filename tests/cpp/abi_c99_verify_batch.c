/* tests/cpp/abi_c99_verify_batch.c — the declarations of the batched verifiers are plain C: compiled with `gcc -std=c99 -pedantic -Wall -Werror`
 * and linked against libglprover.so by tests/test_emu_verify_batch.py.  It takes the addresses of the device calls and runs what needs no GPU:
 * the reason table, and glp_fri_verify_batch_host on a two-word "proof" (refused as truncated), on B = 0 and on a null table. */
#include <stdio.h>
#include <string.h>
#include "glprover.h"

int main(void) {
    int (*pb)(glp_ctx*, const uint8_t* const*, const size_t*, uint32_t, const uint64_t*, size_t, const uint64_t*, size_t, uint32_t, uint32_t,
              glp_verify_verdict*, uint64_t*) = glp_plonk_verify_batch;
    int (*fb)(glp_ctx*, const uint8_t* const*, const size_t*, uint32_t, uint32_t, uint32_t, uint32_t, glp_verify_verdict*, glp_fri_statement*) =
        glp_fri_verify_batch;
    int (*counts)(glp_ctx*, uint32_t*, uint32_t*, uint32_t*, uint32_t*) = glp_verify_last_batch_counts;
    uint64_t rc[360], circ[12], diag[12], words[2] = {1, 2};
    const uint8_t* proofs[1];
    size_t lens[1] = {16};
    glp_verify_verdict v;
    uint32_t n_dev = 9, n_fb = 9;
    int i, ok;
    for (i = 0; i < 360; i++) rc[i] = (uint64_t)i + 1;
    for (i = 0; i < 12; i++) { circ[i] = (uint64_t)i + 1; diag[i] = 1; }
    proofs[0] = (const uint8_t*)words;
    memset(&v, 0xFF, sizeof(v));
    ok = glp_fri_verify_batch_host(rc, circ, diag, proofs, lens, 1, 1, 0, 1, &v, 0, &n_dev, &n_fb) == GLP_OK;
    ok = ok && v.status == GLP_E_REJECT && v.reason == GLP_VR_TRUNCATED && v.query == 0xFFFFFFFFu && v.on_device == 0 && n_dev == 0 && n_fb == 0;
    ok = ok && glp_fri_verify_batch_host(rc, circ, diag, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0) == GLP_OK;
    ok = ok && glp_fri_verify_batch_host(rc, circ, diag, 0, lens, 1, 1, 0, 1, &v, 0, 0, 0) == GLP_E_INVALID;
    ok = ok && glp_plonk_verify_batch_host(rc, circ, diag, proofs, lens, 1, 0, 0, 0, 0, 1, 0, &v, 0, 0, 0) == GLP_OK && v.reason == GLP_VR_TRUNCATED;
    ok = ok && strcmp(glp_verify_reason_text(GLP_VR_TRUNCATED), "truncated") == 0 && strcmp(glp_verify_reason_text(GLP_VR_IDENTITY), "PLONK identity fails at zeta") == 0;
    ok = ok && glp_verify_reason_text(GLP_VR_NONE)[0] == 0 && glp_verify_reason_text(GLP_VR_COUNT)[0] == 0;
    printf("verdict %d %s size %lu ok %d linked %d\n", (int)v.status, glp_verify_reason_text(v.reason), (unsigned long)sizeof(glp_verify_verdict), ok,
           pb && fb && counts);
    return ok ? 0 : 1;
}
