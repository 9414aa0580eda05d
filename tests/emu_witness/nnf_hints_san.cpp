// tests/emu_witness/nnf_hints_san.cpp — TEST INFRASTRUCTURE.  csrc/nnf25519.h ALONE as an ordinary program, built with AddressSanitizer + UBSan
// (make sanitized).  Reads operand rows from stdin — 22 decimal words, a0..a10 b0..b10 — and prints for each one line: the verdict of
// glp_nnf::mul_hints (1 accepted, 0 refused), then its 44 words (zeros when refused).  tests/test_witness_ops_edge.py compares the lines with
// tests/witness_ref.py; a sanitizer report ends the program with a non-zero status.  Never part of the product.
#include <stdio.h>
#include <inttypes.h>
#include "../../0-kno-blobstreamx_amd/csrc/nnf25519.h"

int main() {
    for (;;) {
        uint64_t ab[2 * GLP_NNF_LIMBS], out[GLP_NNF_OUT];
        for (int i = 0; i < 2 * GLP_NNF_LIMBS; i++)
            if (scanf("%" SCNu64, &ab[i]) != 1) return i == 0 && feof(stdin) ? 0 : 2;      // a partial row is an error
        for (int i = 0; i < GLP_NNF_OUT; i++) out[i] = 0;
        const bool ok = glp_nnf::mul_hints(ab, ab + GLP_NNF_LIMBS, out);
        printf("%d", ok ? 1 : 0);
        for (int i = 0; i < GLP_NNF_OUT; i++) printf(" %" PRIu64, ok ? out[i] : (uint64_t)0);
        printf("\n");
    }
}
