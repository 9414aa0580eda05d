/* tests/cpp/abi_c99_chain_inputs.c — the declarations of glp_tm_merkle_root_batch and glp_header_chain_leaf_inputs are plain C: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` and linked against libglprover.so by tests/test_emu_chain_inputs.py.  It takes the addresses of the
 * device calls and runs what needs no GPU: glp_header_chain_leaf_input_words on the default layout and on layouts no leaf statement has,
 * glp_tm_merkle_root_batch_host on one tree without leaves, glp_header_chain_leaf_inputs_host on one all-zero header (which does not link). */
#include <stdio.h>
#include <string.h>
#include "glprover.h"

int main(void) {
    int (*batch)(glp_ctx*, const uint8_t*, uint64_t, const uint64_t*, const uint64_t*, uint64_t, uint64_t, uint8_t*, uint8_t*) = glp_tm_merkle_root_batch;
    int (*inputs)(glp_ctx*, const glp_header_chain_layout*, const uint8_t*, const uint8_t*, uint64_t, uint64_t, uint64_t*, size_t, uint8_t*, int32_t*) =
        glp_header_chain_leaf_inputs;
    int (*counts)(glp_ctx*, uint32_t*, uint32_t*) = glp_header_chain_last_input_counts;
    int (*bcounts)(glp_ctx*, uint32_t*, uint32_t*) = glp_tm_merkle_root_batch_last_counts;
    static const uint32_t lens[14] = {4, 12, 5, 13, 72, 34, 34, 34, 34, 34, 34, 34, 34, 22};
    static uint8_t header[400];
    static uint64_t row[512];
    glp_header_chain_layout l;
    uint64_t w = 0, none = 7, offs[1] = {0}, first[2] = {0, 0};
    uint8_t root[32], start[32];
    int32_t status = -1;
    int bad, i;
    memcpy(l.field_len, lens, sizeof(lens));
    l.leaf_headers = 8; l.n_groups = 4;
    if (glp_header_chain_leaf_input_words(&l, &w) != GLP_OK) return 1;
    l.field_len[6] = 33;
    bad = glp_header_chain_leaf_input_words(&l, &none) == GLP_E_INVALID;
    l.field_len[6] = 34; l.n_groups = 8;
    bad = bad && glp_header_chain_leaf_input_words(&l, &none) == GLP_E_INVALID && glp_header_chain_leaf_input_words(0, &none) == GLP_E_INVALID && none == 7;
    if (glp_tm_merkle_root_batch_host(0, 0, offs, first, 0, 1, root) != GLP_OK) return 1;
    l.n_groups = 4; l.leaf_headers = 1;
    memset(start, 0, sizeof(start));
    if (glp_header_chain_leaf_inputs_host(&l, header, start, 1u << 21, 1, row, 512, 0, &status) != GLP_OK) return 1;
    printf("words %lu refused %d linked %d empty ", (unsigned long)w, bad, batch && inputs && counts && bcounts);
    for (i = 0; i < 32; i++) printf("%02x", root[i]);
    printf(" status %d\n", (int)status);
    return bad ? 0 : 1;
}
