/* tests/cpp/abi_c99_tm_proofs.c — the declarations of glp_tm_forest_* and glp_tm_verify_inclusion_batch are plain C: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` and linked against libglprover.so by tests/test_emu_tm_proofs.py.  It takes the addresses of the
 * device calls and runs what needs no GPU: glp_tm_forest_proofs_host on one tree of five leaves (leaf i = i + 1 bytes of value i), every leaf
 * in numbering order, then glp_tm_verify_inclusion_batch_host on the five proofs, on a changed leaf byte, on a wrong aunt count, and a query
 * past the tree (refused). */
#include <stdio.h>
#include <string.h>
#include "glprover.h"

int main(void) {
    int (*create)(glp_ctx*, const uint8_t*, uint64_t, const uint64_t*, const uint64_t*, uint64_t, uint64_t, uint8_t*, glp_tm_forest**) = glp_tm_forest_create;
    int (*info)(const glp_tm_forest*, uint64_t*, uint64_t*, uint32_t*, uint64_t*) = glp_tm_forest_info;
    int (*roots)(const glp_tm_forest*, const uint8_t**) = glp_tm_forest_roots;
    int (*destroy)(glp_tm_forest*) = glp_tm_forest_destroy;
    int (*proofs)(glp_ctx*, const glp_tm_forest*, const uint64_t*, const uint64_t*, uint64_t, uint8_t*, uint32_t, uint32_t*, uint8_t*) = glp_tm_forest_proofs;
    int (*verify)(glp_ctx*, const uint8_t*, uint64_t, const uint32_t*, const uint8_t*, uint64_t, const uint64_t*, const uint64_t*, const uint64_t*,
                  const uint8_t*, uint32_t, const uint32_t*, uint64_t, int32_t*) = glp_tm_verify_inclusion_batch;
    int (*counts)(glp_ctx*, uint32_t*, uint32_t*) = glp_tm_forest_last_counts;
    uint8_t data[15], root[32], aunts[5 * 3 * 32], hashes[5 * 32];
    uint64_t offs[6], first[2] = {0, 5}, index[5], total[5], qt[1] = {0}, ql[1] = {5};
    uint32_t n_aunts[5];
    int32_t status[5], tampered, shape;
    int i, j, k = 0, refused;
    offs[0] = 0;
    for (i = 0; i < 5; i++) {
        for (j = 0; j <= i; j++) data[k++] = (uint8_t)i;
        offs[i + 1] = (uint64_t)k;
        index[i] = (uint64_t)i;
        total[i] = 5;
    }
    if (!(create && info && roots && destroy && proofs && verify && counts)) return 1;
    if (glp_tm_forest_proofs_host(data, 15, offs, first, 5, 1, 0, 0, 5, root, aunts, 3, n_aunts, hashes) != GLP_OK) return 1;
    if (glp_tm_verify_inclusion_batch_host(root, 1, 0, data, 15, offs, index, total, aunts, 3, n_aunts, 5, status) != GLP_OK) return 1;
    printf("aunts");
    for (i = 0; i < 5; i++) printf(" %u", (unsigned)n_aunts[i]);
    printf(" root ");
    for (i = 0; i < 32; i++) printf("%02x", root[i]);
    printf(" status");
    for (i = 0; i < 5; i++) printf(" %d", (int)status[i]);
    data[14] ^= 1;                                           /* leaf 4 */
    if (glp_tm_verify_inclusion_batch_host(root, 1, 0, data, 15, offs, index, total, aunts, 3, n_aunts, 5, status) != GLP_OK) return 1;
    tampered = status[4];
    data[14] ^= 1;
    n_aunts[4] = 2;
    if (glp_tm_verify_inclusion_batch_host(root, 1, 0, data, 15, offs, index, total, aunts, 3, n_aunts, 5, status) != GLP_OK) return 1;
    shape = status[4];
    memset(aunts, 0xEE, sizeof(aunts));
    refused = glp_tm_forest_proofs_host(data, 15, offs, first, 5, 1, qt, ql, 1, root, aunts, 3, n_aunts, hashes) == GLP_E_INVALID && aunts[0] == 0xEE;
    printf(" tampered %d shape %d refused %d\n", (int)tampered, (int)shape, refused);
    return tampered == GLP_TM_INCLUSION_BAD_ROOT && shape == GLP_TM_INCLUSION_BAD_SHAPE && refused ? 0 : 1;
}
