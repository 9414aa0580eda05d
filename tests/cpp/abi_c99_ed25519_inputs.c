/* tests/cpp/abi_c99_ed25519_inputs.c — the declarations of glp_ed25519_leaf_inputs and glp_ed25519_half_scalars are plain C: compiled with
 * `gcc -std=c99 -pedantic -Wall -Werror` and linked against libglprover.so by tests/test_emu_ed25519_inputs.py.  It takes the addresses of the
 * two device calls and runs glp_ed25519_leaf_input_words, which needs no GPU, on the three forms and on layouts no statement has. */
#include <stdio.h>
#include "glprover.h"

int main(void) {
    int (*leaf)(glp_ctx*, const glp_ed25519_input_layout*, const uint8_t*, const uint8_t*, const uint8_t*, uint32_t, const uint32_t*, const uint8_t*,
                const uint8_t*, uint64_t, uint64_t*, size_t, int32_t*) = glp_ed25519_leaf_inputs;
    int (*half)(glp_ctx*, const uint64_t*, uint64_t, uint64_t*) = glp_ed25519_half_scalars;
    int (*counts)(glp_ctx*, uint32_t*, uint32_t*) = glp_ed25519_last_input_counts;
    glp_ed25519_input_layout l;
    uint64_t w[3] = {0, 0, 0}, none = 7;
    int bad;
    l.form = GLP_ED25519_FORM_PLAIN; l.msg_len_min = 112; l.msg_len_max = 112; l.split_scalars = 0;
    if (glp_ed25519_leaf_input_words(&l, &w[0]) != GLP_OK) return 1;
    l.form = GLP_ED25519_FORM_FLAGGED; l.split_scalars = 1;
    if (glp_ed25519_leaf_input_words(&l, &w[1]) != GLP_OK) return 1;
    l.form = GLP_ED25519_FORM_VOTE; l.msg_len_min = 104; l.msg_len_max = 110;
    if (glp_ed25519_leaf_input_words(&l, &w[2]) != GLP_OK) return 1;
    l.msg_len_min = 111;
    bad = glp_ed25519_leaf_input_words(&l, &none) == GLP_E_INVALID;
    l.form = 3; l.msg_len_min = 104;
    bad = bad && glp_ed25519_leaf_input_words(&l, &none) == GLP_E_INVALID && glp_ed25519_leaf_input_words(0, &none) == GLP_E_INVALID && none == 7;
    printf("words %lu %lu %lu refused %d linked %d\n", (unsigned long)w[0], (unsigned long)w[1], (unsigned long)w[2], bad, leaf && half && counts);
    return bad ? 0 : 1;
}
