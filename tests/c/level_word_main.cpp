// level_word_main.cpp -- bgz::level_with_search (csrc/fc2_bgzf_gpu.h), the word that carries level 2's search effort
// and passes through bgz::gpu_open's `level` argument, alone in a host program: one line "depth nice passes word" per
// setting on the command line's grid, for tests/test_deflate_priced_abi.py to take apart again.
#include <stdio.h>

#include "../../find_circ2_amd/csrc/fc2_bgzf_gpu.h"

using fc2::bgz::level_with_search;

static_assert(level_with_search(0, 0) == 2 && level_with_search(0, 0, 0) == 2 && level_with_search(0, 0, 1) == 2,
              "no search and one pass: the plain level");
static_assert(level_with_search(32, 258, 1) == level_with_search(32, 258) && level_with_search(32, 258, 0) == level_with_search(32, 258),
              "one pass is the two-argument word");
static_assert(level_with_search(128, 258, 3) > 0, "the word stays a positive int");

int main() {
    const unsigned depths[] = {0, 1, 8, 32, 128}, nices[] = {4, 32, 258}, passes[] = {0, 1, 2, 3};
    for (unsigned d : depths)
        for (unsigned n : nices)
            for (unsigned p : passes) printf("%u %u %u %d\n", d, n, p, level_with_search(d, n, p));
    return 0;
}
