// grad_max_check.cpp -- the one-element rule of the max-mode backward (csrc/pimemb_grad_max.h, the text the kernels compile) on the HOST.
//   grad_max_check <fp32 bits, hex>...
// Walks the values as the good positions 0, 1, 2, ... of one bag through max_visit and prints the winner after each;
// tests/test_grad_max_cpu.py compares the line with tests/grad_max_ref.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pimemb_grad_max.h"

using namespace pimemb_grad;

int main(int argc, char **argv) {
    float cur = 0.f;
    uint32_t win = kMaxNoWinner;
    for (int p = 1; p < argc; p++) {
        max_visit(bits_f32((uint32_t)strtoul(argv[p], nullptr, 16)), (uint32_t)(p - 1), &cur, &win);
        printf("%u ", win);
    }
    printf("\n%u %08x\n", max_pick(3, 3, -0.f) == 0.f ? 1u : 0u, f32_bits(max_pick(3, 4, -1.f)));
    return 0;
}
