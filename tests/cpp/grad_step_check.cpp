// grad_step_check.cpp -- the one-element SGD step of the backward pass (csrc/pimemb_grad_step.h, the text the kernels compile) on
// the HOST.
//   grad_step_check <f32|f16|bf16> <lr: fp32 bits, hex> <in: stored elements> <in: float32 gradients> <out: stored elements>
// Reads table elements as the dtype stores them (4 or 2 bytes each) and as many fp32 gradients, and writes step(dtype, stored,
// g, lr) per element; tests/test_grad_cpu.py compares the bytes with tests/grad_ref.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pimemb_grad_step.h"

using namespace pimemb_grad;

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int dtype = !strcmp(argv[1], "f32") ? kStepF32 : !strcmp(argv[1], "f16") ? kStepF16 : !strcmp(argv[1], "bf16") ? kStepBF16 : -1;
    if (dtype < 0) return 2;
    const float lr = bits_f32((uint32_t)strtoul(argv[2], nullptr, 16));
    FILE *in_w = fopen(argv[3], "rb"), *in_g = fopen(argv[4], "rb"), *out = fopen(argv[5], "wb");
    if (!in_w || !in_g || !out) return 2;
    const size_t esz = dtype == kStepF32 ? 4 : 2;
    for (;;) {
        uint32_t stored = 0;
        float g;
        if (fread(&stored, esz, 1, in_w) != 1) break;
        if (fread(&g, 4, 1, in_g) != 1) return 3;
        const uint32_t o = step(dtype, stored, g, lr);
        fwrite(&o, esz, 1, out);
    }
    fclose(out);
    return 0;
}
