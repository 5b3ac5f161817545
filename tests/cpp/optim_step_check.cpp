// optim_step_check.cpp -- the one-element arithmetic of the fused Adagrad steps (csrc/pimemb_grad_optim.h, the text the kernels
// compile) on the HOST.
//   optim_step_check adagrad <f32|f16|bf16> <lr: fp32 bits, hex> <eps: fp32 bits, hex> <in: stored elements> <in: float32 gradients>
//                            <in: float32 states> <out: stored elements> <out: float32 states>
//       per element: adagrad_step(dtype, stored, g, &S, lr, eps)
//   optim_step_check rowwise <f32|f16|bf16> <lr> <eps> <dim> <in: stored elements> <in: float32 gradients> <in: float32 states>
//                            <in: float32 tree sums v> <out: stored elements> <out: float32 states> <out: float32 step sizes>
//       per element: step = rowwise_step_size(v, dim, &S, lr, eps), then step(dtype, stored, g, step): the calls of the kernel's row-wise tail
// tests/test_optim_cpu.py compares the bytes with tests/optim_ref.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pimemb_grad_optim.h"

using namespace pimemb_grad;

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const bool rowwise = !strcmp(argv[1], "rowwise");
    if (!rowwise && strcmp(argv[1], "adagrad")) return 2;
    if (argc != (rowwise ? 13 : 10)) return 2;
    const int dtype = !strcmp(argv[2], "f32") ? kStepF32 : !strcmp(argv[2], "f16") ? kStepF16 : !strcmp(argv[2], "bf16") ? kStepBF16 : -1;
    if (dtype < 0) return 2;
    const float lr = bits_f32((uint32_t)strtoul(argv[3], nullptr, 16)), eps = bits_f32((uint32_t)strtoul(argv[4], nullptr, 16));
    int at = 5;
    const uint32_t dim = rowwise ? (uint32_t)strtoul(argv[at++], nullptr, 10) : 0;
    FILE *in_w = fopen(argv[at], "rb"), *in_g = fopen(argv[at + 1], "rb"), *in_s = fopen(argv[at + 2], "rb");
    at += 3;
    FILE *in_v = rowwise ? fopen(argv[at++], "rb") : nullptr;
    FILE *out_w = fopen(argv[at], "wb"), *out_s = fopen(argv[at + 1], "wb");
    FILE *out_step = rowwise ? fopen(argv[at + 2], "wb") : nullptr;
    if (!in_w || !in_g || !in_s || !out_w || !out_s || (rowwise && (!in_v || !out_step))) return 2;
    const size_t esz = dtype == kStepF32 ? 4 : 2;
    for (;;) {
        uint32_t stored = 0;
        float g, s, v = 0.f;
        if (fread(&stored, esz, 1, in_w) != 1) break;
        if (fread(&g, 4, 1, in_g) != 1 || fread(&s, 4, 1, in_s) != 1) return 3;
        uint32_t o;
        if (rowwise) {
            if (fread(&v, 4, 1, in_v) != 1) return 3;
            const float step_size = rowwise_step_size(v, dim, &s, lr, eps);
            o = step(dtype, stored, g, step_size);
            fwrite(&step_size, 4, 1, out_step);
        } else {
            o = adagrad_step(dtype, stored, g, &s, lr, eps);
        }
        fwrite(&o, esz, 1, out_w);
        fwrite(&s, 4, 1, out_s);
    }
    fclose(out_w);
    fclose(out_s);
    if (out_step) fclose(out_step);
    return 0;
}
