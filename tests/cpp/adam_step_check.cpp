// adam_step_check.cpp -- the one-element arithmetic of the fused Adam steps (csrc/pimemb_grad_adam.h, the text the kernels compile) on
// the HOST.  All numbers travel as fp32 bit patterns; the constants om1, om2, ss and eps are given, not derived.
//   adam_step_check adam <f32|f16|bf16> <om1> <om2> <ss> <eps: fp32 bits, hex> <in> <out>
//       in: records of 4 words (stored element, g, M, V); out: records of 3 words (stored', M', V'): adam_step per element
//   adam_step_check rowwise <f32|f16|bf16> <om1> <om2> <ss> <eps> <dim> <in> <out>
//       in: records of 5 words (stored element, g, M, V[r], the tree's sum); out: records of 4 words (stored', M', V', rate):
//       rowwise_adam_rate, then rowwise_adam_step: the calls of the kernel's row-wise tail
//   adam_step_check constants <lr> <beta1> <beta2> <t>      (decimal; prints om1 om2 ss as fp32 bits, hex)
// tests/test_adam_cpu.py compares the bytes with tests/adam_ref.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pimemb_grad_adam.h"

using namespace pimemb_grad;

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "constants")) {
        float c[3];
        adam_constants(strtod(argv[2], nullptr), strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtoull(argv[5], nullptr, 10), c);
        printf("%x %x %x\n", f32_bits(c[0]), f32_bits(c[1]), f32_bits(c[2]));
        return 0;
    }
    if (argc < 3) return 2;
    const bool rowwise = !strcmp(argv[1], "rowwise");
    if ((!rowwise && strcmp(argv[1], "adam")) || argc != (rowwise ? 10 : 9)) return 2;
    const int dtype = !strcmp(argv[2], "f32") ? kStepF32 : !strcmp(argv[2], "f16") ? kStepF16 : !strcmp(argv[2], "bf16") ? kStepBF16 : -1;
    if (dtype < 0) return 2;
    float k[4];      // om1, om2, ss, eps
    for (int j = 0; j < 4; j++) k[j] = bits_f32((uint32_t)strtoul(argv[3 + j], nullptr, 16));
    const uint32_t dim = rowwise ? (uint32_t)strtoul(argv[7], nullptr, 10) : 0;
    FILE *in = fopen(argv[rowwise ? 8 : 7], "rb"), *out = fopen(argv[rowwise ? 9 : 8], "wb");
    if (!in || !out) return 2;
    uint32_t rec[5];
    while (fread(rec, 4, rowwise ? 5 : 4, in) == (rowwise ? 5u : 4u)) {
        float m = bits_f32(rec[2]), v = bits_f32(rec[3]);
        uint32_t o[4];
        if (rowwise) {
            const float rate = rowwise_adam_rate(bits_f32(rec[4]), dim, &v, k[1], k[2], k[3]);
            o[0] = rowwise_adam_step(dtype, rec[0], bits_f32(rec[1]), &m, k[0], rate);
            o[3] = f32_bits(rate);
        } else {
            o[0] = adam_step(dtype, rec[0], bits_f32(rec[1]), &m, &v, k[0], k[1], k[2], k[3]);
        }
        o[1] = f32_bits(m), o[2] = f32_bits(v);
        fwrite(o, 4, rowwise ? 4 : 3, out);
    }
    fclose(out);
    return 0;
}
