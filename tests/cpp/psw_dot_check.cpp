// psw_dot_check.cpp -- the arithmetic of the gradient of per_sample_weights (csrc/pimemb_grad_dot.h, the text the kernels compile) on
// the HOST.
//   psw_dot_check <f32|f16|bf16> <dim> <in: stored rows, dim elements each> <in: float32 rows of G, dim each> <out: float32 dw, one per row>
//       per row: dot_row(dtype, stored row, G row, dim) -- the serial form of the tree
// tests/test_psw_cpu.py compares the bytes with tests/psw_ref.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pimemb_grad_dot.h"

using namespace pimemb_grad;

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int dtype = !strcmp(argv[1], "f32") ? kStepF32 : !strcmp(argv[1], "f16") ? kStepF16 : !strcmp(argv[1], "bf16") ? kStepBF16 : -1;
    if (dtype < 0) return 2;
    const uint32_t dim = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (dim == 0) return 2;
    FILE *in_w = fopen(argv[3], "rb"), *in_g = fopen(argv[4], "rb"), *out = fopen(argv[5], "wb");
    if (!in_w || !in_g || !out) return 2;
    const size_t esz = dtype == kStepF32 ? 4 : 2;
    std::vector<uint32_t> row((dim * esz + 3) / 4);      // (4-byte aligned storage for either element size)
    std::vector<float> g(dim);
    for (;;) {
        if (fread(row.data(), esz, dim, in_w) != dim) break;
        if (fread(g.data(), 4, dim, in_g) != dim) return 3;
        const float dw = dot_row(dtype, row.data(), g.data(), dim);
        fwrite(&dw, 4, 1, out);
    }
    fclose(out);
    return 0;
}
