// rows_encode_check.cpp -- the row writer's encoders (csrc/pimemb_rows_encode.h, the text the kernels compile) on the HOST.
//   rows_encode_check <f16|bf16|e4m3|e5m2|mxfp4> <dim> <in: float32 bits> <out: table bytes>
// Reads rows of `dim` fp32 values and writes them as the table dtype stores them; tests/test_rows_cpu.py compares the bytes with
// formats.py's encoders.  MXFP4 rows are assembled here in plain loops (the kernel does it with cross-lane shuffles: that part is
// the GPU tests' business); the scale and code arithmetic is the shared header's.  A row with a non-finite value is written as
// 0xEE bytes: the kernels skip such a row.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pimemb_rows_encode.h"

using namespace pimemb_rows;

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const char *kind = argv[1];
    const uint32_t dim = (uint32_t)atoi(argv[2]);
    FILE *in = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    if (!in || !out || dim == 0) return 2;
    std::vector<uint32_t> row(dim);
    const bool mx = !strcmp(kind, "mxfp4");
    if (mx && dim % 32) return 2;
    const uint32_t nb = dim / 32, stride = mx ? ((dim / 2 + nb + 15u) & ~15u) : 0;
    while (fread(row.data(), 4, dim, in) == dim) {
        if (mx) {
            std::vector<uint8_t> o(stride, 0);
            bool bad = false;
            for (uint32_t b = 0; b < nb; b++) {
                uint32_t amax = 0;
                for (uint32_t j = 0; j < 32; j++) {
                    const uint32_t a = row[b * 32 + j] & 0x7fffffffu;
                    amax = a > amax ? a : amax;
                }
                if (amax >= 0x7f800000u) {
                    bad = true;
                    break;
                }
                uint32_t s = mx_scale_of(amax);
                bool zeros = true;
                for (uint32_t j = 0; j < 32; j++) {
                    const uint32_t v = row[b * 32 + j];
                    const uint32_t code = mx_code_of(v & 0x7fffffffu, s);
                    zeros = zeros && code == 0;
                    o[b * 16 + j / 2] |= (uint8_t)((code | ((v >> 28) & 8u)) << (4 * (j & 1)));
                }
                o[dim / 2 + b] = (uint8_t)(zeros ? 127 : s);
            }
            if (bad) memset(o.data(), 0xEE, stride);
            fwrite(o.data(), 1, stride, out);
            continue;
        }
        for (uint32_t j = 0; j < dim; j++) {
            if (!strcmp(kind, "f16") || !strcmp(kind, "bf16")) {
                const uint16_t v = (uint16_t)(kind[0] == 'f' ? enc_f16(row[j]) : enc_bf16(row[j]));
                fwrite(&v, 2, 1, out);
            } else {
                const uint8_t v = (uint8_t)(!strcmp(kind, "e4m3") ? enc_e4m3(row[j]) : enc_e5m2(row[j]));
                fwrite(&v, 1, 1, out);
            }
        }
    }
    fclose(in);
    fclose(out);
    return 0;
}
