// master_block_check.cpp -- the one-block MXFP4 arithmetic of the master-weight steps (csrc/pimemb_grad_master.h, the text the kernels
// compile) on the HOST.
//   master_block_check mx <in: blocks of 32 float32> <out: 18 bytes per block>
//       per block: mx_block -> its 16 element bytes, its scale byte, and 1 where the block holds an inf or a NaN (else 0)
//   master_block_check piece <f16|bf16|e4m3|e5m2> <in: float32, a multiple of 4> <out: stored elements>
//       per piece of four: master_enc_piece16 / master_enc_piece8, the bytes in memory order
// tests/test_master_cpu.py compares the bytes with formats.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pimemb_grad_master.h"

using namespace pimemb_grad;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "mx")) {
        if (argc != 4) return 2;
        FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        uint32_t v[32];
        while (fread(v, 4, 32, in) == 32) {
            uint32_t words[4], scale;
            bool non_finite;
            mx_block(v, words, &scale, &non_finite);
            uint8_t rec[18];
            memcpy(rec, words, 16);              // (little endian: the words are the bytes in memory order)
            rec[16] = (uint8_t)scale;
            rec[17] = non_finite ? 1 : 0;
            fwrite(rec, 1, 18, out);
        }
        fclose(out);
        return 0;
    }
    if (strcmp(argv[1], "piece") || argc != 5) return 2;
    const int dtype = !strcmp(argv[2], "f16") ? kMasterF16 : !strcmp(argv[2], "bf16") ? kMasterBF16 : !strcmp(argv[2], "e4m3") ? kMasterE4M3
                    : !strcmp(argv[2], "e5m2") ? kMasterE5M2 : -1;
    if (dtype < 0) return 2;
    FILE *in = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    if (!in || !out) return 2;
    uint32_t v[4];
    while (fread(v, 4, 4, in) == 4) {
        if (dtype == kMasterF16 || dtype == kMasterBF16) {
            uint32_t w[2];
            master_enc_piece16(dtype, v, &w[0], &w[1]);
            fwrite(w, 4, 2, out);
        } else {
            const uint32_t w = master_enc_piece8(dtype, v);
            fwrite(&w, 4, 1, out);
        }
    }
    fclose(out);
    return 0;
}
