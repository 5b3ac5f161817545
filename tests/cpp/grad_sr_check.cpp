// Host-side run of csrc/pimemb_grad_sr.h, the text the kernels of the stochastically rounded steps compile (tests/test_sr_cpu.py
// compares it with tests/sr_ref.py).
//   grad_sr_check philox c0 c1 c2 c3 k0 k1        (hex)  -> the four output words, hex
//   grad_sr_check words seed t row pieces out.bin (hex seed and t) -> uint32[4 * pieces]: sr_words of the row's pieces
//   grad_sr_check enc f16|bf16 in.bin out.bin     in: pairs of uint32 (fp32 bits, R) -> uint16 per pair: enc_sr
//   grad_sr_check step f16|bf16 in.bin out.bin    in: records of uint32 (stored bits, g bits, lr bits, R) -> uint16: step_sr
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pimemb_grad_sr.h"

using namespace pimemb_grad;

static std::vector<uint32_t> read_u32(const char *path) {
    std::vector<uint32_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint32_t x;
    while (fread(&x, 4, 1, f) == 1) v.push_back(x);
    fclose(f);
    return v;
}

template <typename T>
static int write_all(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb");
    if (!f) return 1;
    const size_t n = fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
    return n == v.size() ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 8 && !strcmp(argv[1], "philox")) {
        uint32_t a[6], out[4];
        for (int i = 0; i < 6; i++) a[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 16);
        philox4x32_10(a[0], a[1], a[2], a[3], a[4], a[5], out);
        printf("%08x %08x %08x %08x\n", out[0], out[1], out[2], out[3]);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "words")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 16), t = strtoull(argv[3], nullptr, 16);
        const uint32_t row = (uint32_t)strtoul(argv[4], nullptr, 10), pieces = (uint32_t)strtoul(argv[5], nullptr, 10);
        std::vector<uint32_t> out(4 * (size_t)pieces);
        for (uint32_t c = 0; c < pieces; c++) sr_words(seed, t, row, c, &out[4 * (size_t)c]);
        return write_all(argv[6], out);
    }
    if (argc == 5 && (!strcmp(argv[1], "enc") || !strcmp(argv[1], "step"))) {
        const int dtype = !strcmp(argv[2], "f16") ? kStepF16 : kStepBF16;
        const std::vector<uint32_t> in = read_u32(argv[3]);
        const size_t rec = !strcmp(argv[1], "enc") ? 2 : 4;
        std::vector<uint16_t> out(in.size() / rec);
        for (size_t i = 0; i < out.size(); i++) {
            const uint32_t *r = &in[rec * i];
            if (rec == 2) out[i] = (uint16_t)enc_sr(dtype, r[0], r[1]);
            else out[i] = (uint16_t)step_sr(dtype, r[0], pimemb_rows::bits_f32(r[1]), pimemb_rows::bits_f32(r[2]), r[3]);
        }
        return write_all(argv[4], out);
    }
    fprintf(stderr, "usage: grad_sr_check philox|words|enc|step ...\n");
    return 2;
}
