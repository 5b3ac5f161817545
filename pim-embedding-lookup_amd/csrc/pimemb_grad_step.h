// pimemb_grad_step.h -- the one-element SGD step of the backward pass (include/pimemb_grad.h):
//     stored' = enc(dec(stored) - (lr * g))
// dec is the exact widening of a table element to fp32 (integer work on the bits), lr * g ONE fp32 multiply, the subtraction ONE
// fp32 subtract -- never contracted into an FMA: step_f32 switches contraction off for its own statements (clang: the fp
// pragma; elsewhere a volatile temporary pins the rounded product) -- and enc the encoder of pimemb_rows_encode.h for the
// table's dtype (identity, enc_f16, enc_bf16).
// `__host__ __device__` like that header: the kernels of pimemb_grad.hip and the host-side check
// (tests/cpp/grad_step_check.cpp, compared with tests/grad_ref.py by tests/test_grad_cpu.py) compile the same text.
#pragma once

#include <stdint.h>

#include "pimemb_rows_encode.h"

namespace pimemb_grad {

using pimemb_rows::bits_f32;
using pimemb_rows::f32_bits;

// table dtypes the step takes (the emb_dtype values of pimemb.h)
constexpr int kStepF32 = 0, kStepF16 = 1, kStepBF16 = 3;

PIMEMB_ROWS_HD uint32_t dec_f32(uint32_t stored) { return stored; }

PIMEMB_ROWS_HD uint32_t dec_bf16(uint32_t stored) { return (stored & 0xffffu) << 16; }

// IEEE binary16 -> the fp32 bits of the same value: every fp16 value, subnormals included, is an fp32 normal (or zero); an
// infinity stays one, a NaN keeps its payload in the upper mantissa bits.
PIMEMB_ROWS_HD uint32_t dec_f16(uint32_t stored) {
    const uint32_t sign = (stored & 0x8000u) << 16, e = (stored >> 10) & 0x1fu;
    uint32_t m = stored & 0x3ffu;
    if (e == 0x1fu) return sign | 0x7f800000u | (m << 13);
    if (e != 0) return sign | ((e + 112u) << 23) | (m << 13);
    if (m == 0) return sign;
    uint32_t ex = 113u;                       // m * 2^-24: shift the leading one up to bit 10, one exponent step each
    while (!(m & 0x400u)) {
        m <<= 1;
        ex--;
    }
    return sign | (ex << 23) | ((m & 0x3ffu) << 13);
}

PIMEMB_ROWS_HD uint32_t dec(int dtype, uint32_t stored) { return dtype == kStepF16 ? dec_f16(stored) : dtype == kStepBF16 ? dec_bf16(stored) : stored; }

PIMEMB_ROWS_HD uint32_t enc(int dtype, uint32_t f32) {
    return dtype == kStepF16 ? pimemb_rows::enc_f16(f32) : dtype == kStepBF16 ? pimemb_rows::enc_bf16(f32) : f32;
}

// fp32: w - (lr * g), two roundings.
PIMEMB_ROWS_HD float step_f32(float w, float g, float lr) {
#if defined(__clang__)
#pragma clang fp contract(off)
    const float prod = lr * g;
#else
    volatile float prod = lr * g;             // (rounded to fp32 here: nothing may fuse it into the subtraction)
#endif
    return w - prod;
}

// stored bits of one element (the low 16 for the 2-byte dtypes) -> the stored bits after the step
PIMEMB_ROWS_HD uint32_t step(int dtype, uint32_t stored_bits, float g, float lr) {
    return enc(dtype, f32_bits(step_f32(bits_f32(dec(dtype, stored_bits)), g, lr)));
}

}  // namespace pimemb_grad
