// pimemb_grad_sr.h -- the arithmetic of the stochastically rounded steps of the backward pass (include/pimemb_grad.h, THE
// STOCHASTICALLY ROUNDED STEPS):
//     stored' = enc_sr_T(x, R)       x the fp32 value the in-place step would have rounded to nearest, R a 32-bit word
//     R       = word (d mod 4) of Philox4x32-10 with key (seed_lo, seed_hi) and counter (r, d div 4, t_lo, t_hi)
// enc_sr rounds x to one of its two neighbours in T: away from zero for exactly F of the 2^32 words, F = floor(f * 2^32), f the
// place of |x| between the neighbours -- all of it integer work on the fp32 bits; NaN and infinity go through the row writer's
// encoders (pimemb_rows_encode.h).  The steps in front of it are those of pimemb_grad_step.h and pimemb_grad_optim.h, unchanged.
// `__host__ __device__` like those headers: the kernels of pimemb_grad.hip and the host-side check (tests/cpp/grad_sr_check.cpp,
// compared with tests/sr_ref.py by tests/test_sr_cpu.py) compile the same text.
#pragma once

#include <stdint.h>

#include "pimemb_grad_optim.h"
#include "pimemb_grad_step.h"
#include "pimemb_rows_encode.h"

namespace pimemb_grad {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds of two 32 x 32 -> 64
// bit multiplications, the key raised by the Weyl constants between rounds.  out = the four words of the block.
PIMEMB_ROWS_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// The block of the piece that holds elements 4 * piece .. 4 * piece + 3 of row `row` at step number t: word j is element 4 * piece + j's.
PIMEMB_ROWS_HD void sr_words(uint64_t seed, uint64_t t, uint32_t row, uint32_t piece, uint32_t out[4]) {
    philox4x32_10(row, piece, (uint32_t)t, (uint32_t)(t >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

// 1 if F + R >= 2^32
PIMEMB_ROWS_HD uint32_t sr_carry(uint32_t F, uint32_t R) { return (uint32_t)(F + R) < F ? 1u : 0u; }

// bf16: the dropped 16 bits are the fraction; the carry runs into the exponent and can reach inf (0x7f80), never a NaN.
PIMEMB_ROWS_HD uint32_t enc_sr_bf16(uint32_t u, uint32_t R) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return pimemb_rows::enc_bf16(u);
    return (u >> 16) + sr_carry(u << 16, R);
}

// fp16.  From 2^-14 up (biased fp32 exponent e >= 113) the grid is the fp32 one with 13 bits dropped; below it the spacing is
// 2^-24 whatever the exponent: with e' = max(e, 1), the 24-bit significand m and s = 126 - e' (14 .. 125), |x| = m * 2^-s quanta.
// For s > 32 the fraction is finer than 2^-32 and F = floor(f * 2^32) truncates it: the one place where the chance of rounding
// away from zero is not exactly f (it is below f by less than 2^-32, and 0 from s = 56 on).
PIMEMB_ROWS_HD uint32_t enc_sr_f16(uint32_t u, uint32_t R) {
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return pimemb_rows::enc_f16(u);
    if (a >= 0x47800000u) return 0x7c00u | sign;      // |x| >= 65536
    const uint32_t e = a >> 23;
    if (e >= 113u) {
        const uint32_t up = a + (sr_carry((a & 0x1fffu) << 19, R) << 13);
        return ((up - 0x38000000u) >> 13) | sign;     // (exact: the low 13 bits are dropped; 65536 itself is 0x7c00, inf)
    }
    const uint32_t m = (a & 0x007fffffu) | (e ? 0x00800000u : 0u);
    const uint32_t s = 126u - (e ? e : 1u);
    const uint32_t lo = s >= 24u ? 0u : m >> s;
    const uint32_t rem = s >= 24u ? m : m & ((1u << s) - 1u);
    const uint32_t F = s <= 32u ? rem << (32u - s) : s >= 56u ? 0u : rem >> (s - 32u);
    return (lo + sr_carry(F, R)) | sign;              // (lo <= 0x3ff: the carry of 0x3ff is 0x400, 2^-14)
}

PIMEMB_ROWS_HD uint32_t enc_sr(int dtype, uint32_t f32, uint32_t R) { return dtype == kStepF16 ? enc_sr_f16(f32, R) : enc_sr_bf16(f32, R); }

// stored bits of one fp16 / bf16 element -> the stored bits after the SGD step (step of pimemb_grad_step.h but for the last rounding)
PIMEMB_ROWS_HD uint32_t step_sr(int dtype, uint32_t stored_bits, float g, float lr, uint32_t R) {
    return enc_sr(dtype, f32_bits(step_f32(bits_f32(dec(dtype, stored_bits)), g, lr)), R);
}

// ... and after the element-wise Adagrad step (adagrad_step of pimemb_grad_optim.h but for the last rounding)
PIMEMB_ROWS_HD uint32_t adagrad_step_sr(int dtype, uint32_t stored_bits, float g, float *state, float lr, float eps, uint32_t R) {
    const float s = adagrad_add(*state, adagrad_square(g));
    *state = s;
    const float x = adagrad_div(g, adagrad_den(s, eps));
    return step_sr(dtype, stored_bits, x, lr, R);
}

}  // namespace pimemb_grad
