// pimemb_rows_encode.h -- fp32 bits -> the bits of every table dtype, as formats.py's host encoders write them.
// Plain integer arithmetic (and one exact fp32 addition), `__host__ __device__`: the row-writer kernels (pimemb_rows.hip) and
// the host-side check (tests/cpp/rows_encode_check.cpp, compared with formats.py by tests/test_rows_cpu.py) compile the same
// text, so what the CPU test proves about NaN payloads, overflow and denormals holds for the kernels' arithmetic as well.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PIMEMB_ROWS_HD __host__ __device__ inline
#else
#define PIMEMB_ROWS_HD inline
#endif

namespace pimemb_rows {

PIMEMB_ROWS_HD uint32_t f32_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
PIMEMB_ROWS_HD float bits_f32(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// bfloat16, formats.to_bf16_bits: nearest even on the bits; a NaN keeps sign and upper payload and gets the quiet bit.
PIMEMB_ROWS_HD uint32_t enc_bf16(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
    return (u + (0x7fffu + ((u >> 16) & 1u))) >> 16;
}

// The magnitude of a small float format with EB exponent bits, MB mantissa bits and bias BIAS, before the format's own
// overflow rule: formats.to_f8_bits' arithmetic.  Normal range: re-bias, round the dropped bits to nearest even (a carry runs
// into the exponent).  Subnormal range: adding 2^(1 - BIAS - MB + 23) in fp32 leaves the rounded multiple of the format's
// quantum in the low bits -- one IEEE addition of a value below the format's smallest normal to a power of two far above it,
// exact but for the one rounding wanted, whatever the denormal mode (an fp32 denormal `a` adds nothing either way).
template <int EB, int MB, int BIAS>
PIMEMB_ROWS_HD uint32_t enc_small_mag(uint32_t a /* fp32 bits, sign cleared, finite */) {
    constexpr int shift = 23 - MB;
    constexpr uint32_t min_normal = (uint32_t)(127 - BIAS + 1) << 23;
    if (a < min_normal) {
        constexpr uint32_t magic = (uint32_t)(127 + 1 - BIAS - MB + 23) << 23;
        return f32_bits(bits_f32(a) + bits_f32(magic)) - magic;
    }
    uint32_t v = a - ((uint32_t)(127 - BIAS) << 23);
    return (v + ((1u << (shift - 1)) - 1u) + ((v >> shift) & 1u)) >> shift;
}

// OCP e4m3fn: no infinity -- whatever rounds beyond 448, infinities and NaNs included, is 0x7f | sign.
PIMEMB_ROWS_HD uint32_t enc_e4m3(uint32_t u) {
    const uint32_t sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
    uint32_t r = a >= 0x7f800000u ? 0x7fu : enc_small_mag<4, 3, 7>(a);
    if (r >= 0x7fu) r = 0x7fu;
    return r | sign;
}

// OCP e5m2: beyond 57344 (or inf) is 0x7c | sign, NaN 0x7f | sign.
PIMEMB_ROWS_HD uint32_t enc_e5m2(uint32_t u) {
    const uint32_t sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return 0x7fu | sign;
    uint32_t r = a == 0x7f800000u ? 0x7cu : enc_small_mag<5, 2, 15>(a);
    if (r >= 0x7cu) r = 0x7cu;
    return r | sign;
}

// IEEE binary16 as numpy's astype(float16) writes it: nearest even, overflow to +-inf; a NaN keeps its sign and the upper ten
// payload bits unquieted, and a payload that lies wholly in the dropped bits becomes payload 1.
PIMEMB_ROWS_HD uint32_t enc_f16(uint32_t u) {
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) {
        uint32_t r = 0x7c00u + ((a & 0x007fffffu) >> 13);
        return (r == 0x7c00u ? r + 1u : r) | sign;
    }
    uint32_t r = a == 0x7f800000u ? 0x7c00u : enc_small_mag<5, 10, 15>(a);
    if (r >= 0x7c00u) r = 0x7c00u;
    return r | sign;
}

// ---- MXFP4 (formats.to_mxfp4) -------------------------------------------------------------------------------------------
// Scale byte of a block from the largest |fp32 bits| in it: floor(log2 amax) - 2 + 127 clamped to [0, 254].  A normal amax has
// floor(log2) = exponent field - 127; a denormal one (field 0) lies below 2^-126 and clamps to 0 like every amax below 2^-125;
// amax = 0 takes any value here (its block quantises to zeros and gets 127 from the caller).  The field of a finite fp32 is at
// most 254, so the upper clamp is never reached.
PIMEMB_ROWS_HD uint32_t mx_scale_of(uint32_t amax_bits) {
    const uint32_t e = amax_bits >> 23;
    return e > 2u ? e - 2u : 0u;
}

// The E2M1 code (0 .. 7) of |v| / 2^(s - 127), to nearest, ties to the even code.  |v| = sig * 2^(e - 150) with the 24-bit
// significand sig (e = max(exponent field, 1)), so in QUARTERS |v| / X = sig * 2^(e - s - 21): below 32 quarters, since
// |v| <= amax < 8 X by the choice of s.  q = its integer part, sticky = whether anything was shifted out; t = 2 q + sticky
// orders the value against the seven midpoints 0.25 .. 5 (1, 3, 5, 7, 10, 14, 20 quarters): above an even code's upper
// midpoint is t > 2 m, at or above an odd code's is t >= 2 m.
PIMEMB_ROWS_HD uint32_t mx_code_of(uint32_t a /* fp32 bits, sign cleared, finite */, uint32_t s) {
    const uint32_t field = a >> 23;
    const uint32_t sig = (a & 0x007fffffu) | (field ? 0x00800000u : 0u);
    const int k = (int)(field ? field : 1u) - (int)s - 21;
    uint32_t q, sticky;
    if (k >= 0) {
        q = k > 7 ? 0xffu : (sig << k);       // (k > 7 cannot happen for |v| <= amax; kept total: saturates)
        sticky = 0;
        if (q > 0xffu) q = 0xffu;
    } else if (k <= -25) {
        q = 0;
        sticky = sig != 0;
    } else {
        q = sig >> (-k);
        sticky = (sig & ((1u << (-k)) - 1u)) != 0;
    }
    const uint32_t t = 2u * q + sticky;
    return (t > 2u) + (t >= 6u) + (t > 10u) + (t >= 14u) + (t > 20u) + (t >= 28u) + (t > 40u);
}

}  // namespace pimemb_rows
