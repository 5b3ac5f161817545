// pimemb_grad_master.h -- the table-row encoding of the fused master-weight steps (include/pimemb_grad.h, THE MASTER-WEIGHT STEPS):
//     W[r] = enc_T(M'[r])
// from the lane's point of view: a lane of the lane-group kernels owns 4 consecutive fp32 elements of the new master row (a PIECE).
//   the 2-byte and 1-byte dtypes   master_enc_piece: the four elements through enc_f16 / enc_bf16 / enc_e4m3 / enc_e5m2 of
//                                  pimemb_rows_encode.h, packed in element order into 8 or 4 bytes
//   MXFP4                          eight adjacent pieces are one block of 32.  mx_piece_amax: the largest magnitude bits of a piece (the
//                                  block's amax is the integer max over its eight pieces: order-free); mx_piece_codes: the piece's four
//                                  E2M1 nibbles under the block's scale, packed into 16 bits; mx_block: the whole block -- amax, the
//                                  scale byte (mx_scale_of), the codes (mx_code_of), scale 127 where every code is a zero, and the
//                                  non-finite flag -- by the very piece functions, combined as the kernel's xor butterfly combines them.
// Plain integer arithmetic, `__host__ __device__` like pimemb_rows_encode.h, whose encoders it calls: the kernels of pimemb_grad.hip
// and the host-side check (tests/cpp/master_block_check.cpp, compared with formats.to_mxfp4 by tests/test_master_cpu.py) compile the
// same text.
#pragma once

#include <stdint.h>

#include "pimemb_rows_encode.h"

namespace pimemb_grad {

// table dtypes the master step encodes to (the emb_dtype values of pimemb.h)
constexpr int kMasterF16 = 1, kMasterBF16 = 3, kMasterE4M3 = 8, kMasterE5M2 = 9, kMasterMXFP4 = 10;

// One element of a 2-byte or 1-byte table from the fp32 bits of the master element.
PIMEMB_ROWS_HD uint32_t master_enc(int dtype, uint32_t bits) {
    switch (dtype) {
        case kMasterF16: return pimemb_rows::enc_f16(bits);
        case kMasterBF16: return pimemb_rows::enc_bf16(bits);
        case kMasterE4M3: return pimemb_rows::enc_e4m3(bits);
        default: return pimemb_rows::enc_e5m2(bits);
    }
}

// A piece of a 2-byte dtype: elements 0, 1 in lo, elements 2, 3 in hi (little endian: element order in memory).
PIMEMB_ROWS_HD void master_enc_piece16(int dtype, const uint32_t bits[4], uint32_t *lo, uint32_t *hi) {
    *lo = master_enc(dtype, bits[0]) | (master_enc(dtype, bits[1]) << 16);
    *hi = master_enc(dtype, bits[2]) | (master_enc(dtype, bits[3]) << 16);
}

// A piece of a 1-byte dtype: four bytes in element order.
PIMEMB_ROWS_HD uint32_t master_enc_piece8(int dtype, const uint32_t bits[4]) {
    return master_enc(dtype, bits[0]) | (master_enc(dtype, bits[1]) << 8) | (master_enc(dtype, bits[2]) << 16) | (master_enc(dtype, bits[3]) << 24);
}

// ---- MXFP4 ------------------------------------------------------------------------------------------------------------------

// The largest magnitude (fp32 bits, sign cleared) of a piece.  Compared as integers: for finite values that is the order of the
// magnitudes, an infinity lies above them all and a NaN above the infinity.
PIMEMB_ROWS_HD uint32_t mx_piece_amax(const uint32_t bits[4]) {
    uint32_t amax = 0;
    for (int j = 0; j < 4; j++) {
        const uint32_t a = bits[j] & 0x7fffffffu;
        amax = a > amax ? a : amax;
    }
    return amax;
}

PIMEMB_ROWS_HD uint32_t mx_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Whether an amax (of a piece, a block or a row) says that an inf or a NaN is among the values.
PIMEMB_ROWS_HD bool mx_non_finite(uint32_t amax) { return amax >= 0x7f800000u; }

// The four nibbles of a piece under the block's scale byte s, element j in bits 4j .. 4j + 3: sign (bit 3) and the E2M1 code.
// (Total for non-finite values too: the row is not stored then.)
PIMEMB_ROWS_HD uint32_t mx_piece_codes(const uint32_t bits[4], uint32_t s) {
    uint32_t codes = 0;
    for (int j = 0; j < 4; j++) codes |= (pimemb_rows::mx_code_of(bits[j] & 0x7fffffffu, s) | ((bits[j] >> 28) & 8u)) << (4 * j);
    return codes;
}

// Whether every code of a piece is a zero of either sign.
PIMEMB_ROWS_HD bool mx_piece_zeros(uint32_t codes) { return (codes & 0x7777u) == 0; }

// One block: 32 fp32 values (as bits) -> its 16 element bytes (four little-endian words), its scale byte, and whether it holds an
// inf or a NaN (then bytes and scale mean nothing).  Piece by piece with the functions above, the pieces combined in the order of
// the kernel's butterfly over xor distances 1, 2 and 4 -- integer max and logical and: any order gives the same.
PIMEMB_ROWS_HD void mx_block(const uint32_t v[32], uint32_t words[4], uint32_t *scale, bool *non_finite) {
    uint32_t amax[8];
    for (int l = 0; l < 8; l++) amax[l] = mx_piece_amax(v + 4 * l);
    for (int h = 1; h < 8; h <<= 1) {
        uint32_t next[8];
        for (int l = 0; l < 8; l++) next[l] = mx_max(amax[l], amax[l ^ h]);
        for (int l = 0; l < 8; l++) amax[l] = next[l];
    }
    *non_finite = mx_non_finite(amax[0]);
    uint32_t s = pimemb_rows::mx_scale_of(amax[0]);
    bool zeros = true;
    uint32_t codes[8];
    for (int l = 0; l < 8; l++) {
        codes[l] = mx_piece_codes(v + 4 * l, s);
        zeros = zeros && mx_piece_zeros(codes[l]);
    }
    if (zeros) s = 127;
    for (int w = 0; w < 4; w++) words[w] = codes[2 * w] | (codes[2 * w + 1] << 16);
    *scale = s;
}

}  // namespace pimemb_grad
