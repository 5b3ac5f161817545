// pimemb_grad_dot.h -- the arithmetic of the gradient of per_sample_weights (include/pimemb_grad.h, THE GRADIENT OF
// PER_SAMPLE_WEIGHTS): one position's dw = < G[bag] , dec(W[row]) > over a fixed tree.
//     prod[d] = G[d] * dec(W[d])                                  one fp32 multiply;  +0 for dim <= d < 4 * pieces
//     t[c]    = ((prod[4c] + prod[4c+1]) + prod[4c+2]) + prod[4c+3]     c < pieces = ceil(dim / 4)
//     v[l]    = ((t[l] + t[l+64]) + t[l+128]) + ...                 l < L = min(64, pow2ceil(pieces));  +0 where l >= pieces
//     adjacent pairs, level by level, down to v[0]
// Every fp32 operation is a statement of its own and never contracted into an FMA, as in pimemb_grad_optim.h, whose switches this
// header uses; dec is pimemb_grad_step.h's.
// `__host__ __device__`: the kernels of pimemb_grad.hip (dot_mul / dot_add / dot_fold4 on registers in the lane-group kernel,
// dot_leaf with scalar element loads in the fallback kernel) and the host-side check (tests/cpp/psw_dot_check.cpp: dot_row, the
// serial form of the tree, compared with tests/psw_ref.py by tests/test_psw_cpu.py) compile the same text.
#pragma once

#include <stdint.h>

#include "pimemb_grad_optim.h"

namespace pimemb_grad {

PIMEMB_ROWS_HD float dot_mul(float g, float w) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 p = g * w;
    return p;
}

PIMEMB_ROWS_HD float dot_add(float a, float b) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 s = a + b;
    return s;
}

// t[c] from a piece's four products
PIMEMB_ROWS_HD float dot_fold4(float p0, float p1, float p2, float p3) { return dot_add(dot_add(dot_add(p0, p1), p2), p3); }

// L of the definition: the entries of v, and the lanes of a group
PIMEMB_ROWS_HD uint32_t dot_pieces(uint32_t dim) { return (dim + 3u) / 4u; }
PIMEMB_ROWS_HD uint32_t dot_lanes(uint32_t dim) {
    uint32_t l = 1;
    while (l < dot_pieces(dim) && l < 64u) l <<= 1;
    return l;
}

// dec(W[d]) of a stored row: a scalar element load
PIMEMB_ROWS_HD float dot_load(int dtype, const void *row, uint32_t d) {
    if (dtype == kStepF32) return static_cast<const float *>(row)[d];
    return bits_f32(dec(dtype, static_cast<const uint16_t *>(row)[d]));
}

// t[c] with scalar element loads; the elements at and beyond dim are +0 and are added
PIMEMB_ROWS_HD float dot_piece(int dtype, const void *row, const float *g, uint32_t dim, uint32_t c) {
    float p[4];
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t d = 4u * c + k;
        p[k] = d < dim ? dot_mul(g[d], dot_load(dtype, row, d)) : 0.f;
    }
    return dot_fold4(p[0], p[1], p[2], p[3]);
}

// v[l] before the pair tree
PIMEMB_ROWS_HD float dot_leaf(int dtype, const void *row, const float *g, uint32_t dim, uint32_t l) {
    const uint32_t pieces = dot_pieces(dim);
    if (l >= pieces) return 0.f;
    float v = dot_piece(dtype, row, g, dim, l);
    for (uint32_t c = l + 64u; c < pieces; c += 64u) v = dot_add(v, dot_piece(dtype, row, g, dim, c));
    return v;
}

// The serial form of the tree: dw of one position from its stored row and its bag's row of G.
PIMEMB_ROWS_HD float dot_row(int dtype, const void *row, const float *g, uint32_t dim) {
    float v[64];
    uint32_t len = dot_lanes(dim);
    for (uint32_t l = 0; l < len; l++) v[l] = dot_leaf(dtype, row, g, dim, l);
    for (; len > 1; len /= 2)
        for (uint32_t k = 0; k < len / 2; k++) v[k] = dot_add(v[2 * k], v[2 * k + 1]);
    return v[0];
}

}  // namespace pimemb_grad
