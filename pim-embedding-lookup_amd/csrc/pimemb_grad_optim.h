// pimemb_grad_optim.h -- the one-element arithmetic of the fused Adagrad steps of the backward pass (include/pimemb_grad.h):
//     element-wise   q = g * g;  S' = S + q;  den = sqrt(S') + eps;  x = g / den;  stored' = enc(dec(stored) - (lr * x))
//     row-wise       m = v / (float)dim;  S' = S + m;  step = lr / (sqrt(S') + eps);  stored' = enc(dec(stored) - (step * g))
//                    (v = the pair tree over the row's g * g; the tree itself is the kernel's: adagrad_square and
//                    adagrad_add are its two operations)
// Every fp32 operation is a statement of its own and never contracted into an FMA, as in pimemb_grad_step.h, whose step_f32 / dec
// / enc do the last line.  Division and square root are the IEEE correctly rounded ones: on the device the language's own `/` and
// __builtin_sqrtf, which HIP compiles correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt, the default, and spelled out on
// the unit's compile line; the runtime's __fsqrt_rn is the approximate instruction in this ROCM's headers, so it is NOT used); on
// the host the compiler's division and sqrtf.
// `__host__ __device__`: the kernels of pimemb_grad.hip and the host-side check (tests/cpp/optim_step_check.cpp, compared with
// tests/optim_ref.py by tests/test_optim_cpu.py) compile the same text.
#pragma once

#include <stdint.h>

#include "pimemb_grad_step.h"

namespace pimemb_grad {

#if defined(__clang__)
#define PIMEMB_OPTIM_NO_CONTRACT _Pragma("clang fp contract(off)")
#define PIMEMB_OPTIM_F32 const float
#else
#define PIMEMB_OPTIM_NO_CONTRACT
#define PIMEMB_OPTIM_F32 volatile float      // (rounded to fp32 here: nothing fuses across it)
#endif

PIMEMB_ROWS_HD float adagrad_square(float g) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 q = g * g;
    return q;
}

PIMEMB_ROWS_HD float adagrad_add(float a, float b) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 s = a + b;
    return s;
}

// sqrt(s) + eps: one correctly rounded square root, one addition
PIMEMB_ROWS_HD float adagrad_den(float s, float eps) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 root = __builtin_sqrtf(s);
    PIMEMB_OPTIM_F32 den = root + eps;
    return den;
}

PIMEMB_ROWS_HD float adagrad_div(float a, float b) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 x = a / b;
    return x;
}

// Element-wise Adagrad on one element: *state becomes S' = S + g * g; returns the stored bits after the step.
PIMEMB_ROWS_HD uint32_t adagrad_step(int dtype, uint32_t stored_bits, float g, float *state, float lr, float eps) {
    const float s = adagrad_add(*state, adagrad_square(g));
    *state = s;
    const float x = adagrad_div(g, adagrad_den(s, eps));
    return step(dtype, stored_bits, x, lr);
}

// Row-wise Adagrad, once per row: v = the tree's sum of squares.  *state becomes S' = S + v / (float)dim; returns
// step = lr / (sqrt(S') + eps).
PIMEMB_ROWS_HD float rowwise_step_size(float v, uint32_t dim, float *state, float lr, float eps) {
    const float m = adagrad_div(v, (float)dim);
    const float s = adagrad_add(*state, m);
    *state = s;
    return adagrad_div(lr, adagrad_den(s, eps));
}

// ... and per element: enc(dec(stored) - (step * g)) is pimemb_grad_step.h's step(dtype, stored, g, step size), as the kernel calls it.

}  // namespace pimemb_grad
