// pimemb_grad_adam.h -- the one-element arithmetic of the fused Adam steps of the backward pass (include/pimemb_grad.h, THE ADAM STEPS):
//     EMB_ADAM           dm = g - M;  um = dm * om1;  M' = M + um;   q = g * g;  dv = q - V;  uv = dv * om2;  V' = V + uv;
//                        den = sqrt(V') + eps;  x = M' / den;  stored' = enc(dec(stored) - (ss * x))
//     EMB_ROWWISE_ADAM   once per row: ms = v / (float)dim;  dv = ms - V;  uv = dv * om2;  V' = V + uv;  rate = ss / (sqrt(V') + eps)
//                        (v = the row-wise Adagrad pair tree over the row's g * g: the kernel's, from adagrad_square / adagrad_add);
//                        per element: M' as above;  stored' = enc(dec(stored) - (rate * M'))
// and of their master-weight forms (THE MASTER-WEIGHT ADAM STEPS), which take the moments' half of the above as it is -- adam_moments,
// rowwise_adam_moment -- and subtract from the fp32 master element instead:  P' = P - (ss * x)  or  P' = P - (rate * M')  (adam_master);
// built from pimemb_grad_optim.h's helpers: every fp32 operation is a statement of its own, never contracted into an FMA, division and
// square root the correctly rounded ones.  om1, om2 and ss are computed once per call on the HOST, in double, and rounded to fp32
// (adam_constants below: what torch.optim.SparseAdam computes in Python floats and then casts).
// `__host__ __device__` like that header: the kernels of pimemb_grad.hip and the host-side check (tests/cpp/adam_step_check.cpp, compared
// with tests/adam_ref.py by tests/test_adam_cpu.py) compile the same text.
#pragma once

#include <math.h>
#include <stdint.h>

#include "pimemb_grad_optim.h"
#include "pimemb_grad_step.h"

namespace pimemb_grad {

PIMEMB_ROWS_HD float adam_sub(float a, float b) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 d = a - b;
    return d;
}

PIMEMB_ROWS_HD float adam_mul(float a, float b) {
    PIMEMB_OPTIM_NO_CONTRACT
    PIMEMB_OPTIM_F32 p = a * b;
    return p;
}

// A moving average stepped towards x: avg + ((x - avg) * om), three roundings.
PIMEMB_ROWS_HD float adam_average(float avg, float x, float om) { return adagrad_add(avg, adam_mul(adam_sub(x, avg), om)); }

// The moments of EMB_ADAM on one element, without the stored value: *m and *v become M' and V'; returns x = M' / (sqrt(V') + eps).
// (The in-place tail and the master-weight tail -- THE MASTER-WEIGHT ADAM STEPS -- differ only in what they subtract ss * x from.)
PIMEMB_ROWS_HD float adam_moments(float g, float *m, float *v, float om1, float om2, float eps) {
    const float m1 = adam_average(*m, g, om1);
    const float v1 = adam_average(*v, adagrad_square(g), om2);
    *m = m1;
    *v = v1;
    return adagrad_div(m1, adagrad_den(v1, eps));
}

// EMB_ADAM on one element: *m and *v become M' and V'; returns the stored bits after the step.
PIMEMB_ROWS_HD uint32_t adam_step(int dtype, uint32_t stored_bits, float g, float *m, float *v, float om1, float om2, float ss, float eps) {
    const float x = adam_moments(g, m, v, om1, om2, eps);
    return step(dtype, stored_bits, x, ss);
}

// EMB_ROWWISE_ADAM, once per row: sum = the tree's sum of squares.  *v becomes V'; returns rate = ss / (sqrt(V') + eps).
PIMEMB_ROWS_HD float rowwise_adam_rate(float sum, uint32_t dim, float *v, float om2, float ss, float eps) {
    const float v1 = adam_average(*v, adagrad_div(sum, (float)dim), om2);
    *v = v1;
    return adagrad_div(ss, adagrad_den(v1, eps));
}

// ... and per element, without the stored value: *m becomes M', which is returned (the step subtracts rate * M').
PIMEMB_ROWS_HD float rowwise_adam_moment(float g, float *m, float om1) {
    const float m1 = adam_average(*m, g, om1);
    *m = m1;
    return m1;
}

// ... and per element: *m becomes M'; returns the stored bits after the step.
PIMEMB_ROWS_HD uint32_t rowwise_adam_step(int dtype, uint32_t stored_bits, float g, float *m, float om1, float rate) {
    const float m1 = rowwise_adam_moment(g, m, om1);
    return step(dtype, stored_bits, m1, rate);
}

// The master element of THE MASTER-WEIGHT ADAM STEPS: P' = P - (scale * x), with (scale, x) = (ss, adam_moments' x) or (rate, M').
PIMEMB_ROWS_HD float adam_master(float p, float x, float scale) { return step_f32(p, x, scale); }

// The three constants of a call, on the host: out = {om1, om2, ss}, each computed in double and rounded to fp32 once.
inline void adam_constants(double lr, double beta1, double beta2, uint64_t t, float out[3]) {
    out[0] = (float)(1.0 - beta1);
    out[1] = (float)(1.0 - beta2);
    out[2] = (float)(lr * sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t)));
}

}  // namespace pimemb_grad
