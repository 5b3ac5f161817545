// pimemb_grad_max.h -- the one-element rule of the max-mode backward (include/pimemb_grad.h, THE MAX-MODE BACKWARD): which position of
// a bag wins an element.  The forward's rule: the first good position is the winner, a later one takes over only where its decoded
// value is GREATER, one strict fp32 compare -- equal values keep the earlier position, and so does -0 against +0 (they compare
// equal).  NaN ordering is out of scope, as in the forward: a compare with a NaN is false, so whatever holds the place keeps it.
// `__host__ __device__` like pimemb_grad_step.h: the kernels of pimemb_grad.hip and the host-side check
// (tests/cpp/grad_max_check.cpp, compared with tests/grad_max_ref.py by tests/test_grad_max_cpu.py) compile the same text.
#pragma once

#include <stdint.h>

#include "pimemb_grad_step.h"

namespace pimemb_grad {

constexpr uint32_t kMaxNoWinner = 0xffffffffu;      // win[b][d] of a bag with no good position (a position is below 2^30)

// Does x, the value of a later position, take over from cur?
PIMEMB_ROWS_HD bool max_takes_over(float x, float cur) { return x > cur; }

// One good position p with the decoded value x, seen in position order: the first becomes the winner, a later one by the rule.
PIMEMB_ROWS_HD void max_visit(float x, uint32_t p, float *cur, uint32_t *win) {
    if (*win == kMaxNoWinner || max_takes_over(x, *cur)) {
        *cur = x;
        *win = p;
    }
}

// c_p[d] of the definition: the bag's gradient where p won the element, +0 elsewhere.
PIMEMB_ROWS_HD float max_pick(uint32_t win, uint32_t p, float g) { return win == p ? g : 0.f; }

}  // namespace pimemb_grad
