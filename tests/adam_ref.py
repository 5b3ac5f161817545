"""The definition of the fused Adam steps (include/pimemb_grad.h, THE ADAM STEPS) as a plain Python loop over the rows of
tests/grad_ref.py's sparse gradient: the reference of tests/test_adam_cpu.py and tests/test_gpu_adam.py.  numpy float32, one operation
per statement (one rounding each; a statement works on all elements of ONE row, which round independently); the constants in Python
floats -- doubles -- rounded to fp32 once; the row-wise mean of squares is optim_ref's pair tree.  Nothing here runs the code under test."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402

F = np.float32
_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def constants(lr, betas, step):
    """(om1, om2, ss) as fp32: what torch.optim.SparseAdam computes in Python floats and then casts."""
    b1, b2 = float(betas[0]), float(betas[1])
    return F(1.0 - b1), F(1.0 - b2), F(float(lr) * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step))


def average(avg, x, om):
    """avg + ((x - avg) * om): three roundings."""
    with np.errstate(**_QUIET):
        d = x - avg
        u = d * om
        new = avg + u
    return new


def adam_values(w, g, m, v, om1, om2, ss, eps):
    """EMB_ADAM on fp32 values (arrays of one shape): (new w, M', V', x)."""
    w, g, m, v = (np.asarray(a, F) for a in (w, g, m, v))
    with np.errstate(**_QUIET):
        m1 = average(m, g, F(om1))
        q = g * g
        v1 = average(v, q, F(om2))
        root = np.sqrt(v1)
        den = root + F(eps)
        x = m1 / den
        prod = F(ss) * x
        new = w - prod
    assert new.dtype == F and m1.dtype == F and v1.dtype == F
    return new, m1, v1, x


def rowwise_values(w, g, m, v, om1, om2, ss, eps):
    """EMB_ROWWISE_ADAM on one row of fp32 values, v its one second moment: (new w, M', V')."""
    w, g, m = (np.asarray(a, F) for a in (w, g, m))
    with np.errstate(**_QUIET):
        ms = orf.pair_tree(g) / F(len(g))
        v1 = average(F(v), ms, F(om2))
        root = np.sqrt(v1)
        den = root + F(eps)
        rate = F(ss) / den
        m1 = average(m, g, F(om1))
        prod = rate * m1
        new = w - prod
    assert new.dtype == F and m1.dtype == F and isinstance(v1, F)
    return new, m1, v1


def adam_step(kind, table_bytes, exp_avg, exp_avg_sq, rows, grads, lr, betas, eps, step, rowwise=False, ss=None):
    """(table bytes, exp_avg, exp_avg_sq) after the fused step: the rows of U stepped, every other row's bytes and states kept.
    exp_avg: float32 [nr_rows, dim]; exp_avg_sq the same, or [nr_rows] row-wise.  ss: a step size given instead of step's."""
    table = np.array(table_bytes, copy=True)
    m, v = np.array(exp_avg, dtype=F, copy=True), np.array(exp_avg_sq, dtype=F, copy=True)
    om1, om2, ss_t = constants(lr, betas, step)
    ss_t = ss_t if ss is None else F(ss)
    for k, r in enumerate(rows):
        r = int(r)
        w = gr.decode(kind, table[r][None, :])[0]
        if rowwise:
            new, m[r], v[r] = rowwise_values(w, grads[k], m[r], v[r], om1, om2, ss_t, eps)
        else:
            new, m[r], v[r], _x = adam_values(w, grads[k], m[r], v[r], om1, om2, ss_t, eps)
        table[r] = gr.encode(kind, new[None, :])[0]
    return table, m, v
