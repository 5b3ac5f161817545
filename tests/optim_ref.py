"""The definition of the fused Adagrad steps (include/pimemb_grad.h, THE ADAGRAD STEPS) as a plain Python loop over the rows of
tests/grad_ref.py's sparse gradient: the reference of tests/test_optim_cpu.py and tests/test_gpu_optim.py.  numpy float32, one
operation per statement (one rounding each; a statement works on all elements of ONE row, which round independently), the pair
tree as list halving.  Nothing here runs the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402

F = np.float32
_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def adagrad_values(w, g, s, lr, eps):
    """Element-wise Adagrad on fp32 values (arrays of one shape): (new w, new s)."""
    w, g, s = np.asarray(w, F), np.asarray(g, F), np.asarray(s, F)
    with np.errstate(**_QUIET):
        q = g * g
        s1 = s + q
        root = np.sqrt(s1)
        den = root + F(eps)
        x = g / den
        prod = F(lr) * x
        new = w - prod
    assert new.dtype == F and s1.dtype == F
    return new, s1


def pair_tree(g):
    """v[0] of the definition: the sum of squares of one row over its fixed tree.  dim % 4 == 0, dim <= 512."""
    g = np.asarray(g, F)
    dim = len(g)
    assert dim % 4 == 0 and 0 < dim <= 512
    pieces = dim // 4
    with np.errstate(**_QUIET):
        sq = g * g
        t = sq[0::4] + sq[1::4]
        t = t + sq[2::4]
        t = t + sq[3::4]
        L = 1
        while L < pieces:
            L *= 2
        L = min(64, L)
        v = [t[l] if l < pieces else F(0.0) for l in range(L)]
        for l in range(L):
            if l + 64 < pieces:
                v[l] = t[l] + t[l + 64]
        while len(v) > 1:
            v = [v[2 * k] + v[2 * k + 1] for k in range(len(v) // 2)]
    assert isinstance(v[0], F)
    return v[0]


def rowwise_step_size(v, dim, s, lr, eps):
    """(step, S') from the tree's sum v: m = v / (float)dim; S' = S + m; step = lr / (sqrt(S') + eps)."""
    with np.errstate(**_QUIET):
        m = F(v) / F(dim)
        s1 = F(s) + m
        root = np.sqrt(s1)
        den = root + F(eps)
        step = F(lr) / den
    assert isinstance(step, F) and isinstance(s1, F)
    return step, s1


def rowwise_values(w, g, s, lr, eps):
    """Row-wise Adagrad on one row of fp32 values: (new w, new s)."""
    w, g = np.asarray(w, F), np.asarray(g, F)
    step, s1 = rowwise_step_size(pair_tree(g), len(g), s, lr, eps)
    with np.errstate(**_QUIET):
        prod = step * g
        new = w - prod
    assert new.dtype == F
    return new, s1


def adagrad_step(kind, table_bytes, state, rows, grads, lr, eps, rowwise=False):
    """(table bytes, state) after the fused step: the rows of U stepped, every other row's bytes and state kept.
    state: float32 [nr_rows, dim], or [nr_rows] row-wise."""
    table = np.array(table_bytes, copy=True)
    state = np.array(state, dtype=F, copy=True)
    for k, r in enumerate(rows):
        r = int(r)
        w = gr.decode(kind, table[r][None, :])[0]
        new, state[r] = (rowwise_values if rowwise else adagrad_values)(w, grads[k], state[r], lr, eps)
        table[r] = gr.encode(kind, new[None, :])[0]
    return table, state
