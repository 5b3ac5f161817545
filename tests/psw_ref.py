"""The definition of the gradient of per_sample_weights (include/pimemb_grad.h, THE GRADIENT OF PER_SAMPLE_WEIGHTS) as a plain
Python loop over positions: the reference of tests/test_psw_cpu.py and tests/test_gpu_psw.py.  numpy float32, one operation per
statement (one rounding each), the tree as list halving; bags, classes and dec are tests/grad_ref.py's.  Nothing here runs the
code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402

F = np.float32
_QUIET = dict(over="ignore", invalid="ignore", under="ignore")


def tree(prod):
    """v[0] of the definition from the products of one position: float32 [dim], any dim >= 1."""
    prod = np.asarray(prod, F)
    dim = len(prod)
    assert dim >= 1
    pieces = (dim + 3) // 4
    with np.errstate(**_QUIET):
        p = np.zeros(4 * pieces, F)                      # absent elements hold +0 and are added
        p[:dim] = prod
        t = p[0::4] + p[1::4]
        t = t + p[2::4]
        t = t + p[3::4]
        L = 1
        while L < pieces:
            L *= 2
        L = min(64, L)
        v = [t[l] if l < pieces else F(0.0) for l in range(L)]
        for l in range(L):
            c = l + 64
            while c < pieces:                            # ((t[l] + t[l+64]) + t[l+128]) + ...
                v[l] = v[l] + t[c]
                c += 64
        while len(v) > 1:
            v = [v[2 * k] + v[2 * k + 1] for k in range(len(v) // 2)]
    assert isinstance(v[0], F)
    return v[0]


def dot(g_row, w_row):
    """dw of one good position: G[b] and dec(W[r]) as float32 [dim]."""
    with np.errstate(**_QUIET):
        prod = np.asarray(g_row, F) * np.asarray(w_row, F)
    return tree(prod)


def weights_grad(kind, table_bytes, indices, offsets, grad, padding_idx=None, n_bags=None, fixed_pooling=0):
    """(dw float32 [n], number of bad positions).  table_bytes: uint8 [nr_rows, stride] of a `kind` ("f32" / "f16" / "bf16")
    table; grad: float32 [B, dim] (any view).  A position that is not good has dw = +0."""
    G = np.asarray(grad, dtype=F)
    W = gr.decode(kind, table_bytes)
    nr_rows = W.shape[0]
    n = len(indices)
    B = len(offsets) if offsets is not None else n_bags
    bags = gr.bags_of(n, offsets, B, fixed_pooling)
    kinds = gr.classify(nr_rows, indices, bags, padding_idx)
    dw = np.zeros(n, F)
    for p in range(n):
        if kinds[p] == "good":
            dw[p] = dot(G[bags[p]], W[int(indices[p])])
    return dw, sum(k == "bad" for k in kinds)
