"""The definition of the fused master-weight Adam steps (include/pimemb_grad.h, THE MASTER-WEIGHT ADAM STEPS) as a loop, composed from the
references the suite already has: the gradient is grad_ref.sparse_grad (position order) or grad_seg_ref.seg_sparse_grad (segmented order);
the moments and the master subtract are adam_ref.adam_step applied to the master as an "f32" table (its decode and encode are the identity
there: new = P - (ss * x), or P - (rate * M')); the table row is master_ref.encode_rows of the new master row -- rows_cases.host_encode,
and for MXFP4 a row with an inf or a NaN skipped and counted, its master and moments stored all the same.  The reference of
tests/test_master_adam_cpu.py and tests/test_gpu_master_adam.py.  Nothing here runs the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as ar  # noqa: E402
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
import master_ref as mr  # noqa: E402

F = np.float32
KINDS = mr.KINDS


def master_adam_step(kind, table_bytes, master, exp_avg, exp_avg_sq, ids, off, G, mode="sum", w=None, pad=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                     step=1, rowwise=False, segment=None, ss=None):
    """One fused step: (table bytes, master, exp_avg, exp_avg_sq, rows int64 [|U|], n_bad, rows that could not be encoded).
    segment None: the position order, else the segmented order with that S.  ss: a step size given instead of step's."""
    assert kind in KINDS
    n, dim = master.shape
    if segment is None:
        rows, g, n_bad = gr.sparse_grad(n, ids, off, G, mode, w, pad)
    else:
        rows, g, n_bad = sr.seg_sparse_grad(n, ids, off, G, segment, mode, w, pad)
    as_table = np.array(master, dtype=F, copy=True).view(np.uint8).reshape(n, -1)
    as_table, m, v = ar.adam_step("f32", as_table, exp_avg, exp_avg_sq, rows, g, lr, betas, eps, step, rowwise=rowwise, ss=ss)
    master = np.ascontiguousarray(as_table).view(F).reshape(n, dim).copy()
    table, unenc = mr.encode_rows(kind, table_bytes, rows, master[rows] if len(rows) else np.zeros((0, dim), F))
    return table, master, m, v, rows, n_bad, unenc


def initial_moments(n, dim, rowwise):
    return np.zeros((n, dim), F), np.zeros((n,) if rowwise else (n, dim), F)
