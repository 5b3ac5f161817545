"""The definition of the fused master-weight steps (include/pimemb_grad.h, THE MASTER-WEIGHT STEPS) as a loop, composed from the
references the suite already has: the gradient is grad_ref.sparse_grad (position order) or grad_seg_ref.seg_sparse_grad (segmented
order); the SGD step is train_ref.master_step's arithmetic (t = lr * g; M' = M - t: two roundings); Adagrad and row-wise Adagrad
are optim_ref.adagrad_step applied to the master as an "f32" table; the table row is rows_cases.host_encode of the new master row,
written by rows_cases.sequential_update.  For MXFP4 a row with an inf or a NaN is skipped and counted, its master (and state) stored
all the same.  The reference of tests/test_master_cpu.py and tests/test_gpu_master_step.py.  Nothing here runs the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
import optim_ref as orf  # noqa: E402
import rows_cases as rc  # noqa: E402
import train_ref as tr  # noqa: E402

F = np.float32
KINDS = ("f16", "bf16", "e4m3", "e5m2", "mxfp4")
OPTIMIZERS = ("sgd", "adagrad", "rowwise")


def encode_rows(kind, table_bytes, rows, new_rows):
    """table[rows] = enc_T(new_rows): (table bytes, rows left unwritten).  Only MXFP4 leaves a row: one with an inf or a NaN."""
    rows = [int(r) for r in rows]
    new_rows = np.asarray(new_rows, F).reshape(len(rows), -1)
    bad = set()
    if kind == "mxfp4":
        bad = {p for p in range(len(rows)) if not np.isfinite(new_rows[p]).all()}
    src = new_rows.copy()
    for p in bad:
        src[p] = 0                                   # (never written: host_encode wants finite rows)
    if not rows:
        return table_bytes.copy(), 0
    table, skipped = rc.sequential_update(table_bytes, rows, rc.host_encode(kind, src), bad_rows=bad)
    assert skipped == len(bad)
    return table, len(bad)


def master_step(kind, table_bytes, master, opt, ids, off, G, mode="sum", w=None, pad=None, optimizer="sgd", lr=tr.LR, eps=tr.EPS, segment=None,
                contract=False):
    """One fused master step: (table bytes, master, optimizer state, rows int64 [|U|], n_bad, rows that could not be encoded).
    segment None: the position order, else the segmented order with that S.  contract=True is a WRONG step for
    tests/test_master_cpu.py, as in train_ref.master_step: M - lr * g in one rounding."""
    assert kind in KINDS and optimizer in OPTIMIZERS
    n = master.shape[0]
    if segment is None:
        rows, g, n_bad = gr.sparse_grad(n, ids, off, G, mode, w, pad)
    else:
        rows, g, n_bad = sr.seg_sparse_grad(n, ids, off, G, segment, mode, w, pad)
    master = np.array(master, dtype=F, copy=True)
    if optimizer == "sgd":
        if len(rows):
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                if contract:
                    master[rows] = tr.pool_ref.fma32(-F(lr), g, master[rows])
                else:
                    t = F(lr) * g
                    master[rows] = master[rows] - t
    else:
        as_table = master.view(np.uint8).reshape(n, -1)
        as_table, opt = orf.adagrad_step("f32", as_table, opt, rows, g, F(lr), F(eps), rowwise=optimizer == "rowwise")
        master = np.ascontiguousarray(as_table).view(F).reshape(master.shape).copy()
    table, unenc = encode_rows(kind, table_bytes, rows, master[rows] if len(rows) else np.zeros((0, master.shape[1]), F))
    return table, master, opt, rows, n_bad, unenc


def initial_opt(optimizer, n, dim):
    return None if optimizer == "sgd" else np.zeros((n, dim) if optimizer == "adagrad" else (n,), F)


def iterate(kind, dim, mode_name, optimizer, width="i64", k=tr.K, segment=None, grads=None):
    """k master steps over train_ref's batches from train_ref.initial_state: [(table, master, opt, n_bad, unenc) after every step]."""
    st = tr.initial_state(kind, dim)
    table, master, opt = st.table, st.master, initial_opt(optimizer, tr.N_ROWS, dim)
    out = []
    for j, (b, G) in enumerate(tr.train_batches("f32", dim, k)):
        ids, off, mode, w, pad = b.args(mode_name, width)
        table, master, opt, _rows, n_bad, unenc = master_step(kind, table, master, opt, ids, off, G if grads is None else grads[j], mode, w, pad, optimizer,
                                                              segment=segment)
        out.append((table, master, opt, n_bad, unenc))
    return out
