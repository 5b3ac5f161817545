"""GPU: the backward pass under stream capture.  include/pimemb_grad.h promises for emb_grad_sparse, emb_grad_sgd, emb_grad_step and
the two _multi calls "a pure enqueue": no allocation, no copy, no host wait, the descriptor records as kernel arguments.  A training
step captured once and replayed is where that has to hold: here one graph holds a fused SGD step of two tables, a multi-table
row-wise Adagrad step of three, a prepared pooled lookup over one of the stepped tables and emb_grad_sparse, captured on a side
stream in torch's default capture error mode -- an allocation, a copy or a wait inside a call makes the capture fail -- and replayed
three times with a new gradient in the same buffers each time.  Once on a position-order context, once on a segmented one (S = 8),
on the ragged batch of tests/grad_seg_ref.py; the references are grad_ref.sparse_grad and grad_seg_ref.seg_sparse_grad applied
three times.  One stream, a linear chain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_order_cases as oc  # noqa: E402
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
import pool_ref  # noqa: E402
from grad_gpu import DEV, F, RaggedBatch, bits, check_state, check_table, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

LR, EPS = sr.LR, sr.EPS
S, DIM = 8, 16
SCALES = (F(1), F(-0.75), F(1.3))    # the gradient of replay r is fl(G * SCALES[r])
GUARD = 12345.0
T_SGD, T_MULTI, T_SHAPE = [0, 1], [2, 3, 4], 5
KINDS_SGD, KINDS_MULTI = ("f32", "bf16"), ("f32", "f16", "f32")


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    e.alloc_table(T_SHAPE, sr.RAGGED_ROWS, DIM, pel.lib.EMB_F16)      # (emb_grad_sparse looks at the table's shape only)
    yield e
    e.close()


def reference(batch, order, G):
    ids, off, mode, w, pad = batch.host_args
    if order == "position":
        return gr.sparse_grad(batch.case.nr_rows, ids, off, G, mode, w, pad)
    return sr.seg_sparse_grad(batch.case.nr_rows, ids, off, G, S, mode, w, pad)


@pytest.mark.parametrize("order", ["position", "segmented"])
def test_a_captured_training_step_replays_with_new_gradients(eng, pel, order):
    case = sr.ragged_case(S)
    kw = dict(order="segmented", segment=S, max_dim=DIM) if order == "segmented" else {}
    ctx = eng.grad_context(4096, 1024, **kw)
    B = case.B
    batches = [RaggedBatch(case, "weighted+pad", "i64", DIM, narrow=True), RaggedBatch(case, "sum", "i64", DIM, narrow=True, bags=3 * B // 4),
               RaggedBatch(case, "mean+pad", "i64", DIM, lead=True, narrow=True, bags=B // 2)]
    G0 = [case.grads(DIM, narrow=True)[:b.key[5]] for b in batches]
    Gs = [[(g * c).astype(F) for g in G0] for c in SCALES]                 # [replay][batch]
    d_Gs = [[to_dev(g) for g in row] for row in Gs]
    inits_sgd, inits_multi = [case.step_table(k, DIM) for k in KINDS_SGD], [case.step_table(k, DIM) for k in KINDS_MULTI]
    s0 = oc.init_state(case.nr_rows, DIM, True)
    states = [to_dev(s0) for _ in T_MULTI]

    # ---- what three replays have to leave -----------------------------------------------------------------------------------------
    want_sgd, want_multi, want_state = list(inits_sgd), list(inits_multi), [s0] * 3
    for r in range(3):
        refs = [reference(b, order, Gs[r][k]) for k, b in enumerate(batches)]
        want_sgd = [sr.sgd_table(kind, w, refs[k]) for k, (kind, w) in enumerate(zip(KINDS_SGD, want_sgd))]
        stepped = [sr.adagrad_tables(kind, w, st, refs[k], True) for k, (kind, w, st) in enumerate(zip(KINDS_MULTI, want_multi, want_state))]
        want_multi, want_state = [x[0] for x in stepped], [x[1] for x in stepped]
    want_sparse = refs[2]                                                   # (of the last replay)
    lidx = np.concatenate([np.array(sorted(sr.ragged_runs(S))), np.random.default_rng(7).integers(0, case.nr_rows, size=250)]).astype(np.int64)
    loff = np.arange(0, len(lidx), 4, dtype=np.int64)
    want_out = pool_ref.embedding_bag(gr.decode("f32", want_multi[0]), lidx, loff, "sum")
    once = pool_ref.embedding_bag(gr.decode("f32", sr.adagrad_tables("f32", inits_multi[0], s0, reference(batches[0], order, Gs[0][0]), True)[0]), lidx, loff, "sum")
    assert np.isfinite(want_out).all() and not np.array_equal(bits(want_out), bits(once))
    if order == "segmented":                                                # the two orders leave other bytes on this batch
        assert (sr.sgd_table("f32", inits_sgd[0], reference(batches[0], "position", Gs[0][0])) != sr.sgd_table("f32", inits_sgd[0], reference(batches[0], order, Gs[0][0]))).any()

    # ---- everything the calls read or write lies on the device before the capture ---------------------------------------------------------
    def load():
        for t, k, init in zip(T_SGD + T_MULTI, KINDS_SGD + KINDS_MULTI, inits_sgd + inits_multi):
            load_bytes(eng, t, k, init)
        for st in states:
            st.copy_(to_dev(s0))

    load()
    plan = eng.plan([T_MULTI[0]], [to_dev(lidx)], [to_dev(loff)])
    sp = batches[2]
    rows_out = torch.full((sp.n,), -7, dtype=torch.int64, device=DEV)
    grads_out = torch.full((sp.n, DIM), GUARD, dtype=torch.float32, device=DEV)
    n_unique = torch.zeros((1,), dtype=torch.int64, device=DEV)
    desc, keep = pel.lib.EmbGradDesc(), []
    itype, on_device = ctx._desc(desc, T_SHAPE, sp.idx, sp.off, sp.G, sp.mode, sp.w, sp.pad, 0, keep)
    assert on_device and desc.grad == sp.G.data_ptr()
    step = dict(modes=[b.mode for b in batches], per_sample_weights=[b.w for b in batches], padding_idx=[b.pad for b in batches])
    first = {k: v[:2] for k, v in step.items()}
    stream = torch.cuda.Stream()

    def enqueue():
        h = stream.cuda_stream
        ctx.sgd_step(T_SGD, [b.idx for b in batches[:2]], [b.off for b in batches[:2]], [b.G for b in batches[:2]], LR, stream=h, **first)
        ctx.adagrad_step(T_MULTI, [b.idx for b in batches], [b.off for b in batches], [b.G for b in batches], states, LR, eps=EPS, rowwise=True, multi=True,
                         stream=h, **step)
        plan.launch(h)
        pel.lib.check_grad(ctx._G.emb_grad_sparse(ctx._h, C.byref(desc), itype, rows_out.data_ptr(), grads_out.data_ptr(), sp.n, n_unique.data_ptr(), h))

    try:
        load()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue()                                                       # the warm-up, uncaptured: the code objects are loaded
        torch.cuda.synchronize()
        n_bad = batches[0].n_bad + batches[1].n_bad + sum(b.n_bad for b in batches) + sp.n_bad
        assert ctx.report() == n_bad > 0
        load()
        grads_out.fill_(GUARD)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):                        # (torch's default capture error mode)
            enqueue()
        torch.cuda.synchronize()
        for t, init in zip(T_SGD + T_MULTI, inits_sgd + inits_multi):       # the capture itself ran nothing
            check_table(table_bytes(eng, t), init, ("after the capture", t))
        for r in range(3):
            for b, g in zip(batches, d_Gs[r]):
                b.G.copy_(g)                                                # a new gradient in the same buffer
            graph.replay()
            torch.cuda.synchronize()
        # ---- the results ---------------------------------------------------------------------------------------------------------------
        for k, t in enumerate(T_SGD):
            check_table(table_bytes(eng, t), want_sgd[k], (order, "sgd", k))
        for k, t in enumerate(T_MULTI):
            check_table(table_bytes(eng, t), want_multi[k], (order, "row-wise multi", k))
            check_state(states[k], want_state[k], (order, "row-wise multi", k))
        assert np.array_equal(bits(plan.outputs[0].cpu().numpy()), bits(want_out))
        u = int(n_unique.item())
        oc.check_sparse(rows_out[:u].cpu().numpy(), grads_out[:u].cpu().numpy(), want_sparse, (order, "sparse"))
        assert u < sp.n and (grads_out[u:] == GUARD).all().item()           # nothing is written beyond |U|
        assert ctx.report() == 3 * n_bad
    finally:
        torch.cuda.synchronize()
        plan.destroy()
        ctx.close()
