"""GPU: lookups (include/pimemb.h), the backward pass (include/pimemb_grad.h) and the row writer (include/pimemb_rows.h) back to
back on shared tables and one stream, bit for bit against tests/train_ref.py -- the suite's loop-form references put behind one
another.  Each library is compared with its own reference elsewhere; here the three run as a training loop does:
  1  the master-row recipe the headers give for fp8 and MXFP4 tables: emb_grad_sparse, fp32 master rows, emb_rows_update
  2  the same with no host wait, through the C ABI: rows_out pre-filled with -1, a spare master row, the writer's skip count
  3  that loop captured in a graph and replayed with new gradients (the first capture of emb_rows_update)
  4  fused Adagrad / row-wise Adagrad steps with a writer update between them, per table and as multi-table calls
  5  the gradient of per_sample_weights before and behind a write
  6  the hot-set dance: clear the set, step / update, set it again -- the LDS hot-row kernel then serves the new bytes
  7  a segmented context in the same loop, against the position order from the same start
One engine, one position-order context, one writer, one stream; no synchronize between the enqueues of an iteration unless a case
says so.  Tables of 300 rows, three iterations, batches of about 190 positions (train_ref.Batch).  Whole tables are compared with
check_table, states with check_state, outputs and masters by their bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ref as tr  # noqa: E402
from grad_gpu import CODE, DEV, F, SparseCall, bits, check_state, check_table, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

N = tr.N_ROWS
LR, EPS = float(tr.LR), float(tr.EPS)
CANARY = 4321.0
T = 0                                        # the table of the one-table cases


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.grad_context(2048, 512)
    yield c
    c.close()


@pytest.fixture(scope="module")
def writer(eng):
    w = eng.row_writer(2048)
    yield w
    w.close()


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream()


@pytest.fixture(autouse=True)
def counts_start_at_zero(ctx, writer):
    """Every case asserts both reports: a case that failed before reading its own must not fail the next one."""
    ctx.report()
    writer.report()


def same_bits(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, (what, "rows", bad[:8], got[bad[0]], want[bad[0]])


class DevBatch:
    """A train_ref.Batch on the device, with what the calls take."""

    def __init__(self, b, G, mode_name, width="i64"):
        _ids, _off, self.mode, w, self.pad = b.args(mode_name, width)
        self.idx, self.off, self.G = to_dev(b.ids_array(width)), to_dev(b.offsets_array(width)), to_dev(G)
        self.w = None if w is None else to_dev(w)
        self.n, self.n_bad = b.n, b.n_bad

    def step_kw(self):
        return dict(modes=self.mode, per_sample_weights=None if self.w is None else [self.w], padding_idx=self.pad)


class Lookup:
    """train_ref.lookup_batch() on the device."""

    def __init__(self, mode_name):
        _ids, _off, self.mode, w, self.pad = tr.lookup_batch().args(mode_name)
        self.idx, self.off = to_dev(tr.lookup_batch().ids), to_dev(tr.lookup_batch().offsets)
        self.w = None if w is None else [to_dev(w)]

    def plan(self, eng, t=T):
        return eng.plan_pooled([t], [self.idx], [self.off], self.mode, self.w, self.pad)

    def loose(self, eng, t=T):
        return eng.lookup_pooled([t], [self.idx], [self.off], self.mode, self.w, self.pad)[0]


def load_from_master(eng, t, state):
    """The table encoded on the GPU from the master rows; returns the master on the device."""
    master = to_dev(state.master)
    eng.load_table_f32(t, master, CODE[state.kind])
    check_table(table_bytes(eng, t), state.table, (state.kind, "loaded"))
    return master


# ---- 1: the master-row recipe, with the Python API's wait for |U| ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,mode", tr.RECIPE_CASES, ids=[f"{k}-{d}-{m}" for k, d, m in tr.RECIPE_CASES])
def test_master_row_recipe_with_a_host_wait(eng, ctx, writer, stream, kind, dim, mode):
    state = tr.initial_state(kind, dim)
    ref = tr.run(tr.recipe_events(dim, mode), state)
    master = load_from_master(eng, T, state)
    look = Lookup(mode)
    plan = look.plan(eng)                                                           # prepared before the loop
    batches = [DevBatch(b, G, mode) for b, G in tr.train_batches(kind, dim)]
    h = stream.cuda_stream
    torch.cuda.synchronize()
    try:
        for k, b in enumerate(batches):
            with torch.cuda.stream(stream):
                plan.launch(h)
                first = plan.outputs[0].clone()
                rows, grads = ctx.sparse_grad(T, b.idx, b.off, b.G, mode=b.mode, per_sample_weights=b.w, padding_idx=b.pad)
                t = grads * LR                                                      # two torch ops: two roundings
                master[rows] -= t
                assert writer.update(T, rows, master[rows], unique=True) == 0       # `rows` exactly as sparse_grad returned it
                plan.launch(h)
                loose = look.loose(eng)
            torch.cuda.synchronize()
            (_s0, out0), (s1, (want_rows, n_bad)), (_s2, out1) = ref[3 * k:3 * k + 3]
            assert rows.dtype == torch.int64 and np.array_equal(rows.cpu().numpy(), want_rows), (kind, k)
            check_table(table_bytes(eng, T), s1.table, (kind, dim, k))
            same_bits(master, s1.master, (kind, "master", k))
            same_bits(first, out0, (kind, "lookup before the step", k))
            same_bits(plan.outputs[0], out1, (kind, "plan behind the write", k))
            same_bits(loose, out1, (kind, "plan-less lookup behind the write", k))
            assert ctx.report() == n_bad == 3 and writer.report() == 0
    finally:
        torch.cuda.synchronize()
        plan.destroy()


# ---- 2 + 3: the recipe as enqueues only -----------------------------------------------------------------------------------------------
class NoWaitLoop:
    """The recipe with no host wait: every buffer is allocated once, an iteration is enqueue() on the stream.
    rows_out keeps capacity n and is filled with -1 first ("rows and gradients beyond |U| are left as they were"), the master has
    one spare row that the -1 slots are steered to, and the writer gets all n slots: it skips and counts the -1 ids."""

    def __init__(self, eng, ctx, writer, state, mode, width="i64"):
        self.eng, self.ctx, self.writer, self.mode, self.width = eng, ctx, writer, mode, width
        self.dim = state.master.shape[1]
        self.master = torch.zeros((N + 1, self.dim), dtype=torch.float32, device=DEV)
        self.master[:N] = load_from_master(eng, T, state)
        self.n_unique = torch.zeros((1,), dtype=torch.int64, device=DEV)
        self.look = Lookup(mode)
        self.plan = self.look.plan(eng)
        self.first = torch.zeros_like(self.plan.outputs[0])
        self.keep = []

    def set_batch(self, b, G):
        """The buffers of one batch: rows_out and grads_out of capacity n, the descriptor of the raw call."""
        self.b = DevBatch(b, G, self.mode, self.width)
        n = self.n = self.b.n
        self.call = SparseCall(self.ctx, T, self.b.idx, self.b.off, self.b.G, self.b.mode, self.b.w, self.b.pad)
        self.rows_out = torch.zeros((n,), dtype=torch.int64, device=DEV)
        self.grads_out = torch.zeros((n, self.dim), dtype=torch.float32, device=DEV)
        self.spare = torch.full((n,), N, dtype=torch.int64, device=DEV)
        assert self.b.idx.dtype == (torch.int64 if self.width == "i64" else torch.int32)
        return self

    def enqueue(self, h):
        """On torch's current stream, which is `h`."""
        self.rows_out.fill_(-1)
        self.grads_out.fill_(CANARY)
        self.plan.launch(h)
        self.first.copy_(self.plan.outputs[0])
        self.call.enqueue(self.rows_out, self.grads_out, self.n_unique, h)
        r = torch.where(self.rows_out >= 0, self.rows_out, self.spare)
        t = self.grads_out * LR
        new = self.master[r] - t
        self.master.index_copy_(0, r, new)
        self.writer.update(T, self.rows_out, new, stream=h)                         # all n slots, flags 0
        self.plan.launch(h)
        self.keep = [r, t, new]

    def check(self, ref3, what):
        """After the one synchronize of an iteration."""
        (_s0, out0), (s1, (want_rows, n_bad)), (_s2, out1) = ref3
        u = int(self.n_unique.item())
        rows, grads = self.rows_out.cpu().numpy(), self.grads_out.cpu().numpy()
        assert u == len(want_rows) < self.n and np.array_equal(rows[:u], want_rows) and (rows[u:] == -1).all(), what
        assert (grads[u:] == F(CANARY)).all(), (what, "gradients beyond |U| were written")
        check_table(table_bytes(self.eng, T), s1.table, what)
        same_bits(self.master[:N], s1.master, (what, "master"))
        same_bits(self.first, out0, (what, "lookup before the step"))
        same_bits(self.plan.outputs[0], out1, (what, "lookup behind the write"))
        assert self.writer.report() == self.n - u and self.ctx.report() == n_bad == 3, what

    def close(self):
        torch.cuda.synchronize()
        self.plan.destroy()


@pytest.mark.parametrize("kind,dim,mode,width", tr.NOWAIT_CASES, ids=[f"{k}-{d}-{m}-{w}" for k, d, m, w in tr.NOWAIT_CASES])
def test_master_row_recipe_without_a_host_wait(eng, ctx, writer, stream, kind, dim, mode, width):
    state = tr.initial_state(kind, dim)
    ref = tr.run(tr.recipe_events(dim, mode, width), state)
    loop = NoWaitLoop(eng, ctx, writer, state, mode, width)
    try:
        for k, (b, G) in enumerate(tr.train_batches(kind, dim)):
            loop.set_batch(b, G)                                                    # (the batches differ in n; table and master go on)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                loop.enqueue(stream.cuda_stream)
            torch.cuda.synchronize()                                                # the one wait of the iteration: for the comparison
            loop.check(ref[3 * k:3 * k + 3], (kind, dim, width, k))
    finally:
        loop.close()


def test_the_recipe_captured_in_a_graph_replays_with_new_gradients(eng, ctx, writer, stream):
    """Iteration 0 runs uncaptured; then fill_, plan launch, emb_grad_sparse, the master ops, emb_rows_update and the second plan
    launch are captured on the same stream in torch's default capture error mode -- an allocation, a copy or a wait inside a call
    makes the capture fail -- and replayed three times with a new gradient in the same buffer.
    (This case found the writer clearing its duplicate hash with hipMemsetAsync: replays then stored no row.  It is a kernel now.)"""
    kind, dim, mode = "e4m3", 16, "sum"
    state = tr.initial_state(kind, dim)
    ref = tr.run(tr.graph_events(dim, mode), state)
    Gs = tr.graph_grads(dim)
    b = tr.train_batches(kind, dim, 1)[0][0]
    loop = NoWaitLoop(eng, ctx, writer, state, mode).set_batch(b, Gs[0])
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            loop.enqueue(stream.cuda_stream)                                        # the warm-up: the code objects are loaded
        torch.cuda.synchronize()
        loop.check(ref[0:3], "uncaptured")
        before = (table_bytes(eng, T), loop.master.cpu().numpy(), loop.rows_out.cpu().numpy(), loop.plan.outputs[0].cpu().numpy())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            loop.enqueue(stream.cuda_stream)
        torch.cuda.synchronize()
        check_table(table_bytes(eng, T), before[0], "the capture itself ran nothing")
        assert np.array_equal(bits(loop.master.cpu().numpy()), bits(before[1])) and np.array_equal(loop.rows_out.cpu().numpy(), before[2])
        assert np.array_equal(bits(loop.plan.outputs[0].cpu().numpy()), bits(before[3]))
        assert writer.report() == 0 and ctx.report() == 0
        for j in (1, 2, 3):
            loop.b.G.copy_(to_dev(Gs[j]))                                           # a new gradient in the same buffer
            graph.replay()
            torch.cuda.synchronize()
            loop.check(ref[3 * j:3 * j + 3], ("replay", j))
    finally:
        loop.close()


# ---- 4 + 7: fused steps and row writes interleaved ------------------------------------------------------------------------------------
def run_interleaved(eng, c, writer, stream, tables, events, multi=False):
    """tables: [(table id, kind, optimizer, state tensor or None)], events: per table the four events of
    train_ref.interleaved_events.  Step, write, step on every table, then ONE launch of a plan prepared before the first step --
    all on the stream, no wait in between.  Returns the plan's outputs as numpy arrays."""
    look = Lookup("sum")
    plan = eng.plan([t for t, *_ in tables], [look.idx] * len(tables), [look.off] * len(tables))
    h = stream.cuda_stream

    def on_device(ev):                                                              # everything lies on the device before the first enqueue
        _name, ids, off, G, mode, w, pad = ev[:7]
        return (to_dev(np.array(ids, dtype=np.int64)), to_dev(off), to_dev(G), mode, None if w is None else [to_dev(w)], pad)

    steps = {at: [on_device(ev[at]) for ev in events] for at in (0, 2)}
    writes = [(to_dev(ev[1][1]), to_dev(ev[1][2])) for ev in events]

    def step(at):
        for (t, _kind, optimizer, st), (idx, off, G, mode, w, pad) in zip(tables, steps[at]):
            kw = dict(modes=mode, per_sample_weights=w, padding_idx=pad, stream=h, multi=multi)
            if optimizer == "sgd":
                c.sgd_step([t], [idx], [off], [G], LR, **kw)
            else:
                c.adagrad_step([t], [idx], [off], [G], [st], LR, eps=EPS, rowwise=optimizer == "rowwise", **kw)

    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            step(0)
            for (t, *_), (ids, rows) in zip(tables, writes):
                writer.update(t, ids, rows, stream=h)                               # duplicates: the last occurrence wins
            step(2)
            plan.launch(h)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in plan.outputs]
    finally:
        torch.cuda.synchronize()
        plan.destroy()


INTERLEAVED = (("f32", 16, "weighted+pad", "adagrad"), ("bf16", 48, "mean", "rowwise"))


@pytest.mark.parametrize("multi", [False, True], ids=["per-table", "multi"])
def test_fused_steps_and_row_writes_interleaved(eng, ctx, writer, stream, multi):
    """Step on batch 0, a writer update of 64 rows (half of them rows the step just changed), step on batch 1 -- it reads the
    written rows, and an overwritten row keeps its optimizer state --, then the lookup through a plan prepared before all of it."""
    tables, events, want = [], [], []
    for t, (kind, dim, mode, optimizer) in enumerate(INTERLEAVED):
        s0 = tr.initial_state(kind, dim, master=False, optimizer=optimizer)
        load_bytes(eng, t + 1, kind, s0.table)
        ev = tr.interleaved_events(dim, mode, optimizer)
        tables.append((t + 1, kind, optimizer, to_dev(s0.opt)))
        events.append(ev)
        want.append(tr.run(ev, s0))
    outs = run_interleaved(eng, ctx, writer, stream, tables, events, multi)
    for (t, kind, _o, st), res, out in zip(tables, want, outs):
        end = res[2][0]
        check_table(table_bytes(eng, t), end.table, (kind, multi))
        check_state(st, end.opt, (kind, multi))
        same_bits(out, res[3][1], (kind, multi, "lookup"))
        assert res[1][1] == 0
    assert ctx.report() == sum(r[0][1][1] + r[2][1][1] for r in want) == 12 and writer.report() == 0


def test_a_segmented_context_in_the_loop(eng, ctx, writer, stream):
    """Fused SGD on a context of EMB_GRAD_ORDER_SEGMENTED, S = 8, over batches in which row HOT occurs 21 times, a writer update
    in between; then the same events on the position-order context from the same start.  Each equals its own reference
    (grad_seg_ref / grad_ref), and the two references end in different tables: column 0 of row HOT shows the order."""
    kind, dim = "bf16", 16
    s0 = tr.initial_state(kind, dim, master=False)
    ends = {}
    with eng.grad_context(2048, 512, order="segmented", segment=8, max_dim=64) as seg:
        for name, c, S in (("segmented", seg, 8), ("position", ctx, None)):
            ev = tr.interleaved_events(dim, "sum", "sgd", S, witness=True)
            res = tr.run(ev, s0)
            load_bytes(eng, T, kind, s0.table)
            out, = run_interleaved(eng, c, writer, stream, [(T, kind, "sgd", None)], [ev])
            check_table(table_bytes(eng, T), res[2][0].table, name)
            same_bits(out, res[3][1], (name, "lookup"))
            assert c.report() == 6 and writer.report() == 0
            ends[name] = res[2][0].table
    assert (ends["segmented"][tr.HOT] != ends["position"][tr.HOT]).any()


# ---- 5: the gradient of per_sample_weights around a write ---------------------------------------------------------------------------------
def test_weights_gradient_before_and_behind_a_write(eng, ctx, writer, stream):
    kind, dim = "f16", 8
    s0 = tr.initial_state(kind, dim, master=False)
    ev = tr.psw_events(dim)
    (_a, (dw0, n0)), (s1, skipped), (_b, (dw1, n1)) = tr.run(ev, s0)
    assert skipped == 0 and (bits(dw0) != bits(dw1)).sum() > 150
    load_bytes(eng, T, kind, s0.table)
    b, G = tr.train_batches(kind, dim, 1)[0]
    d = DevBatch(b, G, "weighted+pad")
    outs = [torch.full((d.n + 8,), CANARY, dtype=torch.float32, device=DEV) for _ in range(2)]
    ids, rows = to_dev(ev[1][1]), to_dev(ev[1][2])
    h = stream.cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ctx.weights_grad(T, d.idx, d.off, d.G, padding_idx=d.pad, outs=outs[0][:d.n], stream=h)
        writer.update(T, ids, rows, unique=True, stream=h)
        ctx.weights_grad(T, d.idx, d.off, d.G, padding_idx=d.pad, outs=outs[1][:d.n], stream=h)
    torch.cuda.synchronize()
    for o, want, what in zip(outs, (dw0, dw1), ("over the old bytes", "over the new bytes")):
        got = o.cpu().numpy()
        assert np.array_equal(bits(got[:d.n]), bits(want)), what
        assert (got[d.n:] == F(CANARY)).all()
    check_table(table_bytes(eng, T), s1.table, "written")
    assert ctx.report() == n0 + n1 == 6 and writer.report() == 0


# ---- 6: the hot-set dance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,fused", [("f32", 32, True), ("e4m3", 16, False)], ids=["f32-32-fused-sgd", "e4m3-16-master-recipe"])
def test_the_hot_set_dance_serves_the_new_bytes(eng, ctx, writer, stream, pel, oracle, kind, dim, fused):
    """set_hot_rows(top), lookup (the LDS hot-row kernel, kind 4); the step / update is refused; clear, step / update, set again,
    lookup: kind 4 again, over the NEW rows.  A plan from before the dance is refused at launch, one built after it is right."""
    UNS = pel.lib.EMB_ERR_UNSUPPORTED
    s0 = tr.initial_state(kind, dim, master=not fused)
    b, G = tr.train_batches(kind, dim, 1)[0]
    a = b.args("sum")
    if fused:
        load_bytes(eng, T, kind, s0.table)
        s1 = s0._replace(table=tr.fused_step(kind, s0.table, None, a[0], a[1], G, "sum", optimizer="sgd", lr=tr.LR)[0])
    else:
        master = load_from_master(eng, T, s0)
        table, m1, want_rows, _n = tr.master_step(kind, s0.table, s0.master, a[0], a[1], G, "sum", lr=tr.LR)
        s1 = s0._replace(table=table, master=m1)
    lb = tr.lookup_batch()
    want0, want1 = (tr.forward(kind, s.table, lb.ids, lb.offsets) for s in (s0, s1))
    assert not np.array_equal(bits(want0), bits(want1)) and set(tr.TOP) <= set(b.named_rows().tolist())
    assert np.array_equal(bits(want1), bits(oracle.c_bag_sum(tr.decode(kind, s1.table), lb.ids, lb.offsets)))
    d = DevBatch(b, G, "sum")
    look = Lookup("sum")
    top = list(tr.TOP)
    h = stream.cuda_stream
    stale = eng.plan([T], [look.idx], [look.off])                                   # built before the dance
    cache, eng.plan_cache_size = eng.plan_cache_size, 0                             # (plain launches: one launch per lookup, every one counted)
    try:
        eng.set_hot_rows(T, top)
        eng.reset_stats()
        with torch.cuda.stream(stream):
            out0 = eng.lookup_batched([T], [look.idx], [look.off])[0]
        torch.cuda.synchronize()
        assert eng.stats()["n_launches_by_kind"][4] == 1
        same_bits(out0, want0, (kind, "hot set staged"))
        # the step / update is refused while the set is staged, and writes nothing
        with pytest.raises(pel.PimembError) as ei:
            if fused:
                ctx.sgd_step([T], [d.idx], [d.off], [d.G], LR, stream=h)
            else:
                writer.update(T, to_dev(np.arange(8, dtype=np.int64)), torch.zeros((8, dim), dtype=torch.float32, device=DEV), stream=h)
        assert ei.value.code == UNS and "clear the set" in str(ei.value) and "set it again" in str(ei.value)
        check_table(table_bytes(eng, T), s0.table, (kind, "refused"))
        # clear the set, step / update, set it again
        eng.set_hot_rows(T, [])
        with torch.cuda.stream(stream):
            if fused:
                ctx.sgd_step([T], [d.idx], [d.off], [d.G], LR, stream=h)
            else:
                rows, grads = ctx.sparse_grad(T, d.idx, d.off, d.G)
                t = grads * LR
                master[rows] -= t
                writer.update(T, rows, master[rows], unique=True)
        eng.set_hot_rows(T, top)
        with torch.cuda.stream(stream):
            out1 = eng.lookup_batched([T], [look.idx], [look.off])[0]
        torch.cuda.synchronize()
        assert eng.stats()["n_launches_by_kind"][4] == 2                            # the hot-row kernel again
        check_table(table_bytes(eng, T), s1.table, (kind, "stepped"))
        same_bits(out1, want1, (kind, "the re-staged set serves the new bytes"))
        assert not np.array_equal(bits(out1.cpu().numpy()), bits(out0.cpu().numpy()))
        # prepared plans over the table must be re-created
        with pytest.raises(pel.PimembError) as ei:
            stale.launch(h)
        assert "stale" in str(ei.value)
        fresh = eng.plan([T], [look.idx], [look.off])
        try:
            fresh.launch(h)
            torch.cuda.synchronize()
            assert eng.stats()["n_launches_by_kind"][4] == 3
            same_bits(fresh.outputs[0], want1, (kind, "a plan built after the dance"))
        finally:
            torch.cuda.synchronize()
            fresh.destroy()
        assert ctx.report() == 3 and writer.report() == 0
    finally:
        torch.cuda.synchronize()
        eng.plan_cache_size = cache
        eng.set_hot_rows(T, [])
        stale.destroy()
