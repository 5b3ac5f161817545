"""CPU: the composed reference of tests/test_gpu_train_loop.py (tests/train_ref.py) is pinned, and its comparisons bite.
train_ref puts the suite's loop-form references behind one another -- lookup, backward pass, row writer on one table -- so what
is checked here is the ORDER and the batches: the master-row recipe equals torch's sparse EmbeddingBag + SGD loop bit for bit on
exact-valued inputs; the stored rows are the encoding of the master rows; six wrong loops (a lookup before the write, a step over
the wrong table, a contracted product, a writer whose first occurrence wins, a hot copy kept over a step, an id 2^32 + r taken
for row r) are each rejected by the very assertions the GPU file uses; and the generated batches hold what the GPU cases need in
order not to be vacuous.  No GPU work is called."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import rows_cases as rc  # noqa: E402
import train_ref as tr  # noqa: E402
from grad_gpu import bits, check_state, check_table  # noqa: E402
from test_psw_cpu import exact_inputs  # noqa: E402

F = np.float32
RECIPE_SHAPES = sorted({c[:3] for c in tr.RECIPE_CASES + tr.NOWAIT_CASES})


def rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def same_bits(got, want, what):
    """The assertion of every output and master comparison of the GPU file."""
    assert np.array_equal(bits(got), bits(want)), what


# ---- the recipe against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
def test_master_step_equals_torchs_sparse_embedding_bag_with_sgd_on_exact_inputs(padded):
    """Three iterations of nn.EmbeddingBag(sparse=True) + torch.optim.SGD on the CPU: table values k/8, gradients k/4, lr 1/2 --
    every sum, product and difference is exact, so torch's own order and roundings give the same bits."""
    import torch
    dim, lr, pad = 8, 0.5, 5 if padded else None
    table = exact_inputs(dim)[0]
    bag = torch.nn.EmbeddingBag(16, dim, mode="sum", sparse=True, padding_idx=pad, _weight=torch.from_numpy(table.copy()))
    opt = torch.optim.SGD(bag.parameters(), lr=lr)
    state = tr.State("f32", gr.encode("f32", table), table.copy(), None)
    for it in range(3):
        _t, ids, offsets, G, _w = exact_inputs(dim, seed=it)
        opt.zero_grad()
        bag(torch.from_numpy(ids), torch.from_numpy(offsets)).backward(torch.from_numpy(G.copy()))
        opt.step()
        (state, (rows, n_bad)), = tr.run([("master_step", ids, offsets, G, "sum", None, pad, F(lr))], state)
        want = bag.weight.detach().numpy()
        assert n_bad == 0 and len(rows) >= 8
        same_bits(state.master, want, ("master", it))
        check_table(state.table, want.view(np.uint8).reshape(16, -1), ("table", it))
    assert not np.array_equal(state.master, table)


# ---- the stored rows are the encoding of the master rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("e4m3", 16), ("e5m2", 48), ("mxfp4", 32), ("bf16", 24)])
def test_updated_rows_decode_to_the_encoded_master_and_the_others_keep_their_bytes(kind, dim):
    state = tr.initial_state(kind, dim)
    for b, G in tr.train_batches(kind, dim):
        before = state
        (state, (rows, _n)), = tr.run([("master_step",) + b.args("sum")[:2] + (G,) + b.args("sum")[2:] + (tr.LR,)], state)
        same_bits(tr.decode(kind, state.table[rows]), tr.decode(kind, rc.host_encode(kind, state.master[rows])), (kind, b.k))
        rest = np.setdiff1d(np.arange(tr.N_ROWS), rows)
        assert np.array_equal(state.table[rest], before.table[rest]) and np.array_equal(bits(state.master[rest]), bits(before.master[rest]))


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
def test_the_batches_hold_what_the_cases_need():
    batches = [b for b, _G in tr.train_batches("f32", 16)]
    assert len(batches) == tr.K == 3
    for b in batches:
        ids, off = b.ids("i64"), b.offsets
        assert b.B == 40 and len(ids) == b.n and all(0 <= L <= 9 for L in b.lens) and b.lens.max() == 9
        assert all(b.lens[e] == 0 for e in tr.EMPTY_BAGS) and tr.EMPTY_BAGS[-1] == b.B - 1 and 0 < tr.EMPTY_BAGS[0] < b.B - 1
        assert ids.count(tr.HOT) == tr.N_HOT >= 20                                         # (a run of at least 20 for the segmented case)
        lo, hi = int(off[tr.TRIPLE_BAG]), int(off[tr.TRIPLE_BAG + 1])
        assert ids[lo:hi].count(tr.HOT) == 3
        assert ids.count(tr.PAD) == 2
        bad = [v for v in ids if not 0 <= v < tr.N_ROWS]
        assert len(bad) == b.n_bad == 3 and any(v >= 2 ** 32 and 0 <= v % 2 ** 32 < tr.N_ROWS for v in bad) and any(v < 0 for v in bad)
        bad32 = [v for v in b.ids("u32") if not 0 <= v < tr.N_ROWS]
        assert len(bad32) == 3 and all(tr.N_ROWS <= v < 2 ** 32 for v in bad32)
        assert int(off[0]) == b.lead == (2 if b.k == 0 else 0) and all(p >= b.lead for p in b.bad_at + b.pad_at)
        assert set(tr.TOP) <= set(b.named_rows("sum+pad").tolist())
        for mode in ("sum", "mean+pad", "weighted+pad"):                                   # named_rows is grad_ref's unique list
            a = b.args(mode)
            rows, _g, n_bad = gr.sparse_grad(tr.N_ROWS, a[0], a[1], b.grads(4), a[2], a[3], a[4])
            assert np.array_equal(rows, b.named_rows(mode)) and n_bad == 3
        G = b.grads(16)
        binades = np.unique(np.floor(np.log2(np.abs(G).max(axis=1))))
        assert 7 <= len(binades) <= 9 and (G != 0).all() and (b.weights != 0).all()
    lead = batches[0]
    assert tuple(lead.ids()[:2]) == tr.LEAD_ROWS and not set(tr.LEAD_ROWS) & set(lead.named_rows().tolist())
    for a, b in zip(batches[:-1], batches[1:]):
        ra, rb = set(a.named_rows().tolist()), set(b.named_rows().tolist())
        assert len(ra & rb) > len(tr.TOP) + 5 and ra - rb and rb - ra
    lb = tr.lookup_batch()
    assert lb.n > 2 * lb.B and ((0 <= lb.ids) & (lb.ids < tr.N_ROWS)).all() and (lb.ids == tr.PAD).sum() == 2
    count = np.bincount(lb.ids, minlength=tr.N_ROWS)
    assert set(np.argsort(-count, kind="stable")[:16].tolist()) == set(tr.TOP) and (count[list(tr.TOP)] == 8).all()
    assert np.sort(count)[-17] <= 5
    ends = np.append(lb.offsets[1:], lb.n)
    assert ((ends - lb.offsets) == 0).sum() == 2 and ends[-1] == lb.offsets[-1]


@pytest.mark.parametrize("kind,dim,mode", RECIPE_SHAPES, ids=[f"{k}-{d}-{m}" for k, d, m in RECIPE_SHAPES])
def test_every_iteration_of_the_recipe_shows_in_the_master_the_table_and_the_output(kind, dim, mode):
    """What keeps the GPU cases from being vacuous: in every iteration every named row changes its master bits, at least one
    named row changes its stored bytes, no other row changes, and the pooled output after the step differs from the one before."""
    state = tr.initial_state(kind, dim)
    res = tr.run(tr.recipe_events(dim, mode), state)
    batches = tr.train_batches(kind, dim)
    for k, (b, _G) in enumerate(batches):
        (s0, out0), (s1, (rows, n_bad)), (s2, out1) = res[3 * k:3 * k + 3]
        assert n_bad == 3 and np.array_equal(rows, b.named_rows(mode)) and len(rows) > 60
        assert (bits(s1.master[rows]) != bits(s0.master[rows])).any(axis=1).all(), (kind, k)
        changed = np.flatnonzero((s1.table != s0.table).any(axis=1))
        assert changed.size >= 1 and np.isin(changed, rows).all(), (kind, k)
        assert np.isfinite(s1.master).all() and np.isfinite(tr.decode(kind, s1.table)).all()
        assert s2 is s1 and not np.array_equal(bits(out0), bits(out1)), (kind, k)
        assert np.isfinite(out1).all()


def test_the_captured_loop_changes_the_output_in_every_iteration():
    res = tr.run(tr.graph_events(16, "sum"), tr.initial_state("e4m3", 16))
    assert len(res) == 12
    for j in range(4):
        (s0, out0), (s1, (rows, n_bad)), (_s, out1) = res[3 * j:3 * j + 3]
        assert n_bad == 3 and (s1.table != s0.table).any() and not np.array_equal(bits(out0), bits(out1))
    assert not np.array_equal(bits(tr.graph_grads(16)[0]), bits(tr.graph_grads(16)[3]))


# ---- the wrong loops --------------------------------------------------------------------------------------------------------------------
def recipe_step(state, b, G, mode, **kw):
    a = b.args(mode)
    table, master, rows, n_bad = tr.master_step(state.kind, state.table, state.master, a[0], a[1], G, a[2], a[3], a[4], tr.LR, **kw)
    return state._replace(table=table, master=master), rows


@pytest.mark.parametrize("kind,dim,mode", [("e4m3", 16, "sum"), ("mxfp4", 32, "mean+pad"), ("bf16", 24, "sum")])
def test_a_lookup_placed_before_the_write_is_rejected(kind, dim, mode):
    b, G = tr.train_batches(kind, dim)[0]
    lb = ("lookup",) + tr.lookup_batch().args(mode)
    step = ("master_step",) + b.args(mode)[:2] + (G,) + b.args(mode)[2:] + (tr.LR,)
    want = tr.run([step, lb], tr.initial_state(kind, dim))[1][1]
    early = tr.run([lb, step], tr.initial_state(kind, dim))[0][1]
    rejected(same_bits, early, want, "lookup before the write")


def test_a_step_over_the_wrong_table_is_rejected():
    """The gradient of per_sample_weights taken from the written table instead of the one the forward read; and a fused step
    that did not wait for the writer: it steps the rows as they were before the write."""
    ev = tr.psw_events(8)
    state = tr.initial_state("f16", 8, master=False)
    (_s0, (dw0, n0)), (_s1, skipped), (_s2, (dw1, n1)) = tr.run(ev, state)
    assert n0 == n1 == 3 and skipped == 0
    rejected(same_bits, dw1, dw0, "weights gradient over the written table")
    for kind, dim, mode, optimizer in (("f32", 16, "weighted+pad", "adagrad"), ("bf16", 48, "mean", "rowwise")):
        step0, write, step1, _lookup = tr.interleaved_events(dim, mode, optimizer)
        state = tr.initial_state(kind, dim, master=False, optimizer=optimizer)
        want = tr.run([step0, write, step1], state)[-1][0]
        late = tr.run([step0, step1, write], state)[-1][0]
        rejected(check_table, late.table, want.table, (kind, "write behind the second step"))
        check_state(late.opt, want.opt, (kind, "state"))                                       # (the state follows the gradients alone)
        both = np.intersect1d(write[1], step1[1])                                              # written, then stepped again
        assert both.size >= 4


@pytest.mark.parametrize("kind,dim,mode", [("e4m3", 16, "sum"), ("mxfp4", 32, "weighted+pad"), ("f16", 8, "mean+pad")])
def test_a_contracted_master_update_is_rejected(kind, dim, mode):
    """master - lr * g in one rounding (an FMA) instead of two: the master differs in bits in the first iteration already."""
    b, G = tr.train_batches(kind, dim)[0]
    state = tr.initial_state(kind, dim)
    want, _rows = recipe_step(state, b, G, mode)
    fused, _rows = recipe_step(state, b, G, mode, contract=True)
    rejected(same_bits, fused.master, want.master, "contracted")
    assert (bits(fused.master) != bits(want.master)).sum() > 20


@pytest.mark.parametrize("kind,dim", [("f32", 16), ("bf16", 48), ("bf16", 16)])
def test_a_writer_whose_first_occurrence_wins_is_rejected(kind, dim):
    _step0, write, _step1, _lookup = tr.interleaved_events(dim, "sum", "sgd")
    state = tr.initial_state(kind, dim, master=False)
    want, _m, skipped = tr.write_rows(kind, state.table, None, write[1], write[2])
    first, _m, _s = tr.write_rows(kind, state.table, None, write[1], write[2], first_wins=True)
    assert skipped == 0 and len(write[1]) == tr.WRITE_ROWS and len(np.unique(write[1])) == tr.WRITE_ROWS - 8
    rejected(check_table, first, want, "first occurrence wins")


@pytest.mark.parametrize("kind,dim,fused", [("f32", 32, True), ("e4m3", 16, False)])
def test_a_hot_copy_kept_over_a_step_is_rejected(kind, dim, fused):
    """Lookups that go on serving the rows of TOP as they were before the step."""
    b, G = tr.train_batches(kind, dim)[0]
    state = tr.initial_state(kind, dim, master=not fused)
    a = b.args("sum")
    if fused:
        table = tr.fused_step(kind, state.table, None, a[0], a[1], G, "sum")[0]
    else:
        table = recipe_step(state, b, G, "sum")[0].table
    stale = table.copy()
    stale[list(tr.TOP)] = state.table[list(tr.TOP)]
    assert (stale != table).any(axis=1).sum() >= 8
    lb = tr.lookup_batch().args("sum")
    rejected(same_bits, tr.forward(kind, stale, *lb), tr.forward(kind, table, *lb), "hot copy kept")
    rejected(same_bits, tr.forward(kind, state.table, *lb), tr.forward(kind, table, *lb), "the first output")


@pytest.mark.parametrize("kind,dim,mode", [("e4m3", 16, "sum"), ("bf16", 24, "sum"), ("mxfp4", 32, "mean+pad")])
def test_an_id_truncated_to_its_low_word_is_rejected(kind, dim, mode):
    b, G = tr.train_batches(kind, dim)[0]
    state = tr.initial_state(kind, dim)
    want, _rows = recipe_step(state, b, G, mode)
    a = b.args(mode)
    low = [v % 2 ** 32 if v >= 2 ** 32 else v for v in a[0]]
    assert low != a[0]
    table, master, _rows, n_bad = tr.master_step(kind, state.table, state.master, low, a[1], G, a[2], a[3], a[4], tr.LR)
    assert n_bad == 2
    rejected(same_bits, master, want.master, "2^32 + r as row r")
    if kind == "bf16":
        rejected(check_table, table, want.table, "2^32 + r as row r")


# ---- what the GPU cases assert on the reference -----------------------------------------------------------------------------------------
def test_the_weights_gradient_differs_on_every_named_position_after_the_write():
    ev = tr.psw_events(8)
    (_s0, (dw0, _n0)), _w, (_s2, (dw1, _n1)) = tr.run(ev, tr.initial_state("f16", 8, master=False))
    b = tr.train_batches("f16", 8, 1)[0][0]
    named = np.isin(np.array([v if 0 <= v < tr.N_ROWS else -1 for v in b.ids()]), b.named_rows("weighted+pad"))
    named[:b.lead] = False
    assert named.sum() > 150 and (bits(dw0) != bits(dw1))[named].all() and (bits(dw0[~named]) == 0).all() and (bits(dw1[~named]) == 0).all()


def test_the_segmented_loop_and_the_position_order_loop_end_in_different_tables():
    b = tr.train_batches("bf16", 16, 1)[0][0]
    a = b.args("sum")
    G = b.witness_grads(16)
    rows, g, _n = gr.sparse_grad(tr.N_ROWS, a[0], a[1], G, "sum")
    seg = tr.sr.seg_sparse_grad(tr.N_ROWS, a[0], a[1], G, 8, "sum")[1]
    at = int(np.searchsorted(rows, tr.HOT))
    assert g[at, 0] == 0 and seg[at, 0] == 12 and np.isfinite(g).all() and np.isfinite(seg).all()
    state = tr.initial_state("bf16", 16, master=False)
    pos_end = tr.run(tr.interleaved_events(16, "sum", "sgd", None, witness=True), state)[-1]
    seg_end = tr.run(tr.interleaved_events(16, "sum", "sgd", 8, witness=True), state)[-1]
    rejected(check_table, seg_end[0].table, pos_end[0].table, "the two orders")
    assert (seg_end[0].table[tr.HOT] != pos_end[0].table[tr.HOT]).any()
    assert np.isfinite(pos_end[1]).all() and np.isfinite(seg_end[1]).all()


def test_the_interleaved_sequence_keeps_the_state_of_overwritten_rows():
    for kind, dim, mode, optimizer in (("f32", 16, "weighted+pad", "adagrad"), ("bf16", 48, "mean", "rowwise")):
        ev = tr.interleaved_events(dim, mode, optimizer)
        res = tr.run(ev, tr.initial_state(kind, dim, master=False, optimizer=optimizer))
        (s0, _r0), (s1, skipped), (s2, _r2), (_s3, out) = res
        assert skipped == 0 and np.array_equal(bits(s1.opt), bits(s0.opt)) and (s1.table != s0.table).any()
        only_written = np.setdiff1d(np.intersect1d(ev[1][1], res[0][1][0]), res[2][1][0])
        if only_written.size:                                                               # stepped, overwritten, not stepped again
            assert np.array_equal(bits(s2.opt[only_written]), bits(s0.opt[only_written])) and (s0.opt[only_written] != 0).any()
        assert np.isfinite(out).all() and np.isfinite(tr.decode(kind, s2.table)).all()
