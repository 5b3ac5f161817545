"""GPU: the order of additions in the backward pass (libpimemb_grad.so, include/pimemb_grad.h), and the structural edges of its
sort, scan and run walk.  The inputs are tests/grad_order_cases.py's: batches of one-index bags whose gradient columns 0 and 1 hold
+-FLT_MAX in a pattern that overflows to inf as soon as two neighbouring occurrences of a row (beyond the first pair) are added
in the wrong order, column 2 the position's number (exact sums: a dropped, doubled or foreign position), the other columns
randoms, and NaN wherever a position is not good.  tests/test_grad_order_cpu.py shows that EVERY such exchange changes the
reference, and that the comparison used here rejects it.  Every comparison is bit for bit; report() is checked in every case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_order_cases as oc  # noqa: E402
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402
from grad_gpu import DEV, F, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

LR, EPS = oc.LR, F(1e-10)
MAX_N = 4097
# (coefficient path, index width, offsets None with fixed_pooling = 1)
VARIANTS = [(p, w, f) for p in oc.PATHS for w in ("u32", "i64") for f in (False, True)]
ROW_SENTINEL, GRAD_SENTINEL = -7, 12345.0


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.grad_context(MAX_N, MAX_N)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def fresh_count(ctx):
    """Every test starts from a count of 0: a test that failed before its report() does not fail its successors."""
    ctx.report()


_shape_tables = {}


def shape_table(eng, pel, nr_rows, dim):
    """An fp16 table of [nr_rows, dim], allocated once: the sparse gradient depends on the table's shape only."""
    key = (nr_rows, dim)
    if key not in _shape_tables:
        t = 30 + len(_shape_tables)
        eng.alloc_table(t, nr_rows, dim, pel.lib.EMB_F16)
        _shape_tables[key] = t
    return _shape_tables[key]


def device_batch(case, dim, path, width, fixed, narrow=False):
    """(indices, offsets or None, G, mode, weights or None, fixed_pooling) on the device, as the context's methods take them."""
    return (to_dev(case.ids_array(width)), None if fixed else to_dev(case.offsets_array(width)), to_dev(case.grads(dim, narrow, weighted=path == "weighted")),
            "mean" if path == "mean" else "sum", to_dev(case.weights()) if path == "weighted" else None, 1 if fixed else 0)


def sparse(ctx, t, case, dim, path, width, fixed):
    idx, off, G, mode, w, fp = device_batch(case, dim, path, width, fixed and case.one_index)
    return ctx.sparse_grad(t, idx, off, G, mode=mode, per_sample_weights=w, padding_idx=case.pad, fixed_pooling=fp)


def check_all_variants(ctx, t, case, dim, variants=VARIANTS):
    want = case.reference(dim)
    for path, width, fixed in variants:
        rows, grads = sparse(ctx, t, case, dim, path, width, fixed)
        oc.check_sparse(host(rows), host(grads), want, (case.name, dim, path, width, fixed))
        assert ctx.report() == case.n_bad, (case.name, path, width, fixed)


def sgd(ctx, t, batch, pad=None):
    idx, off, G, mode, w, fp = batch
    ctx.sgd_step([t], [idx], None if off is None else [off], [G], LR, modes=mode, per_sample_weights=w, padding_idx=pad, fixed_pooling=fp)


def adagrad(ctx, t, batch, d_state, rowwise, pad=None):
    idx, off, G, mode, w, fp = batch
    ctx.adagrad_step([t], [idx], None if off is None else [off], [G], [d_state], LR, eps=EPS, rowwise=rowwise, modes=mode, per_sample_weights=w,
                     padding_idx=pad, fixed_pooling=fp)


def check_table(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "table rows", bad[:8], got[bad[0]][:16], want[bad[0]][:16])


def check_state(d_state, want, what):
    got = host(d_state).reshape(want.shape)
    bad = np.flatnonzero((oc.bits(got) != oc.bits(want)).reshape(want.shape[0], -1).any(axis=1))
    assert bad.size == 0, (what, "state rows", bad[:8], got[bad[0]], want[bad[0]])


def sgd_case(eng, ctx, case, kind, dim, path, width, fixed, t=2):
    """One fused SGD step; the WHOLE table is compared."""
    rows, grads, _ = case.reference(dim)
    init = oc.step_table(kind, case.nr_rows, dim)
    want = gr.sgd_step(kind, init, rows, grads, LR)
    assert (want != init).any()
    load_bytes(eng, t, kind, init)
    sgd(ctx, t, device_batch(case, dim, path, width, fixed), case.pad)
    check_table(table_bytes(eng, t), want, (case.name, kind, dim, path, width, fixed))
    assert ctx.report() == case.n_bad


def step_case(eng, ctx, case, kind, dim, rowwise, path, width, fixed, t=2):
    """One Adagrad / row-wise Adagrad step on the NARROW columns; the WHOLE table and the WHOLE state are compared."""
    rows, grads, _ = case.reference(dim, narrow=True)
    init, s0 = oc.step_table(kind, case.nr_rows, dim), oc.init_state(case.nr_rows, dim, rowwise)
    want_table, want_state = orf.adagrad_step(kind, init, s0, rows, grads, LR, EPS, rowwise=rowwise)
    assert np.isfinite(want_state).all() and (oc.bits(want_state) != oc.bits(s0)).any()
    load_bytes(eng, t, kind, init)
    d_state = to_dev(s0)
    adagrad(ctx, t, device_batch(case, dim, path, width, fixed, narrow=True), d_state, rowwise, case.pad)
    what = (case.name, kind, dim, "row-wise" if rowwise else "adagrad", path, width, fixed)
    check_table(table_bytes(eng, t), want_table, what)
    check_state(d_state, want_state, what)
    assert ctx.report() == case.n_bad


# ---- run lengths around the look-ahead of eight ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 8, 12, 5])      # one lane; two; three pieces in four lanes; the element-wise kernel
@pytest.mark.parametrize("last_len,with_bad", oc.RUN_CASES)
def test_runs_around_the_look_ahead_keep_position_order(eng, ctx, pel, last_len, with_bad, dim):
    """Runs of 1 .. 129 occurrences, the lengths 7, 8, 9, 15, 16, 17, ... on both sides of every multiple of the eight loads in
    flight; the run of the last row of the sorted order has 1, 7, 8, 9 or 16 occurrences and ends exactly at n, or has exactly one
    position that is not good behind it.  Both index widths, offsets and fixed_pooling = 1, all three coefficient paths."""
    check_all_variants(ctx, shape_table(eng, pel, oc.RUN_ROWS, dim), oc.run_case(last_len, with_bad), dim)


SGD_SHAPES = [("f32", 8, "sum", "i64", False), ("bf16", 4, "weighted", "u32", True), ("f32", 5, "mean", "i64", True)]


@pytest.mark.parametrize("kind,dim,path,width,fixed", SGD_SHAPES, ids=["-".join(map(str, s[:3])) for s in SGD_SHAPES])
@pytest.mark.parametrize("last_len,with_bad", oc.RUN_CASES)
def test_runs_around_the_look_ahead_through_the_sgd_step(eng, ctx, last_len, with_bad, kind, dim, path, width, fixed):
    sgd_case(eng, ctx, oc.run_case(last_len, with_bad), kind, dim, path, width, fixed)


STEP_SHAPES = [("f16", 12, False, "sum", "u32", False), ("f32", 6, False, "mean", "i64", True), ("f32", 8, True, "weighted", "i64", False),
               ("bf16", 320, True, "sum", "u32", True)]


@pytest.mark.parametrize("kind,dim,rowwise,path,width,fixed", STEP_SHAPES, ids=["-".join(map(str, s[:3])) for s in STEP_SHAPES])
@pytest.mark.parametrize("last_len,with_bad", oc.RUN_CASES)
def test_runs_around_the_look_ahead_through_the_adagrad_steps(eng, ctx, last_len, with_bad, kind, dim, rowwise, path, width, fixed):
    """The same ids with columns 0 and 1 replaced by narrow randoms: the squares of +-FLT_MAX would overflow the state.  So in
    these two tails the ORDER rests on the random columns -- which alone witness only a part of the exchanges
    (test_grad_order_cpu prints the share) -- and on the run walk they share with the sparse kernel, which the tests above
    witness in full; what these cases add is the tails on runs of every length: Adagrad on the lane-group kernel (f16, three
    pieces in four lanes) and on the element-wise one (dim 6), row-wise Adagrad with 32 lane groups in a wavefront (f32 dim 8:
    runs of 1 next to 129) and with two walks per lane (bf16 dim 320)."""
    step_case(eng, ctx, oc.run_case(last_len, with_bad), kind, dim, rowwise, path, width, fixed)


# ---- n on the structural boundaries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", oc.EDGE_NS)
def test_n_on_a_slice_wavefront_tile_or_capacity_boundary(eng, ctx, pel, n):
    """n one below, on and one above a 64-position slice, a 256-thread round, a 1024-position tile, two tiles, and the context's
    max_indices (4097); runs that cross all of them."""
    check_all_variants(ctx, shape_table(eng, pel, oc.EDGE_ROWS, 4), oc.edge_case(n), 4)


@pytest.mark.parametrize("n", [1024, 4096, 4097])
def test_n_equal_to_the_contexts_max_indices(eng, pel, n):
    with eng.grad_context(n, n) as own:
        check_all_variants(own, shape_table(eng, pel, oc.EDGE_ROWS, 4), oc.edge_case(n), 4)


# ---- sort passes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 5])
@pytest.mark.parametrize("nr_rows", oc.PASS_ROWS)
def test_one_to_four_sort_passes_and_nr_rows_at_a_byte_boundary(eng, ctx, pel, nr_rows, dim):
    """One pass (up to 255 rows) to four (2^24 rows and more); at 256, 65536 and 2^24 rows the key of a position that is not good,
    nr_rows, needs one more pass than the largest row id.  Rows 0 and nr_rows - 1, and rows that differ in one byte only."""
    eng.alloc_table(21, nr_rows, dim, pel.lib.EMB_F16)
    check_all_variants(ctx, 21, oc.pass_case(nr_rows), dim, [v for k, v in enumerate(VARIANTS) if k % 2 == (dim == 5)])


def test_sgd_over_a_table_of_one_sort_pass(eng, ctx):
    sgd_case(eng, ctx, oc.pass_case(255), "f32", 8, "sum", "i64", False)


def test_sgd_over_a_table_of_four_sort_passes(eng, ctx):
    """2^24 + 1 rows of bf16, dim 4, loaded from a zero tensor on the device: 128 MB, read back once."""
    nr_rows, dim = 2 ** 24 + 1, 4
    case = oc.pass_case(nr_rows)
    rows, grads, _ = case.reference(dim)
    assert rows[-1] == 2 ** 24
    eng.load_table(22, torch.zeros((nr_rows, dim), dtype=torch.bfloat16, device=DEV))
    try:
        sgd(ctx, 22, device_batch(case, dim, "sum", "i64", False))
        got = table_bytes(eng, 22)
        assert ctx.report() == case.n_bad
    finally:
        eng.load_table(22, np.zeros((1, dim), dtype=np.float32))            # (gives the 128 MB back)
    stepped = gr.step_values("bf16", np.zeros((len(rows), 2 * dim), np.uint8), grads, LR)
    assert stepped.any(axis=1).all()
    check_table(got[rows], stepped, "the stepped rows")
    got[rows] = 0
    assert not got.any()                                                          # every other row kept its bytes


# ---- one long run -----------------------------------------------------------------------------------------------------------------
def test_one_run_of_4096_positions_sparse(eng, ctx, pel):
    want = oc.long_case().reference(8)
    assert len(want[0]) == 1
    check_all_variants(ctx, shape_table(eng, pel, oc.RUN_ROWS, 8), oc.long_case(), 8)


def test_one_run_of_4096_positions_through_the_sgd_step(eng, ctx):
    sgd_case(eng, ctx, oc.long_case(), "f32", 8, "weighted", "i64", False)


def test_one_run_of_4096_positions_through_the_rowwise_step(eng, ctx):
    step_case(eng, ctx, oc.long_case(), "f32", 8, True, "sum", "u32", True)


# ---- no host wait: the raw call -----------------------------------------------------------------------------------------------------
def sparse_raw(ctx, pel, t, dim, idx, off, G, mode="sum", w=None, pad=None, fixed_pooling=0):
    """emb_grad_sparse enqueued into sentinel-filled outputs, with no host wait: (rows, grads, count, what must stay alive)."""
    d, keep = pel.lib.EmbGradDesc(), []
    itype, _dev = ctx._desc(d, t, idx, off, G, mode, w, pad, fixed_pooling, keep)
    n = int(idx.shape[0])
    rows = torch.full((n,), ROW_SENTINEL, dtype=torch.int64, device=DEV)
    grads = torch.full((n, dim), GRAD_SENTINEL, dtype=torch.float32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    rc = ctx._G.emb_grad_sparse(ctx._h, C.byref(d), itype, rows.data_ptr(), grads.data_ptr(), n, count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == pel.lib.EMB_OK, ctx._G.emb_grad_last_error()
    return rows, grads, count, keep


def check_raw(raw, want, what):
    rows, grads, count, _keep = raw
    u = int(count.item())
    assert u == len(want[0]), (what, "|U|", u, len(want[0]))
    rows, grads = host(rows), host(grads)
    oc.check_sparse(rows[:u], grads[:u], want, what)
    assert (rows[u:] == ROW_SENTINEL).all() and (grads[u:] == F(GRAD_SENTINEL)).all(), (what, "written beyond |U|")


# ---- nothing good -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", oc.NOTHING)
def test_a_batch_without_a_good_position_changes_nothing(eng, ctx, pel, which):
    """300 positions: all bad ids; all padding; all before offsets[0].  |U| = 0, the outputs keep their sentinels, tables and states
    keep their bytes, and report() says 300, 0 and 0."""
    case, dim = oc.nothing_case(which), 8
    t = shape_table(eng, pel, oc.RUN_ROWS, dim)
    for path, width in (("sum", "i64"), ("mean", "u32"), ("weighted", "i64")):
        idx, off, G, mode, w, _fp = device_batch(case, dim, path, width, False)
        check_raw(sparse_raw(ctx, pel, t, dim, idx, off, G, mode, w, case.pad), (np.zeros(0, np.int64), np.zeros((0, dim), F)), (which, path, width))
        assert ctx.report() == case.n_bad == {"bad": 300, "padding": 0, "nobag": 0}[which]
    for kind in ("f32", "bf16"):
        init = oc.step_table(kind, oc.RUN_ROWS, dim)
        load_bytes(eng, 2, kind, init)
        batch = device_batch(case, dim, "sum", "i64", False)
        sgd(ctx, 2, batch, case.pad)
        assert ctx.report() == case.n_bad
        for rowwise in (False, True):
            s0 = oc.init_state(oc.RUN_ROWS, dim, rowwise)
            d_state = to_dev(s0)
            adagrad(ctx, 2, batch, d_state, rowwise, case.pad)
            assert ctx.report() == case.n_bad
            check_state(d_state, s0, (which, kind, rowwise))
        check_table(table_bytes(eng, 2), init, (which, kind))


# ---- scratch reuse ------------------------------------------------------------------------------------------------------------------
def test_a_context_is_reused_for_smaller_and_other_batches_without_a_host_wait(eng, ctx, pel):
    """On one context, enqueued back to back: the run of 4096 (two passes over 600 rows, five tiles); 65 positions over 255 rows (one
    pass: the result lies in the other buffer, and the scratch beyond 65 still holds the long run's keys); a mean-mode call with
    another B (cnt is zeroed per call); an SGD step; the sparse gradient directly behind it (the scan sums follow the step's
    histogram sums in one buffer).  The first host wait comes after the last of them."""
    dim = 8
    long, small, bags, runs = oc.long_case(), oc.small_case(), oc.bag_case(7), oc.run_case(9, True)
    t600, t255 = shape_table(eng, pel, oc.RUN_ROWS, dim), shape_table(eng, pel, oc.SMALL_ROWS, dim)
    init = oc.step_table("f32", oc.SMALL_ROWS, dim)
    load_bytes(eng, 2, "f32", init)
    b_long, b_small, b_runs = device_batch(long, dim, "sum", "i64", False), device_batch(small, dim, "weighted", "u32", True), device_batch(runs, dim, "mean", "i64", False)
    b_step = device_batch(small, dim, "sum", "i64", False)
    bag_idx, bag_off, bag_G = to_dev(bags.ids), to_dev(bags.offsets), to_dev(bags.grads(dim))
    ctx.report()
    torch.cuda.synchronize()
    r_long = sparse_raw(ctx, pel, t600, dim, *b_long[:5], fixed_pooling=b_long[5])
    r_small = sparse_raw(ctx, pel, t255, dim, *b_small[:5], fixed_pooling=b_small[5])
    r_bags = sparse_raw(ctx, pel, t600, dim, bag_idx, bag_off, bag_G, "mean")
    sgd(ctx, 2, b_step)
    r_runs = sparse_raw(ctx, pel, t600, dim, *b_runs[:5], fixed_pooling=b_runs[5])
    torch.cuda.synchronize()                                                      # the first host wait
    check_raw(r_long, long.reference(dim), "the long run")
    check_raw(r_small, small.reference(dim), "65 positions behind 4096")
    check_raw(r_bags, bags.reference(dim, "mean"), "mean with another B")
    check_raw(r_runs, runs.reference(dim), "sparse behind a step")
    rows, grads, _ = small.reference(dim)
    check_table(table_bytes(eng, 2), gr.sgd_step("f32", init, rows, grads, LR), "the step in between")
    assert ctx.report() == 2 * small.n_bad + runs.n_bad == 3


# ---- bag search -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 5])
@pytest.mark.parametrize("B", oc.BAG_COUNTS)
def test_bag_search_over_empty_leading_and_trailing_bags(eng, ctx, pel, B, dim):
    """B around the powers of two of the binary search; runs of empty bags, several offsets equal to 0 (position 0 belongs to the
    LAST of them) and several equal to n.  G[b, :] = cnt(b) * (b + 1): a position given to a neighbouring bag changes an exact
    integer sum, in sum mode (cnt(b) * (b + 1)) and in mean mode (b + 1)."""
    case = oc.bag_case(B)
    t = shape_table(eng, pel, oc.RUN_ROWS, dim)
    for width in ("u32", "i64"):
        ids = case.ids if width == "i64" else case.ids.astype(np.uint32)
        idx, off, G = to_dev(ids), to_dev(case.offsets.astype(ids.dtype)), to_dev(case.grads(dim))
        for mode in ("sum", "mean"):
            rows, grads = ctx.sparse_grad(t, idx, off, G, mode=mode)
            oc.check_sparse(host(rows), host(grads), case.reference(dim, mode), (B, dim, width, mode))
            assert ctx.report() == 0
