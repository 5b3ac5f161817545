"""GPU: the backward pass through libpimemb_grad.so (include/pimemb_grad.h), bit for bit.  The reference is tests/grad_ref.py, the
definition as an explicit loop over positions (pinned against torch's CPU autograd by tests/test_grad_cpu.py); the inputs are
tests/grad_cases.py's: about 2 000 positions in 301 bags over tables of 3001 rows, with everything that can break a kernel in
them.  Every comparison is np.array_equal on bytes or bits -- no tolerance."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as gc  # noqa: E402
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402
import pool_ref  # noqa: E402
import rows_cases as rc  # noqa: E402
from grad_gpu import DEV, bits, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

N = gc.NR_ROWS
WIDTHS = ["u32", "i64"]
GROUP_DIMS, ELEM_DIMS = [4, 12, 128, 256, 512], [5, 17]


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.grad_context(4096, 512)
    yield c
    c.close()


_shape_tables = {}


def shape_table(eng, dim):
    """An fp32 table of [3001, dim] for the calls that depend on the table's shape only; loaded once per dim."""
    if dim not in _shape_tables:
        t = 32 + len(_shape_tables)
        eng.load_table(t, np.zeros((N, dim), dtype=np.float32))
        _shape_tables[dim] = t
    return _shape_tables[dim]


def batch_on_device(width, mode_name, lead=False):
    """(indices, offsets, weights or None, padding_idx or None, mode) of the big batch as the engine takes them."""
    mode, weighted, padded = gc.MODES[mode_name]
    ids, offsets = gc.bad_ids(width)
    if lead:
        offsets = gc.offsets_lead()
    arr = gc.ids_array(ids, width)
    return to_dev(arr), to_dev(offsets.astype(arr.dtype)), to_dev(gc.weights()) if weighted else None, gc.PAD if padded else None, mode


def check_sparse(got, want, what):
    rows, grads = got
    w_rows, w_grads, _bad = want
    rows, grads = rows.cpu().numpy() if hasattr(rows, "cpu") else rows, grads.cpu().numpy() if hasattr(grads, "cpu") else grads
    assert rows.dtype == np.int64 and grads.dtype == np.float32
    assert len(rows) == len(w_rows), (what, len(rows), len(w_rows))              # |U|
    assert np.array_equal(rows, w_rows), what
    bad = np.flatnonzero((bits(grads) != bits(w_grads)).any(axis=1))
    assert bad.size == 0, (what, rows[bad[:4]], grads[bad[0]][:8], w_grads[bad[0]][:8])


# ---- the sparse gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", GROUP_DIMS + ELEM_DIMS)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode_name", list(gc.MODES))
def test_sparse_grad_equals_the_definition(eng, ctx, mode_name, width, dim):
    idx, off, w, pad, mode = batch_on_device(width, mode_name)
    want = gc.reference(width, mode_name, dim)
    assert want[2] == 5 and gc.HOT in want[0] and 0 in want[0] and 3000 in want[0] and 5 in want[0]
    if mode_name == "sum":
        assert np.isposinf(want[1][list(want[0]).index(5), 0])                   # the row whose sum overflows
    got = ctx.sparse_grad(shape_table(eng, dim), idx, off, to_dev(gc.grads(dim)), mode=mode, per_sample_weights=w, padding_idx=pad)
    check_sparse(got, want, (mode_name, width, dim))
    assert ctx.report() == 5 and ctx.report() == 0                               # the bad positions, counted once


@pytest.mark.parametrize("width", WIDTHS)
def test_positions_before_the_first_offset_belong_to_no_bag(eng, ctx, width):
    idx, off, w, pad, mode = batch_on_device(width, "weighted+pad", lead=True)
    want = gc.reference(width, "weighted+pad", 12, lead=True)
    assert want[2] == 4                                                          # position 1 holds a bad id, but has no bag now
    got = ctx.sparse_grad(shape_table(eng, 12), idx, off, to_dev(gc.grads(12)), mode=mode, per_sample_weights=w, padding_idx=pad)
    check_sparse(got, want, width)
    assert ctx.report() == 4


@pytest.mark.parametrize("dim,col,wide", [(128, 128, 384), (12, 4, 32), (12, 3, 27), (5, 2, 9)])
def test_gradient_is_read_in_place_out_of_a_wider_buffer(eng, ctx, dim, col, wide):
    """grad = buffer + col, grad_ld = the buffer's width.  The other columns hold NaN: one of them read as gradient would show.
    (128 from column 128 of 384 is the [B, 3 * dim] buffer of a concatenated output; column 3 / width 27 is no 16-byte multiple:
    the element-wise kernel.)"""
    idx, off, w, pad, mode = batch_on_device("i64", "mean+pad")
    buf = np.full((gc.N_BAGS, wide), np.nan, dtype=np.float32)
    buf[:, col:col + dim] = gc.grads(dim)
    d_buf = to_dev(buf)
    got = ctx.sparse_grad(shape_table(eng, dim), idx, off, d_buf[:, col:col + dim], mode=mode, padding_idx=pad)
    check_sparse(got, gc.reference("i64", "mean+pad", dim), (dim, col, wide))
    assert ctx.report() == 5


@pytest.mark.parametrize("width", WIDTHS)
def test_fixed_pooling_without_offsets(eng, ctx, width):
    L, dim = 6, 12
    ids, _ = gc.bad_ids(width)
    ids = ids[:gc.N_BAGS * L]
    want = gr.sparse_grad(N, ids, None, gc.grads(dim), "mean", n_bags=gc.N_BAGS, fixed_pooling=L)
    got = ctx.sparse_grad(shape_table(eng, dim), to_dev(gc.ids_array(ids, width)), None, to_dev(gc.grads(dim)), mode="mean", fixed_pooling=L)
    check_sparse(got, want, width)
    assert ctx.report() == want[2]


def test_empty_and_one_position_batches(eng, ctx):
    dim = 12
    G = to_dev(gc.grads(dim))
    t = shape_table(eng, dim)
    rows, grads = ctx.sparse_grad(t, to_dev(np.zeros(0, np.int64)), to_dev(np.zeros(gc.N_BAGS, np.int64)), G)
    assert tuple(rows.shape) == (0,) and tuple(grads.shape) == (0, dim)
    for row, bag in ((3000, 0), (0, 300)):
        off = np.zeros(gc.N_BAGS, np.int64)
        off[bag + 1:] = 1                                                        # the one position lies in bag `bag`
        want = gr.sparse_grad(N, [row], off, gc.grads(dim))
        assert list(want[0]) == [row]
        check_sparse(ctx.sparse_grad(t, to_dev(np.array([row], np.int64)), to_dev(off), G), want, (row, bag))
    rows, grads = ctx.sparse_grad(t, to_dev(np.array([N], np.int64)), to_dev(np.zeros(1, np.int64)), G[:1])      # one bad position: nothing
    assert rows.numel() == 0 and ctx.report() == 1


BIG_ROWS = 70001      # 17 id bits: three passes of the sort, so its result lies in the other buffer than after two


def test_a_batch_of_several_sort_tiles_keeps_position_order(eng):
    """5 157 positions: six tiles of the sort and two chunks of its scan.  Half of the ids come from 300 rows, so runs are long and
    their positions lie tiles apart.  The gradients are randoms over many magnitudes: a rotation or a gross scramble of a run
    shows, but the exchange of two neighbouring occurrences mostly does NOT change these sums (measured: the last two occurrences
    exchanged changed 1 to 7 of 15 runs) -- that every such exchange shows is the business of tests/test_gpu_grad_order.py."""
    rng = np.random.default_rng(77)
    n, B, dim = 5 * 1024 + 37, 200, 8
    ids = np.where(rng.random(n) < 0.5, rng.integers(0, 300, size=n), rng.integers(0, BIG_ROWS, size=n)).astype(np.int64)
    ids[[17, 4000]] = [BIG_ROWS, -3]
    off = np.sort(rng.integers(0, n, size=B)).astype(np.int64)
    off[0] = 0
    G = (rng.standard_normal((B, dim)) * np.exp2(rng.integers(-20, 20, size=(B, 1)))).astype(np.float32)
    w = rng.standard_normal(n).astype(np.float32)
    want = gr.sparse_grad(BIG_ROWS, ids, off, G, "sum", w)
    eng.load_table(20, np.zeros((BIG_ROWS, dim), dtype=np.float32))
    with eng.grad_context(n, B) as big:
        check_sparse(big.sparse_grad(20, to_dev(ids), to_dev(off), to_dev(G), per_sample_weights=to_dev(w)), want, "tiles")
        assert big.report() == 2


def test_a_batch_beyond_one_round_of_the_second_scan_level(eng):
    """4.2 million positions: more than 4096 tiles, so the digit counts fill more than 1024 scan chunks and the single workgroup
    that scans the chunk sums goes round twice.  Gradients are small integers -- every sum is exact in any order -- so the
    reference can be numpy's bincount; the order of additions at scale is the previous test's business."""
    rng = np.random.default_rng(78)
    B, L, dim = 1000, 4200, 4
    n = B * L
    assert (n + 1023) // 1024 * 256 > 1024 * 1024
    ids = rng.integers(0, BIG_ROWS, size=n).astype(np.uint32)
    ids[rng.integers(0, n, size=5000)] = 7
    ids[[5, n - 1]] = [BIG_ROWS, 0xFFFFFFFF]
    G = (rng.integers(1, 3, size=(B, dim)) * rng.choice([-1, 1], size=(B, dim))).astype(np.float32)
    good = ids < BIG_ROWS
    bag = np.arange(n) // L
    w_rows = np.unique(ids[good]).astype(np.int64)
    dense = np.stack([np.bincount(ids[good], weights=G[bag[good], c], minlength=BIG_ROWS) for c in range(dim)], axis=1)
    assert np.abs(dense).max() < 2 ** 20
    eng.load_table(20, np.zeros((BIG_ROWS, dim), dtype=np.float32))
    with eng.grad_context(n, B) as big:
        rows, grads = big.sparse_grad(20, to_dev(ids), None, to_dev(G), fixed_pooling=L)
        assert big.report() == 2
    assert np.array_equal(rows.cpu().numpy(), w_rows)
    assert np.array_equal(grads.cpu().numpy() + np.float32(0), dense[w_rows].astype(np.float32) + np.float32(0))      # (+0: bincount has no -0.0)


def test_numpy_arrays_are_copied_to_the_device_and_back(eng, ctx):
    ids, offsets = gc.bad_ids("u32")
    got = ctx.sparse_grad(shape_table(eng, 17), gc.ids_array(ids, "u32"), offsets, gc.grads(17), mode="sum", per_sample_weights=gc.weights())
    assert isinstance(got[0], np.ndarray)
    check_sparse(got, gc.reference("u32", "weighted", 17), "numpy")
    assert ctx.report() == 5


@pytest.mark.parametrize("kind,dim", [("e4m3", 16), ("e5m2", 12), ("mxfp4", 32)])
def test_sparse_grad_depends_on_the_tables_shape_only(eng, ctx, kind, dim):
    raw = rc.host_encode(kind, np.random.default_rng(1).standard_normal((N, dim)).astype(np.float32))
    load_bytes(eng, 1, kind, raw)
    idx, off, w, pad, mode = batch_on_device("i64", "sum")
    check_sparse(ctx.sparse_grad(1, idx, off, to_dev(gc.grads(dim)), mode=mode), gc.reference("i64", "sum", dim), kind)
    assert ctx.report() == 5
    assert np.array_equal(table_bytes(eng, 1), raw)


def test_sparse_grad_of_a_fixed_point_table_is_unsupported(eng, ctx, pel):
    eng.load_table(1, np.zeros((N, 8), dtype=np.int32))
    idx, off, *_ = batch_on_device("i64", "sum")
    with pytest.raises(pel.PimembError) as ei:
        ctx.sparse_grad(1, idx, off, to_dev(gc.grads(8)))
    assert ei.value.code == pel.lib.EMB_ERR_UNSUPPORTED and "EMB_FIXED32" in str(ei.value)


def test_too_small_a_capacity_is_invalid(eng, ctx, pel):
    import ctypes as C
    idx, off, *_ = batch_on_device("i64", "sum")
    G, d = to_dev(gc.grads(12)), pel.lib.EmbGradDesc()
    ctx._desc(d, shape_table(eng, 12), idx, off, G, "sum", None, None, 0, [])
    rows, grads, count = torch.zeros(64, dtype=torch.int64, device=DEV), torch.zeros((64, 12), device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    rc_ = ctx._G.emb_grad_sparse(ctx._h, C.byref(d), 1, rows.data_ptr(), grads.data_ptr(), 64, count.data_ptr(), None)
    assert rc_ == pel.lib.EMB_ERR_INVALID and b"room for 64 rows" in ctx._G.emb_grad_last_error()
    torch.cuda.synchronize()
    assert not rows.any() and not grads.any()


# ---- the fused SGD step -------------------------------------------------------------------------------------------------------
STEP_CASES = [(k, d, "sum", "i64") for k in ("f32", "f16", "bf16") for d in (4, 8, 24, 128, 5, 17)] + \
             [("f32", 24, "weighted+pad", "u32"), ("bf16", 8, "mean", "u32"), ("f16", 17, "mean+pad", "u32"), ("bf16", 256, "weighted", "i64"),
              ("f16", 512, "sum", "u32")]


@pytest.mark.parametrize("kind,dim,mode_name,width", STEP_CASES, ids=["-".join(map(str, c)) for c in STEP_CASES])
def test_fused_step_equals_the_definition_over_the_whole_table(eng, ctx, kind, dim, mode_name, width):
    """After the step the WHOLE table read back equals grad_ref's bytes: the rows of U stepped (the crafted ties, subnormal and
    overflowing results among them), every other row untouched."""
    idx, off, w, pad, mode = batch_on_device(width, mode_name)
    init = gc.step_table(kind, dim)
    rows, grads, n_bad = gc.reference(width, mode_name, dim)
    want = gr.sgd_step(kind, init, rows, grads, gc.LR)
    changed = np.flatnonzero((want != init).any(axis=1))
    assert len(changed) > len(rows) // 4 and set(changed) <= set(rows.tolist())      # (a small step on a 2-byte weight rounds away)
    load_bytes(eng, 2, kind, init)
    ctx.sgd_step([2], [idx], [off], [to_dev(gc.grads(dim))], gc.LR, modes=mode, per_sample_weights=w, padding_idx=pad)
    got = table_bytes(eng, 2)
    assert ctx.report() == n_bad == 5
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (kind, dim, bad[:8], got[bad[0]][:16], want[bad[0]][:16], init[bad[0]][:16])


@pytest.mark.parametrize("kind,dim", [("f32", 12), ("f16", 8), ("bf16", 17)])
def test_two_steps_in_a_row_without_a_host_wait(eng, ctx, kind, dim):
    idx, off, w, pad, mode = batch_on_device("i64", "weighted")
    init = gc.step_table(kind, dim)
    rows, grads, _ = gc.reference("i64", "weighted", dim)
    rows2, grads2, _ = gc.reference("i64", "mean+pad", dim)
    want = gr.sgd_step(kind, gr.sgd_step(kind, init, rows, grads, gc.LR), rows2, grads2, gc.LR)
    load_bytes(eng, 2, kind, init)
    G = to_dev(gc.grads(dim))
    ctx.sgd_step([2], [idx], [off], [G], gc.LR, modes="sum", per_sample_weights=w)           # the second reuses the scratch of the first
    ctx.sgd_step([2], [idx], [off], [G], gc.LR, modes="mean", padding_idx=gc.PAD)
    assert np.array_equal(table_bytes(eng, 2), want)
    assert ctx.report() == 10


@pytest.mark.parametrize("kind,dim", [("f32", 16), ("bf16", 24)])
def test_a_lookup_behind_the_step_reads_the_stepped_rows(eng, ctx, kind, dim):
    idx, off, w, pad, mode = batch_on_device("i64", "sum")
    init = gc.step_table(kind, dim)
    rows, grads, _ = gc.reference("i64", "sum", dim, overflow=False)
    new = gr.sgd_step(kind, init, rows, grads, gc.LR)
    rng = np.random.default_rng(5)
    lidx = np.concatenate([rows[:300], rng.integers(0, N, size=724)]).astype(np.int64)
    lidx = lidx[~np.isin(lidx, [gc.SPECIAL[("bf16", "over")], gc.SPECIAL[("f16", "over")]])]      # (their stepped rows hold infinities)
    loff = np.arange(0, len(lidx), 4, dtype=np.int64)
    want_old = pool_ref.embedding_bag(gr.decode(kind, init), lidx, loff, "sum")
    want_new = pool_ref.embedding_bag(gr.decode(kind, new), lidx, loff, "sum")
    assert np.isfinite(want_new).all() and not np.array_equal(bits(want_old), bits(want_new))
    load_bytes(eng, 2, kind, init)
    d_lidx, d_loff, G = to_dev(lidx), to_dev(loff), to_dev(gc.grads(dim, overflow=False))
    plan = eng.plan([2], [d_lidx], [d_loff])                                     # prepared BEFORE the step
    torch.cuda.synchronize()
    cache, eng.plan_cache_size = eng.plan_cache_size, 0                          # (plain launches: no plan is built on the way)
    try:
        first = eng.lookup_pooled([2], [d_lidx], [d_loff], "sum")[0]
        ctx.sgd_step([2], [idx], [off], [G], gc.LR)
        second = eng.lookup_pooled([2], [d_lidx], [d_loff], "sum")[0]
        plan.launch(torch.cuda.current_stream().cuda_stream)
    finally:
        eng.plan_cache_size = cache
    torch.cuda.synchronize()                                                     # the first host wait
    got1, got2, got3 = first.cpu().numpy(), second.cpu().numpy(), plan.outputs[0].cpu().numpy()
    plan.destroy()
    assert np.array_equal(bits(got1), bits(want_old))
    assert np.array_equal(bits(got2), bits(want_new)) and np.array_equal(bits(got3), bits(want_new))
    assert np.array_equal(table_bytes(eng, 2), new)
    ctx.report()


def test_several_tables_in_one_call_from_column_views(eng, ctx):
    """Three tables of different dtypes stepped by one call, their gradients the column blocks of ONE [B, 3 * dim] buffer."""
    dim, kinds, modes = 8, ("f32", "f16", "bf16"), ("sum", "mean+pad", "weighted")
    wide = np.concatenate([gc.grads(dim), gc.grads(dim)[::-1], gc.grads(dim) * np.float32(0.5)], axis=1)
    d_wide = to_dev(wide)
    args = [batch_on_device("i64", m) for m in modes]
    for k, kind in enumerate(kinds):
        load_bytes(eng, 3 + k, kind, gc.step_table(kind, dim))
    ctx.sgd_step([3, 4, 5], [a[0] for a in args], [a[1] for a in args], [d_wide[:, k * dim:(k + 1) * dim] for k in range(3)], gc.LR,
                 modes=[a[4] for a in args], per_sample_weights=[a[2] for a in args], padding_idx=[a[3] for a in args])
    ids, offsets = gc.bad_ids("i64")
    for k, kind in enumerate(kinds):
        mode, weighted, padded = gc.MODES[modes[k]]
        rows, grads, _ = gr.sparse_grad(N, ids, offsets, wide[:, k * dim:(k + 1) * dim], mode, gc.weights() if weighted else None, gc.PAD if padded else None)
        assert np.array_equal(table_bytes(eng, 3 + k), gr.sgd_step(kind, gc.step_table(kind, dim), rows, grads, gc.LR)), kind
    assert ctx.report() == 15


# ---- refusals: the documented code, and the table's bytes unchanged ---------------------------------------------------------------
def test_step_refusals_leave_the_table_alone(eng, ctx, pel):
    UNS, INV = pel.lib.EMB_ERR_UNSUPPORTED, pel.lib.EMB_ERR_INVALID
    idx, off, *_ = batch_on_device("i64", "sum")

    def refused(t, dim, code, text, **kw):
        before = table_bytes(eng, t)
        with pytest.raises(pel.PimembError) as ei:
            ctx.sgd_step([t], [idx], [off], [to_dev(gc.grads(dim))], gc.LR, **kw)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
        assert np.array_equal(table_bytes(eng, t), before)
    load_bytes(eng, 6, "f32", gc.step_table("f32", 16))
    eng.set_hot_rows(6, [1, 2, 3])                                               # a hot set is a copy: no step while one is staged
    refused(6, 16, UNS, "clear the set")
    eng.set_hot_rows(6, [])
    refused(6, 16, UNS, "EMB_POOL_MAX", modes="max")
    for kind, dim in (("e4m3", 16), ("e5m2", 16), ("mxfp4", 32)):
        load_bytes(eng, 7, kind, rc.host_encode(kind, np.random.default_rng(2).standard_normal((N, dim)).astype(np.float32)))
        refused(7, dim, UNS, "fp8 or MXFP4")
    eng.load_table(7, np.ones((N, 8), dtype=np.int32))
    refused(7, 8, UNS, "EMB_FIXED32")
    with eng.grad_context(1024, 512) as small:                                   # the batch holds about 2 000 indices
        before = table_bytes(eng, 6)
        with pytest.raises(pel.PimembError) as ei:
            small.sgd_step([6], [idx], [off], [to_dev(gc.grads(16))], gc.LR)
        assert ei.value.code == INV and "created for 1024" in str(ei.value)
        with pytest.raises(pel.PimembError) as ei:                               # ... and a refused second table keeps the first one unstepped
            ctx.sgd_step([6, 7], [idx, idx], [off, off], [to_dev(gc.grads(16)), to_dev(gc.grads(8))], gc.LR)
        assert ei.value.code == UNS
        assert np.array_equal(table_bytes(eng, 6), before)
    ctx.sgd_step([6], [idx], [off], [to_dev(gc.grads(16))], gc.LR)               # and without the hot set the step runs
    rows, grads, _ = gc.reference("i64", "sum", 16)
    assert np.array_equal(table_bytes(eng, 6), gr.sgd_step("f32", gc.step_table("f32", 16), rows, grads, gc.LR))
    ctx.report()


def test_a_refusal_by_launch_size_leaves_the_earlier_table_alone(eng, pel):
    """Descriptor 1 is more than one launch of the element-wise kernel takes: its dim, 524 289, is odd, and 2^20 indices of it are
    2^20 * 524 289 / 256 = 2 147 487 744 workgroups, above 2^31 - 1.  That is found in the plan of the call, before anything is
    enqueued: descriptor 0's table and state keep every byte, no bad position is counted, and a step issued right afterwards on
    the same context gives the reference's bytes -- nothing of the refused call was left on the stream."""
    wide, big_n, eps = 524289, 1 << 20, np.float32(1e-10)
    assert (big_n * wide + 255) // 256 == 2147487744 > 2 ** 31 - 1
    idx, off, *_ = batch_on_device("u32", "sum")
    G = to_dev(gc.grads(8, overflow=False))
    rows, grads, n_bad = gc.reference("u32", "sum", 8, overflow=False)
    init = gc.step_table("f32", 8)
    s0 = np.abs(np.random.default_rng(3).standard_normal((N, 8))).astype(np.float32)
    eng.alloc_table(9, 1, wide, pel.lib.EMB_F32)
    idx1, off1 = to_dev(np.zeros(big_n, np.uint32)), to_dev(np.zeros(1, np.uint32))      # 2^20 times row 0, in one bag
    G1, st1 = (torch.zeros((1, wide), dtype=torch.float32, device=DEV) for _ in range(2))
    with eng.grad_context(big_n, 512) as big:
        def step(which, tables, idxs, offs, Gs, states):
            if which == "adagrad":
                big.adagrad_step(tables, idxs, offs, Gs, states, gc.LR, eps=eps)
            else:
                big.sgd_step(tables, idxs, offs, Gs, gc.LR, multi=which == "sgd_multi")
        for which in ("sgd", "sgd_multi", "adagrad"):
            load_bytes(eng, 8, "f32", init)
            st0 = to_dev(s0)
            with pytest.raises(pel.PimembError) as ei:
                step(which, [8, 9], [idx, idx1], [off, off1], [G, G1], [st0, st1])
            assert ei.value.code == pel.lib.EMB_ERR_UNSUPPORTED, which
            assert "more elements than one launch of the element-wise kernel takes" in str(ei.value), str(ei.value)
            assert np.array_equal(table_bytes(eng, 8), init), which
            assert np.array_equal(bits(st0.cpu().numpy()), bits(s0)), which
            assert big.report() == 0, which
            step(which, [8], [idx], [off], [G], [st0])
            if which == "adagrad":
                want, want_state = orf.adagrad_step("f32", init, s0, rows, grads, gc.LR, eps, rowwise=False)
            else:
                want, want_state = gr.sgd_step("f32", init, rows, grads, gc.LR), s0
            assert np.array_equal(table_bytes(eng, 8), want), which
            assert np.array_equal(bits(st0.cpu().numpy()), bits(want_state)), which
            assert big.report() == n_bad == 5, which


# ---- the torch surface ----------------------------------------------------------------------------------------------------------
tm = import_module("pim-embedding-lookup_amd.torch_module")
EXACT_MODES = ["sum", "weighted", "mean", "sum+pad", "weighted+pad", "mean+pad"]


def torch_cpu_bag(mode_name):
    mode, weighted, padded = gc.MODES[mode_name]
    ids, offsets, G, w = gc.exact_batch(padded)
    bag = torch.nn.EmbeddingBag(gc.EXACT_ROWS, 8, mode=mode, sparse=True, padding_idx=gc.PAD if padded else None,
                                _weight=torch.from_numpy(gc.exact_table().copy()))
    return bag, torch.from_numpy(ids), torch.from_numpy(offsets), torch.from_numpy(G), torch.from_numpy(w) if weighted else None


def our_bag(eng, mode_name, table_id, dtype=torch.float32):
    mode, _weighted, padded = gc.MODES[mode_name]
    return tm.PoolingEmbeddingBag(gc.EXACT_ROWS, 8, mode=mode, padding_idx=gc.PAD if padded else None, _weight=torch.from_numpy(gc.exact_table().copy()),
                                  engine=eng, table_id=table_id, dtype=dtype)


@pytest.mark.parametrize("mode_name", EXACT_MODES)
def test_module_sparse_grad_equals_torchs_weight_grad(eng, mode_name):
    ref, ids, offsets, G, w = torch_cpu_bag(mode_name)
    (ref(ids, offsets, w) * G).sum().backward()
    sp = ref.weight.grad.coalesce()
    bag = our_bag(eng, mode_name, 10)
    got = bag.sparse_grad(ids, offsets, G, w)
    assert got.is_sparse and got.is_coalesced() and tuple(got.shape) == (gc.EXACT_ROWS, 8) and got.dtype == torch.float32
    g_rows, g_vals = got.indices()[0].cpu().numpy(), got.values().cpu().numpy()
    t_rows, t_vals = sp.indices()[0].numpy(), sp.values().numpy()
    keep = np.isin(t_rows, g_rows) | t_vals.any(axis=1)                          # torch lists padding entries' rows with all-zero gradients
    assert np.array_equal(t_rows[keep], g_rows) and np.array_equal(bits(t_vals[keep]), bits(g_vals))
    assert np.array_equal(bits(bag.weight.cpu().numpy()), bits(gc.exact_table()))      # the weight itself is not touched


@pytest.mark.parametrize("mode_name", EXACT_MODES)
def test_three_backward_rounds_equal_torchs_sgd(eng, mode_name):
    ref, ids, offsets, G, w = torch_cpu_bag(mode_name)
    opt = torch.optim.SGD(ref.parameters(), lr=0.5)
    bag = our_bag(eng, mode_name, 11).enable_fused_sgd(0.5)
    d_ids, d_off, d_G, d_w = ids.to(DEV), offsets.to(DEV), G.to(DEV), None if w is None else w.to(DEV)
    for _ in range(3):
        opt.zero_grad()
        want_out = ref(ids, offsets, w)
        (want_out * G).sum().backward()
        opt.step()
        out = bag(d_ids, d_off, d_w)
        assert out.requires_grad and np.array_equal(bits(out.detach().cpu().numpy()), bits(want_out.detach().numpy()))
        (out * d_G).sum().backward()                                             # updates the served table: nothing else to do
    assert np.array_equal(bits(bag.weight.cpu().numpy()), bits(ref.weight.detach().numpy()))
    assert not np.array_equal(bits(bag.weight.cpu().numpy()), bits(gc.exact_table()))
    assert list(bag.state_dict()) == ["weight"]
    assert eng._module_grad.report() == 0


def test_fused_module_steps_three_tables_from_one_concat_gradient(eng):
    names = ["sum", "mean", "sum+pad"]
    refs = [torch_cpu_bag(m) for m in names]
    fused = tm.FusedPoolingEmbeddingBags([our_bag(eng, m, 12 + k, dtype=torch.float32 if k != 1 else torch.bfloat16) for k, m in enumerate(names)], concat=True)
    lS_i, lS_o = [r[1].to(DEV) for r in refs], [r[2].to(DEV) for r in refs]
    wide = torch.cat([refs[0][3], refs[1][3] * 2, -refs[2][3]], dim=1)            # ONE [B, 3 * dim] gradient
    out = fused(lS_o, lS_i)
    assert not out.requires_grad and tuple(out.shape) == (gc.EXACT_BAGS, 24)
    fused.sgd_step_(lS_o, lS_i, wide.to(DEV), 0.5)
    fused.enable_fused_sgd(0.25)
    out = fused(lS_o, lS_i)
    assert out.requires_grad
    (out * wide.to(DEV)).sum().backward()
    for k, (ref, ids, offsets, _G, _w) in enumerate(refs):
        g = wide[:, 8 * k:8 * k + 8].numpy()
        mode, _weighted, padded = gc.MODES[names[k]]
        rows, grads, _ = gr.sparse_grad(gc.EXACT_ROWS, ids.numpy(), offsets.numpy(), g, mode, None, gc.PAD if padded else None)
        kind = "bf16" if k == 1 else "f32"
        want = gr.encode(kind, gc.exact_table())
        for lr in (0.5, 0.25):
            want = gr.sgd_step(kind, want, rows, grads, np.float32(lr))
        assert np.array_equal(fused.bags[k].weight.cpu().contiguous().view(torch.uint8).numpy().reshape(gc.EXACT_ROWS, -1), want), k


def test_modules_without_fused_sgd_return_plain_tensors(eng):
    _ref, ids, offsets, _G, _w = torch_cpu_bag("mean")
    bag = our_bag(eng, "mean", 15)
    out = bag(ids.to(DEV), offsets.to(DEV))
    assert out.requires_grad is False and out.grad_fn is None
    fused = tm.FusedPoolingEmbeddingBags([bag])
    assert all(o.requires_grad is False for o in fused([offsets.to(DEV)], [ids.to(DEV)]))
    assert bag.enable_fused_sgd(0.1)(ids.to(DEV), offsets.to(DEV)).requires_grad
    assert bag.enable_fused_sgd(None)(ids.to(DEV), offsets.to(DEV)).requires_grad is False


def test_harness_fused_sgd_steps_its_tables(pel):
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    rng = np.random.default_rng(43)
    ln_emb, m, B = [257, 583, N], 16, 64
    weights = [rng.integers(-8, 9, size=(n, m)).astype(np.float32) for n in ln_emb]
    lS_i = [rng.integers(0, n, size=B * 4) for n in ln_emb]
    lS_o = [np.arange(0, B * 4, 4) for _ in ln_emb]
    ebc = h.EmbeddingBagCollection(ln_emb, m, weights=weights).enable_fused_sgd(0.5)
    ly = ebc.apply_emb([torch.from_numpy(o).to(DEV) for o in lS_o], [torch.from_numpy(i).to(DEV) for i in lS_i])
    sum(y.sum() for y in ly).backward()                                          # the dummy loss: every gradient element is 1
    for k, n in enumerate(ln_emb):
        rows, grads, _ = gr.sparse_grad(n, lS_i[k], lS_o[k], np.ones((B, m), np.float32))
        want = gr.sgd_step("f32", weights[k].view(np.uint8).reshape(n, -1), rows, grads, np.float32(0.5))
        assert np.array_equal(table_bytes(ebc.engine, k), want), k
    ebc.engine.close()
