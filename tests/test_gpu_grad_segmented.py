"""GPU: the segmented order of additions of the backward pass (EMB_GRAD_ORDER_SEGMENTED, include/pimemb_grad.h) on contexts of
S = 8, 16 and 64 (GradContext's default) with every case, of S = 1024 (the maximum) and of S = 32, 128, 256 and 512 with a reduced
set of runs, bit for bit against tests/grad_seg_ref.py's loop.  The inputs are that module's: one-index bags whose gradient
columns 0 and 1 overflow as soon as two neighbours inside a segment are added in the wrong order, column 2 the position's number
(exact sums), column 3 the absorb column -- exactly 1.0 in the position order, above it by an amount that depends on S in the
segmented one, and on where the segments are cut -- and NaN wherever a position is not good.  tests/test_grad_segmented_cpu.py
shows that the comparison used here rejects the wrong orders.  n <= 4097 on the contexts of S = 8 and 16, up to 15 374 on the wider
ones (where column 2 is no longer exact in any order: grad_seg_ref.reduced_case); report() is checked in every case."""
import ctypes as C
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_order_cases as oc  # noqa: E402
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
from grad_gpu import DEV, F, check_state, check_table, host, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

LR, EPS = sr.LR, sr.EPS
MAX_N, MAX_DIM = 4097, 320
WIDE_N = 16384                       # the contexts of S >= 32: lengths_case(64) has 5523 positions, reduced_case(1024) 15 374
FULL = sr.SEGMENTS + sr.WIDE_SEGMENTS[:1]      # the segment lengths that run every case
tm = import_module("pim-embedding-lookup_amd.torch_module")


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctxs(eng):
    """{S: a segmented context}, and under "position" a position-order one."""
    c = {S: eng.grad_context(MAX_N, MAX_N, order="segmented", segment=S, max_dim=MAX_DIM) for S in sr.SEGMENTS}
    c.update({S: eng.grad_context(WIDE_N, WIDE_N, order="segmented", segment=S, max_dim=MAX_DIM) for S in sr.WIDE_SEGMENTS + sr.MID_SEGMENTS})
    c["position"] = eng.grad_context(MAX_N, MAX_N)
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(autouse=True)
def fresh_count(ctxs):
    for x in ctxs.values():
        x.report()


_shape_tables = {}


def shape_table(eng, pel, nr_rows, dim):
    """An fp16 table of [nr_rows, dim], allocated once: the sparse gradient depends on the table's shape only."""
    key = (nr_rows, dim)
    if key not in _shape_tables:
        t = 30 + len(_shape_tables)
        eng.alloc_table(t, nr_rows, dim, pel.lib.EMB_F16)
        _shape_tables[key] = t
    return _shape_tables[key]


def device_batch(case, dim, path, width, fixed, narrow=False, misaligned=False):
    """(indices, offsets or None, G, mode, weights or None, fixed_pooling) on the device.  misaligned: G is a view one float into
    a wider buffer -- 4-byte aligned only, an odd row stride: the element-wise kernel."""
    G = to_dev(case.grads(dim, narrow, weighted=path == "weighted"))
    if misaligned:
        wide = torch.full((G.shape[0], dim + 3), float("nan"), dtype=torch.float32, device=DEV)
        wide[:, 1:1 + dim] = G
        G = wide[:, 1:1 + dim]
        assert G.data_ptr() % 16 != 0 and G.stride(0) % 4 != 0
    return (to_dev(case.ids_array(width)), None if fixed else to_dev(case.offsets_array(width)), G, "mean" if path == "mean" else "sum",
            to_dev(case.weights()) if path == "weighted" else None, 1 if fixed else 0)


def sparse(ctx, t, case, dim, path, width, fixed, misaligned=False):
    idx, off, G, mode, w, fp = device_batch(case, dim, path, width, fixed, misaligned=misaligned)
    return ctx.sparse_grad(t, idx, off, G, mode=mode, per_sample_weights=w, padding_idx=case.pad, fixed_pooling=fp)


def check_sparse(ctx, t, case, dim, variants, misaligned=False):
    want = case.seg_reference(ctx.segment, dim)
    for path, width, fixed in variants:
        rows, grads = sparse(ctx, t, case, dim, path, width, fixed, misaligned)
        oc.check_sparse(host(rows), host(grads), want, (case.name, ctx.segment, dim, path, width, fixed))
        assert ctx.report() == case.n_bad, (case.name, path, width, fixed)


def sgd(ctx, t, batch, pad=None, multi=False):
    idx, off, G, mode, w, fp = batch
    ctx.sgd_step([t], [idx], None if off is None else [off], [G], LR, modes=mode, per_sample_weights=w, padding_idx=pad, fixed_pooling=fp, multi=multi)


def adagrad(ctx, t, batch, d_state, rowwise, pad=None):
    idx, off, G, mode, w, fp = batch
    ctx.adagrad_step([t], [idx], None if off is None else [off], [G], [d_state], LR, eps=EPS, rowwise=rowwise, modes=mode, per_sample_weights=w,
                     padding_idx=pad, fixed_pooling=fp)


def sgd_case(eng, ctx, case, kind, dim, path, width, fixed, t=2, misaligned=False):
    """One fused SGD step in the segmented order; the WHOLE table is compared."""
    init = oc.step_table(kind, case.nr_rows, dim)
    want = sr.sgd_table(kind, init, case.seg_reference(ctx.segment, dim))
    assert (want != init).any()
    load_bytes(eng, t, kind, init)
    sgd(ctx, t, device_batch(case, dim, path, width, fixed, misaligned=misaligned), case.pad)
    check_table(table_bytes(eng, t), want, (case.name, ctx.segment, kind, dim, path, width, fixed))
    assert ctx.report() == case.n_bad


def step_case(eng, ctx, case, kind, dim, rowwise, path, width, fixed, t=2, misaligned=False):
    """One Adagrad / row-wise Adagrad step on the NARROW columns (the absorb column stays); the WHOLE table and state are compared."""
    ref = case.seg_reference(ctx.segment, dim, narrow=True)
    assert not np.array_equal(oc.bits(ref[1]), oc.bits(case.fold(dim, "sum", narrow=True)[1]))      # (the order shows on the narrow columns too)
    init, s0 = oc.step_table(kind, case.nr_rows, dim), oc.init_state(case.nr_rows, dim, rowwise)
    want_table, want_state = sr.adagrad_tables(kind, init, s0, ref, rowwise)
    assert np.isfinite(want_state).all() and (oc.bits(want_state) != oc.bits(s0)).any()
    load_bytes(eng, t, kind, init)
    d_state = to_dev(s0)
    adagrad(ctx, t, device_batch(case, dim, path, width, fixed, narrow=True, misaligned=misaligned), d_state, rowwise, case.pad)
    what = (case.name, ctx.segment, kind, dim, "row-wise" if rowwise else "adagrad", path, width, fixed)
    check_table(table_bytes(eng, t), want_table, what)
    check_state(d_state, want_state, what)
    assert ctx.report() == case.n_bad


# ---- emb_grad_sparse: run lengths, dims, paths ---------------------------------------------------------------------------------------
ALL = [(p, w, f) for p in oc.PATHS for w in ("u32", "i64") for f in (False, True)]
# dim -> the variants it runs: every one at dim 4 (one lane); a rotating choice elsewhere
SPARSE_DIMS = {4: ALL, 16: ALL[1::4], 48: ALL[2::4], 128: ALL[3::4], 320: ALL[0::5], 6: ALL[::3]}


@pytest.mark.parametrize("dim", list(SPARSE_DIMS))
@pytest.mark.parametrize("S", FULL)
def test_run_lengths_on_both_sides_of_the_segment_boundaries(eng, ctxs, pel, S, dim):
    """In one batch: runs of S-1, S, S+1, S+2, 2S-1, 2S, 2S+1, 3S+5, 8S+3 (nine partials) and 65S+1 (66: several rounds of partial
    loads); three bad ids and a padding id in between, whose NaN rows must never show.  dim 4: one lane; 16; 48: idle lanes in the
    group; 128; 320: two pieces per lane; 6: the element-wise kernel."""
    case = sr.lengths_case(S, True)
    assert ctxs[S].order == "segmented" and ctxs[S].segment == S and ctxs[S].max_dim == MAX_DIM
    check_sparse(ctxs[S], shape_table(eng, pel, case.nr_rows, dim), case, dim, SPARSE_DIMS[dim])


@pytest.mark.parametrize("S", FULL)
def test_a_misaligned_gradient_runs_the_element_wise_kernel_in_the_same_order(eng, ctxs, pel, S):
    case = sr.lengths_case(S, True)
    check_sparse(ctxs[S], shape_table(eng, pel, case.nr_rows, 8), case, 8, ALL[::5], misaligned=True)
    check_sparse(ctxs[S], shape_table(eng, pel, case.nr_rows, 8), case, 8, ALL[1:2])      # ... and the lane-group kernel gives the same rows


# ---- run placement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 16, 5])
@pytest.mark.parametrize("tail", ["bad", "end"])
@pytest.mark.parametrize("S", FULL)
def test_long_runs_at_the_end_next_to_each_other_and_around_a_short_one(eng, ctxs, pel, S, tail, dim):
    """A long run that ends the good positions with the keys of the positions that are not good directly behind it ("bad"), or ends
    the array ("end"); a run of 2S + 3 directly followed by a run of 2S, so that two segment starts share one S-aligned block of
    sorted places; a short run between two long ones."""
    case = sr.placement_case(S, tail)
    check_sparse(ctxs[S], shape_table(eng, pel, case.nr_rows, dim), case, dim, ALL[(dim + S) % 4::4])


@pytest.mark.parametrize("S", FULL)
def test_one_row_holds_every_position(eng, ctxs, pel, S):
    case = sr.one_row_case(S)
    assert len(case.seg_reference(S, 8)[0]) == 1
    check_sparse(ctxs[S], shape_table(eng, pel, case.nr_rows, 8), case, 8, [("sum", "i64", False), ("weighted", "u32", True)])
    sgd_case(eng, ctxs[S], case, "f32", 8, "mean", "i64", False)
    step_case(eng, ctxs[S], case, "f32", 8, True, "sum", "u32", True)


# ---- the steps -------------------------------------------------------------------------------------------------------------------------
SGD_SHAPES = [("f32", 128, "sum", "i64", False), ("f16", 48, "weighted", "u32", True), ("bf16", 4, "mean", "i64", True), ("bf16", 320, "sum", "u32", False),
              ("f32", 6, "weighted", "i64", False)]


@pytest.mark.parametrize("kind,dim,path,width,fixed", SGD_SHAPES, ids=["-".join(map(str, s[:3])) for s in SGD_SHAPES])
@pytest.mark.parametrize("S", FULL)
def test_sgd_step_in_the_segmented_order(eng, ctxs, S, kind, dim, path, width, fixed):
    sgd_case(eng, ctxs[S], sr.lengths_case(S, True), kind, dim, path, width, fixed)


STEP_SHAPES = [("f16", 16, False, "sum", "u32", False), ("f32", 6, False, "mean", "i64", True), ("f32", 128, False, "weighted", "i64", False),
               ("f32", 48, True, "weighted", "i64", False), ("bf16", 320, True, "sum", "u32", True), ("f32", 4, True, "mean", "u32", False)]


@pytest.mark.parametrize("kind,dim,rowwise,path,width,fixed", STEP_SHAPES, ids=["-".join(map(str, s[:3])) for s in STEP_SHAPES])
@pytest.mark.parametrize("S", FULL)
def test_adagrad_steps_in_the_segmented_order(eng, ctxs, S, kind, dim, rowwise, path, width, fixed):
    """Narrow gradients (the squares of +-FLT_MAX would overflow the state): the order rests on the absorb column and the randoms.
    Adagrad on the lane-group kernel and on the element-wise one (dim 6); row-wise Adagrad with idle lanes (dim 48), with two walks
    per lane (dim 320) and with sixteen lane groups in a wavefront (dim 4)."""
    step_case(eng, ctxs[S], sr.lengths_case(S, True), kind, dim, rowwise, path, width, fixed)


@pytest.mark.parametrize("S", FULL)
def test_steps_on_the_placement_cases(eng, ctxs, S):
    sgd_case(eng, ctxs[S], sr.placement_case(S, "bad"), "f32", 16, "sum", "u32", False)
    step_case(eng, ctxs[S], sr.placement_case(S, "end"), "bf16", 16, True, "mean", "i64", True)
    step_case(eng, ctxs[S], sr.placement_case(S, "bad"), "f32", 5, False, "sum", "i64", False)


# ---- the wider segment lengths on the reduced runs ---------------------------------------------------------------------------------------
WIDE_DIMS = {4: ALL[0::4], 8: ALL[2::4], 5: ALL[1::4]}


@pytest.mark.parametrize("dim", list(WIDE_DIMS))
def test_segments_of_1024_on_both_sides_of_their_boundaries(eng, ctxs, pel, dim):
    """The longest segment: 128 rounds of eight loads per segment, a look-ahead of up to 7168 sorted places, 15 374 positions (a
    binary search over sixteen sort tiles).  Runs of S-1, S, S+1, S+2, 2S+1 and 9S+3 (ten partials: one full round and one more);
    dims 4 and 8 on the lane-group kernel, 5 on the element-wise one."""
    S = sr.WIDE_SEGMENTS[-1]
    case = sr.reduced_case(S)
    assert ctxs[S].segment == S == 1024 and case.n <= WIDE_N
    check_sparse(ctxs[S], shape_table(eng, pel, case.nr_rows, dim), case, dim, WIDE_DIMS[dim])


def test_steps_in_segments_of_1024(eng, ctxs):
    S = sr.WIDE_SEGMENTS[-1]
    case = sr.reduced_case(S)
    sgd_case(eng, ctxs[S], case, "bf16", 8, "weighted", "u32", False)
    sgd_case(eng, ctxs[S], case, "f32", 5, "sum", "i64", True)
    step_case(eng, ctxs[S], case, "f32", 4, True, "mean", "i64", True)


@pytest.mark.parametrize("S", sr.MID_SEGMENTS)
def test_the_segment_lengths_in_between_on_the_reduced_runs(eng, ctxs, pel, S):
    case = sr.reduced_case(S)
    assert ctxs[S].segment == S
    check_sparse(ctxs[S], shape_table(eng, pel, case.nr_rows, 4), case, 4, ALL[S.bit_length() % 4::4])


# ---- the multi-table steps -----------------------------------------------------------------------------------------------------------------
MULTI_DIM = 16


def multi_batches(cases, paths, narrow):
    batches = [device_batch(c, MULTI_DIM, p, "i64", False, narrow=narrow) for c, p in zip(cases, paths)]
    return ([b[0] for b in batches], [b[1] for b in batches], [b[2] for b in batches]), dict(modes=[b[3] for b in batches], per_sample_weights=[b[4] for b in batches])


@pytest.mark.parametrize("S", FULL)
def test_multi_table_steps_equal_the_per_table_calls_and_the_reference(eng, ctxs, S):
    """Three tables of one dim in one group; the last row of table k and row 0 of table k + 1 both carry long runs: adjacent
    composite keys, which must not merge.  SGD, Adagrad and row-wise Adagrad; the grouping is what it was."""
    ctx, cases, paths = ctxs[S], sr.multi_cases(S), ("sum", "weighted", "mean")
    ids, twins = [10, 11, 12], [13, 14, 15]
    kinds = ("f32", "bf16", "f16")
    n, b = [c.n for c in cases], [c.B for c in cases]
    for t, c, k in zip(ids + twins, cases + cases, kinds + kinds):
        load_bytes(eng, t, k, oc.step_table(k, c.nr_rows, MULTI_DIM))
    assert ctx.multi_groups(ids, n, b) == ctxs["position"].multi_groups(ids, n, b) == [0, 0, 0]
    inits = [oc.step_table(k, c.nr_rows, MULTI_DIM) for c, k in zip(cases, kinds)]
    # SGD
    args, kw = multi_batches(cases, paths, narrow=False)
    ctx.sgd_step(ids, *args, LR, multi=True, **kw)
    assert ctx.report() == sum(c.n_bad for c in cases) == 3
    ctx.sgd_step(twins, *args, LR, multi=False, **kw)
    ctx.report()
    for t, tw, c, k, init in zip(ids, twins, cases, kinds, inits):
        got = table_bytes(eng, t)
        check_table(got, sr.sgd_table(k, init, c.seg_reference(S, MULTI_DIM)), (c.name, "multi sgd against the reference"))
        check_table(got, table_bytes(eng, tw), (c.name, "multi sgd against the per-table call"))
    # Adagrad and row-wise Adagrad, narrow gradients
    args, kw = multi_batches(cases, paths, narrow=True)
    for rowwise in (False, True):
        for t, k, init in zip(ids + twins, kinds + kinds, inits + inits):
            load_bytes(eng, t, k, init)
        s0 = [oc.init_state(c.nr_rows, MULTI_DIM, rowwise) for c in cases]
        st, st_twin = [to_dev(s) for s in s0], [to_dev(s) for s in s0]
        ctx.adagrad_step(ids, *args, st, LR, eps=EPS, rowwise=rowwise, multi=True, **kw)
        ctx.adagrad_step(twins, *args, st_twin, LR, eps=EPS, rowwise=rowwise, multi=False, **kw)
        assert ctx.report() == 6
        for j, (t, tw, c, k, init) in enumerate(zip(ids, twins, cases, kinds, inits)):
            want_table, want_state = sr.adagrad_tables(k, init, s0[j], c.seg_reference(S, MULTI_DIM, narrow=True), rowwise)
            got = table_bytes(eng, t)
            check_table(got, want_table, (c.name, rowwise, "multi against the reference"))
            check_table(got, table_bytes(eng, tw), (c.name, rowwise, "multi against the per-table call"))
            check_state(st[j], want_state, (c.name, rowwise))
            check_state(st_twin[j], want_state, (c.name, rowwise, "twin"))


# ---- compatibility with the position order ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", FULL)
def test_runs_of_at_most_S_plus_1_give_the_position_orders_bytes(eng, ctxs, pel, S):
    case = sr.short_case(S)
    for dim, path, width in ((8, "sum", "i64"), (5, "weighted", "u32")):
        t = shape_table(eng, pel, case.nr_rows, dim)
        rows_p, grads_p = sparse(ctxs["position"], t, case, dim, path, width, False)
        rows_s, grads_s = sparse(ctxs[S], t, case, dim, path, width, False)
        oc.check_sparse(host(rows_s), host(grads_s), (host(rows_p), host(grads_p)), (case.name, dim))
        oc.check_sparse(host(rows_s), host(grads_s), case.fold(dim, "sum"), (case.name, dim, "Case.fold"))
        assert ctxs["position"].report() == ctxs[S].report() == case.n_bad
    init = oc.step_table("bf16", case.nr_rows, 8)
    tables = []
    for ctx in (ctxs["position"], ctxs[S]):
        load_bytes(eng, 2, "bf16", init)
        sgd(ctx, 2, device_batch(case, 8, "mean", "i64", True))
        tables.append(table_bytes(eng, 2))
    check_table(tables[1], tables[0], "sgd on the short runs")
    assert (tables[0] != init).any()


def test_a_position_order_context_made_through_create_ex_is_emb_grad_creates(eng, ctxs, pel):
    """On a long-run case: a context of emb_grad_create, one of emb_grad_create_ex with EMB_GRAD_ORDER_POSITION -- the same bytes,
    the position order's reference, the same scratch size, and not the segmented order's bits."""
    case, dim = sr.lengths_case(16, True), 8
    t = shape_table(eng, pel, case.nr_rows, dim)
    G_lib = pel.lib.load_grad()
    old = eng.grad_context(MAX_N, MAX_N)                 # (a wrapper whose handle is replaced by one of the old entry point)
    h = C.c_void_p()
    assert G_lib.emb_grad_create(eng._h, MAX_N, MAX_N, C.byref(h)) == pel.lib.EMB_OK
    G_lib.emb_grad_destroy(old._h)
    old._h = h.value
    cfg = pel.lib.EmbGradConfig()
    assert G_lib.emb_grad_config_of(old._h, C.byref(cfg)) == 0 and (cfg.order, cfg.segment, cfg.max_dim, cfg.reserved) == (0, 0, 0, 0)
    new = ctxs["position"]
    assert new.order == "position" and new.segment is None and new.max_dim is None
    want = case.fold(dim, "sum")
    got = []
    for ctx in (old, new):
        rows, grads = sparse(ctx, t, case, dim, "sum", "i64", False)
        oc.check_sparse(host(rows), host(grads), want, "the position order")
        assert ctx.report() == case.n_bad
        got.append(host(grads))
    assert np.array_equal(oc.bits(got[0]), oc.bits(got[1]))
    assert not np.array_equal(oc.bits(got[0]), oc.bits(case.seg_reference(16, dim)[1]))
    old.close()


# ---- determinism -----------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_and_two_runs_give_the_same_bits_and_S_8_differs_from_S_16(eng, ctxs, pel):
    case, dim = sr.lengths_case(16, True), 16            # (built for S = 16; finite for S = 8 too: test_grad_segmented_cpu)
    t = shape_table(eng, pel, case.nr_rows, dim)
    got = {}
    with eng.grad_context(MAX_N, MAX_N, order="segmented", segment=16, max_dim=dim) as other:
        assert other.max_dim == dim
        for name, ctx, S in (("a", ctxs[16], 16), ("b", ctxs[16], 16), ("other", other, 16), ("eight", ctxs[8], 8)):
            rows, grads = sparse(ctx, t, case, dim, "sum", "i64", False)
            oc.check_sparse(host(rows), host(grads), sr.fold(case, S, dim, "sum"), (name, S))
            assert ctx.report() == case.n_bad
            got[name] = host(grads)
    assert np.array_equal(oc.bits(got["a"]), oc.bits(got["b"])) and np.array_equal(oc.bits(got["a"]), oc.bits(got["other"]))
    assert (got["eight"][:, sr.ABSORB] != got["a"][:, sr.ABSORB]).any()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_a_table_wider_than_max_dim_is_refused_and_nothing_changes(eng, pel):
    case, dim = sr.lengths_case(8, True), 16
    init, s0 = oc.step_table("f32", case.nr_rows, dim), oc.init_state(case.nr_rows, dim, False)
    load_bytes(eng, 2, "f32", init)
    batch = device_batch(case, dim, "sum", "i64", False, narrow=True)
    d_state = to_dev(s0)
    with eng.grad_context(MAX_N, MAX_N, order="segmented", segment=8, max_dim=8) as narrow:
        for call in (lambda: sgd(narrow, 2, batch), lambda: sgd(narrow, 2, batch, multi=True), lambda: adagrad(narrow, 2, batch, d_state, False),
                     lambda: narrow.sparse_grad(2, batch[0], batch[1], batch[2])):
            with pytest.raises(pel.PimembError) as ei:
                call()
            assert ei.value.code == pel.lib.EMB_ERR_INVALID and "max_dim of 8" in str(ei.value), str(ei.value)
        assert narrow.report() == 0                      # refused in the plan: nothing was enqueued, nothing counted
        check_table(table_bytes(eng, 2), init, "the refused steps")
        check_state(d_state, s0, "the refused steps")
    with pytest.raises(pel.PimembError):
        eng.grad_context(16, 16, order="segmented", segment=12)
    with pytest.raises(ValueError):
        eng.grad_context(16, 16, order="position", segment=16)


# ---- the modules --------------------------------------------------------------------------------------------------------------------------------
def test_module_backward_in_the_segmented_order_equals_the_explicit_step(eng, pel):
    """enable_fused_sgd(lr, order="segmented") through loss.backward() equals sgd_step_(..., order="segmented") on a twin and the
    reference at the modules' default segment length; the position order gives other bytes on this batch."""
    S = pel.GradContext.DEFAULT_SEGMENT
    nr, dim = 50, 8
    ids = np.concatenate([np.full(3 * S + 7, 4), np.full(S + 1, 9), np.full(2 * S + 2, nr - 1), np.arange(20)])
    ids = ids[np.random.default_rng(5).permutation(len(ids))]
    case = sr.SegCase(f"seg-module-S{S}", nr, ids, S)
    weight = gr.decode("f32", oc.step_table("f32", nr, dim))
    G = case.grads(dim, narrow=True)
    bags = [tm.PoolingEmbeddingBag(nr, dim, mode="sum", _weight=torch.from_numpy(weight.copy()), engine=eng, table_id=20 + k) for k in range(3)]
    d_ids, d_off, d_G = to_dev(case.ids), to_dev(case.offsets), to_dev(G)
    out = bags[0].enable_fused_sgd(float(LR), order="segmented")(d_ids, d_off)
    assert out.requires_grad
    (out * d_G).sum().backward()
    bags[1].sgd_step_(d_ids, d_off, d_G, float(LR), order="segmented")
    bags[2].sgd_step_(d_ids, d_off, d_G, float(LR))
    assert eng._module_grad_segmented.order == "segmented" and eng._module_grad_segmented.segment == S and eng._module_grad.order == "position"
    want = sr.sgd_table("f32", oc.step_table("f32", nr, dim), sr.fold(case, S, dim, "sum", narrow=True))
    check_table(table_bytes(eng, 20), want, "loss.backward()")
    check_table(table_bytes(eng, 21), want, "sgd_step_")
    check_table(table_bytes(eng, 22), gr.sgd_step("f32", oc.step_table("f32", nr, dim), *case.fold(dim, "sum", narrow=True)[:2], LR), "the position order")
    assert (table_bytes(eng, 22) != table_bytes(eng, 20)).any()
    sp = bags[2].sparse_grad(d_ids, d_off, d_G, order="segmented")
    oc.check_sparse(sp.indices()[0].cpu().numpy(), sp.values().cpu().numpy(), sr.fold(case, S, dim, "sum", narrow=True), "module sparse_grad")
    fused = tm.FusedPoolingEmbeddingBags([bags[1]]).enable_fused_sgd(float(LR), order="segmented")
    (fused([d_off], [d_ids])[0] * d_G).sum().backward()
    bags[0].sgd_step_(d_ids, d_off, d_G, float(LR), order="segmented")
    check_table(table_bytes(eng, 21), table_bytes(eng, 20), "the fused module's second step")
    assert eng._module_grad_segmented.report() == 0
