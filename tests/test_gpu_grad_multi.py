"""GPU: the multi-table steps (emb_grad_sgd_multi / emb_grad_step_multi, include/pimemb_grad.h), bit for bit.  One multi call steps
tables A; the existing single call steps twin tables B loaded with the same bytes; whole tables and whole states are compared byte
for byte, with each other and with the loop references (tests/grad_ref.py, tests/optim_ref.py).  The shapes are the smallest at
which a composite sort key can go wrong: key bases that are no multiple of 256, table boundaries inside a sort tile and inside a
64-position slice, bad ids that are the NEXT table's rows in key space, three passes of the sort.  No tolerance anywhere."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as gc  # noqa: E402
import grad_order_cases as goc  # noqa: E402
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402
import pool_ref  # noqa: E402
import rows_cases as rc  # noqa: E402
from grad_gpu import DEV, F, bits, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

LR, EPS = gc.LR, F(1e-10)
ROWS3 = (3001, 257, 70000)       # key bases 3001 and 3258; 73258 keys: 17 bits, three passes
ROWS_SMALL = (3001, 257, 4099)   # the Adagrad cases: the states are compared whole
A0, B0 = 0, 20                   # table numbers of the stepped tables and of their twins


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.grad_context(8192, 1024)
    yield c
    c.close()


_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def init_table(kind, nr, dim):
    """uint8 [nr, stride]: grad_cases' table (with its crafted rows) at 3001 rows, the host encoding of seeded randoms otherwise."""
    if nr == gc.NR_ROWS:
        return gc.step_table(kind, dim)
    return once(("table", kind, nr, dim), lambda: gr.encode(kind, (np.random.default_rng(nr + dim).standard_normal((nr, dim)) * 3).astype(F)))


def init_state(nr, dim, rowwise):
    def make():
        rng = np.random.default_rng(900 + nr + dim + rowwise)
        shape = (nr,) if rowwise else (nr, dim)
        s = (np.abs(rng.standard_normal(shape)) * np.exp2(rng.integers(-12, 12, size=(nr,) + (1,) * (len(shape) - 1)))).astype(F)
        s[::5] = 0
        return s
    return once(("state", nr, dim, rowwise), make)


class Desc:
    """One table's share of a call, on the host: grad_cases' batch (its ids are made for 3001 rows: in a table of 257 rows most
    of them are bad, in one of 70 000 rows its `bad` ids 3001 and 3008 are good) over a table of nr rows."""

    def __init__(self, nr, mode_name, width, dim, lead=False, fixed=0, G=None, overflow=True, ids=None, offsets=None):
        self.nr, self.mode_name, self.width, self.dim, self.fixed = nr, mode_name, width, dim, fixed
        self.mode, self.weighted, self.padded = gc.MODES[mode_name]
        b_ids, b_off = gc.bad_ids(width)
        self.ids = list(b_ids) if ids is None else list(ids)
        self.offsets = (gc.offsets_lead() if lead else b_off) if offsets is None else offsets
        self.n_bags = len(self.offsets) if not fixed else gc.N_BAGS
        if fixed:
            self.ids, self.offsets = self.ids[:gc.N_BAGS * fixed], None
        self.G = gc.grads(dim, overflow) if G is None else G
        self.w = gc.weights()[:len(self.ids)] if self.weighted else None
        self.pad = gc.PAD if self.padded else None
        self.key = (nr, mode_name, width, dim, lead, fixed, overflow, None if G is None else G.tobytes()[:64], ids is None, offsets is None)

    def sparse(self):
        """(rows, grads, n_bad) by grad_ref, once per case."""
        return once(("sparse",) + self.key, lambda: gr.sparse_grad(self.nr, self.ids, self.offsets, self.G, self.mode, self.w, self.pad,
                                                                   n_bags=self.n_bags, fixed_pooling=self.fixed))

    def on_device(self):
        arr = gc.ids_array(self.ids, self.width) if self.width in ("u32", "i64") else None
        return (to_dev(arr), None if self.offsets is None else to_dev(self.offsets.astype(arr.dtype)), to_dev(self.G),
                None if self.w is None else to_dev(self.w))


def step_ref(opt, kind, init, state, d):
    """(table bytes, state or None) after one step of `opt` over descriptor d, by the loop references."""
    rows, grads, _ = d.sparse()
    if opt == "sgd":
        return gr.sgd_step(kind, init, rows, grads, LR), None
    return orf.adagrad_step(kind, init, state, rows, grads, LR, EPS, rowwise=opt == "rowwise")


def call(ctx, opt, tables, dev, descs, states, multi, cols=None):
    idx, off, G, w = ([x[j] for x in dev] for j in range(4))
    fixed = max(d.fixed for d in descs)
    kw = dict(modes=[d.mode for d in descs], per_sample_weights=w, padding_idx=[d.pad for d in descs], fixed_pooling=fixed, multi=multi)
    if opt == "sgd":
        ctx.sgd_step(tables, idx, off, G if cols is None else cols, LR, **kw)
    else:
        ctx.adagrad_step(tables, idx, off, G if cols is None else cols, states, LR, eps=EPS, rowwise=opt == "rowwise", **kw)


def run_both(eng, ctx, kinds, descs, opt="sgd", tables=None, want=True, cols=None):
    """The multi call on tables A, the single call on their twins B, and the references.  `tables`: the position of every
    descriptor's table among the loaded ones (default: one table each); a table named twice is stepped twice."""
    tables = list(range(len(descs))) if tables is None else tables
    n_tab = max(tables) + 1
    first = [tables.index(t) for t in range(n_tab)]
    dims = [descs[j].dim for j in first]
    inits = [init_table(kinds[t], descs[first[t]].nr, dims[t]) for t in range(n_tab)]
    s0 = [None if opt == "sgd" else init_state(descs[first[t]].nr, dims[t], opt == "rowwise") for t in range(n_tab)]
    for t in range(n_tab):
        load_bytes(eng, A0 + t, kinds[t], inits[t])
        load_bytes(eng, B0 + t, kinds[t], inits[t])
    sA, sB = ([None if s is None else to_dev(s) for s in s0] for _ in range(2))
    dev = [d.on_device() for d in descs]
    ctx.report()
    call(ctx, opt, [A0 + t for t in tables], dev, descs, [sA[t] for t in tables], True, cols)
    bad_multi = ctx.report()
    call(ctx, opt, [B0 + t for t in tables], dev, descs, [sB[t] for t in tables], False, cols)
    bad_single = ctx.report()
    assert bad_multi == bad_single == sum(d.sparse()[2] for d in descs), (bad_multi, bad_single)
    w_tab, w_st = list(inits), list(s0)
    for j, t in enumerate(tables):
        if want:
            w_tab[t], w_st[t] = step_ref(opt, kinds[t], w_tab[t], w_st[t], descs[j])
    for t in range(n_tab):
        a, b = table_bytes(eng, A0 + t), table_bytes(eng, B0 + t)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, ("multi against single", t, bad[:8], a[bad[0]][:16], b[bad[0]][:16], inits[t][bad[0]][:16])
        assert (a != inits[t]).any(), t
        if want:
            bad = np.flatnonzero((a != w_tab[t]).any(axis=1))
            assert bad.size == 0, ("multi against the definition", t, bad[:8], a[bad[0]][:16], w_tab[t][bad[0]][:16])
        if opt != "sgd":
            ga, gb = sA[t].cpu().numpy(), sB[t].cpu().numpy()
            assert np.array_equal(bits(ga), bits(gb)), ("state: multi against single", t)
            assert not np.array_equal(bits(ga), bits(s0[t])), t
            if want:
                bad = np.flatnonzero((bits(ga) != bits(w_st[t])).reshape(len(ga), -1).any(axis=1))
                assert bad.size == 0, ("state against the definition", t, bad[:8])
    return w_tab


# ---- the main case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["u32", "i64"])
@pytest.mark.parametrize("mode_name", ["sum", "weighted", "mean+pad"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_three_tables_in_one_group_equal_the_single_calls_and_the_definition(eng, ctx, kind, mode_name, width):
    """3001, 257 and 70 000 rows: the batch's bad ids 3001 and 3008 (u32) are rows 0 and 7 of the NEXT table in key space, most ids
    of the batch lie beyond the second table's 257 rows -- in the third table's keys -- and the int64 ids 2^32 + 5 and the negative
    ones must not be truncated into any table.  About 6 000 positions: six sort tiles, the table boundaries inside tiles."""
    descs = [Desc(nr, mode_name, width, 16) for nr in ROWS3]
    assert sum(len(d.ids) for d in descs) > 5 * 1024 and goc.passes_of(sum(ROWS3)) == 3
    assert descs[1].sparse()[2] > 1000 and 3001 in descs[2].sparse()[0]
    run_both(eng, ctx, [kind] * 3, descs)
    assert ctx.multi_groups([A0, A0 + 1, A0 + 2], [len(d.ids) for d in descs], [d.n_bags for d in descs]) == [0, 0, 0]


def test_the_same_row_in_three_tables_gives_three_runs(eng, ctx):
    """Row 1234 occurs 140 times in each of three tables of 3001 rows (key bases 3001 and 6002), with three different gradients and
    coefficient paths: runs that merged, or a run walked with a neighbour's pointers, would show."""
    G = gc.grads(16)
    descs = [Desc(3001, "weighted", "i64", 16), Desc(3001, "mean", "i64", 16, G=np.ascontiguousarray(G[::-1])), Desc(3001, "sum+pad", "i64", 16, G=G * F(0.5))]
    assert all(gc.HOT in d.sparse()[0] for d in descs)
    want = run_both(eng, ctx, ["f32", "bf16", "f16"], descs)
    assert not np.array_equal(want[0][gc.HOT], gc.step_table("f32", 16)[gc.HOT])


@pytest.mark.parametrize("width", ["u32", "i64"])
def test_bags_are_searched_in_each_descriptors_own_offsets(eng, ctx, width):
    """Mean mode throughout, so cnt is kept apart too: the first descriptor ends in an empty bag; the second has offsets[0] = 3 --
    its first three positions have no bag (they are not the first descriptor's last bag's); the third has no offsets at all
    (fixed_pooling 6), so its bags hold other counts than the same bag numbers of the first two."""
    descs = [Desc(3001, "mean", width, 16), Desc(257, "mean+pad", width, 16, lead=True), Desc(70000, "mean", width, 16, fixed=6)]
    assert descs[0].offsets[-1] == len(descs[0].ids) and descs[1].offsets[0] == 3
    run_both(eng, ctx, ["f32", "f32", "bf16"], descs)


def test_the_order_witness_over_two_descriptors(eng):
    """grad_order_cases' witness (columns of +-FLT_MAX: two neighbouring occurrences of a run exchanged give inf) laid over two
    descriptors of 70 001 rows each at once: 18 key bits, three passes, 3 074 positions, five long runs per table."""
    cases = [goc.edge_case(2049), goc.edge_case(1025)]
    dim = 8
    assert goc.passes_of(2 * goc.EDGE_ROWS) == 3
    for path in goc.PATHS:
        descs = []
        for c in cases:
            d = Desc(c.nr_rows, {"sum": "sum", "weighted": "weighted", "mean": "mean"}[path], "i64", dim, fixed=0, G=c.grads(dim, weighted=path == "weighted"),
                     ids=c.ids.tolist(), offsets=c.offsets)
            d.w = c.weights() if path == "weighted" else None
            d.key = ("order", c.name, path)
            _cache[("sparse",) + d.key] = c.reference(dim)
            descs.append(d)
        with eng.grad_context(sum(c.n for c in cases), sum(c.B for c in cases)) as small:
            want = run_both(eng, small, ["f32", "f32"], descs)
        for t, c in enumerate(cases):
            assert np.isfinite(gr.decode("f32", want[t])).all(), (path, t)      # in the right order no sum overflows


# ---- the optimizers with a state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,dim,mode_name,width", [("adagrad", 16, "weighted+pad", "u32"), ("adagrad", 8, "mean", "i64"), ("rowwise", 48, "sum", "i64"),
                                                     ("rowwise", 48, "mean+pad", "u32"), ("rowwise", 320, "weighted", "i64")])
def test_adagrad_steps_of_three_tables_with_their_states(eng, ctx, opt, dim, mode_name, width):
    """dim 48: 12 pieces in 16 lanes, idle lanes in the butterfly; dim 320: two accumulators per lane."""
    descs = [Desc(nr, mode_name, width, dim, overflow=False) for nr in ROWS_SMALL]
    run_both(eng, ctx, ["f32", "bf16", "f16"], descs, opt=opt)


# ---- splits -------------------------------------------------------------------------------------------------------------------------
def test_seventeen_tables_split_into_sixteen_and_one(eng, ctx):
    rng = np.random.default_rng(17)
    descs = []
    for t in range(17):
        ids = rng.integers(0, 64, size=50).tolist()
        ids[3] = 64 + t                                                          # one bad id each: the next table's row t
        off = np.sort(rng.integers(0, 50, size=10)).astype(np.int64)
        off[0] = 0
        G = rng.standard_normal((10, 16)).astype(F)
        d = Desc(64, "sum", "i64", 16, G=G, ids=ids, offsets=off)
        d.key = ("tiny", t)
        descs.append(d)
    run_both(eng, ctx, ["f32"] * 17, descs)
    assert ctx.multi_groups([A0 + t for t in range(17)], [50] * 17, [10] * 17) == [0] * 16 + [1]


def test_a_table_named_twice_is_stepped_twice_in_order(eng, ctx):
    descs = [Desc(3001, "sum", "i64", 16, overflow=False), Desc(257, "sum", "i64", 16, overflow=False), Desc(3001, "mean+pad", "i64", 16, overflow=False)]
    run_both(eng, ctx, ["bf16", "f32"], descs, tables=[0, 1, 0])
    assert ctx.multi_groups([A0, A0 + 1, A0], [len(d.ids) for d in descs], [d.n_bags for d in descs]) == [0, 0, 1]


def test_an_element_wise_descriptor_in_the_middle_of_a_call(eng, ctx):
    """dims 16, 16, 12, 16: the table of dim 12 reads its gradient from column 3 of a [B, 27] buffer -- no 16-byte multiple, the
    element-wise kernel -- and runs alone between a group of two and a group of one."""
    buf = np.full((gc.N_BAGS, 27), np.nan, dtype=F)
    buf[:, 3:15] = gc.grads(12)
    d_buf = to_dev(buf)
    descs = [Desc(3001, "sum", "u32", 16), Desc(257, "weighted", "u32", 16), Desc(3001, "mean+pad", "u32", 12), Desc(70000, "sum", "u32", 16)]
    dev = [d.on_device() for d in descs]
    cols = [x[2] for x in dev]
    cols[2] = d_buf[:, 3:15]
    run_both(eng, ctx, ["f32", "f16", "bf16", "f32"], descs, cols=cols)
    assert ctx.multi_groups([A0 + t for t in range(4)], [len(d.ids) for d in descs], [d.n_bags for d in descs], lane_group=[True, True, False, True]) == [0, 0, 1, 2]


def test_a_context_of_exactly_two_descriptors_indices_takes_three(eng):
    descs = [Desc(nr, "sum", "i64", 16) for nr in ROWS3]
    n = len(descs[0].ids)
    with eng.grad_context(2 * n, 1024) as small:
        run_both(eng, small, ["f32"] * 3, descs)
        assert small.multi_groups([A0, A0 + 1, A0 + 2], [n] * 3, [gc.N_BAGS] * 3) == [0, 0, 1]
    with eng.grad_context(8192, 2 * gc.N_BAGS) as small:
        run_both(eng, small, ["f32"] * 3, descs)
        assert small.multi_groups([A0, A0 + 1, A0 + 2], [n] * 3, [gc.N_BAGS] * 3) == [0, 0, 1]


def test_gradients_as_column_views_of_one_buffer(eng, ctx):
    """grad_ld = 3 * dim for every descriptor: the [B, 3 * dim] gradient of a concatenated output, read in place."""
    dim = 16
    g = gc.grads(dim, overflow=False)      # (no infinite sum: the row-wise step would make a NaN of it, whose sign and payload are unspecified)
    wide = np.concatenate([g, g[::-1], g * F(0.5)], axis=1)
    d_wide = to_dev(wide)
    descs = [Desc(nr, m, "i64", dim, G=np.ascontiguousarray(wide[:, k * dim:(k + 1) * dim])) for k, (nr, m) in enumerate(zip(ROWS3, ("sum", "mean+pad", "weighted")))]
    run_both(eng, ctx, ["f32", "f16", "bf16"], descs, cols=[d_wide[:, k * dim:(k + 1) * dim] for k in range(3)])
    run_both(eng, ctx, ["f32", "f16", "bf16"], descs, opt="rowwise", cols=[d_wide[:, k * dim:(k + 1) * dim] for k in range(3)])


# ---- stream order -------------------------------------------------------------------------------------------------------------------
def test_two_multi_steps_and_a_prepared_lookup_without_a_host_wait(eng, ctx):
    """The second multi step reuses the scratch of the first; a plan prepared before the steps and launched behind them reads the
    stepped rows.  Nothing waits for the device in between."""
    dim = 16
    first = [Desc(nr, "weighted", "i64", dim, overflow=False) for nr in ROWS3]
    second = [Desc(nr, "mean+pad", "i64", dim, overflow=False) for nr in ROWS3]
    inits = [init_table("f32", nr, dim) for nr in ROWS3]
    want = []
    for t in range(3):
        w1, _ = step_ref("sgd", "f32", inits[t], None, first[t])
        want.append(step_ref("sgd", "f32", w1, None, second[t])[0])
        load_bytes(eng, A0 + t, "f32", inits[t])
        load_bytes(eng, B0 + t, "f32", inits[t])
    rows = first[0].sparse()[0]
    lidx = np.concatenate([rows[:300], np.random.default_rng(5).integers(0, 3001, size=724)]).astype(np.int64)
    loff = np.arange(0, len(lidx), 4, dtype=np.int64)
    want_out = pool_ref.embedding_bag(gr.decode("f32", want[0]), lidx, loff, "sum")
    assert np.isfinite(want_out).all() and not np.array_equal(bits(want_out), bits(pool_ref.embedding_bag(gr.decode("f32", inits[0]), lidx, loff, "sum")))
    d_lidx, d_loff = to_dev(lidx), to_dev(loff)
    plan = eng.plan([A0], [d_lidx], [d_loff])
    dev1, dev2 = [d.on_device() for d in first], [d.on_device() for d in second]
    torch.cuda.synchronize()
    call(ctx, "sgd", [A0, A0 + 1, A0 + 2], dev1, first, None, True)
    call(ctx, "sgd", [A0, A0 + 1, A0 + 2], dev2, second, None, True)
    plan.launch(torch.cuda.current_stream().cuda_stream)
    call(ctx, "sgd", [B0, B0 + 1, B0 + 2], dev1, first, None, False)
    call(ctx, "sgd", [B0, B0 + 1, B0 + 2], dev2, second, None, False)
    torch.cuda.synchronize()                                                     # the first host wait
    got = plan.outputs[0].cpu().numpy()
    plan.destroy()
    assert np.array_equal(bits(got), bits(want_out))
    for t in range(3):
        a = table_bytes(eng, A0 + t)
        assert np.array_equal(a, table_bytes(eng, B0 + t)) and np.array_equal(a, want[t]), t
    assert ctx.report() == 2 * sum(d.sparse()[2] for d in first + second)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_a_refusal_in_the_last_descriptor_leaves_every_table_and_state_alone(eng, ctx, pel):
    UNS = pel.lib.EMB_ERR_UNSUPPORTED
    descs = [Desc(nr, "sum", "i64", 16, overflow=False) for nr in ROWS_SMALL]
    dev = [d.on_device() for d in descs]
    tabs = [A0, A0 + 1, A0 + 2]

    def refused(opt, text, descs=descs, dev=dev):
        before = [table_bytes(eng, t) for t in tabs]
        s0 = [init_state(d.nr, d.dim, opt == "rowwise") for d in descs]
        states = None if opt == "sgd" else [to_dev(s) for s in s0]
        with pytest.raises(pel.PimembError) as ei:
            call(ctx, opt, tabs, dev, descs, states, True)
        assert ei.value.code == UNS and text in str(ei.value) and "_multi" in str(ei.value), str(ei.value)
        for k, t in enumerate(tabs):
            assert np.array_equal(table_bytes(eng, t), before[k]), (opt, t)
            assert states is None or np.array_equal(bits(states[k].cpu().numpy()), bits(s0[k])), (opt, t)
    for t, nr in zip(tabs[:2], ROWS_SMALL[:2]):
        load_bytes(eng, t, "f32", init_table("f32", nr, 16))
    load_bytes(eng, tabs[2], "e4m3", rc.host_encode("e4m3", np.random.default_rng(2).standard_normal((ROWS_SMALL[2], 16)).astype(F)))
    for opt in ("sgd", "adagrad", "rowwise"):
        refused(opt, "fp8 or MXFP4")
    load_bytes(eng, tabs[2], "f32", init_table("f32", ROWS_SMALL[2], 16))
    eng.set_hot_rows(tabs[2], [1, 2, 3])
    for opt in ("sgd", "rowwise"):
        refused(opt, "clear the set")
    eng.set_hot_rows(tabs[2], [])
    load_bytes(eng, tabs[2], "f32", init_table("f32", ROWS_SMALL[2], 6))
    descs6 = descs[:2] + [Desc(ROWS_SMALL[2], "sum", "i64", 6, overflow=False)]
    refused("rowwise", "lane-group shape", descs=descs6, dev=dev[:2] + [descs6[2].on_device()])
    ctx.report()


# ---- the torch surface --------------------------------------------------------------------------------------------------------------
tm = import_module("pim-embedding-lookup_amd.torch_module")


@pytest.mark.parametrize("opt", ["sgd", "rowwise"])
def test_fused_module_with_multi_table_equals_the_module_without(eng, opt):
    """Three backward rounds of FusedPoolingEmbeddingBags(concat=True): weights and Adagrad states equal, bit for bit."""
    names = ["sum", "mean", "sum+pad"]
    batches = [gc.exact_batch(gc.MODES[m][2]) for m in names]
    lS_i, lS_o = [torch.from_numpy(b[0]).to(DEV) for b in batches], [torch.from_numpy(b[1]).to(DEV) for b in batches]
    wide = torch.from_numpy(np.concatenate([batches[0][2], batches[1][2] * 3, -batches[2][2]], axis=1) * F(0.37)).to(DEV)
    results = []
    for multi, base in ((True, 40), (False, 44)):
        bags = [tm.PoolingEmbeddingBag(gc.EXACT_ROWS, 8, mode=gc.MODES[m][0], padding_idx=gc.PAD if gc.MODES[m][2] else None,
                                       _weight=torch.from_numpy(gc.exact_table().copy()), engine=eng, table_id=base + k,
                                       dtype=torch.float32 if k != 1 else torch.bfloat16) for k, m in enumerate(names)]
        fused = tm.FusedPoolingEmbeddingBags(bags, concat=True)
        if opt == "sgd":
            fused.enable_fused_sgd(0.5, multi_table=multi)
        else:
            fused.enable_fused_adagrad(0.1, rowwise=True, multi_table=multi)
        for _ in range(3):
            out = fused(lS_o, lS_i)
            (out * wide).sum().backward()
        if opt == "sgd":
            fused.sgd_step_(lS_o, lS_i, wide, 0.25, multi_table=multi)
        else:
            fused.adagrad_step_(lS_o, lS_i, wide, 0.05, multi_table=multi)
        torch.cuda.synchronize()
        results.append(([b.weight.cpu().contiguous().view(torch.uint8).numpy().copy() for b in fused.bags],
                        [None if opt == "sgd" else b.adagrad_sum.cpu().numpy().copy() for b in fused.bags]))
    (wa, sa), (wb, sb) = results
    for k in range(3):
        assert np.array_equal(wa[k], wb[k]), k
        assert not np.array_equal(wa[k], gr.encode("bf16" if k == 1 else "f32", gc.exact_table()).reshape(wa[k].shape)), k
        assert opt == "sgd" or (np.array_equal(bits(sa[k]), bits(sb[k])) and sa[k].any()), k


def test_harness_flag_runs_and_needs_a_fused_step(pel, capsys):
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    common = ["--arch-sparse-feature-size=16", "--arch-embedding-size=1000-2000-300", "--mini-batch-size=64", "--num-batches=2", "--num-indices-per-lookup=4"]
    for flag, name in (("--fused-sgd", "SGD"), ("--fused-rowwise-adagrad", "row-wise Adagrad")):
        assert h.main(common + [flag, "0.05", "--multi-table-step"]) == 0
        assert f"with the fused {name} step (lr 0.05), multi-table" in capsys.readouterr().out
    with pytest.raises(SystemExit) as ei:
        h.main(common + ["--multi-table-step"])
    assert "--multi-table-step goes with" in str(ei.value)


def test_harness_multi_table_step_steps_its_tables(pel):
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    rng = np.random.default_rng(43)
    ln_emb, m, B = [257, 583, 3001], 16, 64
    weights = [rng.integers(-8, 9, size=(n, m)).astype(F) for n in ln_emb]
    lS_i = [rng.integers(0, n, size=B * 4) for n in ln_emb]
    lS_o = [np.arange(0, B * 4, 4) for _ in ln_emb]
    ebc = h.EmbeddingBagCollection(ln_emb, m, weights=weights).enable_fused_sgd(0.5)
    ebc.multi_table_step = True
    ly = ebc.apply_emb([torch.from_numpy(o).to(DEV) for o in lS_o], [torch.from_numpy(i).to(DEV) for i in lS_i])
    sum(y.sum() for y in ly).backward()
    for k, n in enumerate(ln_emb):
        rows, grads, _ = gr.sparse_grad(n, lS_i[k], lS_o[k], np.ones((B, m), F))
        want = gr.sgd_step("f32", weights[k].view(np.uint8).reshape(n, -1), rows, grads, F(0.5))
        assert np.array_equal(table_bytes(ebc.engine, k), want), k
    ebc.engine.close()
