"""GPU: half-width pooled output (EMB_POOL_OUT_TABLE_DTYPE, out_dtype="table"): fp16 / bf16 tables return rows of their own
dtype, the fp32 pooled value rounded once to nearest even.  The reference of every test is torch on the CPU over the widened
table, rounded by torch -- F.embedding_bag(idx, W.float(), ...).to(W.dtype) -- and every comparison is of the 16-bit patterns
(int16 views, np.array_equal / torch.equal): no tolerance.  Deliberately NOT torch's own half-dtype F.embedding_bag, which
rounds more than once in its bf16 sum and in both dtypes' mean (pimemb.h)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ID_TYPES = [("u32", np.uint32), ("i64", np.int64)]
DTYPES = [("fp16", torch.float16), ("bf16", torch.bfloat16)]
IDS = dict(ids=[n for n, _ in ID_TYPES])
DTS = dict(ids=[n for n, _ in DTYPES])


def table_of(rows, dim, tdt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, dim), generator=g) * scale).to(tdt)


def reference(table, idx, off, mode="sum", weights=None, pad=None):
    """The contract's reference: torch's CPU fp32 embedding_bag over the widened table, rounded once by torch; as int16 bits."""
    w = None if weights is None else torch.as_tensor(weights)
    r = F.embedding_bag(torch.as_tensor(np.asarray(idx).astype(np.int64)), table.float(), torch.as_tensor(np.asarray(off).astype(np.int64)),
                        mode=mode, per_sample_weights=w, padding_idx=pad)
    return r.to(table.dtype).view(torch.int16).numpy()


def bits(x):
    """Pooled rows as int16 bit patterns: torch half tensors (any device), np.float16 arrays, np.uint16 bf16 bits."""
    if isinstance(x, np.ndarray):
        assert x.dtype in (np.float16, np.uint16), x.dtype
        return x.view(np.int16)
    assert x.dtype in (torch.float16, torch.bfloat16), x.dtype
    return x.cpu().contiguous().view(torch.int16).numpy()


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def ragged(rng, rows, bags, max_len, dt):
    """Bags of 0 .. max_len entries (some empty, the last one not: it runs to n_indices)."""
    lens = rng.integers(0, max_len + 1, size=bags)
    lens[-1] = max_len
    off = np.zeros(bags, np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    idx = rng.integers(0, rows, size=int(lens.sum()))
    assert (lens == 0).any()
    return idx.astype(dt), off.astype(dt)


def kinds_delta(eng, before):
    return [a - b for a, b in zip(eng.stats()["n_launches_by_kind"], before)]


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


# ---- every row width: the tuned widths (1 .. 64 lanes per row) and the any-dim paths: 12, 5 and 1 are element-wise (output rows
# that are only 2-byte aligned for 5 and 1), 20 is the piece path with a partial last piece ---------------------------------------
WIDTHS = [8, 16, 32, 64, 128, 256, 512, 12, 5, 1, 20]


@pytest.mark.parametrize("ids", ID_TYPES, **IDS)
@pytest.mark.parametrize("tdt", DTYPES, **DTS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_every_row_width(eng, pel, dim, tdt, ids):
    (_tn, tdt), (_in, dt) = tdt, ids
    rows, bags = 1009, 193
    table = table_of(rows, dim, tdt, 100 + dim)
    eng.load_table(0, table.to(DEV))
    idx, off = ragged(np.random.default_rng(dim), rows, bags, 9, dt)
    want = reference(table, idx, off)
    # device tensors, plan-less
    d_idx, d_off = to_dev(idx), to_dev(off)
    got = eng.lookup_batched([0], [d_idx], [d_off], out_dtype="table")[0]
    torch.cuda.synchronize()
    assert got.dtype is tdt and tuple(got.shape) == (bags, dim)
    assert np.array_equal(bits(got), want)
    # a prepared plan
    plan = eng.plan([0], [d_idx], [d_off], out_dtype="table")
    recs = plan.describe()
    rb = 2 * dim
    anydim = rb % 16 != 0 or rb > 1024
    assert len(recs) == 1 and recs[0]["out"] == 1 and recs[0]["kind"] == (3 if anydim else 1) and "pool" not in recs[0]
    if anydim:
        assert recs[0]["anydim_vec"] == int(rb % 4 == 0 and rb >= 32)
    assert plan.bytes()[0] == len(idx) * (rb + idx.itemsize) + bags * idx.itemsize + bags * dim * 2      # 2 bytes per output element
    assert plan.outputs[0].dtype is tdt
    plan.outputs[0].fill_(7.0)
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan.outputs[0]), want)
    plan.destroy()
    # host pointers: np.float16, or uint16 bits for bf16
    got = eng.lookup_batched([0], [idx], [off], out_dtype="table")[0]
    assert isinstance(got, np.ndarray) and got.dtype == (np.float16 if tdt is torch.float16 else np.uint16)
    assert np.array_equal(bits(got), want)


# ---- the kernel kinds (choose_kernel: >= 2048 x 64 one-hot bags; two batches from 4096 x 128 bags of <= 4 lanes per row) --------
@pytest.mark.parametrize("tdt", DTYPES, **DTS)
@pytest.mark.parametrize("kind,dim,B", [(0, 64, 131072 + 1), (2, 16, 524288 + 3)], ids=["wavebatch", "two-batch"])
def test_one_hot_wave_batch_kinds(eng, pel, kind, dim, B, tdt):
    _tn, tdt = tdt
    rows = 5000
    table = table_of(rows, dim, tdt, 11 + kind)
    eng.load_table(1, table.to(DEV))
    rng = np.random.default_rng(11)
    for _name, dt in ID_TYPES:
        idx = rng.integers(0, rows, size=B).astype(dt)
        i, o = to_dev(idx), to_dev(np.arange(B).astype(dt))
        plan = eng.plan([1], [i], [o], out_dtype="table")
        recs = plan.describe()
        assert len(recs) == 1 and recs[0]["kind"] == kind and recs[0]["out"] == 1 and "pool" not in recs[0]
        before = eng.stats()["n_launches_by_kind"]
        plan.launch(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        delta = kinds_delta(eng, before)
        assert delta[kind] == 1 and sum(delta) == 1              # counted under its existing kind
        # a one-index bag returns the table's values bit for bit (a sum starts at +0: a -0 element comes back as +0)
        got = plan.outputs[0].cpu().view(torch.int16).numpy()
        plan.destroy()
        want = table[torch.from_numpy(idx.astype(np.int64))].view(torch.int16).numpy().copy()
        want[want == -32768] = 0
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s ids: %d of %d elements differ; first (bag, col, got, want): %s" % (
            _name, len(bad), got.size, [(int(b), int(c), int(got[b, c]), int(want[b, c])) for b, c in bad[:6]])


@pytest.mark.parametrize("tdt", DTYPES, **DTS)
def test_lane_group_kind1_pooled(eng, pel, tdt):
    """37 indices per bag of N(0, 3^2) rows: where torch's own bf16 sum rounds more than once, this one does not."""
    _tn, tdt = tdt
    rows, dim, B, L = 3000, 64, 1500, 37
    table = table_of(rows, dim, tdt, 21, scale=3.0)
    eng.load_table(2, table.to(DEV))
    idx = np.random.default_rng(21).integers(0, rows, size=B * L)
    off = np.arange(B) * L
    plan = eng.plan([2], [to_dev(idx)], [to_dev(off)], out_dtype="table")
    assert [(r["kind"], r.get("out")) for r in plan.describe()] == [(1, 1)]
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan.outputs[0]), reference(table, idx, off))
    plan.destroy()


# ---- rounding: once, to nearest even ---------------------------------------------------------------------------------------------
def rounding_rows(tdt):
    """(values, {name: (row a, row b, expected fp32 value of the half result)}): two-row bags a + b."""
    if tdt is torch.bfloat16:
        vals = [1.0, 2.0 ** -8, 1.0078125, 2.0 ** 127, -(2.0 ** 127), 2.0 ** -133, 0.0, -0.0, 1.5, -1.5, 0.337890625]
        exp = {"tie to even, down": (0, 1, 1.0), "tie to even, up": (2, 1, 1.015625), "subnormal": (5, 5, 2.0 ** -132),
               "+inf": (3, 3, float("inf")), "-inf": (4, 4, float("-inf"))}
    else:
        vals = [1.0, 2.0 ** -11, 1.0 + 2.0 ** -10, 60000.0, -60000.0, 2.0 ** -24, 0.0, -0.0, 1.5, -1.5, 0.337890625]
        exp = {"tie to even, down": (0, 1, 1.0), "tie to even, up": (2, 1, 1.0 + 2.0 ** -9), "subnormal": (5, 5, 2.0 ** -23),
               "+inf": (3, 3, float("inf")), "-inf": (4, 4, float("-inf"))}
    exp.update({"+0 + -0": (6, 7, 0.0), "-0 + -0": (7, 7, 0.0), "x + -x": (8, 9, 0.0)})
    return vals, exp


@pytest.mark.parametrize("dim", [8, 64, 5], ids=["lanes1", "lanes8", "anydim"])
@pytest.mark.parametrize("tdt", DTYPES, **DTS)
def test_rounds_once_to_nearest_even(eng, pel, tdt, dim):
    _tn, tdt = tdt
    vals, exp = rounding_rows(tdt)
    table = torch.tensor(vals, dtype=torch.float32).to(tdt)[:, None].repeat(1, dim).contiguous()
    assert torch.equal(table[:, 0].float(), torch.tensor(vals))          # every value is exact in the table's dtype
    eng.load_table(3, table.to(DEV))
    names = list(exp)
    idx = np.array([r for n in names for r in exp[n][:2]], np.int64)
    off = np.arange(len(names), dtype=np.int64) * 2
    want = reference(table, idx, off)
    got = eng.lookup_batched([3], [to_dev(idx)], [to_dev(off)], out_dtype="table")[0]
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), want)
    for k, n in enumerate(names):                                          # ... and the reference says what the case is there for
        v = torch.tensor([exp[n][2]]).to(tdt)
        assert bool((got[k].cpu().view(torch.int16) == v.view(torch.int16)).all()), (n, got[k, 0].item())
    assert not bool(torch.signbit(got[names.index("-0 + -0")].float()).any())       # a sum starts at +0
    # max keeps the first of equal values and returns table bits: -0 stays -0
    got = eng.lookup_pooled([3], [to_dev(np.array([7, 7, 6], np.int64))], [to_dev(np.array([0, 2], np.int64))], "max", out_dtype="table")[0]
    torch.cuda.synchronize()
    assert bits(got)[:, 0].tolist() == [-32768, 0]
    if tdt is torch.bfloat16:                                              # a weighted bag and a mean over 3
        i3, o3 = np.array([0, 2, 10, 8, 0, 2], np.int64), np.array([0, 3], np.int64)
        w = np.array([0.3, 1.7, -2.9, 0.1, 3.3, 0.7], np.float32)
        got = eng.lookup_pooled([3, 3], [to_dev(i3)] * 2, [to_dev(o3)] * 2, ["sum", "mean"],
                                per_sample_weights=[torch.from_numpy(w).to(DEV), None], out_dtype="table")
        torch.cuda.synchronize()
        assert np.array_equal(bits(got[0]), reference(table, i3, o3, "sum", w))
        assert np.array_equal(bits(got[1]), reference(table, i3, o3, "mean"))


@pytest.mark.parametrize("tdt", DTYPES, **DTS)
def test_one_hot_over_every_bit_pattern(eng, pel, tdt):
    """Every non-NaN 16-bit pattern as a one-index bag: the conversion flushes no subnormal and moves no bit (a sum starts at
    +0, so -0 comes back as +0, as in the reference; max returns -0 too)."""
    _tn, tdt = tdt
    allbits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(tdt)
    keep = allbits[~torch.isnan(allbits.float())]
    assert len(keep) == (63490 if tdt is torch.float16 else 65282)            # +-inf included
    keep = torch.cat([keep, torch.zeros((-len(keep)) % 8, dtype=tdt)])        # (whole rows)
    for dim in (8, 2):                                                     # a tuned width, an any-dim element width
        table = keep.reshape(-1, dim).contiguous()
        eng.load_table(4, table.to(DEV))
        n = table.shape[0]
        idx = np.arange(n, dtype=np.int64)
        want = reference(table, idx, idx)
        got = eng.lookup_batched([4], [to_dev(idx)], [to_dev(idx)], out_dtype="table")[0]
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), want)
        tb = table.view(torch.int16).numpy()
        assert np.array_equal(bits(got)[tb != -32768], tb[tb != -32768])  # the table's bits, -0 aside
        got = eng.lookup_pooled([4], [to_dev(idx)], [to_dev(idx)], "max", out_dtype="table")[0]
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), tb)


# ---- pooled modes ----------------------------------------------------------------------------------------------------------------
POOL_SHAPES = {16: (400, 300), 128: (300, 150), 18: (300, 150)}             # dim: rows, bags (18: the any-dim piece path)
MODES = ["sum+weights", "sum+padding", "weights+padding", "mean", "mean+padding", "max"]


@pytest.fixture(scope="module")
def pooled_case():
    cases = {}
    for tn, tdt in DTYPES:
        for dim, (rows, bags) in POOL_SHAPES.items():
            table = table_of(rows, dim, tdt, 40 + dim)
            idx, off = ragged(np.random.default_rng(40 + dim), rows, bags, 9, np.int64)
            pad = 11
            idx[::5] = pad                                                  # padding entries; some bags of padding only
            w = torch.randn(len(idx), generator=torch.Generator().manual_seed(dim)).numpy()
            refs = {"sum+weights": reference(table, idx, off, "sum", w), "sum+padding": reference(table, idx, off, "sum", None, pad),
                    "weights+padding": reference(table, idx, off, "sum", w, pad), "mean": reference(table, idx, off, "mean"),
                    "mean+padding": reference(table, idx, off, "mean", None, pad), "max": reference(table, idx, off, "max")}
            cases[(tn, dim)] = (table, idx, off, w, pad, refs)
    return cases


@pytest.mark.parametrize("ids", ID_TYPES, **IDS)
@pytest.mark.parametrize("tdt", DTYPES, **DTS)
@pytest.mark.parametrize("dim", list(POOL_SHAPES))
def test_pooled_modes(eng, pel, pooled_case, dim, tdt, ids):
    (tn, tdt), (_in, dt) = tdt, ids
    table, idx, off, w, pad, refs = pooled_case[(tn, dim)]
    eng.load_table(5, table.to(DEV))
    i, o, wt = to_dev(idx.astype(dt)), to_dev(off.astype(dt)), torch.from_numpy(w).to(DEV)
    specs = {"sum+weights": ("sum", wt, None), "sum+padding": ("sum", None, pad), "weights+padding": ("sum", wt, pad),
             "mean": ("mean", None, None), "mean+padding": ("mean", None, pad), "max": ("max", None, None)}
    n = len(MODES)
    args = dict(per_sample_weights=[specs[m][1] for m in MODES], padding_idx=[specs[m][2] for m in MODES], out_dtype="table")
    outs = eng.lookup_pooled([5] * n, [i] * n, [o] * n, [specs[m][0] for m in MODES], **args)
    torch.cuda.synchronize()
    for m, out in zip(MODES, outs):
        assert out.dtype is tdt and np.array_equal(bits(out), refs[m]), m
    plan = eng.plan([5] * n, [i] * n, [o] * n, modes=[specs[m][0] for m in MODES], **args)
    recs = plan.describe()
    assert len(recs) == 3 and all(r["out"] == 1 and "pool" in r for r in recs)       # sum, mean, max
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for m, out in zip(MODES, plan.outputs):
        assert np.array_equal(bits(out), refs[m]), m
    plan.destroy()
    # host pointers: the weights are staged with the indices, the rows come back as 2-byte elements
    got = eng.lookup_pooled([5], [idx.astype(dt)], [off.astype(dt)], "sum", per_sample_weights=[w], padding_idx=pad, out_dtype="table")[0]
    assert np.array_equal(bits(got), refs["weights+padding"])


def test_pooled_one_hot_wave_batch(eng, pel):
    """The pooled wave-batch twin: weighted one-index bags."""
    rows, dim, B = 3000, 32, 131072 + 5
    table = table_of(rows, dim, torch.bfloat16, 50)
    eng.load_table(6, table.to(DEV))
    rng = np.random.default_rng(50)
    idx, w = rng.integers(0, rows, size=B), rng.standard_normal(B).astype(np.float32)
    off = np.arange(B)
    plan = eng.plan_pooled([6], [to_dev(idx)], [to_dev(off)], "sum", per_sample_weights=[torch.from_numpy(w).to(DEV)], out_dtype="table")
    assert [(r["kind"], r["out"], r["pool"]) for r in plan.describe()] == [(0, 1, 0)]
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(plan.outputs[0]), reference(table, idx, off, "sum", w))
    plan.destroy()


# ---- one call, mixed outputs -----------------------------------------------------------------------------------------------------
def test_mixed_call_and_signatures(eng, pel):
    rows, dim, bags = 700, 32, 333
    f32 = torch.randn((rows, dim), generator=torch.Generator().manual_seed(60))
    bf = table_of(rows, dim, torch.bfloat16, 61)
    eng.load_table(7, f32.to(DEV))
    eng.load_table(8, bf.to(DEV))
    idx, off = ragged(np.random.default_rng(60), rows, bags, 9, np.int64)
    i, o = to_dev(idx), to_dev(off)
    two = eng.lookup_batched([7, 8], [i, i], [o, o])
    three = eng.lookup_batched([7, 8, 8], [i] * 3, [o] * 3, out_dtype=[None, None, "table"])
    torch.cuda.synchronize()
    assert [t.dtype for t in three] == [torch.float32, torch.float32, torch.bfloat16]
    assert torch.equal(three[0], two[0]) and torch.equal(three[1], two[1])       # the unflagged outputs: bit for bit
    assert np.array_equal(bits(three[2]), reference(bf, idx, off))
    assert torch.equal(three[2], three[1].to(torch.bfloat16))                     # ... the fp32 row rounded once
    # signatures: without the flag a pooled plan IS emb_plan_create's; with it, it is not
    plain = eng.plan([7, 8], [i, i], [o, o])
    pooled = eng.plan_pooled([7, 8], [i, i], [o, o], "sum")
    mixed = eng.plan([7, 8, 8], [i] * 3, [o] * 3, out_dtype=[None, None, "table"])
    only_f32_out = eng.plan([7, 8, 8], [i] * 3, [o] * 3)
    assert plain.signature() == pooled.signature()
    assert mixed.signature() != only_f32_out.signature()
    assert [r.get("out", 0) for r in mixed.describe()] == [0, 0, 1] and all("out" not in r for r in only_f32_out.describe())
    assert only_f32_out.bytes()[0] - mixed.bytes()[0] == bags * dim * 2
    for p in (plain, pooled, mixed, only_f32_out):
        p.destroy()


# ---- checked calls and refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [True, "deferred"])
def test_checked_calls_refuse_a_bad_index(eng, pel, check):
    rows, dim, bags = 500, 16, 100
    table = table_of(rows, dim, torch.float16, 70)
    eng.load_table(9, table.to(DEV))
    idx, off = ragged(np.random.default_rng(70), rows, bags, 9, np.int64)
    bad = idx.copy()
    bad[17] = rows + 5
    out = torch.full((bags, dim), 3.0, dtype=torch.float16, device=DEV)
    with pytest.raises(IndexError):                                                # EMB_ERR_RANGE; deferred: through emb_check_report
        eng.lookup_batched([9], [to_dev(bad)], [to_dev(off)], outs=[out], check=check, out_dtype="table")
        if check == "deferred":
            eng.check_report()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                                                # the half output is untouched
    res = eng.lookup_batched([9], [to_dev(idx)], [to_dev(off)], outs=[out], check=check, out_dtype="table")[0]
    if check == "deferred":
        eng.check_report()
    torch.cuda.synchronize()
    assert res is out and np.array_equal(bits(out), reference(table, idx, off))
    if check is True:                                                              # a HOST call is checked synchronously
        with pytest.raises(IndexError):
            eng.lookup_batched([9], [bad], [off], check=True, out_dtype="table")


def test_refusals(eng, pel):
    L = pel.lib
    eng.load_table(10, torch.randn(50, 16).to(DEV))
    eng.load_table(11, torch.randint(-5, 5, (50, 16), dtype=torch.int32).to(DEV))
    eng.load_table(12, table_of(50, 16, torch.float16, 80).to(DEV))
    idx = to_dev(np.arange(20, dtype=np.int64))
    for tid in (10, 11):                                                           # an fp32 and a fixed-point table
        for mode in ("sum", "mean"):
            with pytest.raises(pel.PimembError) as ex:
                eng.lookup_pooled([tid], [idx], [idx], mode, out_dtype="table")
            assert ex.value.code == L.EMB_ERR_UNSUPPORTED
        with pytest.raises(pel.PimembError) as ex:
            eng.plan([tid], [idx], [idx], out_dtype="table")
        assert ex.value.code == L.EMB_ERR_UNSUPPORTED
    # an unknown flag bit stays invalid, with or without the known ones
    half = [True]
    arr, n, itype, space, results, _keep = eng._descs([12], [idx], [idx], None, 0, half=half)
    for flags in (4, 4 | L.EMB_POOL_OUT_TABLE_DTYPE):
        pools, _k = eng._pools(n, arr, "sum", None, None, space, half)
        pools[0].flags = flags
        assert eng._L.emb_lookup_pooled(eng._h, arr, pools, n, itype, space, None, 0, None) == L.EMB_ERR_INVALID
        p = C.c_void_p()
        assert eng._L.emb_plan_create_pooled(eng._h, arr, pools, n, itype, C.byref(p)) == L.EMB_ERR_INVALID


# ---- hot rows: a half-output launch never takes the hot-row kernel ---------------------------------------------------------------
def test_hot_rows_change_no_bit(pel):
    rows, dim, B, Lp = 20000, 64, 1500, 32
    table = table_of(rows, dim, torch.bfloat16, 30)
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    eng.load_table(0, table.to(DEV))
    rng = np.random.default_rng(30)
    idx = pel.workloads.zipf_indices(rng, rows, B * Lp, 1.2, dtype=np.int64)
    off = pel.workloads.fixed_offsets(B, Lp, dtype=np.int64)
    d_idx, d_off = to_dev(idx), to_dev(off)
    cold = eng.lookup_batched([0], [d_idx], [d_off], out_dtype="table")[0].clone()
    eng.set_hot_rows(0, pel.workloads.top_rows(idx, 100))
    before = eng.stats()["n_launches_by_kind"]
    hot = eng.lookup_batched([0], [d_idx], [d_off], out_dtype="table")[0]
    torch.cuda.synchronize()
    assert kinds_delta(eng, before) == [0, 1, 0, 0, 0]                               # kind 4 does not move
    assert torch.equal(cold.view(torch.int16), hot.view(torch.int16)) and np.array_equal(bits(hot), reference(table, idx, off))
    before = eng.stats()["n_launches_by_kind"]
    eng.lookup_batched([0], [d_idx], [d_off])                                      # the fp32-out call still does
    torch.cuda.synchronize()
    assert kinds_delta(eng, before) == [0, 0, 0, 0, 1]
    eng.close()


# ---- the modules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", DTYPES, **DTS)
def test_torch_modules(pel, tdt):
    from importlib import import_module
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    _tn, tdt = tdt
    rows, dim, bags = 300, 24, 77
    w = table_of(rows, dim, tdt, 90)
    idx, off = ragged(np.random.default_rng(90), rows, bags, 9, np.int64)
    i, o = torch.from_numpy(idx).to(DEV), torch.from_numpy(off).to(DEV)
    # EmbeddingBag: the weight's dtype on request, fp32 by default
    bag = tm.EmbeddingBag(rows, dim, _weight=w, dtype=tdt, out_dtype="weight")
    plain = tm.EmbeddingBag(rows, dim, _weight=w, dtype=tdt)
    got, got32 = bag(i, o), plain(i, o)
    torch.cuda.synchronize()
    assert got.dtype is tdt and np.array_equal(bits(got), reference(w, idx, off))
    assert got32.dtype is torch.float32 and torch.equal(got32.cpu(), F.embedding_bag(torch.from_numpy(idx), w.float(), torch.from_numpy(off), mode="sum"))
    fused = tm.FusedEmbeddingBags([bag, plain])
    a, b = fused([o, o], [i, i])
    torch.cuda.synchronize()
    assert a.dtype is tdt and b.dtype is torch.float32 and torch.equal(a, got) and torch.equal(b, got32)
    a, b = tm.FusedEmbeddingBags([bag, plain], out_dtype="weight")([o, o], [i, i])
    assert a.dtype is tdt and b.dtype is tdt and torch.equal(a, got) and torch.equal(b, got)
    stacked = tm.FusedEmbeddingBags([bag, bag])(torch.stack([o, o]), torch.stack([i, i]))      # 2-D inputs: still half rows
    assert all(t.dtype is tdt and torch.equal(t, got) for t in stacked)
    # an fp32 weight: "weight" is fp32
    f32 = tm.EmbeddingBag(rows, dim, _weight=w.float(), out_dtype="weight")
    assert f32(i, o).dtype is torch.float32
    # from_torch passes it through; PoolingEmbeddingBag with mean / max / padding / weights
    for mode, pad in (("mean", None), ("max", 11), ("sum", 11)):
        ref_mod = torch.nn.EmbeddingBag(rows, dim, mode=mode, padding_idx=pad, _weight=w.float().clone())
        pb = tm.PoolingEmbeddingBag.from_torch(ref_mod, dtype=tdt, out_dtype="weight")
        pw = torch.randn(len(idx), generator=torch.Generator().manual_seed(3)) if mode == "sum" else None
        got = pb(i, o, per_sample_weights=None if pw is None else pw.to(DEV))
        torch.cuda.synchronize()
        assert got.dtype is tdt and np.array_equal(bits(got), reference(w, idx, off, mode, None if pw is None else pw.numpy(), pad)), mode
        got32 = tm.PoolingEmbeddingBag.from_torch(ref_mod, dtype=tdt)(i, o)
        assert got32.dtype is torch.float32
    mods = [torch.nn.EmbeddingBag(rows, dim, mode=m, _weight=w.float().clone()) for m in ("mean", "max")]
    fp = tm.FusedPoolingEmbeddingBags.from_torch(mods, dtype=tdt, out_dtype="weight")
    outs = fp([o, o], [i, i])
    torch.cuda.synchronize()
    for m, out in zip(("mean", "max"), outs):
        assert out.dtype is tdt and np.array_equal(bits(out), reference(w, idx, off, m)), m
    assert all(t.dtype is torch.float32 for t in tm.FusedPoolingEmbeddingBags.from_torch(mods, dtype=tdt)([o, o], [i, i]))


def test_half_out_plan_launch_is_graph_capturable(eng, pel):
    rows, dim = 5000, 16
    w = table_of(rows, dim, torch.bfloat16, 95)
    eng.load_table(13, w.to(DEV))
    idx = torch.randint(0, rows, (512,), dtype=torch.int64, device=DEV)
    off = torch.arange(0, 512, 2, dtype=torch.int64, device=DEV)
    plan = eng.plan([13, 13], [idx, idx], [off, off], modes=["sum", "mean"], out_dtype="table")
    s = torch.cuda.Stream(torch.device(DEV))
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        plan.launch(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):                              # new indices in the same buffers: replay picks them up
        for out in plan.outputs:
            out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(plan.outputs[0]), reference(w, idx.cpu().numpy(), off.cpu().numpy()))
        assert np.array_equal(bits(plan.outputs[1]), reference(w, idx.cpu().numpy(), off.cpu().numpy(), "mean"))
        idx.copy_(torch.randint(0, rows, (512,), dtype=torch.int64, device=DEV))
    plan.destroy()


def test_dlrm_harness_takes_out_dtype(pel):
    from importlib import import_module
    dh = import_module("pim-embedding-lookup_amd.dlrm_harness")
    ln, m = [300, 50, 1200], 16
    half = dh.EmbeddingBagCollection(ln, m, seed=3, dtype="bf16", out_dtype="weight")
    full = dh.EmbeddingBagCollection(ln, m, seed=3, dtype="bf16")
    rng = np.random.default_rng(3)
    lS_i = [torch.from_numpy(rng.integers(0, n, size=64)).to(DEV) for n in ln]
    lS_o = [torch.arange(0, 64, 2, dtype=torch.int64, device=DEV) for _ in ln]
    a, b = half.apply_emb(lS_o, lS_i), full.apply_emb(lS_o, lS_i)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.dtype is torch.bfloat16 and y.dtype is torch.float32 and torch.equal(x, y.to(torch.bfloat16))
    plan = half.prepare(lS_o, lS_i)
    assert all(t.dtype is torch.bfloat16 for t in plan.outputs) and all(r["out"] == 1 for r in plan.describe())
    half.close()
    full.close()
