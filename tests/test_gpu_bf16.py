"""GPU: bfloat16 tables (EMB_BF16) through every lookup path, bit for bit.  A bf16 row widens to fp32 exactly, so the
reference is the fp32 reference on `table.float()`: the oracle's sequential sum, tests/pool_ref.py for the pooled modes,
torch's CPU F.embedding_bag for the modules.  Every comparison is np.array_equal / torch.equal -- no tolerance."""
import ctypes as C
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ID_TYPES = [("u32", np.uint32), ("i64", np.int64)]


def bf16_table(rows, dim, seed):
    """(torch bf16 CPU tensor, its exact fp32 widening as numpy)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn((rows, dim), generator=g).to(torch.bfloat16)
    return t, t.float().numpy()


def bits_of(t):
    """A bf16 tensor's bits as a numpy uint16 array (what load_table takes with dtype=EMB_BF16)."""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def to_dev(a):
    """numpy ids -> CUDA tensor (uint32 bits travel as int32)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def ragged(rng, rows, bags, max_len, p_empty, dt):
    lens = rng.integers(1, max_len + 1, size=bags)
    lens[rng.random(bags) < p_empty] = 0
    off = np.zeros(bags, np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    idx = rng.integers(0, rows, size=int(lens.sum()))
    return idx.astype(dt), off.astype(dt)


def kinds_delta(eng, before):
    return [a - b for a, b in zip(eng.stats()["n_launches_by_kind"], before)]


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


# ---- every row width: 16-byte lane pieces (1 .. 64 lanes per row, 25 pieces in 32 lanes), the any-dim vector and element paths ----
WIDTHS = [8, 16, 32, 64, 128, 256, 512, 200, 18, 514, 1, 3, 6]


@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("dim", WIDTHS)
def test_every_row_width(eng, pel, oracle, dim, ids):
    name, dt = ids
    rows, bags = 3001, 777
    table, wide = bf16_table(rows, dim, 100 + dim)
    if dt is np.uint32:
        eng.load_table(0, bits_of(table), dtype=pel.EMB_BF16)       # numpy: uint16 bits, declared
    else:
        eng.load_table(0, table.to(DEV))                             # torch (a CPU tensor is loaded by the cases below)
    view = eng.table_tensor(0)
    assert view.dtype is torch.bfloat16 and tuple(view.shape) == (rows, dim) and torch.equal(view.cpu(), table)
    assert eng.table_info(0)[1:] == (rows, dim, pel.EMB_BF16)
    rng = np.random.default_rng(dim * 7 + len(name))
    idx, off = ragged(rng, rows, bags, 70, 0.2, dt)
    want = oracle.c_bag_sum(wide, idx, off)
    # host arrays
    got = eng.lookup_batched([0], [idx], [off])[0]
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    # device tensors
    d_idx, d_off = to_dev(idx), to_dev(off)
    got = eng.lookup_batched([0], [d_idx], [d_off])[0]
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    # a prepared plan
    plan = eng.plan([0], [d_idx], [d_off])
    recs = plan.describe()
    rb = 2 * dim
    anydim = rb % 16 != 0 or rb > 1024
    assert len(recs) == 1 and recs[0]["dtype"] == pel.EMB_BF16 and recs[0]["kind"] == (3 if anydim else 1)
    if anydim:
        assert recs[0]["anydim_vec"] == int(rb % 4 == 0 and rb >= 32)
    else:
        lpr = 1
        while lpr < rb // 16:
            lpr *= 2
        assert recs[0]["lanes_per_row"] == lpr and recs[0]["chunks"] == rb // 16
    assert plan.bytes()[0] == len(idx) * (rb + idx.itemsize) + bags * idx.itemsize + bags * dim * 4    # 2 bytes per element
    plan.outputs[0].fill_(7.0)
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(plan.outputs[0].cpu().numpy(), want)
    plan.destroy()


def test_torch_cpu_tensor_loads_and_unknown_dtype_is_invalid(eng, pel, oracle):
    table, wide = bf16_table(500, 24, 5)
    eng.load_table(1, table)                                         # torch.bfloat16 on the CPU -> EMB_BF16
    assert eng.table_info(1)[3] == pel.EMB_BF16
    idx, off = ragged(np.random.default_rng(5), 500, 64, 9, 0.2, np.int64)
    assert np.array_equal(eng.lookup_batched([1], [idx], [off])[0], oracle.c_bag_sum(wide, idx, off))
    eng.alloc_table(2, 100, 16, pel.EMB_BF16)                        # emb_alloc_table: zero rows
    assert eng.table_tensor(2).dtype is torch.bfloat16 and not bool(eng.table_tensor(2).float().any())
    with pytest.raises(pel.PimembError) as ex:
        eng.alloc_table(3, 100, 16, 4)                               # an unknown dtype value stays invalid
    assert ex.value.code == pel.lib.EMB_ERR_INVALID
    with pytest.raises(KeyError):
        eng.load_table(3, np.zeros((4, 8), np.uint16))               # uint16 without dtype=EMB_BF16: refused as before
    with pytest.raises(pel.PimembError):
        eng.load_table_column(2, 0, np.zeros(100, np.int32))         # columns stay fixed-point only


# ---- the wave-batch kinds (choose_kernel: >= 2048 x 64 one-hot bags; two batches from 4096 x 128 bags of <= 4 lanes per row) ----
def test_wavebatch_one_hot_kind0(eng, pel):
    rows, dim, B = 5000, 64, 131072 + 1
    table, wide = bf16_table(rows, dim, 11)
    eng.load_table(4, table.to(DEV))
    rng = np.random.default_rng(11)
    for _name, dt in ID_TYPES:
        idx = rng.integers(0, rows, size=B).astype(dt)
        off = np.arange(B).astype(dt)
        before = eng.stats()["n_launches_by_kind"]
        got = eng.lookup_batched([4], [to_dev(idx)], [to_dev(off)])[0]
        torch.cuda.synchronize()
        assert kinds_delta(eng, before) == [1, 0, 0, 0, 0]
        assert np.array_equal(got.cpu().numpy(), wide[idx.astype(np.int64)])


def test_wavebatch_two_batches_kind2(eng, pel):
    rows, dim, B, n = 5000, 16, 65537, 8
    table, wide = bf16_table(rows, dim, 12)
    eng.load_table(5, table.to(DEV))
    rng = np.random.default_rng(12)
    for _name, dt in ID_TYPES:
        idxs = [rng.integers(0, rows, size=B).astype(dt) for _ in range(n)]
        off = to_dev(np.arange(B).astype(dt))
        before = eng.stats()["n_launches_by_kind"]
        outs = eng.lookup_batched([5] * n, [to_dev(i) for i in idxs], [off] * n)
        torch.cuda.synchronize()
        assert kinds_delta(eng, before) == [0, 0, 1, 0, 0]
        for k in range(n):
            assert np.array_equal(outs[k].cpu().numpy(), wide[idxs[k].astype(np.int64)]), k


# ---- all 65 536 bit patterns -----------------------------------------------------------------------------------------------
def test_every_bit_pattern(eng, pel, oracle):
    formats = import_module("pim-embedding-lookup_amd.formats")
    bits = np.zeros((8193, 8), np.uint16)                            # row 8192: the zero row
    bits[:8192] = np.arange(65536, dtype=np.uint16).reshape(8192, 8)
    wide = formats.from_bf16_bits(bits)
    eng.load_table(6, bits, dtype=pel.EMB_BF16)
    assert np.array_equal(bits_of(eng.table_tensor(6).cpu()), bits)

    def check(got, want):
        nan = np.isnan(want)
        assert nan.any() and np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan], want[~nan])

    one = np.arange(8192, dtype=np.int64)
    want = oracle.c_bag_sum(wide, one, one)
    assert int(np.isnan(want).sum()) == 2 * 127                      # every NaN pattern of either sign
    got = eng.lookup_batched([6], [to_dev(one)], [to_dev(one)])[0]   # one lookup per row (lane-group kernel)
    torch.cuda.synchronize()
    check(got.cpu().numpy(), want)
    many = np.tile(one, 17)                                           # ... and through the wave-batch kernel (17 x 8192 one-hot bags)
    off = np.arange(len(many), dtype=np.int64)
    before = eng.stats()["n_launches_by_kind"]
    got = eng.lookup_batched([6], [to_dev(many)], [to_dev(off)])[0]
    torch.cuda.synchronize()
    assert kinds_delta(eng, before)[0] == 1
    check(got.cpu().numpy(), np.tile(want, (17, 1)))
    pair = np.stack([one, np.full(8192, 8192)], axis=1).reshape(-1)   # two-entry bags: the row, then the zero row
    off2 = np.arange(0, 2 * 8192, 2, dtype=np.int64)
    got = eng.lookup_batched([6], [to_dev(pair)], [to_dev(off2)])[0]
    torch.cuda.synchronize()
    check(got.cpu().numpy(), oracle.c_bag_sum(wide, pair, off2))
    # pooled modes see the same widening (max keeps a row as it is: every non-NaN pattern comes back exactly)
    got = eng.lookup_pooled([6], [to_dev(one)], [to_dev(one)], "max")[0]
    torch.cuda.synchronize()
    got, nan = got.cpu().numpy(), np.isnan(wide[:8192])
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], wide[:8192].view(np.uint32)[~nan])


# ---- ranged, counted and open-end lookups ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("dim", [16, 64])
def test_ranged_counted_open_end(pel, dim, ids):
    _name, dt = ids
    rows, N, B = 5003, 2, 4001
    table, wide = bf16_table(rows, dim, 20 + dim)
    per = -(-rows // N)
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    for d in range(N):
        eng.load_table(d, table[d * per:min((d + 1) * per, rows)].contiguous())
    rng = np.random.default_rng(dim)
    idx = rng.integers(0, rows, size=B).astype(np.int64)
    nobody = {3: rows + 100, 11: rows, 500: rows + 7, B - 1: (1 << 31) + 5}
    if dt is np.int64:
        nobody.update({12: -1, 1000: (1 << 32) + 5, 2000: -(1 << 45), 3000: 1 << 62})
    for p, v in nobody.items():
        idx[p] = v
    held = (idx >= 0) & (idx < rows)
    rows_of = wide[np.clip(idx, 0, rows - 1)]
    d_idx = to_dev(idx.astype(dt))
    itype = pel.lib.EMB_IDX_U32 if dt is np.uint32 else pel.lib.EMB_IDX_I64
    L = pel.lib.load()
    ctr = torch.zeros((N, 64 * 256 // 4), dtype=torch.int32, device=DEV)      # EMB_SERVED_LANES x EMB_SERVED_STRIDE bytes per counter
    served = (C.c_void_p * N)(*[ctr[d].data_ptr() for d in range(N)])
    mine = [(idx >= d * per) & (idx < min((d + 1) * per, rows)) for d in range(N)]

    def descs(out, which=range(N)):
        return (pel.lib.EmbLookupDesc * len(which))(*[pel.lib.EmbLookupDesc(d, 1, d_idx.data_ptr(), None, B, B, out.data_ptr()) for d in which])

    # one shard at a time, no open end: only its own bags are written, every other bag stays as it was
    out = torch.full((B, dim), float("nan"), device=DEV)
    seen = np.zeros(B, bool)
    for d in range(N):
        pel.lib.check(L.emb_lookup_ranged_typed(eng._h, descs(out, [d]), (C.c_uint64 * 1)(d * per), None, 1, itype, None))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        seen |= mine[d]
        assert np.array_equal(got[seen], rows_of[seen]) and np.isnan(got[~seen]).all()
    assert np.array_equal(seen, held)
    # both shards in one counted launch, the last one answering for the open end: zeros where nobody holds the id
    for prepared in (False, True):
        out = torch.full((B, dim), float("nan"), device=DEV)
        ctr.zero_()
        lo = (C.c_uint64 * N)(*[(d * per) | (pel.lib.EMB_RANGE_OPEN_END if d == N - 1 else 0) for d in range(N)])
        if prepared:
            plan = C.c_void_p()
            pel.lib.check(L.emb_plan_create_ranged_typed(eng._h, descs(out), lo, served, N, itype, C.byref(plan)))
            pel.lib.check(L.emb_plan_launch(plan, None))
            torch.cuda.synchronize()
            pel.lib.check(L.emb_plan_destroy(plan))
        else:
            pel.lib.check(L.emb_lookup_ranged_typed(eng._h, descs(out), lo, served, N, itype, None))
            torch.cuda.synchronize()
        want = np.where(held[:, None], rows_of, np.float32(0))
        assert np.array_equal(out.cpu().numpy(), want), prepared
        counts = ctr.cpu().numpy().astype(np.int64).sum(axis=1).tolist()
        assert counts == [int(m.sum()) for m in mine] and sum(counts) == B - len(nobody)      # the open end's bags are never counted
    eng.close()


# ---- hot rows in LDS -------------------------------------------------------------------------------------------------------
def test_hot_rows_change_no_bit(pel, oracle):
    rows, dim, B, Lp = 20000, 64, 1500, 32
    table, wide = bf16_table(rows, dim, 30)
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    eng.load_table(0, table.to(DEV))
    rng = np.random.default_rng(30)
    for _name, dt in ID_TYPES:
        eng.set_hot_rows(0, [])
        idx = pel.workloads.zipf_indices(rng, rows, B * Lp, 1.2, dtype=dt)
        off = pel.workloads.fixed_offsets(B, Lp, dtype=dt)
        want = oracle.c_bag_sum(wide, idx, off)
        d_idx, d_off = to_dev(idx), to_dev(off)
        before = eng.stats()["n_launches_by_kind"]
        cold = eng.lookup_batched([0], [d_idx], [d_off])[0].clone()
        torch.cuda.synchronize()
        assert kinds_delta(eng, before) == [0, 1, 0, 0, 0]
        eng.set_hot_rows(0, pel.workloads.top_rows(idx, 100))
        before = eng.stats()["n_launches_by_kind"]
        hot = eng.lookup_batched([0], [d_idx], [d_off])[0]
        torch.cuda.synchronize()
        assert kinds_delta(eng, before) == [0, 0, 0, 0, 1]
        assert torch.equal(cold, hot) and np.array_equal(hot.cpu().numpy(), want)
    eng.close()


# ---- pooled modes ----------------------------------------------------------------------------------------------------------
POOL_SHAPES = {16: (400, 16, 300, 9), 128: (300, 128, 150, 9), 18: (300, 18, 150, 9)}      # dim: rows, dim, bags, max entries


@pytest.fixture(scope="module")
def pooled_case():
    cases = {}
    for dim, (rows, _d, bags, max_len) in POOL_SHAPES.items():
        table, wide = bf16_table(rows, dim, 40 + dim)
        rng = np.random.default_rng(40 + dim)
        idx, off = ragged(rng, rows, bags, max_len, 0.2, np.int64)
        pad = 11
        idx[::5] = pad                                              # padding entries; some bags of padding only
        w = torch.randn(len(idx), generator=torch.Generator().manual_seed(dim)).numpy()
        refs = {"mean": pool_ref.embedding_bag(wide, idx, off, "mean"),
                "max": pool_ref.embedding_bag(wide, idx, off, "max"),
                "weighted": pool_ref.embedding_bag(wide, idx, off, "sum", w),
                "weighted+pad": pool_ref.embedding_bag(wide, idx, off, "sum", w, pad),
                "pad": pool_ref.embedding_bag(wide, idx, off, "sum", None, pad),
                "mean+pad": pool_ref.embedding_bag(wide, idx, off, "mean", None, pad),
                "max+pad": pool_ref.embedding_bag(wide, idx, off, "max", None, pad)}
        cases[dim] = (table, idx, off, w, pad, refs)
    return cases


@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("dim", list(POOL_SHAPES))
def test_pooled_modes(eng, pel, pooled_case, dim, ids):
    _name, dt = ids
    table, idx, off, w, pad, refs = pooled_case[dim]
    eng.load_table(8, table.to(DEV))
    i, o, wt = to_dev(idx.astype(dt)), to_dev(off.astype(dt)), torch.from_numpy(w).to(DEV)
    specs = {"mean": ("mean", None, None), "max": ("max", None, None), "weighted": ("sum", wt, None),
             "weighted+pad": ("sum", wt, pad), "pad": ("sum", None, pad), "mean+pad": ("mean", None, pad), "max+pad": ("max", None, pad)}
    names = list(specs)
    outs = eng.lookup_pooled([8] * len(names), [i] * len(names), [o] * len(names), [specs[n][0] for n in names],
                             per_sample_weights=[specs[n][1] for n in names], padding_idx=[specs[n][2] for n in names])
    torch.cuda.synchronize()
    for n, out in zip(names, outs):
        assert np.array_equal(out.cpu().numpy(), refs[n]), n
    # host memspace, and torch's CPU kernel agrees with the numpy restatement
    got = eng.lookup_pooled([8], [idx.astype(dt)], [off.astype(dt)], "sum", per_sample_weights=[w], padding_idx=pad)[0]
    assert np.array_equal(got, refs["weighted+pad"])
    want = F.embedding_bag(torch.from_numpy(idx), table.float(), torch.from_numpy(off), mode="mean", padding_idx=pad)
    assert torch.equal(outs[names.index("mean+pad")].cpu(), want)


def test_pooled_one_hot_wavebatch(eng, pel):
    """The pooled wave-batch kernel: weighted one-hot bags (DLRM's weighted pooling on Criteo shapes)."""
    rows, dim, B = 3000, 32, 131072 + 5
    table, wide = bf16_table(rows, dim, 50)
    eng.load_table(9, table.to(DEV))
    rng = np.random.default_rng(50)
    idx = rng.integers(0, rows, size=B)
    w = rng.standard_normal(B).astype(np.float32)
    i, o, wt = to_dev(idx), to_dev(np.arange(B)), torch.from_numpy(w).to(DEV)
    plan = eng.plan_pooled([9], [i], [o], "sum", per_sample_weights=[wt])
    assert [(r["kind"], r["dtype"]) for r in plan.describe()] == [(0, pel.EMB_BF16)]
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = pool_ref.fma32(w[:, None], wide[idx], np.zeros((B, dim), np.float32))
    assert np.array_equal(plan.outputs[0].cpu().numpy(), want)
    plan.destroy()


# ---- the request queue -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["host", "device"])
def test_request_queue(pel, oracle, space):
    rng = np.random.default_rng(60)
    tabs = [bf16_table(n, 16, 60 + t) for t, n in enumerate([1460, 583, 40000, 24])]
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    for t, (tab, _w) in enumerate(tabs):
        eng.load_table(t, tab)
    ids = list(range(len(tabs)))
    for itype, dt in ((pel.EMB_IDX_U32, np.uint32), (pel.EMB_IDX_I64, np.int64)):
        q = pel.RequestQueue(eng, itype, pel.EMB_MEM_HOST if space == "host" else pel.EMB_MEM_DEVICE)
        reqs = []
        for B in [1, 1, 32, 5, 1, 32, 2, 17]:                       # R = 8 small requests
            idx, off = zip(*[ragged(rng, tab.shape[0], B, 3, 0.2 if B > 1 else 0.0, dt) for tab, _w in tabs])
            outs = [np.full((B, 16), 7.0, np.float32) for _ in tabs]
            if space == "device":
                outs = [torch.from_numpy(a).to(DEV) for a in outs]
                reqs.append((q.add(ids, [to_dev(a) for a in idx], [to_dev(a) for a in off], outs), idx, off, outs))
            else:
                reqs.append((q.add(ids, list(idx), list(off), outs), idx, off, outs))
        launches = eng.stats()["n_kernel_launches"]
        assert q.flush() == 8
        for ticket, _idx, _off, _outs in reqs:
            q.wait(ticket)
        torch.cuda.synchronize()
        assert eng.stats()["n_kernel_launches"] - launches == 1       # fused: ONE launch
        for _ticket, idx, off, outs in reqs:                          # ... equal to the same requests one by one, and to the oracle
            alone = eng.lookup_batched(ids, list(idx), list(off))
            for t, (_tab, wide) in enumerate(tabs):
                got = outs[t].cpu().numpy() if space == "device" else outs[t]
                assert np.array_equal(got, alone[t])
                assert np.array_equal(got, oracle.c_bag_sum(wide, idx[t], off[t]))
        q.close()
    eng.close()


# ---- sharded, a world of one rank, every placement -------------------------------------------------------------------------
@pytest.mark.parametrize("pooling", ["one", "several"])
@pytest.mark.parametrize("check", [True, False])
def test_sharded_world1_every_placement(pel, oracle, pooling, check):
    sh = import_module("pim-embedding-lookup_amd.sharding")
    rows, dim, B = [7, 300, 5000, 64, 2000, 900], 16, 37
    kinds = [sh.REPLICATED, sh.WHOLE, sh.ROW_SPLIT, sh.REPLICATED, sh.ROW_SPLIT, sh.WHOLE]
    units = [sh.Unit(t, -1 if k == sh.REPLICATED else 0, 0, rows[t], t) for t, k in enumerate(kinds)]
    plan = sh.ShardPlan(1, rows, dim, 2, kinds, units, [[t] for t in range(len(rows))])
    tabs = [bf16_table(n, dim, 70 + t) for t, n in enumerate(rows)]
    eng = pel.EmbeddingEngine(device=0, max_tables=len(units) + 1)
    S = sh.ShardedEmbeddingBags(plan, eng, 0, None, depth=0, check=check)
    S.load_tables(lambda t, lo, hi: tabs[t][0][lo:hi].contiguous().to(DEV))
    assert all(eng.table_info(u.uid)[3] == pel.EMB_BF16 for u in units)
    rng = np.random.default_rng(70)
    for batch in range(2):
        if pooling == "one":
            idx = [rng.integers(0, n, size=B) for n in rows]
            off = [np.arange(B, dtype=np.int64) for _ in rows]
            outs = S.forward(None, [to_dev(i) for i in idx], fixed_pooling=1)
        else:
            idx, off = zip(*[ragged(rng, n, B, 5, 0.2, np.int64) for n in rows])
            outs = S.forward([to_dev(o) for o in off], [to_dev(i) for i in idx])
        torch.cuda.synchronize()
        for t in range(len(rows)):
            assert np.array_equal(outs[t].cpu().numpy(), oracle.c_bag_sum(tabs[t][1], idx[t], off[t])), (batch, t, kinds[t])
    S.report()
    S.close()
    eng.close()


# ---- the torch modules -----------------------------------------------------------------------------------------------------
def test_torch_modules(pel):
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    eng = pel.EmbeddingEngine(device=0, max_tables=32)
    torch.manual_seed(80)
    idx = torch.randint(0, 200, (500,))
    off = torch.tensor([0, 0, 7, 40, 41, 300])

    def ref_out(weight_bf16, mode, pad=None, psw=None):
        return F.embedding_bag(idx, weight_bf16.float().cpu(), off, mode=mode, padding_idx=pad, per_sample_weights=psw)

    # EmbeddingBag: constructor, from_pretrained, from_torch; state_dict round trip
    w = torch.randn(200, 24)
    mods = [tm.EmbeddingBag(200, 24, _weight=w, dtype=torch.bfloat16, engine=eng, table_id=0),
            tm.EmbeddingBag.from_pretrained(w, dtype=torch.bfloat16, engine=eng, table_id=1),
            tm.EmbeddingBag.from_torch(torch.nn.EmbeddingBag(200, 24, mode="sum", _weight=w.clone()), dtype=torch.bfloat16, engine=eng, table_id=2),
            tm.EmbeddingBag(200, 24, dtype=torch.bfloat16, engine=eng, table_id=3)]          # its own random init
    for m in mods:
        assert m.weight.dtype is torch.bfloat16
        if m is not mods[3]:
            assert torch.equal(m.weight.cpu(), w.to(torch.bfloat16))
        out = m(idx.to(DEV), off.to(DEV))
        assert out.dtype is torch.float32 and torch.equal(out.cpu(), ref_out(m.weight, "sum"))
    sd = mods[3].state_dict()
    assert list(sd) == ["weight"] and sd["weight"].dtype is torch.bfloat16
    fresh = tm.EmbeddingBag(200, 24, dtype=torch.bfloat16, engine=eng, table_id=4)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.weight, mods[3].weight)
    assert torch.equal(fresh(idx.to(DEV), off.to(DEV)), mods[3](idx.to(DEV), off.to(DEV)))

    # PoolingEmbeddingBag: the pooled modes, padding, weights
    psw = torch.randn(500)
    for k, (mode, pad, weighted) in enumerate([("mean", 3, False), ("max", None, False), ("sum", None, True), ("sum", 4, True), ("sum", 4, False)]):
        m = tm.PoolingEmbeddingBag(200, 24, mode=mode, padding_idx=pad, _weight=w, dtype=torch.bfloat16, engine=eng, table_id=5 + k)
        assert m.weight.dtype is torch.bfloat16
        x = idx.clone()
        if pad is not None:
            x[::5] = pad
        got = m(x.to(DEV), off.to(DEV), per_sample_weights=psw.to(DEV) if weighted else None)
        want = F.embedding_bag(x, m.weight.float().cpu(), off, mode=mode, padding_idx=pad, per_sample_weights=psw if weighted else None)
        assert torch.equal(got.cpu(), want), (mode, pad, weighted)
        other = tm.PoolingEmbeddingBag(200, 24, mode=mode, padding_idx=pad, dtype=torch.bfloat16, engine=eng, table_id=20)
        other.load_state_dict(m.state_dict())
        assert other.weight.dtype is torch.bfloat16
        assert torch.equal(other(x.to(DEV), off.to(DEV), per_sample_weights=psw.to(DEV) if weighted else None), got)
    m = tm.PoolingEmbeddingBag.from_torch(torch.nn.EmbeddingBag(200, 24, mode="max", _weight=w.clone()), dtype=torch.bfloat16, engine=eng, table_id=10)
    assert torch.equal(m(idx.to(DEV), off.to(DEV)).cpu(), ref_out(m.weight, "max"))
    m = tm.PoolingEmbeddingBag.from_pretrained(w, mode="mean", dtype=torch.bfloat16, engine=eng, table_id=11)
    assert torch.equal(m(idx.to(DEV), off.to(DEV)).cpu(), ref_out(m.weight, "mean"))

    # the fused collections
    refs = [torch.nn.EmbeddingBag(300, 16, mode="sum"), torch.nn.EmbeddingBag(50, 16, mode="sum"), torch.nn.EmbeddingBag(80, 32, mode="sum")]
    fused = tm.FusedEmbeddingBags([tm.EmbeddingBag.from_torch(r, dtype=torch.bfloat16, engine=eng, table_id=12 + k) for k, r in enumerate(refs)])
    lS_i = [torch.randint(0, r.num_embeddings, (400,)) for r in refs]
    lS_o = [torch.sort(torch.randint(0, 400, (64,))).values for _ in refs]
    for o in lS_o:
        o[0] = 0
    got = fused([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i])
    for k, r in enumerate(refs):
        assert fused.bags[k].weight.dtype is torch.bfloat16
        want = F.embedding_bag(lS_i[k], r.weight.detach().to(torch.bfloat16).float(), lS_o[k], mode="sum")
        assert torch.equal(got[k].cpu(), want), k
    sd = fused.state_dict()
    assert all(v.dtype is torch.bfloat16 for v in sd.values())
    again = tm.FusedEmbeddingBags([tm.EmbeddingBag(r.num_embeddings, r.embedding_dim, dtype=torch.bfloat16, engine=eng, table_id=15 + k)
                                   for k, r in enumerate(refs)])
    again.load_state_dict(sd)
    for a, b in zip(again([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i]), got):
        assert torch.equal(a, b)
    prefs = [torch.nn.EmbeddingBag(300, 16, mode="sum"), torch.nn.EmbeddingBag(50, 16, mode="mean", padding_idx=2), torch.nn.EmbeddingBag(80, 32, mode="max")]
    pfused = tm.FusedPoolingEmbeddingBags([tm.PoolingEmbeddingBag.from_torch(r, dtype=torch.bfloat16, engine=eng, table_id=21 + k)
                                           for k, r in enumerate(prefs)])
    lS_w = [torch.randn(400), None, None]
    got = pfused([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i], [None if x is None else x.to(DEV) for x in lS_w])
    for k, r in enumerate(prefs):
        want = F.embedding_bag(lS_i[k], r.weight.detach().to(torch.bfloat16).float(), lS_o[k], mode=r.mode, padding_idx=r.padding_idx,
                               per_sample_weights=lS_w[k])
        assert torch.equal(got[k].cpu(), want), k
    psd = pfused.state_dict()
    assert all(v.dtype is torch.bfloat16 for v in psd.values())
    pagain = tm.FusedPoolingEmbeddingBags([tm.PoolingEmbeddingBag(r.num_embeddings, r.embedding_dim, mode=r.mode, padding_idx=r.padding_idx,
                                                                  dtype=torch.bfloat16, engine=eng, table_id=24 + k) for k, r in enumerate(prefs)])
    pagain.load_state_dict(psd)
    for a, b in zip(pagain([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i], [None if x is None else x.to(DEV) for x in lS_w]), got):
        assert torch.equal(a, b)
    eng.close()


# ---- the DLRM harness ------------------------------------------------------------------------------------------------------
def test_harness_collection(pel):
    hz = import_module("pim-embedding-lookup_amd.dlrm_harness")
    rng = np.random.default_rng(90)
    ln = [300, 1000, 50]
    weights = [rng.standard_normal((n, 16)).astype(np.float32) for n in ln]
    ebc = hz.EmbeddingBagCollection(ln, 16, weights=weights, dtype="bf16")
    assert all(ebc.engine.table_info(k)[3] == pel.EMB_BF16 for k in range(len(ln)))
    lS_i = [torch.as_tensor(rng.integers(0, n, 200)) for n in ln]
    lS_o = [torch.as_tensor(np.sort(rng.integers(0, 200, 32))) for _ in ln]
    for o in lS_o:
        o[0] = 0
    ly = ebc.apply_emb([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i])
    torch.cuda.synchronize()
    for k in range(len(ln)):
        want = F.embedding_bag(lS_i[k], torch.from_numpy(weights[k]).to(torch.bfloat16).float(), lS_o[k], mode="sum")
        assert torch.equal(ly[k].cpu(), want), k
    ebc.close()
    with pytest.raises(ValueError):
        hz.EmbeddingBagCollection([10], 16, dtype="f8")


# ---- one batched call over fp32, fp16 and bf16 tables: one launch group per dtype ----------------------------------------------
def test_mixed_dtypes_in_one_call(pel, oracle):
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    rows, dim, B = 2000, 32, 500
    g = torch.Generator().manual_seed(95)
    src = [torch.randn((rows, dim), generator=g) for _ in range(4)]
    tabs = [src[0], src[1].to(torch.float16), src[2].to(torch.bfloat16), src[3].to(torch.bfloat16)]
    for t, w in enumerate(tabs):
        eng.load_table(t, w.to(DEV))
    rng = np.random.default_rng(95)
    order = [2, 0, 3, 1, 2]                                         # (a table twice, dtypes interleaved)
    idx, off = zip(*[ragged(rng, rows, B, 6, 0.2, np.int64) for _ in order])
    d_idx, d_off = [to_dev(i) for i in idx], [to_dev(o) for o in off]
    launches = eng.stats()["n_kernel_launches"]
    outs = eng.lookup_batched(order, d_idx, d_off)
    torch.cuda.synchronize()
    assert eng.stats()["n_kernel_launches"] - launches == 3
    plan = eng.plan(order, d_idx, d_off)
    assert sorted(r["dtype"] for r in plan.describe()) == [pel.EMB_F32, pel.EMB_F16, pel.EMB_BF16]
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, t in enumerate(order):
        want = oracle.c_bag_sum(tabs[t].float().numpy(), idx[k], off[k])
        assert np.array_equal(outs[k].cpu().numpy(), want), (k, t)
        assert np.array_equal(plan.outputs[k].cpu().numpy(), want), (k, t)
    plan.destroy()
    eng.close()
