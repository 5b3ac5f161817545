"""GPU: FP8 tables (EMB_F8_E4M3 = OCP e4m3fn, EMB_F8_E5M2 = OCP e5m2) through every lookup path, bit for bit.  An fp8 row widens
to fp32 exactly, so the reference is the fp32 reference on `table.float()` (torch's CPU conversion): the oracle's sequential
sum, tests/pool_ref.py / torch's CPU F.embedding_bag for the pooled modes and the modules.  Every comparison is np.array_equal /
torch.equal -- no tolerance.  (The big one-hot launches compare on the device against rows gathered by index from the
CPU-widened table: a one-index bag's pooled row IS the table row, no arithmetic is involved in the reference.)"""
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
F8 = [("e4m3", torch.float8_e4m3fn, 8), ("e5m2", torch.float8_e5m2, 9)]
F8_IDS = [k[0] for k in F8]
f8 = pytest.mark.parametrize("enc", F8, ids=F8_IDS)


def f8_table(rows, dim, seed, tdt):
    """(torch float8 CPU tensor, its exact fp32 widening as numpy).  randn rounds into the normal and subnormal range of either
    encoding, never to NaN."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn((rows, dim), generator=g).to(tdt)
    return t, t.float().numpy()


def bits_of(t):
    """A float8 tensor's bytes as a numpy uint8 array (what load_table takes with dtype=EMB_F8_*)."""
    return t.contiguous().view(torch.uint8).cpu().numpy()


def to_dev(a):
    """numpy ids -> CUDA tensor (uint32 bits travel as int32)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def ragged(rng, rows, bags, max_len, p_empty, dt, min_len=1):
    lens = rng.integers(min_len, max_len + 1, size=bags)
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


# ---- all 256 bit patterns: the test of the widening itself (subnormals, +-0, e5m2 +-inf, the largest finite values) ----------
@f8
def test_every_bit_pattern(eng, pel, oracle, enc):
    _name, tdt, dt = enc
    formats = import_module("pim-embedding-lookup_amd.formats")
    wide_row = torch.arange(256, dtype=torch.uint8).view(tdt).float().numpy()            # torch's CPU widening of every byte
    assert np.array_equal(np.isnan(wide_row), np.isnan(formats.from_f8_bits(np.arange(256, dtype=np.uint8), dt)))
    ok = np.flatnonzero(~np.isnan(wide_row))
    assert len(ok) == (254 if dt == 8 else 250)
    if dt == 9:
        assert np.isinf(wide_row[ok]).sum() == 2                                           # +-inf are values like any other
    for dim, kind in ((16, 1), (10, 3), (36, 3)):                                          # tuned path; any-dim by element; by 16-byte piece
        bits = np.repeat(np.arange(256, dtype=np.uint8)[:, None], dim, axis=1)             # row r is filled with byte r
        wide = np.repeat(wide_row[:, None], dim, axis=1)
        eng.load_table(0, bits, dtype=dt)                                                  # numpy: uint8 bits, declared
        assert np.array_equal(bits_of(eng.table_tensor(0)), bits)
        for _n, it in ID_TYPES:
            idx, off = ok.astype(it), np.arange(len(ok)).astype(it)
            want = oracle.c_bag_sum(wide, idx, off)                                        # (a sum starts at +0: the -0 row comes back as +0)
            assert np.array_equal(want, wide[ok]) and not np.signbit(want[want == 0]).any()
            plan = eng.plan([0], [to_dev(idx)], [to_dev(off)])
            rec = plan.describe()[0]
            assert rec["kind"] == kind and rec["dtype"] == dt and (kind != 3 or rec["anydim_vec"] == int(dim == 36))
            plan.launch(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = plan.outputs[0].cpu().numpy()
            plan.destroy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dim, _n)    # bit for bit
            # pooled "max" keeps a row as it is, -0 included: the pooled kernels see the same widening
            got = eng.lookup_pooled([0], [to_dev(idx)], [to_dev(off)], "max")[0]
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.uint32), wide[ok].view(np.uint32)), (dim, _n)
        if dim == 16:      # ... and through the wave-batch kernel's one-hot step: 530 x the valid rows (>= 131 072 bags)
            many = np.tile(ok.astype(np.int64), 530)
            before = eng.stats()["n_launches_by_kind"]
            got = eng.lookup_batched([0], [to_dev(many)], [to_dev(np.arange(len(many)))])[0]
            torch.cuda.synchronize()
            assert kinds_delta(eng, before) == [1, 0, 0, 0, 0]
            assert np.array_equal(got.cpu().numpy().view(np.uint32), np.tile(want, (530, 1)).view(np.uint32))


# ---- each kernel kind at the smallest shape that selects it (choose_kernel) --------------------------------------------------
@f8
@pytest.mark.parametrize("dim", [64, 128, 1024])       # 4 lanes per row; 8 (the wide-row store path); 64
def test_wavebatch_one_hot_kind0(eng, pel, enc, dim):
    _name, tdt, dt = enc
    rows, B = 5000, 131072 + 1
    table, wide = f8_table(rows, dim, 11 + dim, tdt)
    eng.load_table(4, table.to(DEV))
    wide_dev = torch.from_numpy(wide).to(DEV)
    rng = np.random.default_rng(11)
    for _n, it in ID_TYPES:
        idx = rng.integers(0, rows, size=B)
        d_idx, d_off = to_dev(idx.astype(it)), to_dev(np.arange(B).astype(it))
        before = eng.stats()["n_launches_by_kind"]
        got = eng.lookup_batched([4], [d_idx], [d_off])[0]
        torch.cuda.synchronize()
        assert kinds_delta(eng, before) == [1, 0, 0, 0, 0]
        assert torch.equal(got, wide_dev[torch.from_numpy(idx).to(DEV)])
        assert np.array_equal(got[-3:].cpu().numpy(), wide[idx[-3:]])                      # (the odd tail bag, against the host copy)
        del got


@f8
@pytest.mark.parametrize("dim", [16, 64])              # one lane per row; four
def test_wavebatch_two_batches_kind2(eng, pel, enc, dim):
    _name, tdt, dt = enc
    rows, B = 5000, 524288 + 1
    table, wide = f8_table(rows, dim, 12 + dim, tdt)
    eng.load_table(5, table.to(DEV))
    wide_dev = torch.from_numpy(wide).to(DEV)
    rng = np.random.default_rng(12)
    for _n, it in ID_TYPES:
        idx = rng.integers(0, rows, size=B)
        d_idx, d_off = to_dev(idx.astype(it)), to_dev(np.arange(B).astype(it))
        plan = eng.plan([5], [d_idx], [d_off])
        assert [(r["kind"], r["dtype"]) for r in plan.describe()] == [(2, dt)]
        plan.destroy()
        before = eng.stats()["n_launches_by_kind"]
        got = eng.lookup_batched([5], [d_idx], [d_off])[0]
        torch.cuda.synchronize()
        assert kinds_delta(eng, before) == [0, 0, 1, 0, 0]
        assert torch.equal(got, wide_dev[torch.from_numpy(idx).to(DEV)])
        assert np.array_equal(got[-3:].cpu().numpy(), wide[idx[-3:]])
        del got


@f8
@pytest.mark.parametrize("dim", [16, 48, 128, 272])    # 1 lane; 3 pieces in 4 lanes; 8 lanes; 17 pieces in 32 lanes
def test_lane_group_ragged_kind1(eng, pel, oracle, enc, dim):
    _name, tdt, dt = enc
    rows, bags = 3001, 777
    table, wide = f8_table(rows, dim, 13 + dim, tdt)
    eng.load_table(6, table)                                                               # a torch CPU tensor
    assert eng.table_info(6)[1:] == (rows, dim, dt)
    rng = np.random.default_rng(dim)
    for _n, it in ID_TYPES:
        idx, off = ragged(rng, rows, bags, 9, 0.2, it, min_len=0)                          # 0-9 indices, empty bags
        want = oracle.c_bag_sum(wide, idx, off)
        before = eng.stats()["n_launches_by_kind"]
        got = eng.lookup_batched([6], [to_dev(idx)], [to_dev(off)])[0]
        torch.cuda.synchronize()
        assert kinds_delta(eng, before) == [0, 1, 0, 0, 0]
        assert np.array_equal(got.cpu().numpy(), want)


@f8
def test_hot_rows_change_no_bit(pel, oracle, enc):
    _name, tdt, dt = enc
    rows, dim, B, Lp = 20000, 64, 1500, 32
    table, wide = f8_table(rows, dim, 30, tdt)
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    eng.load_table(0, table.to(DEV))
    rng = np.random.default_rng(30)
    for _n, it in ID_TYPES:
        eng.set_hot_rows(0, [])
        idx = pel.workloads.zipf_indices(rng, rows, B * Lp, 1.2, dtype=it)
        off = pel.workloads.fixed_offsets(B, Lp, dtype=it)
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
    n, share = eng.learn_hot_rows(0, d_idx, max_rows=64, min_share=0.01)                   # the engine's own pick stages 1-byte rows too
    assert n > 0
    again = eng.lookup_batched([0], [d_idx], [d_off])[0]
    torch.cuda.synchronize()
    assert torch.equal(again, cold)
    eng.close()


# ---- host, device and plan calls over the row shapes; plan bytes and text ----------------------------------------------------
@f8
@pytest.mark.parametrize("dim", [16, 32, 48, 1024, 1040, 36, 10, 3])
def test_host_device_and_plan_calls(eng, pel, oracle, enc, dim):
    _name, tdt, dt = enc
    rows, bags = 2003, 333
    table, wide = f8_table(rows, dim, 100 + dim, tdt)
    rng = np.random.default_rng(dim * 7)
    for name, it in ID_TYPES:
        if it is np.uint32:
            eng.load_table(7, bits_of(table), dtype=dt)                                    # numpy: uint8 bits, declared
        else:
            eng.load_table(7, table.to(DEV))
        view = eng.table_tensor(7)
        assert view.dtype is tdt and tuple(view.shape) == (rows, dim) and np.array_equal(bits_of(view), bits_of(table))
        idx, off = ragged(rng, rows, bags, 40, 0.2, it)
        want = oracle.c_bag_sum(wide, idx, off)
        got = eng.lookup_batched([7], [idx], [off])[0]                                     # host arrays
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
        d_idx, d_off = to_dev(idx), to_dev(off)
        got = eng.lookup_batched([7], [d_idx], [d_off])[0]                                 # device tensors
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)
        plan = eng.plan([7], [d_idx], [d_off])                                             # a prepared plan
        recs = plan.describe()
        anydim = dim % 16 != 0 or dim > 1024                                               # 1 byte per element: row bytes == dim
        assert len(recs) == 1 and recs[0]["dtype"] == dt and recs[0]["kind"] == (3 if anydim else 1)
        if anydim:
            assert recs[0]["anydim_vec"] == int(dim % 4 == 0 and dim >= 32)
        else:
            lpr = 1
            while lpr < dim // 16:
                lpr *= 2
            assert recs[0]["lanes_per_row"] == lpr and recs[0]["chunks"] == dim // 16
        assert plan.bytes()[0] == len(idx) * (dim + idx.itemsize) + bags * idx.itemsize + bags * dim * 4      # 1 byte per gathered element
        plan.outputs[0].fill_(7.0)
        plan.launch(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(plan.outputs[0].cpu().numpy(), want)
        plan.destroy()


def test_signature_differs_by_dtype(eng, pel):
    """The same shape as e4m3, e5m2 and (at twice the dim in bytes) nothing else: three plans, three signatures."""
    rows, dim, B = 500, 32, 64
    idx, off = to_dev(np.arange(B, dtype=np.int64)), to_dev(np.arange(B, dtype=np.int64))
    sigs = []
    for t, tdt in ((8, torch.float8_e4m3fn), (9, torch.float8_e5m2), (10, torch.bfloat16), (11, torch.float32)):
        eng.load_table(t, torch.zeros((rows, dim)).to(tdt))
        plan = eng.plan([t], [idx], [off])
        sigs.append(plan.signature())
        plan.destroy()
    assert len(set(sigs)) == 4


# ---- ranged, counted and open-end lookups ------------------------------------------------------------------------------------
@f8
@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("dim", [16, 128])
def test_ranged_counted_open_end(pel, enc, dim, ids):
    _name, tdt, dtv = enc
    _n, dt = ids
    rows, N, B = 5003, 2, 4001
    table, wide = f8_table(rows, dim, 20 + dim, tdt)
    per = -(-rows // N)
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    for d in range(N):
        eng.load_table(d, table[d * per:min((d + 1) * per, rows)].contiguous())
        assert eng.table_info(d)[3] == dtv
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

    # one shard at a time, a non-zero row_lo, no open end: only its own bags are written, every other bag stays as it was
    out = torch.full((B, dim), float("nan"), device=DEV)
    seen = np.zeros(B, bool)
    for d in reversed(range(N)):
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


# ---- pooled modes: kinds 1 (lane group) and 3 (any-dim, by piece and by element); kind 0 below ---------------------------------
POOL_SHAPES = {16: (400, 300, 9), 128: (300, 150, 9), 36: (300, 150, 9), 10: (300, 150, 9)}      # dim: rows, bags, max entries
POOL_KIND = {16: 1, 128: 1, 36: 3, 10: 3}


@pytest.fixture(scope="module")
def pooled_case():
    cases = {}
    for _name, tdt, dt in F8:
        for dim, (rows, bags, max_len) in POOL_SHAPES.items():
            table, wide = f8_table(rows, dim, 40 + dim, tdt)
            rng = np.random.default_rng(40 + dim)
            idx, off = ragged(rng, rows, bags, max_len, 0.2, np.int64)
            pad = 11
            idx[::5] = pad                                              # padding entries; some bags of padding only
            w = torch.randn(len(idx), generator=torch.Generator().manual_seed(dim)).numpy()
            ti, to, tw, tf = torch.from_numpy(idx), torch.from_numpy(off), torch.from_numpy(w), table.float()
            refs = {"mean": F.embedding_bag(ti, tf, to, mode="mean"),                      # torch's CPU kernel over W.float()
                    "max": F.embedding_bag(ti, tf, to, mode="max"),
                    "weighted": F.embedding_bag(ti, tf, to, mode="sum", per_sample_weights=tw),
                    "weighted+pad": F.embedding_bag(ti, tf, to, mode="sum", per_sample_weights=tw, padding_idx=pad),
                    "pad": F.embedding_bag(ti, tf, to, mode="sum", padding_idx=pad),
                    "mean+pad": F.embedding_bag(ti, tf, to, mode="mean", padding_idx=pad),
                    "max+pad": F.embedding_bag(ti, tf, to, mode="max", padding_idx=pad)}
            refs = {k: v.numpy() for k, v in refs.items()}
            assert np.array_equal(refs["weighted+pad"], pool_ref.embedding_bag(wide, idx, off, "sum", w, pad))      # (and the numpy restatement)
            cases[(dt, dim)] = (table, idx, off, w, pad, refs)
    return cases


@f8
@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("dim", list(POOL_SHAPES))
def test_pooled_modes(eng, pel, pooled_case, enc, dim, ids):
    _name, tdt, dtv = enc
    _n, dt = ids
    table, idx, off, w, pad, refs = pooled_case[(dtv, dim)]
    eng.load_table(12, table.to(DEV))
    i, o, wt = to_dev(idx.astype(dt)), to_dev(off.astype(dt)), torch.from_numpy(w).to(DEV)
    specs = {"mean": ("mean", None, None), "max": ("max", None, None), "weighted": ("sum", wt, None),
             "weighted+pad": ("sum", wt, pad), "pad": ("sum", None, pad), "mean+pad": ("mean", None, pad), "max+pad": ("max", None, pad)}
    names = list(specs)
    args = ([12] * len(names), [i] * len(names), [o] * len(names), [specs[n][0] for n in names])
    kw = dict(per_sample_weights=[specs[n][1] for n in names], padding_idx=[specs[n][2] for n in names])
    plan = eng.plan_pooled(*args, **kw)
    recs = plan.describe()
    assert all(r["dtype"] == dtv and r["kind"] == POOL_KIND[dim] and "pool" in r for r in recs), recs
    plan.destroy()
    outs = eng.lookup_pooled(*args, **kw)
    torch.cuda.synchronize()
    for n, out in zip(names, outs):
        assert out.dtype is torch.float32 and np.array_equal(out.cpu().numpy(), refs[n]), n
    # host memspace
    got = eng.lookup_pooled([12], [idx.astype(dt)], [off.astype(dt)], "sum", per_sample_weights=[w], padding_idx=pad)[0]
    assert np.array_equal(got, refs["weighted+pad"])


@f8
@pytest.mark.parametrize("dim", [32, 128])             # 2 lanes per row; 8 (the wide-row store path)
def test_pooled_one_hot_wavebatch_kind0(eng, pel, enc, dim):
    """The pooled wave-batch kernel: weighted one-hot bags (DLRM's weighted pooling on Criteo shapes)."""
    _name, tdt, dt = enc
    rows, B = 3000, 131072 + 5
    table, wide = f8_table(rows, dim, 50 + dim, tdt)
    eng.load_table(13, table.to(DEV))
    rng = np.random.default_rng(50)
    idx = rng.integers(0, rows, size=B)
    w = rng.standard_normal(B).astype(np.float32)
    i, o, wt = to_dev(idx), to_dev(np.arange(B)), torch.from_numpy(w).to(DEV)
    plan = eng.plan_pooled([13], [i], [o], "sum", per_sample_weights=[wt])
    assert [(r["kind"], r["dtype"]) for r in plan.describe()] == [(0, dt)]
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = F.embedding_bag(torch.from_numpy(idx), table.float(), torch.arange(B), mode="sum", per_sample_weights=torch.from_numpy(w))
    assert torch.equal(plan.outputs[0].cpu(), want)
    plan.destroy()


# ---- the request queue -------------------------------------------------------------------------------------------------------
@f8
@pytest.mark.parametrize("space", ["host", "device"])
def test_request_queue(pel, oracle, enc, space):
    _name, tdt, dtv = enc
    rng = np.random.default_rng(60)
    tabs = [f8_table(n, 16, 60 + t, tdt) for t, n in enumerate([1460, 583, 40000, 24])]
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
        for _ticket, idx, off, outs in reqs:
            for t, (_tab, wide) in enumerate(tabs):
                got = outs[t].cpu().numpy() if space == "device" else outs[t]
                assert np.array_equal(got, oracle.c_bag_sum(wide, idx[t], off[t]))
        q.close()
    eng.close()


# ---- sharded, a world of one rank, every placement (the exchange carries fp32 rows: multi-rank legs are blind to the dtype) ----
@f8
@pytest.mark.parametrize("pooling", ["one", "several"])
@pytest.mark.parametrize("check", [True, False])
def test_sharded_world1_every_placement(pel, oracle, enc, pooling, check):
    _name, tdt, dtv = enc
    sh = import_module("pim-embedding-lookup_amd.sharding")
    rows, dim, B = [7, 300, 5000, 64, 2000, 900], 16, 37
    kinds = [sh.REPLICATED, sh.WHOLE, sh.ROW_SPLIT, sh.REPLICATED, sh.ROW_SPLIT, sh.WHOLE]
    units = [sh.Unit(t, -1 if k == sh.REPLICATED else 0, 0, rows[t], t) for t, k in enumerate(kinds)]
    plan = sh.ShardPlan(1, rows, dim, 2, kinds, units, [[t] for t in range(len(rows))])
    tabs = [f8_table(n, dim, 70 + t, tdt) for t, n in enumerate(rows)]
    eng = pel.EmbeddingEngine(device=0, max_tables=len(units) + 1)
    S = sh.ShardedEmbeddingBags(plan, eng, 0, None, depth=0, check=check)
    S.load_tables(lambda t, lo, hi: tabs[t][0][lo:hi].contiguous().to(DEV))
    assert all(eng.table_info(u.uid)[3] == dtv for u in units)
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


# ---- the torch modules -------------------------------------------------------------------------------------------------------
def same(a, b):
    """float8 tensors compared by their bytes."""
    return a.dtype is b.dtype and torch.equal(a.contiguous().view(torch.uint8).cpu(), b.contiguous().view(torch.uint8).cpu())


@f8
def test_torch_modules(pel, enc):
    _name, tdt, dtv = enc
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    eng = pel.EmbeddingEngine(device=0, max_tables=32)
    torch.manual_seed(80)
    idx = torch.randint(0, 200, (500,))
    off = torch.tensor([0, 0, 7, 40, 41, 300])
    w = torch.randn(200, 48)
    w8 = w.to(tdt)                                                                        # rounded by torch on the CPU

    def ref_out(weight_f8, mode, pad=None, psw=None):
        return F.embedding_bag(idx, weight_f8.cpu().float(), off, mode=mode, padding_idx=pad, per_sample_weights=psw)

    mods = [tm.EmbeddingBag(200, 48, _weight=w8, dtype=tdt, engine=eng, table_id=0),       # a float8 weight
            tm.EmbeddingBag.from_pretrained(w8, dtype=tdt, engine=eng, table_id=1),
            tm.EmbeddingBag.from_torch(torch.nn.EmbeddingBag(200, 48, mode="sum", _weight=w8.float()), dtype=tdt, engine=eng, table_id=2)]
    for m in mods:
        assert m.weight.dtype is tdt and same(m.weight, w8)
        out = m(idx.to(DEV), off.to(DEV))
        assert out.dtype is torch.float32 and torch.equal(out.cpu(), ref_out(w8, "sum"))
    sd = mods[0].state_dict()
    assert list(sd) == ["weight"] and sd["weight"].dtype is tdt and same(sd["weight"], w8)
    fresh = tm.EmbeddingBag(200, 48, _weight=torch.zeros(200, 48), dtype=tdt, engine=eng, table_id=4)
    fresh.load_state_dict(sd)
    assert same(fresh.weight, w8)
    assert torch.equal(fresh(idx.to(DEV), off.to(DEV)), mods[0](idx.to(DEV), off.to(DEV)))
    with pytest.raises(ValueError):
        tm.EmbeddingBag(200, 48, _weight=w8, dtype=tdt, engine=eng, table_id=5, out_dtype="weight")      # no fp8 output

    psw = torch.randn(500)
    for k, (mode, pad, weighted) in enumerate([("mean", 3, False), ("max", None, False), ("sum", None, True), ("sum", 4, True)]):
        m = tm.PoolingEmbeddingBag(200, 48, mode=mode, padding_idx=pad, _weight=w8, dtype=tdt, engine=eng, table_id=6 + k)
        assert m.weight.dtype is tdt
        x = idx.clone()
        if pad is not None:
            x[::5] = pad
        got = m(x.to(DEV), off.to(DEV), per_sample_weights=psw.to(DEV) if weighted else None)
        want = F.embedding_bag(x, w8.float(), off, mode=mode, padding_idx=pad, per_sample_weights=psw if weighted else None)
        assert torch.equal(got.cpu(), want), (mode, pad, weighted)
        other = tm.PoolingEmbeddingBag(200, 48, mode=mode, padding_idx=pad, _weight=torch.zeros(200, 48), dtype=tdt, engine=eng, table_id=20)
        other.load_state_dict(m.state_dict())
        assert same(other.weight, w8)
        assert torch.equal(other(x.to(DEV), off.to(DEV), per_sample_weights=psw.to(DEV) if weighted else None), got)

    refs = [torch.nn.EmbeddingBag(300, 16, mode="sum"), torch.nn.EmbeddingBag(50, 16, mode="sum"), torch.nn.EmbeddingBag(80, 32, mode="sum")]
    w8s = [r.weight.detach().to(tdt) for r in refs]
    fused = tm.FusedEmbeddingBags([tm.EmbeddingBag(r.num_embeddings, r.embedding_dim, _weight=w8s[k], dtype=tdt, engine=eng, table_id=12 + k)
                                   for k, r in enumerate(refs)])
    lS_i = [torch.randint(0, r.num_embeddings, (400,)) for r in refs]
    lS_o = [torch.sort(torch.randint(0, 400, (64,))).values for _ in refs]
    for o in lS_o:
        o[0] = 0
    got = fused([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i])
    for k in range(len(refs)):
        assert torch.equal(got[k].cpu(), F.embedding_bag(lS_i[k], w8s[k].float(), lS_o[k], mode="sum")), k
    sd = fused.state_dict()
    assert all(v.dtype is tdt for v in sd.values())
    again = tm.FusedEmbeddingBags([tm.EmbeddingBag(r.num_embeddings, r.embedding_dim, _weight=torch.zeros_like(r.weight), dtype=tdt, engine=eng,
                                                   table_id=15 + k) for k, r in enumerate(refs)])
    again.load_state_dict(sd)
    for a, b in zip(again([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i]), got):
        assert torch.equal(a, b)
    eng.close()


# ---- the DLRM harness --------------------------------------------------------------------------------------------------------
def test_harness_collection(pel):
    hz = import_module("pim-embedding-lookup_amd.dlrm_harness")
    rng = np.random.default_rng(90)
    ln = [300, 1000, 50]
    weights = [rng.standard_normal((n, 16)).astype(np.float32) for n in ln]
    ebc = hz.EmbeddingBagCollection(ln, 16, weights=weights, dtype="fp8_e4m3")
    assert all(ebc.engine.table_info(k)[3] == pel.EMB_F8_E4M3 for k in range(len(ln)))
    lS_i = [torch.as_tensor(rng.integers(0, n, 200)) for n in ln]
    lS_o = [torch.as_tensor(np.sort(rng.integers(0, 200, 32))) for _ in ln]
    for o in lS_o:
        o[0] = 0
    ly = ebc.apply_emb([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i])
    torch.cuda.synchronize()
    for k in range(len(ln)):
        want = F.embedding_bag(lS_i[k], torch.from_numpy(weights[k]).to(torch.float8_e4m3fn).float(), lS_o[k], mode="sum")
        assert torch.equal(ly[k].cpu(), want), k
    ebc.close()
    ebc = hz.EmbeddingBagCollection([40], 16, weights=[weights[0][:40]], dtype="fp8_e5m2")
    assert ebc.engine.table_info(0)[3] == pel.EMB_F8_E5M2
    ebc.close()
    with pytest.raises(ValueError):
        hz.EmbeddingBagCollection([10], 16, dtype="fp8_e4m3", out_dtype="weight")


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(eng, pel):
    L = pel.lib.load()
    for bad in (4, 5, 6, 7, 10):
        with pytest.raises(pel.PimembError) as ex:
            eng.alloc_table(20, 100, 16, bad)                        # values 4-7 (and anything beyond 9) stay invalid
        assert ex.value.code == pel.lib.EMB_ERR_INVALID
    with pytest.raises(KeyError):
        eng.load_table(20, np.zeros((4, 16), np.uint8))              # uint8 without dtype=: refused
    for t, dt, tdt in ((21, 8, torch.float8_e4m3fn), (22, 9, torch.float8_e5m2)):
        eng.alloc_table(t, 100, 16, dt)                              # emb_alloc_table: zero rows
        assert eng.table_tensor(t).dtype is tdt and not bool(eng.table_tensor(t).view(torch.uint8).any())
        with pytest.raises(pel.PimembError):
            eng.load_table_column(t, 0, np.zeros(100, np.int32))     # columns stay fixed-point only
        # EMB_POOL_OUT_TABLE_DTYPE at the C ABI: unsupported (Python refuses earlier: tests/test_f8_cpu.py)
        idx = torch.arange(8, device=DEV)
        out = torch.zeros((8, 16), device=DEV)
        d = (pel.lib.EmbLookupDesc * 1)(pel.lib.EmbLookupDesc(t, 0, idx.data_ptr(), idx.data_ptr(), 8, 8, out.data_ptr()))
        for mode in (pel.lib.EMB_POOL_SUM, pel.lib.EMB_POOL_MEAN):
            ps = (pel.lib.EmbPoolSpec * 1)(pel.lib.EmbPoolSpec(mode, pel.lib.EMB_POOL_OUT_TABLE_DTYPE, None, 0))
            rc = L.emb_lookup_pooled(eng._h, d, ps, 1, pel.lib.EMB_IDX_I64, pel.lib.EMB_MEM_DEVICE, None, 0, None)
            assert rc == pel.lib.EMB_ERR_UNSUPPORTED
        with pytest.raises(TypeError):
            eng.lookup_batched([t], [idx], [idx], out_dtype="table")


# ---- one batched call over fp32, bf16 and both fp8 encodings: one launch group per dtype ----------------------------------------
def test_mixed_dtypes_in_one_call(pel, oracle):
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    rows, dim, B = 2000, 32, 500
    g = torch.Generator().manual_seed(95)
    src = [torch.randn((rows, dim), generator=g) for _ in range(4)]
    tabs = [src[0], src[1].to(torch.float8_e4m3fn), src[2].to(torch.bfloat16), src[3].to(torch.float8_e5m2)]
    for t, w in enumerate(tabs):
        eng.load_table(t, w.to(DEV))
    rng = np.random.default_rng(95)
    order = [3, 0, 1, 2, 3, 1]
    idx, off = zip(*[ragged(rng, rows, B, 6, 0.2, np.int64) for _ in order])
    d_idx, d_off = [to_dev(i) for i in idx], [to_dev(o) for o in off]
    launches = eng.stats()["n_kernel_launches"]
    outs = eng.lookup_batched(order, d_idx, d_off)
    torch.cuda.synchronize()
    assert eng.stats()["n_kernel_launches"] - launches == 4
    plan = eng.plan(order, d_idx, d_off)
    assert sorted(r["dtype"] for r in plan.describe()) == [pel.EMB_F32, pel.EMB_BF16, pel.EMB_F8_E4M3, pel.EMB_F8_E5M2]
    plan.destroy()
    for k, t in enumerate(order):
        assert np.array_equal(outs[k].cpu().numpy(), oracle.c_bag_sum(tabs[t].float().numpy(), idx[k], off[k])), (k, t)
    eng.close()
