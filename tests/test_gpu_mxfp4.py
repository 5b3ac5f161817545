"""GPU: MXFP4 tables (EMB_MXFP4) through the lane-group kernels, bit for bit.  An element's value e2m1 * 2^(s - 127) is an fp32
(formats.from_mxfp4), so the reference is the fp32 reference over the dequantised table: the oracle's sequential sum,
tests/pool_ref.py and torch's CPU F.embedding_bag for the pooled modes and the modules.  Every comparison is np.array_equal /
torch.equal on the bits -- no tolerance."""
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
formats = import_module("pim-embedding-lookup_amd.formats")


def to_dev(a):
    """numpy ids -> CUDA tensor (uint32 bits travel as int32)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mx_table(rng, rows, dim, s_lo=117, s_hi=137):
    """(fused rows uint8 [rows, stride], their dequantisation fp32 [rows, dim]): random nibbles, scale bytes uniform in
    s_lo ... s_hi so that sums of a few dozen rows stay finite."""
    el = rng.integers(0, 256, size=(rows, dim // 2), dtype=np.uint8)
    sc = rng.integers(s_lo, s_hi + 1, size=(rows, dim // 32), dtype=np.uint8)
    fused = formats.mxfp4_join(el, sc)
    return fused, formats.from_mxfp4(fused, dim)


def ragged(rng, rows, bags, max_len, dt, trailing_empty=3):
    """Bags of 0 ... max_len indices with empty bags, trailing empty bags and duplicates inside a bag."""
    lens = rng.integers(0, max_len + 1, size=bags)
    lens[rng.random(bags) < 0.1] = 0
    lens[bags - trailing_empty:] = 0
    off = np.zeros(bags, np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    idx = rng.integers(0, rows, size=int(lens.sum()))
    idx[1::7] = idx[0::7][:len(idx[1::7])]                                    # duplicates
    return idx.astype(dt), off.astype(dt)


def lpr_of(dim):
    lpr = 1
    while lpr < dim // 32:
        lpr *= 2
    return lpr


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


# ---- every bit pattern: 16 nibbles x 256 scale bytes.  Decides what v_cvt_scalef32_pk_f32_fp4 does with its scale operand (the
# exponent field alone: s = 0 is 2^-127), with results that are fp32 denormals (s <= 2), and its nibble order within a byte ------
@pytest.mark.parametrize("dim", [32, 256])                 # one lane per row; the same bytes tiled over 8 lanes
def test_every_bit_pattern(eng, pel, oracle, dim):
    blocks = dim // 32
    el = np.tile(np.array([(2 * j + 1) % 16 << 4 | (2 * j) % 16 for j in range(16)], np.uint8), (256, blocks))      # nibbles 0 ... 15 twice
    fused = formats.mxfp4_join(el, np.repeat(np.arange(256, dtype=np.uint8)[:, None], blocks, axis=1))              # row r: scale byte r
    wide = formats.from_mxfp4(fused, dim)
    assert np.isnan(wide[255]).all() and not np.isnan(wide[:255]).any()
    assert np.array_equal(bits(wide[0, :8]), bits(np.float32([0, 2.0 ** -128, 2.0 ** -127, 1.5 * 2.0 ** -127, 2.0 ** -126, 1.5 * 2.0 ** -126, 2.0 ** -125, 1.5 * 2.0 ** -125])))
    eng.load_table(0, fused, dtype=pel.EMB_MXFP4)
    assert np.array_equal(eng.table_tensor(0).cpu().numpy(), fused)
    assert eng.table_info(0)[1:] == (256, dim, pel.EMB_MXFP4)
    for _n, it in ID_TYPES:
        idx, off = np.arange(256).astype(it), np.arange(256).astype(it)
        want = oracle.c_bag_sum(wide[:255], idx[:255], off[:255])            # (a sum starts at +0: a -0 element comes back as +0)
        got = eng.lookup_batched([0], [to_dev(idx)], [to_dev(off)])[0]       # a direct call ...
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert np.array_equal(bits(got[:255]), bits(want)), (dim, _n)
        assert np.isnan(got[255]).all()
        plan = eng.plan([0], [to_dev(idx)], [to_dev(off)])                   # ... and a plan
        rec = plan.describe()[0]
        assert (rec["kind"], rec["dtype"], rec["lanes_per_row"], rec["chunks"]) == (1, pel.EMB_MXFP4, lpr_of(dim), blocks)
        plan.launch(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = plan.outputs[0].cpu().numpy()
        plan.destroy()
        assert np.array_equal(bits(got[:255]), bits(want)) and np.isnan(got[255]).all(), (dim, _n)
        # pooled "max" keeps a row as it is, -0 included: the pooled kernel sees the same widening
        got = eng.lookup_pooled([0], [to_dev(idx[:255])], [to_dev(off[:255])], "max")[0]
        torch.cuda.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(wide[:255])), (dim, _n)


# ---- ragged parity over the row widths ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_case():
    """dim -> (fused rows, dequantised rows); the references are computed per test from these and never changed."""
    rng = np.random.default_rng(410)
    return {dim: mx_table(rng, 1000, dim) for dim in (32, 64, 96, 128, 512, 2048)}


@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("dim", [32, 64, 96, 128, 512, 2048])      # 1, 2, 3 (of 4: one dead lane), 4, 16, 64 lanes per row
def test_ragged_parity(eng, pel, oracle, ragged_case, dim, ids):
    _n, it = ids
    fused, wide = ragged_case[dim]
    rows, bags = 1000, 200
    eng.load_table(1, torch.from_numpy(fused).to(DEV), dtype=pel.EMB_MXFP4)
    rng = np.random.default_rng(dim)
    idx, off = ragged(rng, rows, bags, 40, it)
    want = oracle.c_bag_sum(wide, idx, off)
    assert np.isfinite(want).all() and not want[-3:].any() and want.any()
    got = eng.lookup_batched([1], [idx], [off])[0]                             # host arrays, offsets
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(want))
    got = eng.lookup_batched([1], [to_dev(idx)], [to_dev(off)])[0]             # device tensors
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    L = 7                                                                      # fixed pooling
    fidx = rng.integers(0, rows, size=bags * L).astype(it)
    got = eng.lookup_batched([1], [to_dev(fidx)], [None], fixed_pooling=L)[0]
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(oracle.c_bag_sum(wide, fidx, (np.arange(bags) * L).astype(it))))


def test_mixed_dtypes_in_one_call(pel, oracle, ragged_case):
    """One call carries an MXFP4 table beside an fp32 and an fp8 table: one launch group per dtype."""
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    rows, dim, B = 1000, 128, 200
    fused, wide = ragged_case[dim]
    g = torch.Generator().manual_seed(95)
    f32, f8 = torch.randn((rows, dim), generator=g), torch.randn((rows, dim), generator=g).to(torch.float8_e4m3fn)
    eng.load_table(0, f32.to(DEV))
    eng.load_table(1, fused, dtype=pel.EMB_MXFP4)
    eng.load_table(2, f8.to(DEV))
    tabs = [f32.numpy(), wide, f8.float().numpy()]
    rng = np.random.default_rng(96)
    order = [1, 0, 2, 1]
    idx, off = zip(*[ragged(rng, rows, B, 12, np.int64) for _ in order])
    d_idx, d_off = [to_dev(i) for i in idx], [to_dev(o) for o in off]
    launches = eng.stats()["n_kernel_launches"]
    outs = eng.lookup_batched(order, d_idx, d_off)
    torch.cuda.synchronize()
    assert eng.stats()["n_kernel_launches"] - launches == 3
    for k, t in enumerate(order):
        assert np.array_equal(bits(outs[k].cpu().numpy()), bits(oracle.c_bag_sum(tabs[t], idx[k], off[k]))), (k, t)
    eng.close()


# ---- extremes: the scale bytes at both ends; sums that are fp32 denormals, or overflow to inf -------------------------------------
def test_extremes(eng, pel, oracle):
    scales = [0, 1, 2, 3, 253, 254]
    dim = 64                                                                   # two blocks per row, under different scales
    rng = np.random.default_rng(7)
    el = rng.integers(0, 256, size=(len(scales) * 8, dim // 2), dtype=np.uint8)
    sc = np.repeat(np.array(scales, np.uint8), 8)
    fused = formats.mxfp4_join(el, np.stack([sc, np.roll(sc, 8)], axis=1))
    wide = formats.from_mxfp4(fused, dim)
    assert np.isinf(wide).any() and (np.abs(wide[wide != 0]) < 2.0 ** -126).any()       # products beyond fp32; fp32 denormals
    eng.load_table(2, fused, dtype=pel.EMB_MXFP4)
    for _n, it in ID_TYPES:
        idx, off = [], []
        for k in range(len(scales)):                                           # bags of 1 ... 4 rows of one scale: denormal sums, overflowing sums
            for n in (1, 2, 3, 4):
                off.append(len(idx))
                idx += list(rng.integers(8 * k, 8 * k + 8, size=n))
        same_sign = np.flatnonzero((wide[:, 7] > 0) & (sc == 254))[:2]          # two rows whose finite elements add up beyond fp32
        off.append(len(idx))
        idx += list(same_sign) * 2
        idx, off = np.array(idx).astype(it), np.array(off).astype(it)
        with np.errstate(over="ignore", invalid="ignore"):
            want = oracle.c_bag_sum(wide, idx, off)
        ok = ~np.isnan(want)                                                   # (inf - inf: NaN is out of scope)
        assert np.isinf(want[ok]).any() and ((want != 0) & (np.abs(want) < 2.0 ** -126)).any() and ok.mean() > 0.5
        got = eng.lookup_batched([2], [to_dev(idx)], [to_dev(off)])[0]
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert np.array_equal(bits(got)[ok], bits(want)[ok]) and np.isnan(got[~ok]).all(), _n


# ---- the pooled modes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pooled_case(ragged_case):
    cases = {}
    for dim in (32, 128):
        fused, wide = ragged_case[dim]
        rng = np.random.default_rng(40 + dim)
        idx, off = ragged(rng, 1000, 64, 20, np.int64)
        pad = 11
        idx[::5] = pad                                                         # padding entries; some bags of padding only
        w = torch.randn(len(idx), generator=torch.Generator().manual_seed(dim)).numpy()
        refs = {"mean": pool_ref.embedding_bag(wide, idx, off, "mean"),
                "max": pool_ref.embedding_bag(wide, idx, off, "max"),
                "weighted": pool_ref.embedding_bag(wide, idx, off, "sum", w),
                "weighted+pad": pool_ref.embedding_bag(wide, idx, off, "sum", w, pad),
                "pad": pool_ref.embedding_bag(wide, idx, off, "sum", None, pad),
                "mean+pad": pool_ref.embedding_bag(wide, idx, off, "mean", None, pad),
                "max+pad": pool_ref.embedding_bag(wide, idx, off, "max", None, pad)}
        ti, to, tw, tf = torch.from_numpy(idx), torch.from_numpy(off), torch.from_numpy(w), torch.from_numpy(wide)
        assert np.array_equal(refs["weighted"], F.embedding_bag(ti, tf, to, mode="sum", per_sample_weights=tw).numpy())      # (and torch's CPU kernel)
        assert np.array_equal(refs["mean+pad"], F.embedding_bag(ti, tf, to, mode="mean", padding_idx=pad).numpy())
        cases[dim] = (fused, idx, off, w, pad, refs)
    return cases


@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("dim", [32, 128])
def test_pooled_modes(eng, pel, pooled_case, dim, ids):
    _n, dt = ids
    fused, idx, off, w, pad, refs = pooled_case[dim]
    eng.load_table(3, fused, dtype=pel.EMB_MXFP4)
    i, o, wt = to_dev(idx.astype(dt)), to_dev(off.astype(dt)), torch.from_numpy(w).to(DEV)
    specs = {"mean": ("mean", None, None), "max": ("max", None, None), "weighted": ("sum", wt, None),
             "weighted+pad": ("sum", wt, pad), "pad": ("sum", None, pad), "mean+pad": ("mean", None, pad), "max+pad": ("max", None, pad)}
    names = list(specs)
    args = ([3] * len(names), [i] * len(names), [o] * len(names), [specs[n][0] for n in names])
    kw = dict(per_sample_weights=[specs[n][1] for n in names], padding_idx=[specs[n][2] for n in names])
    plan = eng.plan_pooled(*args, **kw)
    recs = plan.describe()
    assert all(r["dtype"] == pel.EMB_MXFP4 and r["kind"] == 1 and "pool" in r for r in recs), recs
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for n, out in zip(names, plan.outputs):
        assert np.array_equal(bits(out.cpu().numpy()), bits(refs[n])), ("plan", n)
    plan.destroy()
    outs = eng.lookup_pooled(*args, **kw)
    torch.cuda.synchronize()
    for n, out in zip(names, outs):
        assert out.dtype is torch.float32 and np.array_equal(bits(out.cpu().numpy()), bits(refs[n])), n
    got = eng.lookup_pooled([3], [idx.astype(dt)], [off.astype(dt)], "sum", per_sample_weights=[w], padding_idx=pad)[0]      # host memspace
    assert np.array_equal(bits(got), bits(refs["weighted+pad"]))


# ---- the checked call -------------------------------------------------------------------------------------------------------------
def test_checked_call(eng, pel, oracle, ragged_case):
    """One out-of-range index: EMB_ERR_RANGE (IndexError), once.  This library's checked call refuses the WHOLE call -- the lookup
    behind the check is disarmed on the GPU and writes nothing, for any dtype -- so the offending bag's row is still the zero it
    was before the call (and so is every other row); with the index put right, every row, the offending bag's included, is exact."""
    fused, wide = ragged_case[128]
    eng.load_table(4, fused, dtype=pel.EMB_MXFP4)
    rng = np.random.default_rng(5)
    idx, off = ragged(rng, 1000, 50, 9, np.int64)
    bad = idx.copy()
    where = int(off[20])
    assert off[21] > off[20]
    bad[where] = 1000
    d_off, out = to_dev(off), torch.zeros((50, 128), device=DEV)
    with pytest.raises(IndexError):
        eng.lookup_batched([4], [to_dev(bad)], [d_off], outs=[out], check=True)
    torch.cuda.synchronize()
    assert not bool(out[20].any()) and not bool(out.any())
    eng.check_report()                                                          # ... once: nothing is left to report
    eng.lookup_batched([4], [to_dev(idx)], [d_off], outs=[out], check=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(oracle.c_bag_sum(wide, idx, off)))
    out.zero_()                                                                 # the deferred verdict: raised by a later call, once
    eng.lookup_batched([4], [to_dev(bad)], [d_off], outs=[out], check="deferred")
    with pytest.raises(IndexError):
        eng.check_report()
    eng.check_report()
    torch.cuda.synchronize()
    assert not bool(out.any())
    with pytest.raises(IndexError):                                             # host arrays
        eng.lookup_batched([4], [bad], [off], check=True)


# ---- plans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 96, 2048])
def test_plans(eng, pel, oracle, ragged_case, dim):
    codeobj = import_module("pim_embedding_lookup_amd.codeobj")
    fused, wide = ragged_case[dim]
    eng.load_table(5, fused, dtype=pel.EMB_MXFP4)
    rng = np.random.default_rng(dim + 1)
    for _n, it in ID_TYPES:
        idx, off = ragged(rng, 1000, 200, 40, it)
        plan = eng.plan([5], [to_dev(idx)], [to_dev(off)])
        want = oracle.c_bag_sum(wide, idx, off)
        for fill in (7.0, -3.0):                                               # launched twice: equal results
            plan.outputs[0].fill_(fill)
            plan.launch(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(bits(plan.outputs[0].cpu().numpy()), bits(want))
        stride = formats.mxfp4_row_stride(dim)
        assert plan.bytes() == (len(idx) * (stride + idx.itemsize) + 200 * idx.itemsize + 200 * dim * 4, 200, len(idx))      # `stride` bytes per gathered row
        recs = plan.describe()
        assert len(recs) == 1 and (recs[0]["kind"], recs[0]["dtype"], recs[0]["lanes_per_row"], recs[0]["chunks"]) == (1, 10, lpr_of(dim), dim // 32)
        sym, _sha = codeobj.kernel_of_launch(pel.LIB_PATH, recs[0])              # ... and names a kernel the library holds
        assert "bag_mx4sum_group_kernelI%sLi%dE" % ("j" if it is np.uint32 else "l", lpr_of(dim)) in sym
        assert plan.time_us(warmup=1, iters=2) > 0
        plan.destroy()
    # a big one-hot launch -- the shape the wave-batch kernels take for every other dtype -- stays on the lane-group kernel
    if dim == 32:
        B = 64 * 2048 * 2 + 5
        one = rng.integers(0, 1000, size=B)
        before = eng.stats()["n_launches_by_kind"]
        got = eng.lookup_batched([5], [to_dev(one)], [to_dev(np.arange(B))])[0]
        torch.cuda.synchronize()
        assert [a - b for a, b in zip(eng.stats()["n_launches_by_kind"], before)] == [0, 1, 0, 0, 0]
        assert torch.equal(got.cpu(), torch.from_numpy(wide)[torch.from_numpy(one)] + 0.0)        # (+ 0.0: a sum from +0 turns -0 into +0)


# ---- the request queue: its fused launch is launch_bag_sum's, so MXFP4 is served ---------------------------------------------------
def test_request_queue(pel, oracle, ragged_case):
    fused, wide = ragged_case[64]
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    eng.load_table(0, fused, dtype=pel.EMB_MXFP4)
    eng.load_table(1, fused[:500].copy(), dtype=pel.EMB_MXFP4)
    rng = np.random.default_rng(60)
    q = pel.RequestQueue(eng, pel.EMB_IDX_I64, pel.EMB_MEM_DEVICE)
    reqs = []
    for B in (1, 17, 32):                                                      # three small requests
        idx, off = zip(*[ragged(rng, n, B, 3, np.int64, trailing_empty=0) for n in (1000, 500)])
        outs = [torch.full((B, 64), 7.0, device=DEV) for _ in range(2)]
        reqs.append((q.add([0, 1], [to_dev(a) for a in idx], [to_dev(a) for a in off], outs), idx, off, outs))
    launches = eng.stats()["n_kernel_launches"]
    assert q.flush() == 3
    for ticket, _i, _o, _outs in reqs:
        q.wait(ticket)
    torch.cuda.synchronize()
    assert eng.stats()["n_kernel_launches"] - launches == 1                   # fused: ONE launch
    for _ticket, idx, off, outs in reqs:
        direct = eng.lookup_batched([0, 1], [to_dev(a) for a in idx], [to_dev(a) for a in off])
        torch.cuda.synchronize()
        for t in range(2):
            assert torch.equal(outs[t], direct[t])                              # each bit-equal to its direct lookup ...
            assert np.array_equal(bits(outs[t].cpu().numpy()), bits(oracle.c_bag_sum(wide[:1000 if t == 0 else 500], idx[t], off[t])))
    q.close()
    eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(pel, ragged_case):
    L = pel.lib.load()
    sh = import_module("pim-embedding-lookup_amd.sharding")
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    fused, _wide = ragged_case[128]
    eng.load_table(0, fused, dtype=pel.EMB_MXFP4)

    def refused(rc):
        assert rc == pel.lib.EMB_ERR_UNSUPPORTED, rc
        assert "MXFP4" in L.emb_last_error().decode(), L.emb_last_error()

    with pytest.raises(pel.PimembError) as ex:
        eng.alloc_table(1, 100, 48, pel.EMB_MXFP4)                              # no multiple of 32
    assert ex.value.code == pel.lib.EMB_ERR_INVALID
    with pytest.raises(pel.PimembError) as ex:
        eng.alloc_table(1, 100, 4096, pel.EMB_MXFP4)                            # beyond 64 lanes per row
    assert ex.value.code == pel.lib.EMB_ERR_UNSUPPORTED and "MXFP4" in str(ex.value)
    eng.alloc_table(1, 100, 2048, pel.EMB_MXFP4)
    assert tuple(eng.table_tensor(1).shape) == (100, 1088) and not bool(eng.table_tensor(1).any())
    # the ranged / counted / typed lookups and their plans
    B = 16
    idx = torch.arange(B, device=DEV, dtype=torch.int32)
    out = torch.zeros((B, 128), device=DEV)
    d = (pel.lib.EmbLookupDesc * 1)(pel.lib.EmbLookupDesc(0, 1, idx.data_ptr(), None, B, B, out.data_ptr()))
    lo = (C.c_uint64 * 1)(0)
    ctr = torch.zeros(64 * 256 // 4, dtype=torch.int32, device=DEV)
    served = (C.c_void_p * 1)(ctr.data_ptr())
    plan = C.c_void_p()
    refused(L.emb_lookup_ranged(eng._h, d, lo, 1, None))
    refused(L.emb_lookup_ranged_counted(eng._h, d, lo, served, 1, None))
    refused(L.emb_lookup_ranged_typed(eng._h, d, lo, served, 1, pel.lib.EMB_IDX_U32, None))
    refused(L.emb_plan_create_ranged(eng._h, d, lo, 1, C.byref(plan)))
    refused(L.emb_plan_create_ranged_counted(eng._h, d, lo, served, 1, C.byref(plan)))
    refused(L.emb_plan_create_ranged_typed(eng._h, d, lo, served, 1, pel.lib.EMB_IDX_U32, C.byref(plan)))
    # EMB_POOL_OUT_TABLE_DTYPE at the C ABI (Python refuses earlier: tests/test_mxfp4_cpu.py)
    idx64 = torch.arange(B, device=DEV)
    d = (pel.lib.EmbLookupDesc * 1)(pel.lib.EmbLookupDesc(0, 0, idx64.data_ptr(), idx64.data_ptr(), B, B, out.data_ptr()))
    for mode in (pel.lib.EMB_POOL_SUM, pel.lib.EMB_POOL_MEAN):
        ps = (pel.lib.EmbPoolSpec * 1)(pel.lib.EmbPoolSpec(mode, pel.lib.EMB_POOL_OUT_TABLE_DTYPE, None, 0))
        refused(L.emb_lookup_pooled(eng._h, d, ps, 1, pel.lib.EMB_IDX_I64, pel.lib.EMB_MEM_DEVICE, None, 0, None))
        refused(L.emb_plan_create_pooled(eng._h, d, ps, 1, pel.lib.EMB_IDX_I64, C.byref(plan)))
    with pytest.raises(TypeError, match="MXFP4"):
        eng.lookup_batched([0], [idx64], [idx64], out_dtype="table")
    # hot rows, column loads
    for call in (lambda: eng.set_hot_rows(0, [1, 2, 3]), lambda: eng.learn_hot_rows(0, idx64), lambda: eng.load_table_column(0, 0, np.zeros(100, np.int32))):
        with pytest.raises(pel.PimembError, match="MXFP4") as ex:
            call()
        assert ex.value.code == pel.lib.EMB_ERR_UNSUPPORTED
    # a shard over an engine where this rank holds an MXFP4 table
    rows = [1000]
    for kind in (sh.REPLICATED, sh.WHOLE, sh.ROW_SPLIT):
        units = [sh.Unit(0, -1 if kind == sh.REPLICATED else 0, 0, rows[0], 0)]
        splan = sh.ShardPlan(1, rows, 128, 2, [kind], units, [[0]])
        with pytest.raises(pel.PimembError, match="MXFP4") as ex:
            S = sh.ShardedEmbeddingBags(splan, eng, 0, None, depth=0)            # (unit 0 is engine table 0, loaded above)
            S.forward([idx64], [idx64])                                             # emb_shard_create, at the first use
        assert ex.value.code == pel.lib.EMB_ERR_UNSUPPORTED
    eng.close()


# ---- Python: the pair and the fused rows, the float4 / e8m0 tensors, the modules, the harness -------------------------------------
def test_python_loading(eng, pel, ragged_case):
    fused, wide = ragged_case[96]
    el, sc = formats.mxfp4_split(fused, 96)
    eng.load_table(6, fused, dtype=pel.EMB_MXFP4)
    base = eng.table_tensor(6).cpu().numpy()
    assert base.dtype == np.uint8 and np.array_equal(base, fused)
    t4, t8 = torch.from_numpy(el).view(torch.float4_e2m1fn_x2), torch.from_numpy(sc).view(torch.float8_e8m0fnu)
    for t, rows in ((7, (el, sc)), (8, (t4, t8)), (9, (t4.to(DEV), t8.to(DEV))), (10, torch.from_numpy(fused).to(DEV)),
                    (11, (torch.from_numpy(el).to(DEV), torch.from_numpy(sc).to(DEV)))):
        eng.load_table(t, rows, dtype=None if t in (8, 9) else pel.EMB_MXFP4)
        assert eng.table_info(t)[1:] == (1000, 96, pel.EMB_MXFP4)
        assert np.array_equal(eng.table_tensor(t).cpu().numpy(), fused), t
    with pytest.raises(KeyError):
        eng.load_table(12, fused)                                              # plain uint8 without dtype=: refused
    idx = to_dev(np.arange(1000))
    got = eng.lookup_batched([9], [idx], [idx])[0]
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), torch.from_numpy(wide) + 0.0)


def test_torch_modules(pel):
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    eng = pel.EmbeddingEngine(device=0, max_tables=32)
    torch.manual_seed(80)
    idx = torch.randint(0, 200, (500,))
    off = torch.tensor([0, 0, 7, 40, 41, 300])
    w = torch.randn(200, 64)
    q = formats.to_mxfp4(w.numpy())
    wq = torch.from_numpy(formats.from_mxfp4(q, 64))                              # what the table holds, as fp32
    m = tm.EmbeddingBag(200, 64, _weight=w, dtype="mxfp4", engine=eng, table_id=0)       # an fp32 weight: quantised once
    pre = tm.EmbeddingBag(200, 64, _weight=torch.from_numpy(q), dtype="mxfp4", engine=eng, table_id=1)      # prepacked rows
    for mod in (m, pre):
        assert mod.weight.dtype is torch.uint8 and torch.equal(mod.weight.cpu(), torch.from_numpy(q))
        out = mod(idx.to(DEV), off.to(DEV))
        assert out.dtype is torch.float32 and torch.equal(out.cpu(), F.embedding_bag(idx, wq, off, mode="sum"))
    sd = m.state_dict()
    assert list(sd) == ["weight"] and sd["weight"].dtype is torch.uint8 and torch.equal(sd["weight"].cpu(), torch.from_numpy(q))
    fresh = tm.EmbeddingBag(200, 64, _weight=torch.zeros(200, 64), dtype="mxfp4", engine=eng, table_id=2)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.weight.cpu(), torch.from_numpy(q))
    assert torch.equal(fresh(idx.to(DEV), off.to(DEV)), m(idx.to(DEV), off.to(DEV)))
    with pytest.raises(ValueError):
        tm.EmbeddingBag(200, 64, _weight=w, dtype="mxfp4", engine=eng, table_id=3, out_dtype="weight")
    with pytest.raises(ValueError):
        tm.EmbeddingBag(200, 64, _weight=torch.zeros(200, 40, dtype=torch.uint8), dtype="mxfp4", engine=eng, table_id=3)

    psw = torch.randn(500)
    bags = []
    for k, (mode, pad, weighted) in enumerate([("mean", 3, False), ("max", None, False), ("sum", None, True), ("sum", 4, True)]):
        pm = tm.PoolingEmbeddingBag(200, 64, mode=mode, padding_idx=pad, _weight=w, dtype="mxfp4", engine=eng, table_id=6 + k)
        bags.append(pm)
        x = idx.clone()
        if pad is not None:
            x[::5] = pad
        got = pm(x.to(DEV), off.to(DEV), per_sample_weights=psw.to(DEV) if weighted else None)
        want = F.embedding_bag(x, wq, off, mode=mode, padding_idx=pad, per_sample_weights=psw if weighted else None)
        assert torch.equal(got.cpu(), want), (mode, pad, weighted)
        other = tm.PoolingEmbeddingBag(200, 64, mode=mode, padding_idx=pad, _weight=torch.zeros(200, 64), dtype="mxfp4", engine=eng, table_id=20)
        other.load_state_dict(pm.state_dict())
        assert torch.equal(other.weight, pm.weight)
    fused = tm.FusedPoolingEmbeddingBags(bags[:2])
    got = fused([off.to(DEV)] * 2, [idx.to(DEV)] * 2)
    assert torch.equal(got[1].cpu(), F.embedding_bag(idx, wq, off, mode="max"))
    plain = tm.FusedEmbeddingBags([m, pre])
    got = plain([off.to(DEV)] * 2, [idx.to(DEV)] * 2)
    assert torch.equal(got[0].cpu(), F.embedding_bag(idx, wq, off, mode="sum")) and torch.equal(got[0], got[1])
    with pytest.raises(ValueError):
        tm.FusedEmbeddingBags([m, pre], out_dtype="weight")
    eng.close()


def test_harness_collection(pel):
    hz = import_module("pim-embedding-lookup_amd.dlrm_harness")
    rng = np.random.default_rng(90)
    ln = [300, 1000, 50]
    weights = [rng.standard_normal((n, 32)).astype(np.float32) for n in ln]
    ebc = hz.EmbeddingBagCollection(ln, 32, weights=weights, dtype="mxfp4")      # fp32 checkpoints are quantised
    assert all(ebc.engine.table_info(k)[3] == pel.EMB_MXFP4 for k in range(len(ln)))
    lS_i = [torch.as_tensor(rng.integers(0, n, 200)) for n in ln]
    lS_o = [torch.as_tensor(np.sort(rng.integers(0, 200, 32))) for _ in ln]
    for o in lS_o:
        o[0] = 0
    ly = ebc.apply_emb([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i])
    torch.cuda.synchronize()
    for k in range(len(ln)):
        wq = torch.from_numpy(formats.from_mxfp4(formats.to_mxfp4(weights[k]), 32))
        assert torch.equal(ly[k].cpu(), F.embedding_bag(lS_i[k], wq, lS_o[k], mode="sum")), k
    ebc.close()
    with pytest.raises(ValueError):
        hz.EmbeddingBagCollection([10], 32, dtype="mxfp4", out_dtype="weight")
