"""GPU: strided pooled output (emb_lookup_strided / emb_plan_create_strided, engine.lookup_concat): the tables' pooled rows
side by side in ONE [B, W] buffer, written in place by the strided twins of the lookup kernels.

Every test works on ONE buffer pre-filled with a sentinel bit pattern: `col` leading columns, the descriptors' columns, a
trailing gap.  The tables' columns must equal the reference -- oracle.c_bag_sum over the table widened to fp32 for sums,
tests/pool_ref.py for pooled specs -- and EVERY other element must still be the sentinel.  All comparisons are bit for bit
on uint32 views, nothing excluded."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pool_ref import embedding_bag as pool_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x7FC0DEAD      # the bits of a NaN no lookup here produces
ID_TYPES = [("u32", np.uint32), ("i64", np.int64)]
IDS = dict(ids=[n for n, _ in ID_TYPES])
COL, GAP = 4, 8


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def sentinel_buffer(B, W):
    return torch.full((B, W), SENT, dtype=torch.int32, device=DEV).view(torch.float32)


def u32(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().view(torch.int32).numpy()
    return np.ascontiguousarray(x).view(np.uint32)


def check_buffer(buf, col, refs):
    """The tables' columns equal `refs` (one [B, dim] float32 array per descriptor, side by side from `col`); everything
    else is the sentinel."""
    torch.cuda.synchronize()
    got = u32(buf)
    want = np.full(got.shape, SENT, dtype=np.uint32)
    at = col
    for r in refs:
        want[:, at:at + r.shape[1]] = u32(np.ascontiguousarray(r, dtype=np.float32))
        at += r.shape[1]
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d of %d elements differ; first (row, column, got, want): %s" % (
        len(bad), got.size, [(int(b), int(c), hex(got[b, c]), hex(want[b, c])) for b, c in bad[:6]])


def all_sentinel(buf):
    torch.cuda.synchronize()
    return bool((u32(buf) == SENT).all())


def make_table(pel, name, rows, dim, seed):
    """(what load_table takes, its dtype argument, the table widened to fp32) for a table dtype by name."""
    from pim_embedding_lookup_amd import formats
    x = np.random.default_rng(seed).standard_normal((rows, dim)).astype(np.float32)
    if name == "fp32":
        return x, None, x
    if name == "fp16":
        h = x.astype(np.float16)
        return h, None, h.astype(np.float32)
    if name == "bf16":
        b = formats.to_bf16_bits(x)
        return b, pel.EMB_BF16, formats.from_bf16_bits(b)
    if name in ("e4m3", "e5m2"):
        b = formats.to_f8_bits(x, name)
        return b, pel.EMB_F8_E4M3 if name == "e4m3" else pel.EMB_F8_E5M2, formats.from_f8_bits(b, name)
    assert name == "mxfp4"
    fused = formats.to_mxfp4(x)
    return fused, pel.EMB_MXFP4, formats.from_mxfp4(fused, dim)


def ragged(rng, rows, bags, max_len, dt):
    """Ragged bags with empties, trailing empties (the last three bags) and duplicate indices."""
    lens = rng.integers(0, max_len + 1, size=bags)
    lens[3], lens[-3:] = 0, 0
    lens[5] = max_len
    off = np.zeros(bags, np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    idx = rng.integers(0, rows, size=int(lens.sum()))
    idx[off[5]:off[5] + max_len] = idx[off[5]]                 # one bag of duplicates
    return idx.astype(dt), off.astype(dt)


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


# ---- 1. the lane-group twins: every dtype, the row widths of the issue, both index widths ----------------------------------------
LANE_GROUP = [("fp32", 4), ("fp32", 16), ("fp32", 24), ("fp32", 256), ("fp16", 8), ("fp16", 48), ("fp16", 64), ("fp16", 512),
              ("bf16", 8), ("bf16", 48), ("bf16", 64), ("bf16", 512), ("e4m3", 16), ("e4m3", 128), ("e4m3", 1024),
              ("e5m2", 16), ("e5m2", 128), ("e5m2", 1024), ("mxfp4", 32), ("mxfp4", 96), ("mxfp4", 2048)]
GAP_FREE = {("fp32", 16), ("fp16", 64), ("bf16", 64), ("e4m3", 128), ("e5m2", 128), ("mxfp4", 96)}       # once per dtype


@pytest.mark.parametrize("name,dim", LANE_GROUP, ids=["%s-%d" % c for c in LANE_GROUP])
def test_lane_group_twins(eng, pel, oracle, name, dim):
    rows, bags = 1000, 200
    wide = []
    for t in range(3):
        arg, dt, w = make_table(pel, name, rows, dim, 1000 * dim + t)
        eng.load_table(t, arg, dtype=dt)
        wide.append(w)
    for iname, idt in ID_TYPES:
        rng = np.random.default_rng(dim + len(iname))
        inputs = [ragged(rng, rows, bags, 7, idt) for _ in range(3)]
        refs = [oracle.c_bag_sum(w, i, o) for w, (i, o) in zip(wide, inputs)]
        d_idx, d_off = [to_dev(i) for i, _ in inputs], [to_dev(o) for _, o in inputs]
        buf = sentinel_buffer(bags, COL + 3 * dim + GAP)
        out = eng.lookup_concat([0, 1, 2], d_idx, d_off, out=buf, col=COL)
        assert out is buf
        check_buffer(buf, COL, refs)
        plan = eng.plan_concat([0, 1, 2], d_idx, d_off, out=sentinel_buffer(bags, COL + 3 * dim + GAP), col=COL)
        recs = plan.describe()
        assert len(recs) == 1 and recs[0]["kind"] == 1 and recs[0]["strided"] == 1 and recs[0]["descs"] == 3, recs
        plan.launch(torch.cuda.current_stream().cuda_stream)
        check_buffer(plan.outputs, COL, refs)
        plan.destroy()
        if (name, dim) in GAP_FREE and iname == "u32":        # W == 3 * dim, col = 0: no gap anywhere, still strided
            tight = eng.lookup_concat([0, 1, 2], d_idx, d_off)
            assert tuple(tight.shape) == (bags, 3 * dim)
            check_buffer(tight, 0, refs)


# ---- 2. the wave-batch twin: 131 072 + 5 bags, mostly one index, a few hundred empty / two-index / three-index bags --------------
def mostly_one_hot(rng, rows, bags, dt):
    lens = np.ones(bags, np.int64)
    pick = rng.choice(bags, size=600, replace=False)
    lens[pick[:200]], lens[pick[200:400]], lens[pick[400:]] = 0, 2, 3
    assert lens.sum() <= 2 * bags
    off = np.zeros(bags, np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    return rng.integers(0, rows, size=int(lens.sum())).astype(dt), off.astype(dt)


# (fp32 dim 256 under uint32 ids: the one twin that runs under a configuration of its own, WaveCfgStrided64)
@pytest.mark.parametrize("name,dim,idt", [("fp32", 16, np.uint32), ("bf16", 64, np.int64), ("e4m3", 128, np.uint32), ("fp32", 256, np.uint32)],
                         ids=["fp32-16", "bf16-64", "e4m3-128", "fp32-256"])
def test_wave_batch_twin(eng, pel, oracle, name, dim, idt):
    rows, bags = 3000, 131072 + 5
    rng = np.random.default_rng(dim)
    wide, inputs = [], []
    for t in range(2):
        arg, dt, w = make_table(pel, name, rows, dim, 77 + t)
        eng.load_table(10 + t, arg, dtype=dt)
        wide.append(w)
        inputs.append(mostly_one_hot(rng, rows, bags, idt))
    refs = [oracle.c_bag_sum(w, i, o) for w, (i, o) in zip(wide, inputs)]
    d_idx, d_off = [to_dev(i) for i, _ in inputs], [to_dev(o) for _, o in inputs]
    buf = sentinel_buffer(bags, COL + 2 * dim + GAP)
    plan = eng.plan_concat([10, 11], d_idx, d_off, out=buf, col=COL)
    recs = plan.describe()
    assert len(recs) == 1 and recs[0]["kind"] == 0 and recs[0]["strided"] == 1, recs
    before = eng.stats()["n_launches_by_kind"]
    plan.launch(torch.cuda.current_stream().cuda_stream)
    check_buffer(buf, COL, refs)
    delta = [a - b for a, b in zip(eng.stats()["n_launches_by_kind"], before)]
    assert delta[0] == 1 and sum(delta) == 1          # counted under its existing kind
    plan.destroy()


# ---- 3. the two-batch twin: four descriptors of 131 077 one-index bags (>= 524 288 in the launch, <= 4 lanes per row) -----------
def test_two_batch_twin(eng, pel, oracle):
    rows, bags, dim = 3000, 131077, 16
    rng = np.random.default_rng(3)
    wide, inputs = [], []
    for t in range(4):
        arg, dt, w = make_table(pel, "fp32", rows, dim, 300 + t)
        eng.load_table(20 + t, arg, dtype=dt)
        wide.append(w)
        inputs.append((rng.integers(0, rows, size=bags).astype(np.uint32), np.arange(bags, dtype=np.uint32)))
    refs = [oracle.c_bag_sum(w, i, o) for w, (i, o) in zip(wide, inputs)]
    buf = sentinel_buffer(bags, COL + 4 * dim + GAP)
    plan = eng.plan_concat([20, 21, 22, 23], [to_dev(i) for i, _ in inputs], [to_dev(o) for _, o in inputs], out=buf, col=COL)
    recs = plan.describe()
    assert len(recs) == 1 and recs[0]["kind"] == 2 and recs[0]["strided"] == 1, recs
    plan.launch(torch.cuda.current_stream().cuda_stream)
    check_buffer(buf, COL, refs)
    plan.destroy()


# ---- 4. the pooled twins: mean, max, weighted sum, padded weighted sum with a padding-only bag, side by side -------------------
POOLED = [("fp32", 16, 200), ("bf16", 64, 200), ("e4m3", 128, 200), ("mxfp4", 96, 200), ("fp32", 16, 131077), ("bf16", 32, 131077)]


@pytest.mark.parametrize("name,dim,bags", POOLED, ids=["%s-%d-%d" % c for c in POOLED])
def test_pooled_twins(eng, pel, name, dim, bags):
    rows, pad = 500, 7
    rng = np.random.default_rng(bags + dim)
    arg, dt, wide = make_table(pel, name, rows, dim, 41)
    eng.load_table(30, arg, dtype=dt)
    big = bags > 1000
    if big:       # the pooled wave-batch kernel: one-hot steps and general steps
        idx, off = mostly_one_hot(rng, rows, bags, np.int64)
    else:
        idx, off = ragged(rng, rows, bags, 6, np.int64)
    w = rng.standard_normal(len(idx)).astype(np.float32)
    p_idx = idx.copy()
    ends = np.append(off[1:], len(idx))
    b = int(np.argmax(ends - off >= 2)) if not big else int(np.argmax(ends - off == 2))
    p_idx[off[b]:ends[b]] = pad                                    # a bag of padding only
    p_idx[rng.choice(len(idx), size=len(idx) // 10, replace=False)] = pad
    specs = [("mean", idx, None, None), ("max", idx, None, None), ("sum", idx, w, None), ("sum", p_idx, w, pad)]
    refs = [pool_ref(wide, i, off, mode=m, per_sample_weights=ws, padding_idx=p) for m, i, ws, p in specs]
    d_off = to_dev(off)
    buf = sentinel_buffer(bags, COL + 4 * dim + GAP)
    kw = dict(modes=[m for m, *_ in specs], per_sample_weights=[None if ws is None else to_dev(ws) for _, _, ws, _ in specs],
              padding_idx=[p for *_, p in specs])
    d_idx = [to_dev(i) for _, i, _, _ in specs]
    eng.lookup_concat([30] * 4, d_idx, [d_off] * 4, out=buf, col=COL, **kw)
    check_buffer(buf, COL, refs)
    plan = eng.plan_concat([30] * 4, d_idx, [d_off] * 4, out=sentinel_buffer(bags, COL + 4 * dim + GAP), col=COL, **kw)
    recs = plan.describe()
    want_kind = 0 if big else 1
    assert len(recs) == 3 and all(r["strided"] == 1 and "pool" in r and r["kind"] == want_kind for r in recs), recs
    plan.launch(torch.cuda.current_stream().cuda_stream)
    check_buffer(plan.outputs, COL, refs)
    plan.destroy()


# ---- 5. plans -------------------------------------------------------------------------------------------------------------------
def test_plans(eng, pel, oracle):
    rows, bags, dim = 1000, 200, 16
    wide, inputs = [], []
    rng = np.random.default_rng(5)
    for t in range(3):
        arg, dt, w = make_table(pel, "fp32", rows, dim, 500 + t)
        eng.load_table(40 + t, arg, dtype=dt)
        wide.append(w)
        inputs.append(ragged(rng, rows, bags, 5, np.int64))
    refs = [oracle.c_bag_sum(w, i, o) for w, (i, o) in zip(wide, inputs)]
    d_idx, d_off = [to_dev(i) for i, _ in inputs], [to_dev(o) for _, o in inputs]
    ids = [40, 41, 42]
    buf = sentinel_buffer(bags, COL + 3 * dim + GAP)
    plan = eng.plan_concat(ids, d_idx, d_off, out=buf, col=COL)
    stream = torch.cuda.current_stream().cuda_stream
    plan.launch(stream)
    check_buffer(buf, COL, refs)
    first = u32(buf).copy()
    buf.view(torch.int32).fill_(SENT)
    plan.launch(stream)
    check_buffer(buf, COL, refs)
    assert np.array_equal(u32(buf), first)
    dense = eng.plan(ids, d_idx, d_off)
    assert plan.signature() != dense.signature()
    assert plan.bytes() == dense.bytes()                       # the same bytes move
    # stride == dim: the dense plan, to the signature and the text
    L = eng._L
    one = eng.plan_concat([40], d_idx[:1], d_off[:1])          # one table, no gap: row stride == dim
    ref_one = eng.plan([40], d_idx[:1], d_off[:1])
    assert one.signature() == ref_one.signature()
    assert [{k: v for k, v in r.items()} for r in one.describe()] == ref_one.describe() and "strided" not in one.describe()[0]
    one.launch(stream)
    check_buffer(one.outputs, 0, refs[:1])
    # one call mixes dense and strided descriptors: descriptor 0 dense in a buffer of its own, 1 and 2 strided in `buf`
    own = sentinel_buffer(bags, dim)
    buf.view(torch.int32).fill_(SENT)
    arr = (pel.lib.EmbLookupDesc * 3)()
    for k in range(3):
        ptr = own.data_ptr() if k == 0 else buf.data_ptr() + 4 * (COL + k * dim)
        arr[k] = pel.lib.EmbLookupDesc(ids[k], 0, d_idx[k].data_ptr(), d_off[k].data_ptr(), d_idx[k].numel(), bags, ptr)
    strides = (C.c_uint64 * 3)(0, buf.stride(0), buf.stride(0))
    p = C.c_void_p()
    pel.lib.check(L.emb_plan_create_strided(eng._h, arr, None, strides, 3, pel.EMB_IDX_I64, C.byref(p)))
    mixed = pel.Plan(eng, p.value, None, None)
    recs = mixed.describe()
    assert len(recs) == 2 and sorted(r.get("strided", 0) for r in recs) == [0, 1] and sorted(r["descs"] for r in recs) == [1, 2], recs
    mixed.launch(stream)
    check_buffer(own, 0, refs[:1])
    torch.cuda.synchronize()
    got = u32(buf)
    assert (got[:, :COL + dim] == SENT).all() and (got[:, COL + 3 * dim:] == SENT).all()
    assert np.array_equal(got[:, COL + dim:COL + 2 * dim], u32(refs[1])) and np.array_equal(got[:, COL + 2 * dim:COL + 3 * dim], u32(refs[2]))
    for q in (plan, dense, one, ref_one, mixed):
        q.destroy()


# ---- 6. checked calls: a bad index leaves the whole buffer untouched ---------------------------------------------------------
def test_checked_calls_leave_the_buffer_alone(pel, oracle):
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    rows, bags, dim = 1000, 200, 16
    arg, dt, wide = make_table(pel, "fp32", rows, dim, 6)
    for t in range(3):
        eng.load_table(t, arg, dtype=dt)
    idx, off = ragged(np.random.default_rng(6), rows, bags, 5, np.int64)
    good = oracle.c_bag_sum(wide, idx, off)
    bad = idx.copy()
    bad[len(bad) // 2] = rows                                      # one past the end
    d_off, d_good, d_bad = to_dev(off), to_dev(idx), to_dev(bad)
    buf = sentinel_buffer(bags, COL + 3 * dim + GAP)
    with pytest.raises(IndexError):
        eng.lookup_concat([0, 1, 2], [d_good, d_bad, d_good], [d_off] * 3, out=buf, col=COL, check=True)
    assert all_sentinel(buf)
    eng.lookup_concat([0, 1, 2], [d_good, d_bad, d_good], [d_off] * 3, out=buf, col=COL, check="deferred")   # does not raise here
    assert all_sentinel(buf)
    with pytest.raises(IndexError):
        eng.check_report()
    eng.check_report()                                             # reported once
    eng.lookup_concat([0, 1, 2], [d_good] * 3, [d_off] * 3, out=buf, col=COL, check=True)
    check_buffer(buf, COL, [good] * 3)
    eng.close()


# ---- 7. refusals: nothing is launched ----------------------------------------------------------------------------------------
def test_refusals(pel):
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    L, lib = eng._L, pel.lib
    rows, bags = 100, 50
    eng.load_table(0, np.ones((rows, 16), np.float32))
    eng.load_table(1, np.ones((rows, 6), np.float32))
    eng.load_table(2, np.ones((rows, 16), np.int32))
    eng.load_table(3, np.ones((rows, 16), np.float16))
    idx = to_dev(np.arange(bags, dtype=np.int64))
    buf = sentinel_buffer(bags, 64)
    launches = eng.stats()["n_kernel_launches"]

    def call(table, stride, byte_off=0, flags=0, plan=False):
        arr = (lib.EmbLookupDesc * 1)(lib.EmbLookupDesc(table, 0, idx.data_ptr(), idx.data_ptr(), bags, bags, buf.data_ptr() + byte_off))
        pools = (lib.EmbPoolSpec * 1)(lib.EmbPoolSpec(lib.EMB_POOL_SUM, flags, None, 0)) if flags else None
        st = (C.c_uint64 * 1)(stride)
        if plan:
            p = C.c_void_p()
            rc = L.emb_plan_create_strided(eng._h, arr, pools, st, 1, lib.EMB_IDX_I64, C.byref(p))
            assert p.value is None
        else:
            rc = L.emb_lookup_strided(eng._h, arr, pools, st, 1, lib.EMB_IDX_I64, None, 0, None)
        return rc, L.emb_last_error().decode()

    texts = []
    for plan in (False, True):
        assert call(0, 12, plan=plan)[0] == lib.EMB_ERR_INVALID                       # stride < dim
        rc, text = call(0, 18, plan=plan)                                             # stride % 4 != 0
        assert rc == lib.EMB_ERR_INVALID and "desc 0" in text
        assert call(0, 1 << 32, plan=plan)[0] == lib.EMB_ERR_INVALID
        assert call(0, 64, byte_off=8, plan=plan)[0] == lib.EMB_ERR_INVALID           # misaligned pooled
        for args in (dict(table=1, stride=8), dict(table=2, stride=64), dict(table=3, stride=64, flags=lib.EMB_POOL_OUT_TABLE_DTYPE)):
            rc, text = call(plan=plan, **args)
            assert rc == lib.EMB_ERR_UNSUPPORTED, (args, rc, text)
            texts.append(text)
    assert len(set(texts)) == 3, texts                                               # each refusal has a message of its own
    assert eng.stats()["n_kernel_launches"] == launches and all_sentinel(buf)
    # Python refuses a view with inner stride 2 before any C call
    calls = eng.stats()["n_lookup_calls"]
    with pytest.raises(ValueError, match="inner stride"):
        eng.lookup_concat([0], [idx], [idx], out=sentinel_buffer(bags, 64)[:, ::2])
    with pytest.raises(ValueError, match="narrow"):
        eng.lookup_concat([0], [idx], [idx], out=buf[:, :12])
    with pytest.raises(TypeError):
        eng.lookup_concat([0], [idx], [idx], out=buf.double())
    assert eng.stats()["n_lookup_calls"] == calls
    eng.close()


# ---- 8. modules and harness --------------------------------------------------------------------------------------------------
def test_fused_modules_concat(pel):
    from pim_embedding_lookup_amd import torch_module as tm
    g = torch.Generator().manual_seed(8)
    B, dims, rows = 64, [16, 32, 16], [50, 70, 30]
    eng = tm.default_engine(0)
    emb = [torch.nn.EmbeddingBag(n, d, mode="sum") for n, d in zip(rows, dims)]
    lS_i = [torch.randint(0, n, (B * 3,), generator=g) for n in rows]
    lS_o = [torch.arange(0, B * 3, 3) for _ in rows]
    want = torch.cat([m(i, o) for m, i, o in zip(emb, lS_i, lS_o)], dim=1).detach()
    di, do = [i.to(DEV) for i in lS_i], [o.to(DEV) for o in lS_o]
    for kw in (dict(), dict(deferred_check=True), dict(trusted_inputs=True)):
        fused = tm.FusedEmbeddingBags.from_torch(emb, concat=True, **kw)
        as_list = tm.FusedEmbeddingBags(list(fused.bags), **{k: v for k, v in kw.items()})
        got = fused(do, di)
        assert tuple(got.shape) == (B, sum(dims)) and got.dtype is torch.float32
        assert np.array_equal(u32(got), u32(want)) and np.array_equal(u32(got), u32(torch.cat(as_list(do, di), dim=1)))
        # out= / col=: behind a block of dense features, which stays what it was
        x = torch.randn((B, 8), generator=g).to(DEV)
        R = torch.cat([x, sentinel_buffer(B, sum(dims) + 4)], dim=1)
        assert fused(do, di, out=R, col=8) is R
        torch.cuda.synchronize()
        assert torch.equal(R[:, :8], x) and np.array_equal(u32(R[:, 8:8 + sum(dims)]), u32(want))
        assert (u32(R[:, 8 + sum(dims):]) == SENT).all()
    eng.check_report()
    # pooling modules: mean, max with padding, weighted sum
    modes, pads = ["mean", "max", "sum"], [None, 3, None]
    pemb = [torch.nn.EmbeddingBag(n, d, mode=m, padding_idx=p) for n, d, m, p in zip(rows, dims, modes, pads)]
    lS_w = [None, None, torch.randn((B * 3,), generator=g)]
    pwant = torch.cat([m(i, o, per_sample_weights=w) for m, i, o, w in zip(pemb, lS_i, lS_o, lS_w)], dim=1).detach()
    dw = [None if w is None else w.to(DEV) for w in lS_w]
    for kw in (dict(), dict(deferred_check=True)):
        pf = tm.FusedPoolingEmbeddingBags.from_torch(pemb, concat=True, **kw)
        pl = tm.FusedPoolingEmbeddingBags(list(pf.bags), **kw)
        got = pf(do, di, dw)
        assert np.array_equal(u32(got), u32(pwant)) and np.array_equal(u32(got), u32(torch.cat(pl(do, di, dw), dim=1)))
        R = torch.cat([torch.zeros((B, 4), device=DEV), sentinel_buffer(B, sum(dims))], dim=1)
        pf(do, di, dw, out=R, col=4)
        torch.cuda.synchronize()
        assert np.array_equal(u32(R[:, 4:]), u32(pwant)) and not R[:, :4].any()
    eng.check_report()


@pytest.mark.parametrize("weighted", [None, "fixed"], ids=["sum", "weighted"])
def test_harness_apply_emb_concat(pel, weighted):
    from pim_embedding_lookup_amd import dlrm_harness as H
    ln, m, B = [40, 60, 25], 16, 48
    ebc = H.EmbeddingBagCollection(ln, m, weighted_pooling=weighted)
    rng = np.random.default_rng(9)
    lS_i = [to_dev(rng.integers(0, n, size=B * 2)) for n in ln]
    lS_o = [to_dev(np.arange(0, B * 2, 2)) for _ in ln]
    ly = ebc.apply_emb(lS_o, lS_i)
    got = ebc.apply_emb(lS_o, lS_i, concat=True)
    assert tuple(got.shape) == (B, len(ln) * m)
    assert np.array_equal(u32(got), u32(torch.cat(ly, dim=1)))
    cpu = torch.cat([torch.nn.functional.embedding_bag(i.cpu(), ebc.engine.table_tensor(k).cpu(), o.cpu(), mode="sum",
                                                       per_sample_weights=None if weighted is None else torch.ones(i.numel()))
                     for k, (i, o) in enumerate(zip(lS_i, lS_o))], dim=1)
    assert np.array_equal(u32(got), u32(cpu))
    x = torch.ones((B, 4), device=DEV)
    R = torch.cat([x, sentinel_buffer(B, len(ln) * m)], dim=1)
    assert ebc.apply_emb(lS_o, lS_i, concat=True, out=R, col=4) is R
    torch.cuda.synchronize()
    assert torch.equal(R[:, :4], x) and np.array_equal(u32(R[:, 4:]), u32(cpu))
    ebc.close()


def test_harness_cli_concat_output(capsys):
    from pim_embedding_lookup_amd import dlrm_harness as H
    assert H.main(["--arch-embedding-size", "50-60-70", "--mini-batch-size", "32", "--num-batches", "4", "--inference-only",
                   "--concat-output"]) == 0
    assert "one [B, T * m] tensor" in capsys.readouterr().out
