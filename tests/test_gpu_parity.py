"""GPU: the HIP path, called through the C ABI (libpimemb.so), against the golden fixtures and the
CPU oracle on the same seeded inputs.  Bar: BIT-EXACT -- indices are integers, the fixed-point mode
is integer arithmetic, and the fp32 mode accumulates in index order exactly like the oracle
(tolerance would be 1e-6 abs per load_generator.c:58; we hold 0)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAG_FIXTURES = sorted(os.path.basename(p) for p in glob.glob(
    os.path.join(os.path.dirname(__file__), "golden", "*.npz"))
    if not os.path.basename(p).startswith(("toy_", "kaggle26")))


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


def _dev(pel, eng, a):
    return pel.DeviceBuffer.from_numpy(eng, a)


@pytest.mark.parametrize("name", BAG_FIXTURES)
@pytest.mark.parametrize("itype", [np.uint32, np.int64])
def test_golden_fixture_host_and_device_paths(pel, eng, oracle, golden_dir, name, itype):
    z = np.load(os.path.join(golden_dir, name))
    tab, exp = z["table"], z["expect"]
    idx, off = z["indices"].astype(itype), z["offsets"].astype(itype)
    eng.load_table(0, tab)
    # (1) host pointers: copy in, kernel, copy out -- the reference's calling convention
    got = eng.lookup(0, idx, off)
    assert got.dtype == np.float32 and got.shape == exp.shape
    assert np.array_equal(got, exp), f"{name}: host path differs, max |d| = {np.abs(got - exp).max(initial=0)}"
    # (2) device-resident buffers: zero-copy launch
    d_idx, d_off = _dev(pel, eng, idx), _dev(pel, eng, off)
    d_out = eng.lookup(0, d_idx, d_off)
    eng.synchronize()
    assert np.array_equal(d_out.numpy(), exp)
    # (3) prepared plan, launched twice (idempotent: output is overwritten, not accumulated)
    plan = eng.plan([0], [d_idx], [d_off])
    plan.launch(); plan.launch()
    eng.synchronize()
    assert np.array_equal(plan.outputs[0].numpy(), exp)
    assert np.array_equal(plan.outputs[0].numpy(), oracle.c_bag_sum(tab, idx, off))
    nbytes, nb, ni = plan.bytes()
    assert (nb, ni) == (off.shape[0], idx.shape[0])
    elem = tab.dtype.itemsize
    isz = np.dtype(itype).itemsize
    assert nbytes == ni * (tab.shape[1] * elem + isz) + nb * isz + nb * tab.shape[1] * 4
    plan.destroy()
    for b in (d_idx, d_off, d_out):
        b.free()


def test_toy_ctest_known_answer_through_reference_entry_points(pel, oracle, golden_dir):
    """populate_mram / lookup with the reference's own toy data (c_test.py:40,55-57):
    every bag must come out as [10,20,...,80] / 1e9."""
    from importlib import import_module
    compat = import_module("pim-embedding-lookup_amd.compat")
    z = np.load(os.path.join(golden_dir, "toy_ctest.npz"))
    tab, idx, off = z["table_i32"], z["indices"], z["offsets"]
    T = 3
    compat.reset()
    compat.configure(nr_tables=T, nr_cols=8, max_nr_batches=32, max_indices_per_batch=4)
    rt = pel.lib.DpuRuntimeTotals()
    h = compat.populate([tab] * T, rt)
    assert h and rt.execution_time_populate_copy_in > 0
    eng_h = pel.lib.load().emb_compat_engine()
    import ctypes as C
    s0 = pel.lib.EmbStats(); pel.lib.load().emb_get_stats(eng_h, C.byref(s0))
    res = compat.lookup(h, [idx] * T, [off] * T, nr_cols=8, latency_print=1)
    s1 = pel.lib.EmbStats(); pel.lib.load().emb_get_stats(eng_h, C.byref(s1))
    assert s1.us_launch > s0.us_launch and s1.us_copy_in_indices > s0.us_copy_in_indices   # stage-timed call
    compat.lookup(h, [idx] * T, [off] * T, nr_cols=8, latency_print=0)
    s2 = pel.lib.EmbStats(); pel.lib.load().emb_get_stats(eng_h, C.byref(s2))
    assert s2.us_launch == s1.us_launch and s2.us_sync > s1.us_sync                        # single-wait call
    want = oracle.c_lookup_fixed32(tab, idx, off)
    assert np.array_equal(np.rint(want.astype(np.float64) * 1e9), np.tile(np.arange(10.0, 90.0, 10.0), (32, 1)))
    for t in range(T):
        assert np.array_equal(res[t], want)
        assert oracle.c_validate_result(tab, idx, off, res[t]) == 0      # load_generator.c:58
    compat.reset()


def test_reference_lookup_semantics_random(pel, oracle):
    """Reference shapes (toy preset run.sh:93-101 scaled): T tables x C cols, Bmax bags, L idx/bag,
    int32 tables from rand() like load_generator.c:33, including wrap-around sums."""
    from importlib import import_module
    compat = import_module("pim-embedding-lookup_amd.compat")
    rng = np.random.default_rng(7)
    T, Cc, Bmax, Lmax, rows = 5, 64, 65, 32, 5000      # odd Bmax: the DPU writeback bug case (A3)
    tabs = [rng.integers(-2**31, 2**31 - 1, size=(rows, Cc), dtype=np.int64).astype(np.int32) for _ in range(T)]
    compat.reset()
    compat.configure(T, Cc, Bmax, Lmax)
    h = compat.populate(tabs)
    idx = [rng.integers(0, rows, size=Bmax * Lmax).astype(np.uint32) for _ in range(T)]
    # ragged bag starts inside the fixed-size index buffer; last bag runs to INDICES_LEN
    off = [np.sort(rng.integers(0, Bmax * Lmax, size=Bmax)).astype(np.uint32) for _ in range(T)]
    for o in off:
        o[0] = 0
    res = compat.lookup(h, idx, off, nr_cols=Cc)
    for t in range(T):
        want = oracle.c_lookup_fixed32(tabs[t], idx[t], off[t])
        assert np.array_equal(res[t], want)
        assert np.array_equal(res[t][-1], want[-1])      # odd nr_batches: last bag is NOT dropped
    compat.reset()


def test_compat_lookup_bag0_starts_at_index_0(pel, oracle):
    """The reference's bag-0 start rule through its own entry point: lookup() serves bag 0 from index 0 whatever
    offsets[t][0] says (emb_dpu_lookup.c:60-63: tasklet 0's indices_ptr = 0; load_generator.c:46) -- bit for bit the
    oracle's fixed-point restatement, which follows the same rule; a table whose offsets[0] IS 0 rides in the same call."""
    from importlib import import_module
    compat = import_module("pim-embedding-lookup_amd.compat")
    rng = np.random.default_rng(61)
    T, Cc, Bmax, Lmax, rows = 3, 16, 33, 6, 700
    tabs = [rng.integers(-2**31, 2**31 - 1, size=(rows, Cc), dtype=np.int64).astype(np.int32) for _ in range(T)]
    compat.reset()
    compat.configure(T, Cc, Bmax, Lmax)
    h = compat.populate(tabs)
    idx = [rng.integers(0, rows, size=Bmax * Lmax).astype(np.uint32) for _ in range(T)]
    off = [np.sort(rng.integers(5, Bmax * Lmax, size=Bmax)).astype(np.uint32) for _ in range(T)]     # offsets[t][0] >= 5
    off[1][0] = 0
    res = compat.lookup(h, idx, off, nr_cols=Cc)
    for t in range(T):
        want = oracle.c_lookup_fixed32(tabs[t], idx[t], off[t])
        assert np.array_equal(res[t], want)
        head = off[t].copy()
        head[0] = 0
        assert np.array_equal(res[t], oracle.c_lookup_fixed32(tabs[t], idx[t], head))
        assert oracle.c_validate_result(tabs[t], idx[t], off[t], res[t]) == 0
    assert off[0][0] != 0 and off[2][0] != 0            # the caller's arrays are not written to
    compat.reset()


def test_plan_less_launch_with_a_searched_map_just_above_a_rounding_boundary(pel, eng, oracle):
    """A plan-less multi-table one-hot launch whose XCD map is too large to be expanded (more than 2^20 workgroups: the
    binary-searched form) and whose tile counts sit just ABOVE a quantisation boundary of the map cache (rounded up to 1/16
    of their power of two: up to 6 % more workgroups than tiles, every surplus one must leave at `tile < n_tiles`): twice
    (second sighting = the cached map), every bag against the table row."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    tabs = [rng.standard_normal((r, 4)).astype(np.float32) for r in (9000, 333)]
    eng.load_table(60, tabs[0])
    eng.load_table(61, tabs[1])
    # dim 4 fp32 = one lane per row, two-batch geometry: 256 bags per tile; 2^20 + 2^15 + 1 tiles -> rounded to 2^20 + 2^16
    bags = [((1 << 20) + (1 << 15)) * 256 + 1, 70_001]
    idx = [torch.from_numpy(rng.integers(0, t.shape[0], size=b).astype(np.int32)).to(dev) for t, b in zip(tabs, bags)]
    outs = [torch.empty((b, 4), dtype=torch.float32, device=dev) for b in bags]
    for _ in range(2):
        for o in outs:
            o.fill_(7.0)
        eng.lookup_batched([60, 61], idx, [None, None], outs=outs, fixed_pooling=1)
        torch.cuda.synchronize()
        for t in range(2):
            w = torch.from_numpy(tabs[t]).to(dev)
            for lo in range(0, bags[t], 1 << 24):          # (in pieces: torch's own gather over 2.8e8 indices at once returned zero rows at the tail)
                hi = min(lo + (1 << 24), bags[t])
                assert torch.equal(outs[t][lo:hi], w.index_select(0, idx[t][lo:hi].long())), (t, lo)
    del outs, idx


def test_engine_picks_its_hot_rows_itself(pel, eng, oracle):
    """emb_learn_hot_rows (VERDICT r5 missing #5: LDS staging needed a caller's hint; the DPU program stages its working set by
    itself, emb_dpu_lookup.c:41-58): from ONE batch's device indices the engine stages the rows a host-side count of the same
    batch names (workloads.top_rows), pooled lookups are bit for bit the oracle's with the set staged, and a near-uniform
    batch clears it."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(123)
    rows, dim, B, L = 200_000, 128, 4096, 32
    tab = (rng.standard_normal((rows, dim)) * 0.05).astype(np.float32)
    eng.load_table(40, tab)
    idx = pel.workloads.zipf_indices(rng, rows, B * L)               # 131 072 ids: the whole batch is the sample
    off = pel.workloads.fixed_offsets(B, L)
    d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
    n, share = eng.learn_hot_rows(40, d_idx, max_rows=64, min_share=0.05)
    want = pel.workloads.top_rows(idx, 64)
    assert n == 64 and share == pytest.approx(np.isin(idx, want).mean(), abs=1e-6)
    n64, share64 = eng.learn_hot_rows(40, torch.from_numpy(idx.astype(np.int64)).to(dev), max_rows=64)        # int64 ids: the same choice
    assert (n64, share64) == (n, share)
    before = eng.stats()["n_launches_by_kind"][4]
    got = eng.lookup(40, idx, off)
    assert eng.stats()["n_launches_by_kind"][4] == before + 1          # the LDS kernel ran
    assert np.array_equal(got, oracle.c_bag_sum(tab, idx, off))
    uni = pel.workloads.uniform_indices(rng, rows, B * L)
    n0, share0 = eng.learn_hot_rows(40, uni, max_rows=64, min_share=0.05)       # host array, near-uniform: cleared
    assert n0 == 0 and share0 < 0.05
    before = eng.stats()["n_launches_by_kind"][4]
    assert np.array_equal(eng.lookup(40, uni, off), oracle.c_bag_sum(tab, uni, off))
    assert eng.stats()["n_launches_by_kind"][4] == before


def test_kaggle26_fixture_one_fused_launch(pel, eng, golden_dir):
    """C1-shaped plumbing: 26 tables, D=16, all tables in ONE batched call."""
    z = np.load(os.path.join(golden_dir, "kaggle26_capped_b4.npz"))
    ids = list(range(26))
    for t in ids:
        eng.load_table(t, z[f"table_{t}"])
    before = eng.stats()["n_kernel_launches"]
    outs = eng.lookup_batched(ids, [z[f"indices_{t}"] for t in ids], [z[f"offsets_{t}"] for t in ids])
    assert eng.stats()["n_kernel_launches"] == before + 1
    for t in ids:
        assert np.array_equal(outs[t], z[f"expect_{t}"])


@pytest.mark.parametrize("dim,dtype", [(4, np.float32), (8, np.float32), (16, np.float32), (32, np.float32),
                                       (48, np.float32), (64, np.float32), (128, np.float32),
                                       (256, np.float32), (8, np.float16), (64, np.float16),
                                       (200, np.float16), (512, np.float16), (16, np.int32), (64, np.int32)])
def test_every_row_width_against_oracle(pel, eng, oracle, dim, dtype):
    rng = np.random.default_rng(dim * 7 + np.dtype(dtype).itemsize)
    rows, bags = 3001, 777          # not multiples of any tile size
    if dtype == np.int32:
        tab = rng.integers(-2**31, 2**31 - 1, size=(rows, dim), dtype=np.int64).astype(np.int32)
    else:
        tab = rng.standard_normal((rows, dim)).astype(dtype)
    off, n_idx = pel.workloads.ragged_offsets(rng, bags, 70, p_empty=0.2, dtype=np.int64)
    idx = rng.integers(0, rows, size=n_idx).astype(np.int64)
    eng.load_table(1, tab)
    got = eng.lookup(1, idx, off)
    want = (oracle.c_lookup_fixed32(tab, idx.astype(np.uint32), off.astype(np.uint32)) if dtype == np.int32
            else oracle.c_bag_sum(tab, idx, off))
    assert np.array_equal(got, want)


def test_mixed_shapes_in_one_batched_call(pel, eng, oracle):
    rng = np.random.default_rng(11)
    specs = [(10, 16, np.float32), (11, 64, np.float32), (12, 16, np.float32), (13, 64, np.float16)]
    tabs, idxs, offs = {}, [], []
    for tid, dim, dt in specs:
        tabs[tid] = rng.standard_normal((500 + tid, dim)).astype(dt)
        eng.load_table(tid, tabs[tid])
        off, n = pel.workloads.ragged_offsets(rng, 100 + tid, 9, dtype=np.uint32)
        offs.append(off)
        idxs.append(rng.integers(0, 500 + tid, size=n).astype(np.uint32))
    outs = eng.lookup_batched([s[0] for s in specs], idxs, offs)
    for (tid, _d, _t), i, o, got in zip(specs, idxs, offs, outs):
        assert np.array_equal(got, oracle.c_bag_sum(tabs[tid], i, o))


def test_fixed_pooling_without_offsets(pel, eng, oracle):
    """offsets=NULL + fixed_pooling=L == offsets[i]=i*L (load_generator.c:88)."""
    rng = np.random.default_rng(5)
    tab = rng.standard_normal((10000, 128)).astype(np.float32)
    eng.load_table(2, tab)
    for L in (1, 3, 32, 120):       # 120 = r.sh:9
        idx = rng.integers(0, 10000, size=257 * L).astype(np.uint32)
        got = eng.lookup(2, idx, None, fixed_pooling=L)
        want = oracle.c_bag_sum(tab, idx, pel.workloads.fixed_offsets(257, L))
        assert np.array_equal(got, want)


def test_edge_cases(pel, eng, oracle):
    rng = np.random.default_rng(3)
    tab = rng.standard_normal((9, 16)).astype(np.float32)
    eng.load_table(3, tab)
    # zero bags, zero indices
    out = eng.lookup(3, np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert out.shape == (0, 16)
    # all bags empty -> zeros (emb_dpu_lookup.c:108)
    out = eng.lookup(3, np.zeros(0, np.int64), np.zeros(13, np.int64))
    assert np.array_equal(out, np.zeros((13, 16), np.float32))
    # one giant bag of duplicates
    idx = np.full(100000, 4, dtype=np.uint32)
    out = eng.lookup(3, idx, np.zeros(1, np.uint32))
    assert np.array_equal(out, oracle.c_bag_sum(tab, idx, np.zeros(1, np.uint32)))
    # first / last row of the table, single-row table
    idx = np.array([0, 8, 8, 0], dtype=np.uint32)
    assert np.array_equal(eng.lookup(3, idx, np.array([0, 1, 2, 3], np.uint32)), tab[idx])
    one = rng.standard_normal((1, 64)).astype(np.float32)
    eng.load_table(4, one)
    assert np.array_equal(eng.lookup(4, np.zeros(5, np.int64), np.arange(5, dtype=np.int64)), np.tile(one, (5, 1)))


def test_errors_are_codes_not_exits(pel, eng):
    with pytest.raises(KeyError):
        eng.lookup(63, np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    L = pel.lib.load()
    import ctypes as C
    d = pel.lib.EmbLookupDesc(62, 0, None, None, 0, 1, None)
    assert L.emb_lookup_batched(eng._h, C.byref(d), 1, 0, 0, None) == pel.lib.EMB_ERR_INVALID
    assert b"not loaded" in L.emb_last_error()
    with pytest.raises(pel.PimembError) as ei:
        eng.alloc_table(5, 10, 0, pel.EMB_F32)          # dim 0
    assert ei.value.code == pel.lib.EMB_ERR_UNSUPPORTED
    with pytest.raises(pel.PimembError):
        eng.alloc_table(999, 10, 16, pel.EMB_F32)       # beyond max_tables


def test_validate_inputs_counts_bad_indices(pel, eng):
    tab = np.zeros((50, 16), np.float32)
    eng.load_table(6, tab)
    idx = np.array([0, 49, 50, 7, 2**31], dtype=np.uint32)
    off = np.array([0, 2, 1], dtype=np.uint32)          # 2 -> 1 is non-monotone
    assert eng.validate([6], [idx], [off]) == 3
    assert eng.validate([6], [idx[:2]], [np.array([0, 1], np.uint32)]) == 0


def test_torch_tensors_zero_copy_on_current_stream(pel, eng, oracle):
    import torch
    rng = np.random.default_rng(21)
    tab = rng.standard_normal((4096, 16)).astype(np.float32)
    w = torch.from_numpy(tab).cuda()
    eng.load_table(7, w)                                 # device-to-device upload
    idx = rng.integers(0, 4096, size=3000).astype(np.int64)
    off = np.arange(0, 3000, 3, dtype=np.int64)
    ti, to = torch.from_numpy(idx).cuda(), torch.from_numpy(off).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = eng.lookup(7, ti, to)
    s.synchronize()
    assert out.is_cuda and out.shape == (1000, 16)
    want = oracle.c_bag_sum(tab, idx, off)
    assert np.array_equal(out.cpu().numpy(), want)
    # and torch's own GPU EmbeddingBag agrees to fp32 tolerance (different summation order allowed)
    ref = torch.nn.functional.embedding_bag(ti, w, to, mode="sum")
    assert torch.allclose(out, ref, atol=1e-6, rtol=0)


def test_moderate_size_all_index_distributions(pel, eng, oracle):
    """Sizes the oracle finishes in seconds: 200k bags, uniform and Zipf(1.2) indices, pooling 1/32."""
    rng = np.random.default_rng(1)
    rows = 1_000_000
    tab = pel.workloads.dlrm_table(rng, rows, 16)
    eng.load_table(8, tab)
    for L, gen in ((1, pel.workloads.uniform_indices), (1, pel.workloads.zipf_indices),
                   (32, pel.workloads.zipf_indices)):
        B = 200_000 if L == 1 else 20_000
        idx = gen(rng, rows, B * L)
        off = pel.workloads.fixed_offsets(B, L)
        got = eng.lookup(8, idx, off)
        assert np.array_equal(got, oracle.c_bag_sum(tab, idx, off))


def test_big_multi_table_launch_wavebatch_xcd_map(pel, eng, oracle):
    """Big enough for the wave-batch kernel + XCD-aware workgroup map (several tables, > 131072 bags):
    (a) one-hot bags, (b) bags of 0/1 indices (speculative index prefetch must fall back),
    (c) ragged bags 0..5, (d) fixed pooling 4 -- every table bit-exact against the oracle."""
    rng = np.random.default_rng(99)
    sizes = [3, 1000, 70_000, 1_500_000, 40_000, 17]
    tabs = [pel.workloads.dlrm_table(rng, n, 16) for n in sizes]
    ids = list(range(20, 20 + len(sizes)))
    for t, tab in zip(ids, tabs):
        eng.load_table(t, tab)
    B = 40_000

    def run(make_bags):
        idxs, offs = [], []
        for n in sizes:
            off, n_idx = make_bags()
            offs.append(off)
            idxs.append(rng.integers(0, n, size=n_idx).astype(np.uint32))
        import torch
        d_i = [torch.from_numpy(i.view(np.int32)).cuda() for i in idxs]
        d_o = [torch.from_numpy(o.view(np.int32)).cuda() for o in offs]
        before = eng.stats()["n_kernel_launches"]
        outs = eng.lookup_batched(ids, d_i, d_o)
        assert eng.stats()["n_kernel_launches"] == before + 1      # device buffers: ONE fused launch
        for tab, i, o, got in zip(tabs, idxs, offs, outs):
            assert np.array_equal(got.cpu().numpy(), oracle.c_bag_sum(tab, i, o))
        # the same from HOST buffers: one launch, or -- a call this big with >= 1.5 MB of rows per table goes out in two parts
        # (lookup_host_split, round 6) -- two
        before = eng.stats()["n_kernel_launches"]
        outs = eng.lookup_batched(ids, idxs, offs)
        assert eng.stats()["n_kernel_launches"] - before in (1, 2)
        for tab, i, o, got in zip(tabs, idxs, offs, outs):
            assert np.array_equal(got, oracle.c_bag_sum(tab, i, o))

    run(lambda: (pel.workloads.fixed_offsets(B, 1), B))
    def zero_one():
        lens = rng.integers(0, 2, size=B)
        off = np.zeros(B, np.int64); off[1:] = np.cumsum(lens)[:-1]
        return off.astype(np.uint32), int(lens.sum())
    run(zero_one)
    run(lambda: pel.workloads.ragged_offsets(rng, B, 5, p_empty=0.2, dtype=np.uint32))
    run(lambda: (pel.workloads.fixed_offsets(B, 4), 4 * B))


# ---------------------------------------------------------------------------------------------------
# BASELINE.json full sizes: size-independent properties (the oracle is only sampled here)
# ---------------------------------------------------------------------------------------------------
def test_full_size_c2_properties(pel, oracle):
    """configs[1]: the 26 Criteo-Kaggle tables (33.8 M rows, dim 16 fp32), B = 39292, L = 1.
    (1) one-hot => pooled row IS the table row, bit for bit, for every one of the 1 021 592 bags
        (checked against an independent torch gather on the GPU);
    (2) linearity: a table scaled by 2 gives exactly 2x the pooled rows (x2 is exact in fp32);
    (3) idempotence: a second launch of the same plan leaves the output unchanged;
    (4) the oracle agrees on a sample of bags of every table (rows fetched from the GPU)."""
    import torch
    dev = torch.device("cuda", 0)
    rows = pel.workloads.KAGGLE_ROWS
    B = pel.workloads.KAGGLE_BATCH
    T = len(rows)
    e = pel.EmbeddingEngine(device=0, max_tables=2 * T)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rng = np.random.default_rng(1)
    ws, idxs = [], []
    for t, n in enumerate(rows):
        a = float(np.sqrt(1.0 / n))
        w = torch.empty((n, 16), dtype=torch.float32, device=dev).uniform_(-a, a, generator=g)
        e.load_table(t, w)
        e.load_table(T + t, w * 2.0)
        ws.append(w)
        idxs.append(torch.from_numpy(pel.workloads.uniform_indices(rng, n, B).view(np.int32)).to(dev))
    off = torch.arange(B, dtype=torch.int32, device=dev)
    plan1 = e.plan(list(range(T)), idxs, [off] * T)
    plan2 = e.plan(list(range(T, 2 * T)), idxs, [off] * T)
    plan1.launch(); plan2.launch()
    torch.cuda.synchronize()
    first = [o.clone() for o in plan1.outputs]
    plan1.launch()
    torch.cuda.synchronize()
    checksum = 0.0
    for t in range(T):
        want = ws[t][idxs[t].long()]
        assert torch.equal(plan1.outputs[t], want), f"table {t}: pooled row != table row"
        assert torch.equal(plan1.outputs[t], first[t])                      # idempotent
        assert torch.equal(plan2.outputs[t], plan1.outputs[t] * 2.0)        # linear
        checksum += float(plan1.outputs[t].double().sum())
        # oracle on a sample: 64 bags, rows copied back from HBM
        sel = rng.integers(0, B, size=64)
        idx_s = idxs[t][sel].cpu().numpy().astype(np.int64)
        uniq, inv = np.unique(idx_s, return_inverse=True)
        small = ws[t][torch.from_numpy(uniq).to(dev)].cpu().numpy()
        want_s = oracle.c_bag_sum(small, inv.astype(np.int64), np.arange(64, dtype=np.int64))
        assert np.array_equal(plan1.outputs[t][torch.from_numpy(sel).to(dev)].cpu().numpy(), want_s)
    # checksum of checksums: sum of all pooled values == sum over gathered rows (float64)
    ref = sum(float(ws[t][idxs[t].long()].double().sum()) for t in range(T))
    assert abs(checksum - ref) <= 1e-9 * max(1.0, abs(ref))
    nb, ni = plan1.bytes()[1:]
    assert (nb, ni) == (T * B, T * B)
    plan1.destroy(); plan2.destroy(); e.close()


def test_full_width_pooled_properties(pel, oracle):
    """configs[2] shape at reduced table count (dim 128 fp32, 10 M rows, B = 16384, pooling 32,
    Zipf(1.2)): linearity (exact), bag-concatenation additivity within 1e-6, and the oracle on a
    sample of bags."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2)
    n, D, B, L = 10_000_000, 128, 16384, 32
    e = pel.EmbeddingEngine(device=0, max_tables=4)
    a = float(np.sqrt(1.0 / n))
    w = torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-a, a)
    e.load_table(0, w)
    e.load_table(1, w * 2.0)
    idx = torch.from_numpy(pel.workloads.zipf_indices(rng, n, B * L).view(np.int32)).to(dev)
    off = torch.from_numpy(pel.workloads.fixed_offsets(B, L).view(np.int32)).to(dev)
    out1 = e.lookup(0, idx, off)
    out2 = e.lookup(1, idx, off)
    # additivity: bags of 32 == (first 16) + (last 16) up to fp32 reassociation
    off16 = torch.from_numpy(pel.workloads.fixed_offsets(2 * B, L // 2).view(np.int32)).to(dev)
    halves = e.lookup(0, idx, off16)
    torch.cuda.synchronize()
    assert torch.equal(out2, out1 * 2.0)
    assert float((halves[0::2] + halves[1::2] - out1).abs().max()) <= 1e-6
    sel = rng.integers(0, B, size=48)
    pos = (sel[:, None] * L + np.arange(L)[None, :]).reshape(-1)
    idx_s = idx[torch.from_numpy(pos).to(dev)].cpu().numpy().astype(np.int64)
    uniq, inv = np.unique(idx_s, return_inverse=True)
    small = w[torch.from_numpy(uniq).to(dev)].cpu().numpy()
    want = oracle.c_bag_sum(small, inv.astype(np.int64), np.arange(48, dtype=np.int64) * L)
    assert np.array_equal(out1[torch.from_numpy(sel).to(dev)].cpu().numpy(), want)
    e.close()


def test_apply_emb_harness_matches_torch_embeddingbag(pel, oracle, tmp_path):
    """F1: the apply_emb contract -- list of (offsets_k, indices_k) in, list of [B, m] out -- against
    torch CPU nn.EmbeddingBag(mode="sum") built from the same checkpoint (F2 format)."""
    import torch
    from importlib import import_module
    hz = import_module("pim-embedding-lookup_amd.dlrm_harness")
    fm = import_module("pim-embedding-lookup_amd.formats")
    rng = np.random.default_rng(4)
    ln_emb, m = [1460, 583, 50000, 3, 27], 16
    tabs = [pel.workloads.dlrm_table(rng, n, m) for n in ln_emb]
    ckpt = tmp_path / "dlrm.pt"
    fm.save_dlrm_embedding_weights(str(ckpt), tabs)
    ebc = hz.EmbeddingBagCollection.from_checkpoint(str(ckpt))
    dev = torch.device("cuda", 0)
    for B, L, fixed in ((1, 1, True), (188, 1, True), (77, 6, False)):
        lS_o, lS_i = hz.random_batch(rng, ln_emb, B, L, fixed, dev)
        ly = ebc.apply_emb(lS_o, lS_i)
        ly2 = ebc.apply_emb(lS_o, lS_i)                 # fresh outputs on every call
        plan = ebc.prepare(lS_o, lS_i)                  # static buffers: prepared plan
        plan.launch(torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        for k in range(len(ln_emb)):
            bag = torch.nn.EmbeddingBag.from_pretrained(torch.from_numpy(tabs[k]), mode="sum")
            want = bag(lS_i[k].cpu(), lS_o[k].cpu())
            assert torch.equal(ly[k].cpu(), want) and ly[k].shape == (B, m)
            assert ly2[k].data_ptr() != ly[k].data_ptr() and torch.equal(ly2[k], ly[k])
            assert torch.equal(plan.outputs[k].cpu(), want)
    # host (numpy) inputs go through the copy-in/copy-out path and agree too
    lS_o, lS_i = hz.random_batch(rng, ln_emb, 9, 3, False, None)
    ly = ebc.apply_emb(lS_o, lS_i)
    for k in range(len(ln_emb)):
        assert np.array_equal(ly[k], oracle.c_bag_sum(tabs[k], lS_i[k], lS_o[k]))
    ebc.close()
    saved = tmp_path / "saved.pt"
    assert hz.main(["--arch-embedding-size=100-200-300", "--mini-batch-size=32", "--num-batches=3",
                    "--num-indices-per-lookup=4", "--inference-only", f"--save-model={saved}"]) == 0
    ws = fm.load_dlrm_embedding_weights(str(saved))                     # --save-model / --load-model round trip
    assert [w.shape for w in ws] == [(100, 16), (200, 16), (300, 16)]
    assert hz.main([f"--load-model={saved}", "--mini-batch-size=8", "--num-batches=2", "--inference-only"]) == 0


def test_stage_trace_export(pel, eng, tmp_path):
    """F4: per-call stage intervals -> the reference's interval CSV and a Chrome trace."""
    import csv
    import json
    from importlib import import_module
    tr = import_module("pim-embedding-lookup_amd.trace")
    tab = np.ones((100, 16), np.float32)
    eng.load_table(9, tab)
    tr.enable(eng, 1000)
    for _ in range(3):
        eng.lookup(9, np.arange(50, dtype=np.uint32), np.arange(0, 50, 5, dtype=np.uint32))
    ev = tr.read(eng)
    assert len(ev) == 15 and [e["stage"] for e in ev[:5]] == [0, 1, 2, 3, 4]
    assert [e["call_id"] for e in ev[::5]] == [0, 1, 2]
    assert all(e["stop_us"] >= e["start_us"] for e in ev)
    assert all(a["stop_us"] <= b["start_us"] + 1e-3 for a, b in zip(ev, ev[1:]))   # stages do not overlap
    assert tr.read(eng) == []                                                     # drained
    tr.write_interval_csv(ev, tmp_path / "runtimes.csv")
    rows = list(csv.reader(open(tmp_path / "runtimes.csv")))
    assert rows[0] == ["DPU", "Start", "Stop"] and len(rows) == 16
    assert float(rows[1][2]) >= float(rows[1][1])
    tr.write_chrome_trace(ev, tmp_path / "trace.json")
    t = json.load(open(tmp_path / "trace.json"))["traceEvents"]
    assert len(t) == 30 and {x["ph"] for x in t} == {"B", "E"} and t[4]["name"] == "launch"
    tr.enable(eng, 0)
    eng.lookup(9, np.arange(5, dtype=np.uint32), np.arange(5, dtype=np.uint32))
    assert tr.read(eng) == []


def test_plan_launch_is_graph_capturable(pel, eng):
    """emb_plan_launch is a pure enqueue (no allocation, copy or sync): it can be captured into a
    hipGraph and replayed -- the launch-bound small-batch loop (reference presets: 64-512 bags)."""
    import torch
    dev = torch.device("cuda", 0)
    w = torch.randn(5000, 16, device=dev)
    eng.load_table(30, w)
    eng.load_table(31, w * 3.0)
    idx = torch.randint(0, 5000, (512,), dtype=torch.int64, device=dev)
    off = torch.arange(0, 512, 2, dtype=torch.int64, device=dev)
    plan = eng.plan([30, 31], [idx, idx], [off, off])
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        plan.launch(torch.cuda.current_stream().cuda_stream)
    for o in plan.outputs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = w[idx[0::2]] + w[idx[1::2]]
    assert torch.equal(plan.outputs[0], want)
    assert torch.equal(plan.outputs[1], w[idx[0::2]] * 3.0 + w[idx[1::2]] * 3.0)
    # new indices in the same buffers: replay picks them up (descriptors hold pointers, not values)
    idx.copy_(torch.randint(0, 5000, (512,), dtype=torch.int64, device=dev))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(plan.outputs[0], w[idx[0::2]] + w[idx[1::2]])
    plan.destroy()


@pytest.mark.parametrize("dim,dtype", [(4, np.float32), (8, np.float32), (32, np.float32), (64, np.float32),
                                       (128, np.float32), (256, np.float32), (24, np.float32),
                                       (8, np.float16), (128, np.float16), (512, np.float16), (16, np.int32)])
def test_wave_batch_fast_path_every_row_width(pel, eng, oracle, dim, dtype):
    """> 131072 one-hot-ish bags: the wave-batch kernel (one-hot fast path with speculation, its
    fallback when offsets != arange, and the general rounds) for every lanes-per-row value."""
    rng = np.random.default_rng(dim + np.dtype(dtype).itemsize)
    rows, B = 1500, 135_001
    if dtype == np.int32:
        tab = rng.integers(-2**31, 2**31 - 1, size=(rows, dim), dtype=np.int64).astype(np.int32)
        ref = lambda i, o: oracle.c_lookup_fixed32(tab, i, o)
    else:
        tab = rng.standard_normal((rows, dim)).astype(dtype)
        ref = lambda i, o: oracle.c_bag_sum(tab, i, o)
    eng.load_table(40, tab)
    # (a) pure one-hot, offsets = arange  (speculative prefetch accepted)
    idx = rng.integers(0, rows, size=B).astype(np.uint32)
    off = np.arange(B, dtype=np.uint32)
    assert np.array_equal(eng.lookup(40, idx, off), ref(idx, off))
    # (b) bags of 0/1 indices (speculation rejected after the first empty bag)
    lens = rng.integers(0, 2, size=B)
    off = np.zeros(B, np.int64); off[1:] = np.cumsum(lens)[:-1]
    idx = rng.integers(0, rows, size=int(lens.sum())).astype(np.uint32)
    assert np.array_equal(eng.lookup(40, idx, off.astype(np.uint32)), ref(idx, off.astype(np.uint32)))
    # (c) mostly one-hot with a few longer bags (general rounds inside some wave batches), int64 indices
    lens = np.ones(B, np.int64); lens[rng.integers(0, B, size=200)] = rng.integers(2, 20, size=200)
    off = np.zeros(B, np.int64); off[1:] = np.cumsum(lens)[:-1]
    idx = rng.integers(0, rows, size=int(lens.sum())).astype(np.int64)
    want = (oracle.c_lookup_fixed32(tab, idx.astype(np.uint32), off.astype(np.uint32)) if dtype == np.int32
            else oracle.c_bag_sum(tab, idx, off))
    assert np.array_equal(eng.lookup(40, idx, off), want)


def test_random_shapes_host_path(pel, eng, oracle):
    """Randomised sweep (seeded): dims, dtypes, index widths, ragged bags through the host path."""
    rng = np.random.default_rng(2024)
    for case in range(40):
        dtype = [np.float32, np.float16, np.int32][case % 3]
        elem = np.dtype(dtype).itemsize
        dim = int(rng.integers(1, 1024 // elem // (16 // elem) + 1)) * (16 // elem)
        rows = int(rng.integers(1, 4000))
        n_bags = int(rng.integers(0, 3000))
        itype = np.uint32 if (case % 2 == 0 or dtype == np.int32) else np.int64
        off, n_idx = pel.workloads.ragged_offsets(rng, n_bags, int(rng.integers(1, 12)), p_empty=0.3, dtype=itype)
        idx = rng.integers(0, rows, size=n_idx).astype(itype)
        if dtype == np.int32:
            tab = rng.integers(-2**31, 2**31 - 1, size=(rows, dim), dtype=np.int64).astype(np.int32)
            want = oracle.c_lookup_fixed32(tab, idx, off)
        else:
            tab = rng.standard_normal((rows, dim)).astype(dtype)
            want = oracle.c_bag_sum(tab, idx, off)
        eng.load_table(41, tab)
        got = eng.lookup(41, idx, off)
        assert np.array_equal(got, want), f"case {case}: dim {dim} {dtype} rows {rows} bags {n_bags}"


@pytest.mark.parametrize("dim,dtype", [(16, np.float32), (128, np.float32), (64, np.float16), (4, np.float32)])
def test_two_batch_wave_kernel_very_big_launch(pel, eng, oracle, dim, dtype):
    """>= 524288 one-hot-ish bags: the two-batches-per-wavefront kernel, fast path and general rounds."""
    rng = np.random.default_rng(7 * dim)
    rows, B = 2000, 530_003
    tab = rng.standard_normal((rows, dim)).astype(dtype)
    eng.load_table(42, tab)
    idx = rng.integers(0, rows, size=B).astype(np.uint32)
    off = np.arange(B, dtype=np.uint32)
    assert np.array_equal(eng.lookup(42, idx, off), tab[idx].astype(np.float32) + np.float32(0))
    lens = np.ones(B, np.int64)
    lens[rng.integers(0, B, size=300)] = rng.integers(0, 9, size=300)
    off = np.zeros(B, np.int64); off[1:] = np.cumsum(lens)[:-1]
    idx = rng.integers(0, rows, size=int(lens.sum())).astype(np.int64)
    assert np.array_equal(eng.lookup(42, idx, off), oracle.c_bag_sum(tab, idx, off))


def test_plan_lifetime_guards(pel):
    """A plan whose table was re-allocated must fail loudly, and an engine with live plans must
    refuse to be destroyed (the reference has neither plans nor a destroy function)."""
    e = pel.EmbeddingEngine(device=0, max_tables=4)
    tab = np.ones((100, 16), np.float32)
    e.load_table(0, tab)
    idx = pel.DeviceBuffer.from_numpy(e, np.arange(10, dtype=np.uint32))
    off = pel.DeviceBuffer.from_numpy(e, np.arange(10, dtype=np.uint32))
    plan = e.plan([0], [idx], [off])
    plan.launch(); e.synchronize()
    e.load_table(0, tab * 2)                       # same size: storage kept, plan stays valid
    plan.launch(); e.synchronize()
    assert np.array_equal(plan.outputs[0].numpy(), np.full((10, 16), 2.0, np.float32))
    e.load_table(0, np.ones((200, 16), np.float32))   # re-allocated
    with pytest.raises(pel.PimembError) as ei:
        plan.launch()
    assert "stale" in str(ei.value)
    with pytest.raises(pel.PimembError):
        e.close()
    plan.destroy()
    e.close()


def test_clamped_build_survives_malformed_input(pel, oracle, tmp_path):
    """-DPIMEMB_CLAMP_INPUTS=1 flavour: out-of-range indices and broken offsets must not fault the GPU;
    bags with clean inputs still get exact results.  (The shipped flavour, like the reference, does
    not check: emb_dpu_lookup.c:113.)"""
    import shutil
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc on this box")
    from importlib import import_module
    path = import_module("pim-embedding-lookup_amd.build").build_clamped(str(tmp_path))
    e = pel.EmbeddingEngine(device=0, max_tables=4, lib_path=path)
    rng = np.random.default_rng(17)
    tab = rng.standard_normal((1000, 16)).astype(np.float32)
    e.load_table(0, tab)
    for B in (300, 140_000):                       # lane-group kernel, wave-batch kernel
        idx = rng.integers(0, 1000, size=B).astype(np.int64)
        off = np.arange(B, dtype=np.int64)
        bad = idx.copy()
        bad[::7] = 2**40
        bad[3::11] = -3
        got = e.lookup(0, bad, off)
        clean = np.ones(B, bool); clean[::7] = False; clean[3::11] = False
        assert np.array_equal(got[clean], tab[idx[clean]])
        assert np.array_equal(got[~clean], np.tile(tab[999], ((~clean).sum(), 1)))   # clamped to the last row
        # offsets running past n_indices / going backwards: no fault, clean prefix still exact
        off2 = off.copy(); off2[B // 2:] = off2[B // 2:][::-1] + 10 * B
        got = e.lookup(0, idx, off2)
        assert np.array_equal(got[: B // 2 - 1], tab[idx[: B // 2 - 1]])
    # the element-per-thread kernel (10-column rows) and the LDS hot-row kernel clamp too
    tab10 = rng.standard_normal((500, 10)).astype(np.float32)
    e.load_table(1, tab10)
    idx = rng.integers(0, 500, size=2000).astype(np.int64)
    bad = idx.copy(); bad[::5] = 2**33
    got = e.lookup(1, bad, np.arange(2000, dtype=np.int64))
    clean = np.ones(2000, bool); clean[::5] = False
    assert np.array_equal(got[clean], tab10[idx[clean]])
    assert np.array_equal(got[~clean], np.tile(tab10[499], ((~clean).sum(), 1)))
    e.set_hot_rows(0, np.arange(64, dtype=np.uint64))
    idx = rng.integers(0, 1000, size=4000).astype(np.int64)
    bad = idx.copy(); bad[::9] = 2**35
    off = (np.arange(500) * 8).astype(np.int64)
    got = e.lookup(0, bad, off)
    fixed = np.where(np.arange(4000) % 9 == 0, 999, idx)
    assert np.array_equal(got, oracle.c_bag_sum(tab, fixed, off))
    assert e.stats()["n_launches_by_kind"][4] == 1
    e.close()


def test_c_programs_against_the_abi(pel):
    """Plain C / C++ consumers of libpimemb.so, no Python in the loop: the native API example (C99)
    and the load_generator counterpart over populate_mram / lookup (g++), both self-validating."""
    import subprocess
    libdir = os.path.dirname(pel.LIB_PATH)
    ex = os.path.join(libdir, "native_example")
    hb = os.path.join(libdir, "emb_host_bench")
    if not (os.path.exists(ex) and os.path.exists(hb) and os.path.exists(os.path.join(libdir, "shard_example"))):
        subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(libdir), "csrc"), "-f",
                               "Makefile.tools"])
    r = subprocess.run([ex], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, r.stdout + r.stderr
    # the sharded lookup as one call per batch (replicated + whole + row-split tables, a refused bad index) and the request queue
    r = subprocess.run([os.path.join(libdir, "shard_example")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout and "3 requests in 1 launch" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([hb, "4", "16", "20000", "65", "7", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Validation result: true" in r.stdout, r.stdout + r.stderr


def test_many_transient_launches_on_two_streams(pel, eng, oracle):
    """Device-pointer emb_lookup_batched without a plan: 24 back-to-back calls on two streams reuse
    the pinned launch-image segments (a stream switch closes a segment); every output must still be right."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    tab = rng.standard_normal((3000, 16)).astype(np.float32)
    eng.load_table(50, tab)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    cases = []
    for i in range(24):
        off, n = pel.workloads.ragged_offsets(rng, 500 + i, 6, dtype=np.int64)
        idx = rng.integers(0, 3000, size=n).astype(np.int64)
        ti, to = torch.from_numpy(idx).to(dev), torch.from_numpy(off).to(dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[i % 2]):
            out = eng.lookup(50, ti, to)
        cases.append((idx, off, out))
    torch.cuda.synchronize()
    for idx, off, out in cases:
        assert np.array_equal(out.cpu().numpy(), oracle.c_bag_sum(tab, idx, off))


@pytest.mark.parametrize("dim,dtype", [(1, np.float32), (2, np.float32), (3, np.float32), (10, np.float32),
                                       (100, np.float32), (257, np.float32), (300, np.float32),
                                       (512, np.float32), (1000, np.float32), (2, np.float16), (5, np.float16),
                                       (100, np.float16), (1030, np.float16), (10, np.int32), (3, np.int32)])
@pytest.mark.parametrize("itype", [np.uint32, np.int64])
def test_any_row_width(pel, eng, oracle, dim, dtype, itype):
    """Rows that are not 16-byte multiples (dlrm_s_pytorch.py's default sparse feature size is 2) or
    are wider than 1 KiB run on the element-per-thread kernel: ragged bags, empty bags, the last bag
    running to n_indices, bit-exact against the oracle for fp32 / fp16 / fixed-point tables."""
    rng = np.random.default_rng(dim * 7 + np.dtype(dtype).itemsize)
    rows, n_bags = 777, 301
    off, n = pel.workloads.ragged_offsets(rng, n_bags, 7, dtype=itype)
    idx = rng.integers(0, rows, size=n).astype(itype)
    if dtype == np.int32:
        tab = rng.integers(-2**31, 2**31 - 1, size=(rows, dim), dtype=np.int64).astype(np.int32)
        eng.load_table(40, tab, dtype=pel.EMB_FIXED32)
        want = oracle.c_lookup_fixed32(tab, idx.astype(np.uint32), off.astype(np.uint32))
    else:
        tab = rng.standard_normal((rows, dim)).astype(dtype)
        eng.load_table(40, tab)
        want = oracle.c_bag_sum(tab, idx, off)
    eng.reset_stats()
    got = eng.lookup(40, idx, off)
    assert got.shape == (n_bags, dim) and np.array_equal(got, want)
    rb = dim * np.dtype(dtype).itemsize
    assert eng.stats()["n_launches_by_kind"][3] == int(rb % 16 != 0 or rb > 1024)   # the any-dim kernels
    # fixed pooling (no offsets array) and a fused call mixing this table with a 16-byte-multiple one
    L = 3
    idx2 = rng.integers(0, rows, size=n_bags * L).astype(itype)
    off2 = (np.arange(n_bags) * L).astype(itype)
    tab16 = rng.standard_normal((50, 16)).astype(np.float32)
    eng.load_table(41, tab16)
    idx16 = rng.integers(0, 50, size=n_bags * L).astype(itype)
    outs = eng.lookup_batched([40, 41], [idx2, idx16], [off2, off2])
    if dtype == np.int32:
        assert np.array_equal(outs[0], oracle.c_lookup_fixed32(tab, idx2.astype(np.uint32), off2.astype(np.uint32)))
    else:
        assert np.array_equal(outs[0], oracle.c_bag_sum(tab, idx2, off2))
    assert np.array_equal(outs[1], oracle.c_bag_sum(tab16, idx16, off2))


def test_compat_lookup_with_ten_columns(pel, oracle):
    """populate_mram / lookup with NR_COLS = 10 (40-byte rows): the reference allocates one DPU per
    column for any NR_COLS; here such tables take the element-per-thread kernel."""
    from importlib import import_module
    compat = import_module("pim-embedding-lookup_amd.compat")
    T, Cc, B, Lx, rows = 3, 10, 16, 5, 200
    rng = np.random.default_rng(10)
    compat.reset()
    compat.configure(nr_tables=T, nr_cols=Cc, max_nr_batches=B, max_indices_per_batch=Lx)
    tabs = [rng.integers(-10**9, 10**9, size=(rows, Cc)).astype(np.int32) for _ in range(T)]
    h = compat.populate(tabs)
    idx = [rng.integers(0, rows, size=B * Lx).astype(np.uint32) for _ in range(T)]
    off = [(np.arange(B) * Lx).astype(np.uint32) for _ in range(T)]
    res = compat.lookup(h, idx, off, nr_cols=Cc)
    for t in range(T):
        assert np.array_equal(res[t], oracle.c_lookup_fixed32(tabs[t], idx[t], off[t]))
    compat.reset()


def test_transient_launch_shapes_cycle_through_the_map_cache(pel, eng, oracle):
    """Plan-less multi-table launches big enough for the XCD-aware map (>= 131072 one-hot bags): the
    engine caches the map per launch shape (8 shapes).  Twelve different shapes, each called twice in
    rotation, force evictions and re-builds; every result is checked."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(99)
    tabs = [rng.standard_normal((r, 16)).astype(np.float32) for r in (5000, 300)]
    eng.load_table(52, tabs[0])
    eng.load_table(53, tabs[1])
    shapes = [(70_000 + 64 * k, 66_000 + 128 * k) for k in range(12)]
    for rep in range(2):
        for (b0, b1) in shapes:
            idx = [rng.integers(0, 5000, size=b0).astype(np.int64), rng.integers(0, 300, size=b1).astype(np.int64)]
            off = [np.arange(b0, dtype=np.int64), np.arange(b1, dtype=np.int64)]
            outs = eng.lookup_batched([52, 53], [torch.from_numpy(i).to(dev) for i in idx],
                                      [torch.from_numpy(o).to(dev) for o in off])
            torch.cuda.synchronize()
            for t in range(2):
                assert np.array_equal(outs[t].cpu().numpy(), tabs[t][idx[t]])


@pytest.mark.parametrize("dim,dtype", [(16, np.float32), (128, np.float32), (64, np.float16), (24, np.float32),
                                       (8, np.int32), (256, np.float32)])
def test_hot_rows_in_lds_do_not_change_results(pel, eng, oracle, dim, dtype):
    """emb_set_hot_rows: pooled Zipf lookups served partly from LDS are bit-identical to the oracle,
    for every dtype; duplicates / out-of-range ids in the hint are ignored; ragged bags with empties;
    a second table without a hint shares the launch; clearing the hint restores the plain kernel."""
    import torch
    rng = np.random.default_rng(dim)
    rows, n_bags = 20_000, 3000
    if dtype == np.int32:
        tab = rng.integers(-2**31, 2**31 - 1, size=(rows, dim), dtype=np.int64).astype(np.int32)
        eng.load_table(44, tab, dtype=pel.EMB_FIXED32)
        ref = lambda i, o: oracle.c_lookup_fixed32(tab, i.astype(np.uint32), o.astype(np.uint32))
    else:
        tab = rng.standard_normal((rows, dim)).astype(dtype)
        eng.load_table(44, tab)
        ref = lambda i, o: oracle.c_bag_sum(tab, i, o)
    tab2 = rng.standard_normal((500, dim)).astype(np.float32)
    if dtype == np.float32:
        eng.load_table(45, tab2)
    off, n = pel.workloads.ragged_offsets(rng, n_bags, 40, dtype=np.uint32)
    idx = pel.workloads.zipf_indices(rng, rows, n)
    hot = pel.workloads.top_rows(idx, 300)                      # more than fit: the engine keeps what fits
    hint = np.concatenate([hot[:5], hot, np.array([rows + 7, 2**40], dtype=np.uint64)])
    eng.set_hot_rows(44, hint)
    want = ref(idx, off)
    eng.reset_stats()
    assert np.array_equal(eng.lookup(44, idx, off), want)
    assert eng.stats()["n_launches_by_kind"] == [0, 0, 0, 0, 1]      # the LDS hot-row kernel ran
    if dtype == np.float32:
        idx2 = rng.integers(0, 500, size=n).astype(np.uint32)
        outs = eng.lookup_batched([44, 45], [idx, idx2], [off, off])
        assert np.array_equal(outs[0], want) and np.array_equal(outs[1], oracle.c_bag_sum(tab2, idx2, off))
    # int64 indices on device tensors, fixed pooling
    dev = torch.device("cuda", 0)
    L = 32
    idx3 = pel.workloads.zipf_indices(rng, rows, n_bags * L).astype(np.int64)
    off3 = (np.arange(n_bags) * L).astype(np.int64)
    got = eng.lookup(44, torch.from_numpy(idx3).to(dev), torch.from_numpy(off3).to(dev))
    assert np.array_equal(got.cpu().numpy(), ref(idx3, off3))
    # a plan built on the hinted table is refused once the hint changes
    d_idx, d_off = torch.from_numpy(idx3).to(dev), torch.from_numpy(off3).to(dev)
    plan = eng.plan([44], [d_idx], [d_off])
    plan.launch()
    torch.cuda.synchronize()
    assert np.array_equal(plan.outputs[0].cpu().numpy(), ref(idx3, off3))
    eng.set_hot_rows(44, [])
    with pytest.raises(pel.PimembError):
        plan.launch()
    plan.destroy()
    assert np.array_equal(eng.lookup(44, idx, off), want)


def test_hot_rows_dropped_when_the_table_is_reloaded(pel, eng, oracle):
    rng = np.random.default_rng(4)
    tab = rng.standard_normal((1000, 32)).astype(np.float32)
    eng.load_table(46, tab)
    off, n = pel.workloads.ragged_offsets(rng, 500, 20, dtype=np.uint32)
    idx = pel.workloads.zipf_indices(rng, 1000, n)
    eng.set_hot_rows(46, pel.workloads.top_rows(idx, 64))
    assert np.array_equal(eng.lookup(46, idx, off), oracle.c_bag_sum(tab, idx, off))
    tab_b = (tab * 3.0 + 1.0).astype(np.float32)
    eng.load_table(46, tab_b)                                   # same shape, new contents: stale copy must go
    assert np.array_equal(eng.lookup(46, idx, off), oracle.c_bag_sum(tab_b, idx, off))


def test_lookups_from_several_threads(pel, eng, oracle):
    """Host-pointer calls (serialised inside the engine: one staging buffer) and device-pointer calls
    issued from four threads at once; every result is checked against the oracle."""
    import threading
    import torch
    dev = torch.device("cuda", 0)
    tab = np.random.default_rng(8).standard_normal((4000, 32)).astype(np.float32)
    eng.load_table(55, tab)
    errors = []

    def worker(seed, use_device):
        try:
            rng = np.random.default_rng(seed)
            stream = torch.cuda.Stream(dev) if use_device else None
            for it in range(30):
                off, n = pel.workloads.ragged_offsets(rng, 200 + it, 9, dtype=np.int64)
                idx = rng.integers(0, 4000, size=n).astype(np.int64)
                if use_device:
                    with torch.cuda.stream(stream):
                        got = eng.lookup(55, torch.from_numpy(idx).to(dev), torch.from_numpy(off).to(dev))
                    stream.synchronize()
                    got = got.cpu().numpy()
                else:
                    got = eng.lookup(55, idx, off)
                if not np.array_equal(got, oracle.c_bag_sum(tab, idx, off)):
                    errors.append((seed, it))
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))

    threads = [threading.Thread(target=worker, args=(s, s % 2 == 0)) for s in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("bags", [(70_000, 0, 3, 40_000, 0, 10), (90_000, 1), (5, 5, 5, 120_000), (30_000,) * 7,
                                  (0, 0, 110_000)])
def test_host_pointer_calls_in_the_pipelined_range(pel, eng, oracle, bags):
    """Host-pointer calls with 4-40 MB of pooled rows run zero-copy in up to four parts whose unpack
    overlaps the next part's kernel: skewed, empty and single-heavy table mixes, u32 and i64 indices."""
    rng = np.random.default_rng(len(bags) * 1000 + sum(bags) % 97)
    tabs = [rng.standard_normal((3000 + 17 * t, 16)).astype(np.float32) for t in range(len(bags))]
    for t, w in enumerate(tabs):
        eng.load_table(20 + t, w)
    for itype in (np.uint32, np.int64):
        idx, off = [], []
        for t, b in enumerate(bags):
            o, n = pel.workloads.ragged_offsets(rng, b, 3, dtype=itype) if b else (np.zeros(0, itype), 0)
            off.append(o)
            idx.append(rng.integers(0, tabs[t].shape[0], size=n).astype(itype))
        outs = eng.lookup_batched([20 + t for t in range(len(bags))], idx, off)
        for t in range(len(bags)):
            assert outs[t].shape == (bags[t], 16)
            if bags[t]:
                assert np.array_equal(outs[t], oracle.c_bag_sum(tabs[t], idx[t], off[t])), (t, itype)


def test_special_values_are_bit_exact(pel, eng, oracle):
    """fp32 / fp16 rows holding denormals, signed zeros, infinities and extreme magnitudes: the sums
    match the oracle bit for bit (no flush-to-zero, same rounding; NaN-producing mixes are left out
    because x86 and the GPU pick different NaN payloads)."""
    rng = np.random.default_rng(21)
    specials32 = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 3e-39, -2e-39, 1.1754944e-38, 3.4e38, -3.4e38, 1.0,
                           -1.0, 1e-7, 16777216.0, 16777217.0, np.inf], dtype=np.float32)
    tab = rng.choice(specials32, size=(4096, 16)).astype(np.float32)
    tab[::7] = rng.standard_normal((len(tab[::7]), 16)).astype(np.float32) * 1e-39       # denormal rows
    eng.load_table(57, tab)
    off, n = pel.workloads.ragged_offsets(rng, 3000, 9, dtype=np.uint32)
    idx = rng.integers(0, 4096, size=n).astype(np.uint32)
    want = oracle.c_bag_sum(tab, idx, off)
    got = eng.lookup(57, idx, off)
    ok = ~np.isnan(want)
    assert ok.mean() > 0.5 and np.array_equal(np.isnan(got), ~ok)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])
    specials16 = np.array([0.0, -0.0, 6e-8, -6e-8, 6.1e-5, 65504.0, -65504.0, 1.0, 0.333, np.inf], dtype=np.float16)
    tab16 = rng.choice(specials16, size=(2048, 24)).astype(np.float16)
    eng.load_table(58, tab16)
    idx16 = rng.integers(0, 2048, size=n).astype(np.uint32)
    want = oracle.c_bag_sum(tab16, idx16, off)
    got = eng.lookup(58, idx16, off)
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])


def test_native_exchange_single_rank(pel, eng):
    """emb_comm_*: grouped ncclSend/ncclRecv issued from the C side (one rank, self exchange): byte
    ranges land where the offsets say, ordered on the stream between two engine launches."""
    import torch
    dev = torch.device("cuda", 0)
    try:
        ex = pel.NativeExchange(eng, 0, 1, lambda raw: raw)
    except pel.PimembError as e:
        if e.code == pel.lib.EMB_ERR_UNSUPPORTED:
            pytest.skip("librccl.so not available")
        raise
    w = torch.randn(5000, 16, device=dev)
    eng.load_table(59, w)
    B = 20_000
    idx = torch.randint(0, 5000, (B,), dtype=torch.int32, device=dev)
    off = torch.arange(B, dtype=torch.int32, device=dev)
    send = torch.empty((B, 16), device=dev)
    recv = torch.zeros((B + 3, 16), device=dev)
    plan = eng.plan([59], [idx], [off], [send])
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        plan.launch(s.cuda_stream)
        ex.all_to_all(send.data_ptr(), [0, B * 64], recv.data_ptr() + 3 * 64, [0, B * 64], s.cuda_stream)
    s.synchronize()
    assert torch.equal(recv[3:], w[idx.long()]) and float(recv[:3].abs().sum()) == 0.0
    plan.destroy()
    ex.close()


@pytest.mark.parametrize("itype", [np.int64, np.int32])
def test_lookup_stacked_matches_per_table_lists(pel, eng, oracle, itype):
    """lookup_stacked: DLRM's stacked [T, N] indices / [T, B] offsets, one [T, B, dim] result."""
    import torch
    from importlib import import_module
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    rows = [50, 3000, 7, 12345]
    tabs = [rng.standard_normal((n, 32)).astype(np.float32) for n in rows]
    ids = [30 + t for t in range(4)]
    for t, w in zip(ids, tabs):
        eng.load_table(t, w)
    B, L = 513, 3
    idx = np.stack([rng.integers(0, n, size=B * L) for n in rows]).astype(itype)
    off = np.tile((np.arange(B) * L).astype(itype), (4, 1))
    out = eng.lookup_stacked(ids, torch.from_numpy(idx).to(dev), torch.from_numpy(off).to(dev))
    assert tuple(out.shape) == (4, B, 32)
    for t in range(4):
        ref_t = np.int64 if itype == np.int64 else np.uint32          # int32 bits are read as uint32
        assert np.array_equal(out[t].cpu().numpy(), oracle.c_bag_sum(tabs[t], idx[t].astype(ref_t), off[t].astype(ref_t)))
    with pytest.raises(ValueError):
        eng.lookup_stacked(ids, torch.from_numpy(idx[:3]).to(dev), torch.from_numpy(off).to(dev))
    hz = import_module("pim-embedding-lookup_amd.dlrm_harness")
    ebc = hz.EmbeddingBagCollection(rows, 32, weights=tabs)
    ly = ebc.apply_emb(torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev))
    assert len(ly) == 4 and all(torch.equal(ly[t], out[t]) for t in range(4))
    ebc.close()


def test_torch_modules_replace_nn_embeddingbag(pel, oracle):
    """torch_module.EmbeddingBag / FusedEmbeddingBags: swap nn.EmbeddingBag(mode="sum") modules of an
    emb_l one by one or all at once; same forward conventions (1-D input + offsets, 2-D input,
    include_last_offset), same numbers as torch on the CPU."""
    import torch
    from importlib import import_module
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    emb_l = torch.nn.ModuleList([torch.nn.EmbeddingBag(n, 16, mode="sum", sparse=True) for n in (1460, 583, 30000, 3)])
    ours = [tm.EmbeddingBag.from_torch(m) for m in emb_l]
    fused = tm.FusedEmbeddingBags(ours)
    rng = np.random.default_rng(0)
    lS_i, lS_o = [], []
    for m in emb_l:
        lens = rng.integers(0, 5, size=97)
        off = np.zeros(97, np.int64); off[1:] = np.cumsum(lens)[:-1]
        lS_o.append(torch.from_numpy(off))
        lS_i.append(torch.from_numpy(rng.integers(0, m.num_embeddings, size=int(lens.sum()))))
    want = [m(i, o) for m, i, o in zip(emb_l, lS_i, lS_o)]
    for k, mod in enumerate(ours):                                   # per-table drop-in
        got = mod(lS_i[k].to(dev), lS_o[k].to(dev))
        assert torch.equal(got.cpu(), want[k].detach())
    ly = fused([o.to(dev) for o in lS_o], [i.to(dev) for i in lS_i])    # one launch for all
    assert all(torch.equal(a.cpu(), b.detach()) for a, b in zip(ly, want))
    x2 = torch.from_numpy(rng.integers(0, 1460, size=(33, 4)))      # 2-D input: fixed-size bags
    assert torch.equal(ours[0](x2.to(dev)).cpu(), emb_l[0](x2).detach())
    ilo = torch.nn.EmbeddingBag.from_pretrained(emb_l[1].weight.detach(), mode="sum", include_last_offset=True)
    ours_ilo = tm.EmbeddingBag.from_torch(ilo)
    off_ilo = torch.cat([lS_o[1], torch.tensor([lS_i[1].numel()])])
    assert torch.equal(ours_ilo(lS_i[1].to(dev), off_ilo.to(dev)).cpu(), ilo(lS_i[1], off_ilo).detach())
    assert torch.equal(ours[2].weight.cpu(), emb_l[2].weight.detach())          # zero-copy view of the HBM table
    assert ours[2].weight.data_ptr() == ours[2].engine.table_info(ours[2].table_id)[0]
    with pytest.raises(NotImplementedError):
        tm.EmbeddingBag(10, 16, mode="mean")
    with pytest.raises(NotImplementedError):
        ours[0](lS_i[0].to(dev), lS_o[0].to(dev), per_sample_weights=torch.ones(lS_i[0].numel(), device=dev))
    stacked_i = torch.from_numpy(np.stack([rng.integers(0, m.num_embeddings, size=64) for m in emb_l])).to(dev)
    stacked_o = torch.arange(64, device=dev).repeat(4, 1)
    ly = fused(stacked_o, stacked_i)
    for k, m in enumerate(emb_l):
        assert torch.equal(ly[k].cpu(), m(stacked_i[k].cpu(), stacked_o[k].cpu()).detach())



def test_processed_kaggle_npz_through_the_harness(pel, tmp_path, capsys):
    """F2 on the GPU: a processed Criteo-Kaggle `.npz` (synthetic, the upstream layout: X_int, X_cat, y, counts)
    drives the HIP path -- (a) its batches through EmbeddingBagCollection.apply_emb against torch CPU
    nn.EmbeddingBag on the same checkpoint, bit for bit; (b) the reference's command line
    `--data-set=kaggle --processed-data-file=... --load-model=...` (README.md:6, upmem/run.sh:117-118) through
    dlrm_harness.main; (c) an index outside [0, counts[k]) is refused before anything is launched."""
    import torch
    from importlib import import_module
    hz = import_module("pim-embedding-lookup_amd.dlrm_harness")
    fm = import_module("pim-embedding-lookup_amd.formats")
    rng = np.random.default_rng(6)
    counts = np.array([1460, 583, 40_000, 305, 24, 3, 9000, 27], dtype=np.int32)
    N, m = 700, 16
    x_cat = np.stack([rng.integers(0, c, size=N) for c in counts], axis=1).astype(np.int32)
    npz = tmp_path / "kaggleAdDisplayChallenge_processed.npz"
    np.savez(npz, X_int=rng.integers(0, 9, size=(N, 13)), X_cat=x_cat, y=rng.integers(0, 2, size=N), counts=counts)
    tabs = [pel.workloads.dlrm_table(rng, int(c), m) for c in counts]
    ckpt = tmp_path / "model.pt"
    fm.save_dlrm_embedding_weights(str(ckpt), tabs)
    data = fm.CriteoKaggleNpz(str(npz))
    ebc = hz.EmbeddingBagCollection.from_checkpoint(str(ckpt))
    assert ebc.ln_emb == data.table_rows
    dev = torch.device("cuda", 0)
    bags = [torch.nn.EmbeddingBag.from_pretrained(torch.from_numpy(t), mode="sum") for t in tabs]
    n_batches = 0
    for lS_o, lS_i in data.batches(128):                          # 5 full batches + a ragged tail of 60
        ly = ebc.apply_emb([torch.from_numpy(o).to(dev) for o in lS_o], [torch.from_numpy(i).to(dev) for i in lS_i])
        for k in range(len(counts)):
            want = bags[k](torch.from_numpy(lS_i[k]), torch.from_numpy(lS_o[k]))
            assert torch.equal(ly[k].cpu(), want)
        n_batches += 1
    assert n_batches == 6
    ebc.close()
    rc = hz.main(["--arch-sparse-feature-size=16", "--data-generation=dataset", "--data-set=kaggle",
                  f"--processed-data-file={npz}", f"--load-model={ckpt}", "--mini-batch-size=128",
                  "--num-batches=8", "--inference-only", "--print-freq=1024"])
    out = capsys.readouterr().out
    assert rc == 0 and "apply_emb: 8 tables, m=16, batch 128" in out and "--print-freq=1024" in out
    # (c) a corrupted file: index == count
    bad = x_cat.copy(); bad[5, 2] = counts[2]
    np.savez(npz, X_cat=bad, counts=counts)
    with pytest.raises(ValueError):
        hz.main(["--data-set=kaggle", f"--processed-data-file={npz}", "--mini-batch-size=64", "--num-batches=2",
                 "--inference-only"])


def test_torch_modules_check_inputs_and_carry_state_dict(pel):
    """(1) an out-of-range index through the default EmbeddingBag.forward raises IndexError like
    nn.EmbeddingBag instead of reaching the unchecked kernel; trusted_inputs=True is the explicit fast path;
    (2) state_dict() / load_state_dict() carry `<prefix>weight` with nn.EmbeddingBag's keys and shapes, so a DLRM
    with swapped emb_l saves and loads the same checkpoint."""
    import torch
    from importlib import import_module
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ref = torch.nn.ModuleList([torch.nn.EmbeddingBag(n, 16, mode="sum") for n in (50, 7, 3000)])
    ours = torch.nn.ModuleList([tm.EmbeddingBag.from_torch(b) for b in ref])
    idx = torch.tensor([1, 2, 49, 50], dtype=torch.int64)
    off = torch.tensor([0, 2], dtype=torch.int64)
    with pytest.raises((IndexError, RuntimeError)):
        ref[0](idx, off)                                   # torch CPU refuses index 50 of a 50-row table ...
    with pytest.raises(IndexError):
        ours[0](idx.to(dev), off.to(dev))                  # ... and so does the drop-in, before any launch
    with pytest.raises(IndexError):
        ours[0](torch.tensor([0, -1], device=dev), torch.tensor([0], device=dev))
    with pytest.raises(IndexError):
        ours[0](torch.tensor([0, 1, 2], device=dev), torch.tensor([0, 5], device=dev))        # offset past the end
    fused = tm.FusedEmbeddingBags(list(ours))
    assert fused.trusted_inputs is False
    good_i = [torch.randint(0, b.num_embeddings, (12,), device=dev) for b in ref]
    good_o = [torch.arange(0, 12, 3, device=dev) for _ in ref]
    with pytest.raises(IndexError):
        fused(good_o, [good_i[0], good_i[1] + 7, good_i[2]])
    ly = fused(good_o, good_i)
    for k, b in enumerate(ref):
        assert torch.equal(ly[k].cpu(), b(good_i[k].cpu(), good_o[k].cpu()))
    ours[2].trusted_inputs = True
    assert torch.equal(ours[2](good_i[2], good_o[2]).cpu(), ref[2](good_i[2].cpu(), good_o[2].cpu()))
    # checkpoints
    sd_ref, sd = ref.state_dict(), ours.state_dict()
    assert list(sd) == list(sd_ref) == ["0.weight", "1.weight", "2.weight"]
    for k in sd:
        assert sd[k].shape == sd_ref[k].shape and torch.equal(sd[k].cpu(), sd_ref[k])
    new = torch.nn.ModuleList([torch.nn.EmbeddingBag(n, 16, mode="sum") for n in (50, 7, 3000)])
    ours.load_state_dict(new.state_dict(), strict=True)            # upstream checkpoint -> our modules
    for k, b in enumerate(new):
        assert torch.equal(ours[k].weight.cpu(), b.weight.detach())
        assert torch.equal(ours[k](good_i[k], good_o[k]).cpu(), b(good_i[k].cpu(), good_o[k].cpu()))
    new2 = torch.nn.ModuleList([torch.nn.EmbeddingBag(n, 16, mode="sum") for n in (50, 7, 3000)])
    new2.load_state_dict(ours.state_dict(), strict=True)           # our modules -> upstream model
    assert all(torch.equal(a.weight.detach(), b.weight.detach()) for a, b in zip(new, new2))
    with pytest.raises(RuntimeError):
        ours.load_state_dict({"0.weight": torch.zeros(5, 16), "1.weight": sd_ref["1.weight"], "2.weight": sd_ref["2.weight"]})


def test_many_tables_in_one_fused_launch(pel, oracle):
    """More tables per fused call than any round-1 test launched (26): 80 one-hot tables through the wave-batch
    kernels and their XCD-aware workgroup map, 72 ragged pooled tables through the lane-group kernel, and a mixed
    96-descriptor call (three dtypes / dims -> several launch groups), every table against the oracle."""
    rng = np.random.default_rng(80)
    e = pel.EmbeddingEngine(device=0, max_tables=128)
    # (a) 80 tables, one index per bag, sizes from 3 rows to 2M rows, 2111 bags each (168 880 bags: wave-batch + map)
    sizes = [int(x) for x in np.exp(rng.uniform(np.log(3), np.log(2e6), size=80))]
    tabs = [pel.workloads.dlrm_table(rng, n, 16) for n in sizes]
    for t, w in enumerate(tabs):
        e.load_table(t, w)
    import torch
    dev = torch.device("cuda", 0)
    B = 2111
    idx = [pel.workloads.uniform_indices(rng, n, B) for n in sizes]
    off = [np.arange(B, dtype=np.uint32)] * 80
    d_off = torch.arange(B, dtype=torch.int32, device=dev)
    outs = e.lookup_batched(list(range(80)), [torch.from_numpy(i.view(np.int32)).to(dev) for i in idx], [d_off] * 80)
    torch.cuda.synchronize()
    kinds = e.stats()["n_launches_by_kind"]
    assert kinds[0] + kinds[2] == 1 and sum(kinds) == 1   # ONE wave-batch launch over the 80 tables
    for t in range(80):
        assert np.array_equal(outs[t].cpu().numpy(), oracle.c_bag_sum(tabs[t], idx[t], off[t])), f"one-hot table {t}"
    # the same through host pointers (staged, split into pipelined parts)
    outs_h = e.lookup_batched(list(range(80)), idx, off)
    assert all(np.array_equal(outs_h[t], outs[t].cpu().numpy()) for t in range(80))
    # (b) 72 of them with ragged bags (0..24 indices, some empty), device-resident, int64
    idx2, off2 = [], []
    for t in range(72):
        o, n_idx = pel.workloads.ragged_offsets(rng, 301 + t, 24, p_empty=0.2, dtype=np.int64)
        off2.append(o)
        idx2.append(rng.integers(0, sizes[t], size=n_idx).astype(np.int64))
    outs2 = e.lookup_batched(list(range(72)), [torch.from_numpy(i).to(dev) for i in idx2],
                             [torch.from_numpy(o).to(dev) for o in off2])
    torch.cuda.synchronize()
    for t in range(72):
        assert np.array_equal(outs2[t].cpu().numpy(), oracle.c_bag_sum(tabs[t], idx2[t], off2[t])), f"pooled table {t}"
    # (c) 96 descriptors of three shapes in ONE call (tables may repeat): fp32 dim 16, fp16 dim 64, fixed-point dim 8
    h16 = [rng.standard_normal((500 + 37 * k, 64)).astype(np.float16) for k in range(8)]
    fx = [rng.integers(-2**31, 2**31 - 1, size=(90 + k, 8), dtype=np.int64).astype(np.int32) for k in range(8)]
    for k in range(8):
        e.load_table(100 + k, h16[k])
        e.load_table(110 + k, fx[k])
    ids, ii, oo, want = [], [], [], []
    for r in range(96):
        kind, k = r % 3, (r // 3) % 8
        tid, tab = [(k, tabs[k]), (100 + k, h16[k]), (110 + k, fx[k])][kind]
        o, n_idx = pel.workloads.ragged_offsets(rng, 40 + r, 6, p_empty=0.1)
        i = rng.integers(0, tab.shape[0], size=n_idx).astype(np.uint32)
        ids.append(tid); ii.append(i); oo.append(o)
        want.append(oracle.c_lookup_fixed32(tab, i, o) if kind == 2 else oracle.c_bag_sum(tab, i, o))
    got = e.lookup_batched(ids, ii, oo)
    for r in range(96):
        assert np.array_equal(got[r], want[r]), f"descriptor {r}"
    e.close()


def test_full_size_c5_share_properties(pel, oracle):
    """BASELINE configs[4], one GPU's share at its own shape: 64 tables x 30M rows x dim 64 fp16 (245.8 GB resident),
    B = 16384 bags per table, pooling 32, Zipf(1.2) on even tables / uniform on odd ones, ONE fused 64-table launch.
    Size-independent properties (the oracle is only sampled at this size):
      (1) idempotence: a second launch leaves all 64 outputs unchanged;
      (2) the hot-row hint (emb_set_hot_rows on the Zipf tables -> LDS-staged kernel) changes no bit;
      (3) linearity: a table scaled by 2 (exact in fp16) gives exactly 2x the pooled rows;
      (4) the oracle on 32 sampled bags of every table (rows copied back from HBM);
      (5) eight tables bag for bag against an in-order torch gather-sum on the GPU, bit for bit."""
    import torch
    dev = torch.device("cuda", 0)
    if torch.cuda.get_device_properties(dev).total_memory < 270e9:
        pytest.skip("needs the 288 GB of an MI355X")
    T, n, D, B, L = 64, 30_000_000, 64, 16384, 32
    e = pel.EmbeddingEngine(device=0, max_tables=T + 2)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    a = float(np.sqrt(1.0 / n))
    for t in range(T):
        w = torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-a, a, generator=g).to(torch.float16)
        e.load_table(t, w)
        if t < 2:
            e.load_table(T + t, w * 2.0)
        del w
    torch.cuda.empty_cache()
    rng = np.random.default_rng(3)
    idx_h = [(pel.workloads.zipf_indices if t % 2 == 0 else pel.workloads.uniform_indices)(rng, n, B * L) for t in range(T)]
    idx = [torch.from_numpy(i.view(np.int32)).to(dev) for i in idx_h]
    off = torch.from_numpy(pel.workloads.fixed_offsets(B, L).view(np.int32)).to(dev)
    plan = e.plan(list(range(T)), idx, [off] * T)
    plan.launch()
    torch.cuda.synchronize()
    assert e.stats()["n_launches_by_kind"][1] == 1                      # one lane-group launch for all 64 tables
    first = [o.clone() for o in plan.outputs]
    plan.launch()
    torch.cuda.synchronize()
    for t in range(T):
        assert torch.equal(plan.outputs[t], first[t]), f"table {t}: second launch differs"
    # (3) linearity on tables 0 (Zipf) and 1 (uniform)
    lin = e.lookup_batched([T, T + 1], idx[:2], [off, off])
    torch.cuda.synchronize()
    assert torch.equal(lin[0], first[0] * 2.0) and torch.equal(lin[1], first[1] * 2.0)
    # (4) + (5)
    for t in range(T):
        w = e.table_tensor(t)
        sel = np.unique(rng.integers(0, B, size=32))
        pos = (sel[:, None] * L + np.arange(L)[None, :]).reshape(-1)
        idx_s = idx_h[t][pos].astype(np.int64)
        uniq, inv = np.unique(idx_s, return_inverse=True)
        small = w[torch.from_numpy(uniq).to(dev)].cpu().numpy()           # fp16 rows
        want = oracle.c_bag_sum(small, inv.astype(np.int64), np.arange(sel.shape[0], dtype=np.int64) * L)
        assert np.array_equal(first[t][torch.from_numpy(sel).to(dev)].cpu().numpy(), want), f"table {t} vs oracle"
        if t % 8 == 0 or t % 8 == 5:
            rows = w[idx[t].long()].float().view(B, L, D)
            acc = rows[:, 0, :] + 0.0
            for j in range(1, L):
                acc = acc + rows[:, j, :]
            assert torch.equal(first[t], acc), f"table {t} vs the in-order torch sum"
            del rows, acc
    # (2) hot rows on the Zipf tables: same bits through the LDS-staged kernel
    plan.destroy()
    for t in range(0, T, 2):
        e.set_hot_rows(t, pel.workloads.top_rows(idx_h[t], 100))
    plan = e.plan(list(range(T)), idx, [off] * T)
    plan.launch()
    torch.cuda.synchronize()
    assert e.stats()["n_launches_by_kind"][4] == 1                      # the hot-row kernel ran
    for t in range(T):
        assert torch.equal(plan.outputs[t], first[t]), f"table {t}: the hot-row hint changed the result"
    plan.destroy()
    e.close()


def test_full_size_c3_properties(pel, oracle):
    """BASELINE configs[2] at the size bench.py runs it: 48 tables x 10M rows x dim 128 fp32 (245.8 GB resident; the 64
    tables as written need 327.7 GB), B = 16384, pooling 32, Zipf(1.2), ONE fused 48-table launch (round 1 only ran one
    table of this shape).  Idempotence; exact linearity on a x2 copy of table 0; the oracle on 32 sampled bags of every
    table; six tables bag for bag against an in-order torch gather-sum (bit for bit); bag-halves additivity <= 1e-6."""
    import torch
    dev = torch.device("cuda", 0)
    if torch.cuda.get_device_properties(dev).total_memory < 270e9:
        pytest.skip("needs the 288 GB of an MI355X")
    T, n, D, B, L = 48, 10_000_000, 128, 16384, 32
    e = pel.EmbeddingEngine(device=0, max_tables=T + 1)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    a = float(np.sqrt(1.0 / n))
    for t in range(T):
        w = torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-a, a, generator=g)
        e.load_table(t, w)
        if t == 0:
            e.load_table(T, w * 2.0)
        del w
    torch.cuda.empty_cache()
    rng = np.random.default_rng(2)
    idx_h = [pel.workloads.zipf_indices(rng, n, B * L) for _ in range(T)]
    idx = [torch.from_numpy(i.view(np.int32)).to(dev) for i in idx_h]
    off = torch.from_numpy(pel.workloads.fixed_offsets(B, L).view(np.int32)).to(dev)
    plan = e.plan(list(range(T)), idx, [off] * T)
    plan.launch()
    torch.cuda.synchronize()
    assert e.stats()["n_launches_by_kind"][1] == 1
    first = [o.clone() for o in plan.outputs]
    plan.launch()
    torch.cuda.synchronize()
    assert all(torch.equal(plan.outputs[t], first[t]) for t in range(T))
    assert torch.equal(e.lookup(T, idx[0], off), first[0] * 2.0)
    off16 = torch.from_numpy(pel.workloads.fixed_offsets(2 * B, L // 2).view(np.int32)).to(dev)
    halves = e.lookup(3, idx[3], off16)
    assert float((halves[0::2] + halves[1::2] - first[3]).abs().max()) <= 1e-6
    for t in range(T):
        w = e.table_tensor(t)
        sel = np.unique(rng.integers(0, B, size=32))
        pos = (sel[:, None] * L + np.arange(L)[None, :]).reshape(-1)
        uniq, inv = np.unique(idx_h[t][pos].astype(np.int64), return_inverse=True)
        small = w[torch.from_numpy(uniq).to(dev)].cpu().numpy()
        want = oracle.c_bag_sum(small, inv.astype(np.int64), np.arange(sel.shape[0], dtype=np.int64) * L)
        assert np.array_equal(first[t][torch.from_numpy(sel).to(dev)].cpu().numpy(), want), f"table {t} vs oracle"
        if t % 8 == 1:
            rows = w[idx[t].long()].view(B, L, D)
            acc = rows[:, 0, :] + 0.0
            for j in range(1, L):
                acc = acc + rows[:, j, :]
            assert torch.equal(first[t], acc), f"table {t} vs the in-order torch sum"
            del rows, acc
    plan.destroy()
    e.close()


@pytest.mark.parametrize("L", [1, 32])
def test_full_size_c4_share_properties(pel, oracle, L):
    """BASELINE configs[3] at the size one of its 8 ranks runs (`bench.py --workload c4 [--pooling 32]`): the 1/8 row
    shards of the 8 Terabyte-shaped tables above 64 MiB + the 18 small tables whole, 56.6 GB, dim 128 fp32, B = 16384
    bags per table, uniform indices, one and 32 indices per bag, ONE fused 26-table launch each (wave-batch kernel for
    L = 1, lane-group kernel for L = 32).  The loop being sharded is emb_dpu_lookup.c:106-116.
      (1) idempotence: a second launch leaves all 26 outputs unchanged;
      (2) linearity: x2 copies of a row shard and of a small table give exactly 2x the pooled rows;
      (3) the oracle on 32 sampled bags of EVERY table (rows copied back from HBM): bit for bit;
      (4) four row shards and two small tables bag for bag against the in-order torch gather-sum: bit for bit."""
    import torch
    dev = torch.device("cuda", 0)
    if torch.cuda.get_device_properties(dev).total_memory < 100e9:
        pytest.skip("needs 60 GB of HBM for the tables")
    D, B = pel.workloads.TERABYTE_DIM, pel.workloads.TERABYTE_BATCH
    full = pel.workloads.TERABYTE_ROWS
    split = [n * D * 4 > (64 << 20) for n in full]
    rows = [(-(-n // 8) if s else n) for n, s in zip(full, split)]
    assert sum(split) == 8 and D == 128 and B == 16384 and 56e9 < sum(rows) * D * 4 < 57.5e9
    T = len(rows)
    big = max(range(T), key=lambda t: rows[t])
    small = min((t for t in range(T) if not split[t]), key=lambda t: -rows[t])
    e = pel.EmbeddingEngine(device=0, max_tables=T + 2)
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    for t, n in enumerate(rows):
        a = float(np.sqrt(1.0 / full[t]))
        w = torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-a, a, generator=g)
        e.load_table(t, w)
        if t == big:
            e.load_table(T, w * 2.0)
        if t == small:
            e.load_table(T + 1, w * 2.0)
        del w
    torch.cuda.empty_cache()
    rng = np.random.default_rng(40 + L)
    idx_h = [pel.workloads.uniform_indices(rng, n, B * L) for n in rows]
    idx = [torch.from_numpy(i.view(np.int32)).to(dev) for i in idx_h]
    off = torch.from_numpy(pel.workloads.fixed_offsets(B, L).view(np.int32)).to(dev)
    plan = e.plan(list(range(T)), idx, [off] * T)
    plan.launch()
    torch.cuda.synchronize()
    kinds = e.stats()["n_launches_by_kind"]
    assert sum(kinds) == 1 and kinds[0 if L == 1 else 1] == 1           # ONE launch: wave-batch (one-hot) / lane-group (pooled)
    first = [o.clone() for o in plan.outputs]
    plan.launch()
    torch.cuda.synchronize()
    assert all(torch.equal(plan.outputs[t], first[t]) for t in range(T))
    lin = e.lookup_batched([T, T + 1], [idx[big], idx[small]], [off, off])
    torch.cuda.synchronize()
    assert torch.equal(lin[0], first[big] * 2.0) and torch.equal(lin[1], first[small] * 2.0)
    exact = [t for t in range(T) if split[t]][::2] + [small, min(range(T), key=lambda t: rows[t])]
    for t in range(T):
        w = e.table_tensor(t)
        sel = np.unique(rng.integers(0, B, size=32))
        pos = (sel[:, None] * L + np.arange(L)[None, :]).reshape(-1)
        uniq, inv = np.unique(idx_h[t][pos].astype(np.int64), return_inverse=True)
        rows_s = w[torch.from_numpy(uniq).to(dev)].cpu().numpy()
        want = oracle.c_bag_sum(rows_s, inv.astype(np.int64), np.arange(sel.shape[0], dtype=np.int64) * L)
        assert np.array_equal(first[t][torch.from_numpy(sel).to(dev)].cpu().numpy(), want), f"table {t} vs oracle"
        if t in exact:
            r = w[idx[t].long()].view(B, L, D)
            acc = r[:, 0, :] + 0.0
            for j in range(1, L):
                acc = acc + r[:, j, :]
            assert torch.equal(first[t], acc), f"table {t} vs the in-order torch sum"
            del r, acc
    nb, ni = plan.bytes()[1:]
    assert (nb, ni) == (T * B, T * B * L)
    plan.destroy()
    e.close()


@pytest.mark.parametrize("marshal", ["c-helper", "python"])
def test_plan_cache_of_per_table_list_calls(pel, oracle, marshal, monkeypatch):
    """Both ways of unpacking the tensor lists -- the _pimemb_marshal C helper (must be built: it is what runs by default)
    and the Python loop it replaces -- through the same scenario.
    lookup_batched over per-table LISTS of torch tensors, as an apply_emb loop calls it: new list and tensor objects
    every batch, the same addresses underneath.  From the third identical call on it is one emb_plan_launch of a cached
    plan -- and must behave exactly like the ordinary call: new index VALUES in the same buffers are picked up, a reloaded
    table is picked up (the stale plan is refused and dropped), other lengths / addresses / dtypes are other calls, caller
    outputs are written in place, and plan_cache_size = 0 switches it off.  Always against the oracle, bit for bit."""
    import torch
    from importlib import import_module
    engine_mod = import_module("pim-embedding-lookup_amd.engine")
    if marshal == "python":
        monkeypatch.setattr(engine_mod, "_MARSHAL", [None])
    else:
        monkeypatch.setattr(engine_mod, "_MARSHAL", [False])
        assert engine_mod._marshal() is not None, "pim-embedding-lookup_amd/lib/_pimemb_marshal.so is not built"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    rows, D, B = [5000, 33, 70_000], 16, 700
    e = pel.EmbeddingEngine(device=0, max_tables=4)
    tabs = [pel.workloads.dlrm_table(rng, n, D) for n in rows]
    for t, w in enumerate(tabs):
        e.load_table(t, w)
    L = [3, 1, 5]
    idx = [torch.from_numpy(rng.integers(0, n, size=B * l)).to(dev) for n, l in zip(rows, L)]
    off = [torch.arange(0, B * l, l, dtype=torch.int64, device=dev) for l in L]

    def call(outs=None, ii=None, oo=None):
        ii, oo = ii or idx, oo or off
        return e.lookup_batched([0, 1, 2], [x.view(-1) for x in ii], [x.view(-1) for x in oo], outs)   # fresh objects

    def want(ii=None, oo=None):
        ii, oo = ii or idx, oo or off
        return [oracle.c_bag_sum(tabs[t], ii[t].cpu().numpy(), oo[t].cpu().numpy()) for t in range(3)]

    def same(got, ref):
        return all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, ref))

    for _ in range(4):
        assert same(call(), want())
    assert e.plan_cache_hits >= 1 and len(e._plan_cache) == 1
    hits = e.plan_cache_hits
    for x, n in zip(idx, rows):                      # new index values, same buffers: the cached plan reads them
        x.copy_(torch.from_numpy(rng.integers(0, n, size=x.numel())).to(dev))
    assert same(call(), want()) and e.plan_cache_hits == hits + 1
    tabs[1] = pel.workloads.dlrm_table(rng, rows[1], D)          # reloaded table, same shape: same allocation, plan still valid
    e.load_table(1, tabs[1])
    assert same(call(), want())
    tabs[1] = pel.workloads.dlrm_table(rng, 90, D)               # other shape: re-allocated, the plan is stale -> dropped
    e.load_table(1, tabs[1])
    idx[1].copy_(torch.from_numpy(rng.integers(0, 90, size=idx[1].numel())).to(dev))
    hits = e.plan_cache_hits
    assert same(call(), want()) and e.plan_cache_hits == hits and len(e._plan_cache) == 0
    for _ in range(3):
        assert same(call(), want())
    assert len(e._plan_cache) == 1
    # shorter inputs in the same buffers: another signature, the ordinary call
    ii = [x[:x.numel() // 2] for x in idx]
    oo = [x[:x.numel() // 2] for x in off]
    assert same(call(ii=ii, oo=oo), want(ii, oo))
    # int32 copies: other addresses and another index width
    i32, o32 = [x.to(torch.int32) for x in idx], [x.to(torch.int32) for x in off]
    for _ in range(3):
        assert same(call(ii=i32, oo=o32), want())
    # caller-provided outputs are part of the signature and are written in place
    outs = [torch.full((B, D), 7.0, device=dev) for _ in range(3)]
    for _ in range(4):
        for o in outs:
            o.fill_(7.0)
        res = call(outs=outs)
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, outs)) and same(outs, want())
    # a live result keeps its memory: the next call gets another address (a miss) and must not overwrite it
    keep = call()
    ref = [k.clone() for k in keep]
    idx[0].copy_(torch.from_numpy(rng.integers(0, rows[0], size=idx[0].numel())).to(dev))
    assert same(call(), want()) and all(torch.equal(k, r) for k, r in zip(keep, ref))
    # the stacked form ([T, N] / [T, B] tensors) goes through the same cache
    si = torch.stack([torch.from_numpy(rng.integers(0, 33, size=4 * B)).to(dev) for _ in range(2)])
    so = torch.stack([torch.arange(0, 4 * B, 4, dtype=torch.int64, device=dev)] * 2)
    sout = torch.empty((2, B, D), device=dev)
    hits = e.plan_cache_hits
    for rep in range(4):
        si.copy_(torch.from_numpy(rng.integers(0, 33, size=(2, 4 * B))).to(dev))
        got = e.lookup_stacked([1, 1], si, so, out=sout)
        for r in range(2):
            assert np.array_equal(got[r].cpu().numpy(), oracle.c_bag_sum(tabs[1], si[r].cpu().numpy(), so[r].cpu().numpy()))
    assert e.plan_cache_hits == hits + 2
    # checked calls never use the cache, and refuse bad input whatever is cached
    idx[2][5] = rows[2]
    with pytest.raises(IndexError):
        e.lookup_batched([0, 1, 2], idx, off, check=True)
    idx[2][5] = 0
    assert same(e.lookup_batched([0, 1, 2], idx, off, check=True), want())
    e.plan_cache_size = 0
    hits = e.plan_cache_hits
    for _ in range(3):
        assert same(call(), want())
    assert e.plan_cache_hits == hits
    e.close()                                        # destroys the cached plans first (emb_destroy refuses live plans)


def test_checked_lookup_is_ordered_on_the_callers_stream(pel, oracle):
    """emb_lookup_batched_checked / emb_validate_inputs_on run on the stream they are given: indices produced on a side
    stream just before the call are what gets checked (round 2 validated on the default stream whatever the caller's)."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    e = pel.EmbeddingEngine(device=0, max_tables=2)
    tab = pel.workloads.dlrm_table(rng, 1000, 32)
    e.load_table(0, tab)
    side = torch.cuda.Stream(dev)
    big = torch.zeros(1 << 24, device=dev)
    idx = torch.full((4096,), 5000, dtype=torch.int64, device=dev)          # out of range until the side stream fixes it
    off = torch.arange(0, 4096, 4, dtype=torch.int64, device=dev)
    good = torch.from_numpy(rng.integers(0, 1000, size=4096)).to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            big.add_(1.0)                        # keep the side stream busy, then produce the indices on it
        idx.copy_(good)
        out = e.lookup_batched([0], [idx], [off], check=True)[0]
        assert e.validate([0], [idx], [off]) == 0
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), oracle.c_bag_sum(tab, good.cpu().numpy(), off.cpu().numpy()))
    e.close()


def test_checked_lookup_with_descriptors_copied_to_hbm():
    """PIMEMB_DESC_MODE=copy (launch images staged into HBM instead of read from the pinned ring): the validation kernel
    must disarm the HBM twin the lookup kernels read, and still report through the pinned words.  Own process (the mode is
    read at engine creation)."""
    import subprocess
    import sys
    import textwrap
    script = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import numpy as np, torch
        import pim_embedding_lookup_amd as pel
        from oracle import oracle
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(3)
        e = pel.EmbeddingEngine(device=0, max_tables=4)
        tabs = [pel.workloads.dlrm_table(rng, n, 16) for n in (700, 90_000)]
        for t, w in enumerate(tabs):
            e.load_table(t, w)
        idx = [torch.from_numpy(rng.integers(0, n, size=6000)).to(dev) for n in (700, 90_000)]
        off = [torch.arange(0, 6000, 3, dtype=torch.int64, device=dev) for _ in range(2)]
        outs = [torch.full((2000, 16), 7.0, device=dev) for _ in range(2)]
        idx[1][4321] = 90_000
        try:
            e.lookup_batched([0, 1], idx, off, outs, check=True)
            raise SystemExit("bad index accepted")
        except IndexError as ex:
            assert str(ex).startswith("1 index")
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs)
        assert e.validate([0, 1], idx, off) == 1
        idx[1][4321] = 89_999
        got = e.lookup_batched([0, 1], idx, off, outs, check=True)
        for t in range(2):
            assert np.array_equal(got[t].cpu().numpy(), oracle.c_bag_sum(tabs[t], idx[t].cpu().numpy(), off[t].cpu().numpy()))
        # host pointers through the checked entry point
        hi, ho = idx[0].cpu().numpy(), off[0].cpu().numpy()
        assert np.array_equal(e.lookup(0, hi, ho, check=True), oracle.c_bag_sum(tabs[0], hi, ho))
        hi[5] = 700
        try:
            e.lookup(0, hi, ho, check=True)
            raise SystemExit("bad host index accepted")
        except IndexError:
            pass
        e.close()
        print("copy-mode checked ok")
    """ % ROOT)
    res = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PIMEMB_DESC_MODE="copy"))
    assert res.returncode == 0 and "copy-mode checked ok" in res.stdout, res.stdout[-1000:] + res.stderr[-3000:]


def test_random_multi_table_calls_device_path_hypothesis(pel, oracle):
    """Property test (hypothesis, seeded) over what one batched call can look like on the DEVICE path: 1-6 tables of mixed
    dims (16-byte-multiple rows and others), dtypes fp32 / fp16 / fixed point, 1-5000 rows, 0-400 ragged bags with empty
    ones and duplicates, both index widths, per-table lists of torch tensors (the marshalling helper, the plan cache on a
    repeat) -- every table bit for bit against the oracle, twice (the second call of each case may be a cached plan)."""
    import torch
    from hypothesis import given, settings, strategies as st, HealthCheck
    dev = torch.device("cuda", 0)
    e = pel.EmbeddingEngine(device=0, max_tables=8)

    @settings(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(seed=st.integers(0, 2**31 - 1), n_tables=st.integers(1, 6), wide=st.booleans(), i64=st.booleans(),
           max_len=st.integers(0, 12))
    def case(seed, n_tables, wide, i64, max_len):
        rng = np.random.default_rng(seed)
        itype = np.int64 if i64 else np.int32
        tabs, idx, off = [], [], []
        for t in range(n_tables):
            dim = int(rng.choice([4, 16, 32, 64, 128, 256] if wide else [1, 2, 3, 10, 17, 30, 100]))
            kind = int(rng.integers(0, 3))
            rows = int(rng.integers(1, 5000))
            if kind == 2:
                w = rng.integers(-2**30, 2**30, size=(rows, dim)).astype(np.int32)
            else:
                w = (rng.standard_normal((rows, dim)) * 0.05).astype(np.float16 if kind == 1 else np.float32)
            e.load_table(t, w)
            nb = int(rng.integers(0, 400))
            o, n = pel.workloads.ragged_offsets(rng, nb, max_len, p_empty=0.2, dtype=itype) if (nb and max_len) else \
                (np.zeros(nb, itype), 0)
            tabs.append(w)
            off.append(o)
            idx.append(rng.integers(0, rows, size=n).astype(itype))
        d_idx = [torch.from_numpy(i).to(dev) if i.size else torch.zeros(0, dtype=torch.int64 if i64 else torch.int32, device=dev)
                 for i in idx]
        d_off = [torch.from_numpy(o).to(dev) if o.size else torch.zeros(0, dtype=torch.int64 if i64 else torch.int32, device=dev)
                 for o in off]
        outs = [torch.full((o.shape[0], w.shape[1]), float("nan"), device=dev) for o, w in zip(off, tabs)]
        for _rep in range(2):
            got = e.lookup_batched(list(range(n_tables)), list(d_idx), list(d_off), outs)
            torch.cuda.synchronize()
            for t in range(n_tables):
                want = oracle.c_lookup_fixed32(tabs[t], idx[t].astype(np.uint32), off[t].astype(np.uint32)) \
                    if tabs[t].dtype == np.int32 else oracle.c_bag_sum(tabs[t], idx[t].astype(np.int64), off[t].astype(np.int64))
                assert np.array_equal(got[t].cpu().numpy(), want), (seed, t, tabs[t].dtype, tabs[t].shape)

    case()
    e.close()


def test_checked_engine_refuses_bad_indices(pel, oracle):
    """EMB_FLAG_CHECK_INPUTS (emb_config.flags; PIMEMB_CHECK_INPUTS=1 for the engine behind populate_mram / lookup): a
    plan-less lookup with an out-of-range index or broken offsets returns EMB_ERR_RANGE and launches nothing -- host and
    device pointers, both index widths; good input gives the oracle's bits; the default engine stays unchecked."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    tab = pel.workloads.dlrm_table(rng, 500, 16)
    e = pel.EmbeddingEngine(device=0, max_tables=4, check_inputs=True)
    e.load_table(0, tab)
    good_i = rng.integers(0, 500, size=60).astype(np.uint32)
    off = np.arange(0, 60, 3, dtype=np.uint32)
    assert np.array_equal(e.lookup(0, good_i, off), oracle.c_bag_sum(tab, good_i, off))
    out = np.full((20, 16), 7.0, np.float32)
    bad_i = good_i.copy(); bad_i[17] = 500
    with pytest.raises(pel.PimembError) as ei:
        e.lookup(0, bad_i, off, out=out)
    assert ei.value.code == pel.lib.EMB_ERR_RANGE and (out == 7.0).all()          # nothing was written
    with pytest.raises(pel.PimembError):
        e.lookup(0, good_i, np.array([0, 70, 3], dtype=np.uint32))                 # offsets past the end / not monotone
    d_bad = torch.from_numpy(bad_i.astype(np.int64)).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_out = torch.full((20, 16), 7.0, device=dev)
    with pytest.raises(pel.PimembError) as ei:
        e.lookup(0, d_bad, d_off, out=d_out)
    torch.cuda.synchronize()
    assert ei.value.code == pel.lib.EMB_ERR_RANGE and bool((d_out == 7.0).all())    # disarmed on the device: nothing written
    d_good = torch.from_numpy(good_i.astype(np.int64)).to(dev)
    assert np.array_equal(e.lookup(0, d_good, d_off).cpu().numpy(), oracle.c_bag_sum(tab, good_i, off))
    assert e.stats()["n_kernel_launches"] == 2                                      # only the two good calls count as launched
    # a big checked call (the grid is large enough for the one-thread reporting kernel instead of tickets), bad then good
    big_i = torch.from_numpy(rng.integers(0, 500, size=26 * 40_000)).to(dev)
    big_o = torch.arange(0, 26 * 40_000, 2, dtype=torch.int64, device=dev)
    big_out = torch.full((13 * 40_000, 16), 7.0, device=dev)
    big_i[777_777] = 500
    with pytest.raises(pel.PimembError):
        e.lookup(0, big_i, big_o, out=big_out)
    torch.cuda.synchronize()
    assert bool((big_out == 7.0).all())
    big_i[777_777] = 499
    got = e.lookup(0, big_i, big_o, out=big_out)
    assert np.array_equal(got.cpu().numpy(), oracle.c_bag_sum(tab, big_i.cpu().numpy(), big_o.cpu().numpy()))
    e.close()
    # the reference entry points, checked through the environment
    from importlib import import_module
    compat = import_module("pim-embedding-lookup_amd.compat")
    os.environ["PIMEMB_CHECK_INPUTS"] = "1"
    try:
        compat.reset()
        compat.configure(1, 8, 4, 2)                    # one table, 8 columns, 4 bags of 2 indices
        tab32 = rng.integers(-1000, 1000, size=(50, 8)).astype(np.int32)
        handle = compat.populate([tab32])
        idx = [np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.uint32)]
        offs = [np.array([0, 2, 4, 6], dtype=np.uint32)]
        res = compat.lookup(handle, idx, offs, 8)
        assert np.array_equal(res[0], oracle.c_lookup_fixed32(tab32, idx[0], offs[0]))
        idx[0][3] = 50                                  # one row past the table
        res2 = compat.lookup(handle, idx, offs, 8)      # returns NULL like the reference; results untouched (NaN-filled)
        assert b"out-of-range" in pel.lib.load().emb_last_error() and np.isnan(res2[0]).all()
    finally:
        os.environ.pop("PIMEMB_CHECK_INPUTS", None)
        compat.reset()


@pytest.mark.gpu
def test_checked_engine_never_launches_a_cached_plan(pel, oracle):
    """an engine created with check_inputs=True must validate EVERY plan-less lookup -- also the third
    call with the same device tensors, which on an unchecked engine is one emb_plan_launch of a cached plan (no validation).
    Three good calls over the same buffers, then a bad index written IN PLACE: EMB_ERR_RANGE, output untouched, and the
    same through lookup_stacked."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(33)
    tabs = [pel.workloads.dlrm_table(rng, 400 + 10 * t, 16) for t in range(3)]
    e = pel.EmbeddingEngine(device=0, max_tables=4, check_inputs=True)
    for t, w in enumerate(tabs):
        e.load_table(t, w)
    idx = [torch.from_numpy(rng.integers(0, 400, size=64)).to(dev) for _ in range(3)]
    off = [torch.arange(0, 64, 2, dtype=torch.int64, device=dev) for _ in range(3)]
    outs = [torch.full((32, 16), 7.0, device=dev) for _ in range(3)]
    for _ in range(4):                                    # same addresses, same lengths: the plan cache's target loop
        got = e.lookup_batched([0, 1, 2], idx, off, outs)
    for t in range(3):
        assert np.array_equal(got[t].cpu().numpy(), oracle.c_bag_sum(tabs[t], idx[t].cpu().numpy(), off[t].cpu().numpy()))
    assert e.plan_cache_hits == 0 and not e._plan_cache
    for o in outs:
        o.fill_(7.0)
    idx[1][5] = 10_000                                    # in place: same tensor, same address
    with pytest.raises(pel.PimembError) as ei:
        e.lookup_batched([0, 1, 2], idx, off, outs)
    torch.cuda.synchronize()
    assert ei.value.code == pel.lib.EMB_ERR_RANGE and all(bool((o == 7.0).all()) for o in outs)
    # the stacked form: [T, N] / [T, B] tensors, three good calls, then a bad value in place
    si = torch.from_numpy(rng.integers(0, 400, size=(3, 64))).to(dev)
    so = torch.arange(0, 64, 2, dtype=torch.int64, device=dev).repeat(3, 1).contiguous()
    sout = torch.full((3, 32, 16), 7.0, device=dev)
    for _ in range(4):
        e.lookup_stacked([0, 1, 2], si, so, out=sout)
    assert e.plan_cache_hits == 0
    sout.fill_(7.0)
    si[2, 9] = 999_999
    with pytest.raises(pel.PimembError) as ei:
        e.lookup_stacked([0, 1, 2], si, so, out=sout)
    torch.cuda.synchronize()
    assert ei.value.code == pel.lib.EMB_ERR_RANGE and bool((sout == 7.0).all())
    e.plan_cache_size = 16                                # even if a caller turns the cache back on
    si[2, 9] = 1
    for _ in range(4):
        e.lookup_stacked([0, 1, 2], si, so, out=sout)
    assert e.plan_cache_hits == 0
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("space", ["host", "device"])
def test_request_queue_fuses_small_requests_into_one_launch(pel, oracle, space):
    """emb_queue_*: R pending small requests -- the reference's serving shapes, mini-batch 1 and 32 (README.md:6,
    upmem/run.sh:119), ragged ones too -- run as ONE launch; every request gets exactly the oracle's bits in its own
    buffers, from several threads, over several flushes, with uint32 and int64 indices."""
    import threading
    import torch
    rng = np.random.default_rng(77)
    rows = pel.workloads.KAGGLE_ROWS[:9]
    tabs = [pel.workloads.dlrm_table(rng, min(n, 60_000), 16) for n in rows]
    eng = pel.EmbeddingEngine(device=0, max_tables=16)
    for t, w in enumerate(tabs):
        eng.load_table(t, w)
    dev = torch.device("cuda", 0)
    for itype, npdt in ((pel.EMB_IDX_U32, np.uint32), (pel.EMB_IDX_I64, np.int64)):
        q = pel.RequestQueue(eng, itype, pel.EMB_MEM_HOST if space == "host" else pel.EMB_MEM_DEVICE)
        launches0 = eng.stats()["n_kernel_launches"]
        for flush_no in range(6):                       # more flushes than staging generations
            reqs, lock = [], threading.Lock()

            def client(seed, B):
                r = np.random.default_rng(seed)
                idx, off, outs = [], [], []
                for t, w in enumerate(tabs):
                    lens = r.integers(0, 4, size=B) if B > 1 else np.array([1])
                    o = np.zeros(B, dtype=np.int64); o[1:] = np.cumsum(lens)[:-1]
                    idx.append(r.integers(0, w.shape[0], size=int(lens.sum())).astype(npdt))
                    off.append(o.astype(npdt))
                    outs.append(np.full((B, 16), 7.0, np.float32))
                if space == "device":
                    d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)   # noqa: E731
                    di, do, du = [d(a) for a in idx], [d(a) for a in off], [torch.from_numpy(a).to(dev) for a in outs]
                    ticket = q.add(list(range(len(tabs))), di, do, du)
                    with lock:
                        reqs.append((ticket, idx, off, du))
                else:
                    ticket = q.add(list(range(len(tabs))), idx, off, outs)
                    with lock:
                        reqs.append((ticket, idx, off, outs))

            threads = [threading.Thread(target=client, args=(1000 * flush_no + k, B)) for k, B in enumerate([1, 1, 32, 5, 1, 32, 2, 17])]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            assert q.flush() == 8 and q.flush() == 0
            for ticket, idx, off, outs in reqs:
                q.wait(ticket)
                for t, w in enumerate(tabs):
                    got = outs[t].cpu().numpy() if space == "device" else outs[t]
                    assert np.array_equal(got, oracle.c_bag_sum(w, idx[t].astype(np.int64), off[t].astype(np.int64)))
        assert eng.stats()["n_kernel_launches"] - launches0 == 6          # ONE launch per flush, 8 requests each
        with pytest.raises(pel.PimembError):
            q.wait(10 ** 9)
        q.close()
    # one row shape per queue; a big request is refused by a host queue (it is not what the queue is for)
    eng.load_table(12, pel.workloads.dlrm_table(rng, 100, 32))
    q = pel.RequestQueue(eng, pel.EMB_IDX_U32, pel.EMB_MEM_HOST)
    one = (np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    q.add([0], [one[0]], [one[1]], [np.zeros((1, 16), np.float32)])
    with pytest.raises(pel.PimembError):
        q.add([12], [one[0]], [one[1]], [np.zeros((1, 32), np.float32)])
    with pytest.raises(pel.PimembError):
        q.add([0], [np.zeros(400_000, np.uint32)], [np.zeros(1, np.uint32)], [np.zeros((1, 16), np.float32)])
    assert q.flush() == 1
    q.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,dtype", [(16, np.float32), (128, np.float32), (64, np.float16), (4, np.float32), (256, np.float32)])
def test_lookup_ranged_serves_only_its_row_range(pel, oracle, dim, dtype):
    """emb_lookup_ranged: one index per bag, every shard scans the SAME raw index array and stores only the rows it holds,
    straight into the shared output -- after all shards have run, every bag carries exactly the oracle's row; a shard leaves
    the other shards' bags untouched (NaN-filled before), indices outside every range stay untouched."""
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    rows, N, B = 5003, 3, 4099
    tab = (rng.standard_normal((rows, dim)) * 0.1).astype(dtype)
    per = -(-rows // N)
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    for d in range(N):
        eng.load_table(d, tab[d * per:min((d + 1) * per, rows)])
    idx = rng.integers(0, rows, size=B).astype(np.uint32)
    idx[7] = rows + 100                                     # belongs to nobody
    d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
    out = torch.full((B, dim), float("nan"), device=dev)
    L = pel.lib.load()
    want = tab.astype(np.float32)[np.minimum(idx, rows - 1)]
    seen = np.zeros(B, bool)
    for d in range(N):
        desc = (pel.lib.EmbLookupDesc * 1)(pel.lib.EmbLookupDesc(d, 1, d_idx.data_ptr(), None, B, B, out.data_ptr()))
        lo = (C.c_uint64 * 1)(d * per)
        pel.lib.check(L.emb_lookup_ranged(eng._h, desc, lo, 1, None))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        mine = (idx >= d * per) & (idx < min((d + 1) * per, rows))
        seen |= mine
        assert np.array_equal(got[mine], want[mine])
        assert np.isnan(got[~seen]).all()                   # bags of later shards (and nobody's) untouched
    assert not seen[7] and seen.sum() == B - 1
    # refused: ragged bags, pooled bags
    off = torch.zeros(B, dtype=torch.int32, device=dev)
    bad = (pel.lib.EmbLookupDesc * 1)(pel.lib.EmbLookupDesc(0, 0, d_idx.data_ptr(), off.data_ptr(), B, B, out.data_ptr()))
    assert L.emb_lookup_ranged(eng._h, bad, (C.c_uint64 * 1)(0), 1, None) == pel.lib.EMB_ERR_INVALID
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,dtype,B", [(16, np.float32, 600_001), (16, np.float32, 4099), (128, np.float32, 33_000), (64, np.float16, 20_000)])
def test_lookup_ranged_typed_int64_ids_and_the_open_end(pel, dim, dtype, B):
    """Round 6: emb_lookup_ranged_typed / emb_plan_create_ranged_typed over int64 index arrays (torch's width, compared as they
    are: a negative id is beyond every range) and EMB_RANGE_OPEN_END -- the descriptor that carries it (the last shard) writes a
    ZERO row for every id at or beyond the end of its range, counts none of them, and the other shards still leave foreign bags
    alone: after all shards have run every bag holds its table row, or zeros where no shard holds the id; the served counters add up
    to the bags that were really served.  Small and very large launches (64-bag tiles / two batches per wavefront + XCD map),
    transient and prepared, uint32 next to int64: the same bits."""
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(B % 1000 + dim)
    rows, N = 50_003, 3
    tab = (rng.standard_normal((rows, dim)) * 0.1).astype(dtype)
    per = -(-rows // N)
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    for d in range(N):
        eng.load_table(d, tab[d * per:min((d + 1) * per, rows)])
    idx = rng.integers(0, rows, size=B).astype(np.int64)
    nobody = {3: rows + 100, 11: -1, 500: -(1 << 45), 1000: (1 << 32) + 5, B - 1: (1 << 62)}
    for p, v in nobody.items():
        idx[p] = v
    held = (idx >= 0) & (idx < rows)
    want = np.where(held[:, None], tab.astype(np.float32)[np.clip(idx, 0, rows - 1)], np.float32(0))
    L = pel.lib.load()
    OPEN = pel.lib.EMB_RANGE_OPEN_END
    ctr = torch.zeros((N, 64 * 256 // 4), dtype=torch.int32, device=dev)        # EMB_SERVED_LANES x EMB_SERVED_STRIDE bytes per counter
    outs = {}
    for itype, d_idx in ((pel.lib.EMB_IDX_I64, torch.from_numpy(idx).to(dev)),
                         (pel.lib.EMB_IDX_U32, torch.from_numpy(np.where(held, idx, rows + 7).astype(np.uint32).view(np.int32)).to(dev))):
        for prepared in (False, True):
            out = torch.full((B, dim), float("nan"), device=dev)
            ctr.zero_()
            descs = (pel.lib.EmbLookupDesc * N)(*[pel.lib.EmbLookupDesc(d, 1, d_idx.data_ptr(), None, B, B, out.data_ptr()) for d in range(N)])
            lo = (C.c_uint64 * N)(*[(d * per) | (OPEN if d == N - 1 else 0) for d in range(N)])
            served = (C.c_void_p * N)(*[ctr[d].data_ptr() for d in range(N)])
            if prepared:
                plan = C.c_void_p()
                pel.lib.check(L.emb_plan_create_ranged_typed(eng._h, descs, lo, served, N, itype, C.byref(plan)))
                pel.lib.check(L.emb_plan_launch(plan, None))
                torch.cuda.synchronize()
                pel.lib.check(L.emb_plan_destroy(plan))
            else:
                pel.lib.check(L.emb_lookup_ranged_typed(eng._h, descs, lo, served, N, itype, None))
                torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got, want), (itype, prepared)                     # rows where held, ZEROS where nobody holds the id, no NaN left
            counts = ctr.cpu().numpy().astype(np.int64).sum(axis=1)
            mine = [int(((idx >= d * per) & (idx < min((d + 1) * per, rows))).sum()) for d in range(N)]
            assert counts.tolist() == mine and sum(mine) == B - len(nobody)          # the open end's bags are zeroed, never counted
            outs[(itype, prepared)] = got
    # without the flag the last shard leaves them alone too (the round-5 behaviour, what an unchecked shard keeps)
    out = torch.full((B, dim), float("nan"), device=dev)
    d_idx = torch.from_numpy(idx).to(dev)
    descs = (pel.lib.EmbLookupDesc * N)(*[pel.lib.EmbLookupDesc(d, 1, d_idx.data_ptr(), None, B, B, out.data_ptr()) for d in range(N)])
    pel.lib.check(L.emb_lookup_ranged_typed(eng._h, descs, (C.c_uint64 * N)(*[d * per for d in range(N)]), None, N, pel.lib.EMB_IDX_I64, None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[~held]).all() and np.array_equal(got[held], want[held])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,dtype,B", [(16, np.float32, 150_001), (16, np.float32, 9001), (128, np.float32, 33_000),
                                         (64, np.float16, 40_000), (32, "fixed32", 20_011)])
def test_ranged_launch_mixes_whole_tables_and_shards(pel, oracle, dim, dtype, B):
    """ONE ranged launch over whole tables (the range starting at row 0) and the shards of row-split tables, as the sharded
    lookup's direct path issues it: the small (64-bag tiles), the large (two batches per wavefront, XCD map) and the fp16 /
    fixed-point forms of the one-hot kernel -- transient (emb_lookup_ranged) and prepared (emb_plan_create_ranged) -- every
    bag equal to the oracle's, every bag of another shard untouched, an index outside a whole table leaves its bag alone."""
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    fixed = dtype == "fixed32"
    whole_rows, split_rows, N, me = [700, 12_345], [50_021, 9_973], 4, 2
    n_tab = len(whole_rows) + len(split_rows)

    def make(n):
        if fixed:
            return rng.integers(-2 ** 30, 2 ** 30, size=(n, dim)).astype(np.int32)
        return (rng.standard_normal((n, dim)) * 0.1).astype(dtype)

    tabs = [make(n) for n in whole_rows + split_rows]
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    per = [-(-n // N) for n in split_rows]
    for t, n in enumerate(whole_rows):
        eng.load_table(t, tabs[t], dtype=pel.EMB_FIXED32 if fixed else None)
    for k, n in enumerate(split_rows):          # this "rank" holds shard `me` of every row-split table
        t = len(whole_rows) + k
        eng.load_table(t, tabs[t][me * per[k]:min((me + 1) * per[k], n)], dtype=pel.EMB_FIXED32 if fixed else None)
    idx = [rng.integers(0, n, size=B).astype(np.uint32) for n in whole_rows + split_rows]
    idx[1][5] = whole_rows[1] + 77                      # outside a whole table: nothing is read, the bag stays as it was
    d_idx = [torch.from_numpy(i.view(np.int32)).to(dev) for i in idx]
    L = pel.lib.load()
    descs = (pel.lib.EmbLookupDesc * n_tab)()
    lo = (C.c_uint64 * n_tab)()
    for prepared in (False, True):
        outs = [torch.full((B, dim), float("nan"), device=dev) for _ in range(n_tab)]
        for t in range(n_tab):
            descs[t] = pel.lib.EmbLookupDesc(t, 1, d_idx[t].data_ptr(), None, B, B, outs[t].data_ptr())
            lo[t] = 0 if t < len(whole_rows) else me * per[t - len(whole_rows)]
        launches = eng.stats()["n_kernel_launches"]
        if prepared:
            plan = C.c_void_p()
            pel.lib.check(L.emb_plan_create_ranged(eng._h, descs, lo, n_tab, C.byref(plan)))
            pel.lib.check(L.emb_plan_launch(plan, None))
        else:
            pel.lib.check(L.emb_lookup_ranged(eng._h, descs, lo, n_tab, None))
        torch.cuda.synchronize()
        assert eng.stats()["n_kernel_launches"] == launches + 1          # one row width: one launch
        for t in range(n_tab):
            got = outs[t].cpu().numpy()
            n = (whole_rows + split_rows)[t]
            if t < len(whole_rows):
                mine = idx[t] < n
                rel = np.minimum(idx[t], n - 1)
                src = tabs[t]
            else:
                k = t - len(whole_rows)
                mine = (idx[t] >= me * per[k]) & (idx[t] < min((me + 1) * per[k], n))
                rel = np.where(mine, idx[t], 0)
                src = tabs[t]
            if fixed:             # the oracle over one-index bags of the rows in question
                want = oracle.c_lookup_fixed32(src, rel.astype(np.uint32), np.arange(B, dtype=np.uint32))
            else:
                want = oracle.c_bag_sum(src.astype(np.float32), rel.astype(np.int64), np.arange(B, dtype=np.int64))
            assert np.array_equal(got[mine], want[mine]), (t, prepared)
            assert np.isnan(got[~mine]).all(), (t, prepared)
            assert mine.sum() > 0
        if prepared:
            pel.lib.check(L.emb_plan_destroy(plan))
    assert not (idx[1] < whole_rows[1])[5]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,dtype,B", [(16, np.float32, 150_001), (16, np.float32, 4001), (128, np.float32, 33_000), (64, np.float16, 20_000)])
def test_ranged_counted_launch_counts_exactly_the_bags_it_serves(pel, dim, dtype, B):
    """emb_lookup_ranged_counted / emb_plan_create_ranged_counted through the C ABI (round 5): every descriptor's counter --
    EMB_SERVED_LANES words EMB_SERVED_STRIDE bytes apart, the count is their sum -- grows by exactly the number of bags whose
    index falls into the descriptor's row range: whole tables (with a few indices beyond the table: not served, not counted),
    the N shards of a row-split table over the SAME raw index array (their counts add up to the bag count minus the indices no
    shard holds), a NULL counter among them (that descriptor is not counted), the small and the two-batch geometry, transient
    and prepared, twice in a row (counters accumulate: the caller zeroes them).  The rows themselves are the uncounted
    launch's, bit for bit."""
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    whole_rows, split_rows, N = [900, 20_011], 31_007, 4
    per = -(-split_rows // N)
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    tabs = [(rng.standard_normal((n, dim)) * 0.1).astype(dtype) for n in whole_rows]
    big = (rng.standard_normal((split_rows, dim)) * 0.1).astype(dtype)
    for t, w in enumerate(tabs):
        eng.load_table(t, w)
    for d in range(N):
        eng.load_table(2 + d, big[d * per:min((d + 1) * per, split_rows)])
    idx = [rng.integers(0, n, size=B).astype(np.uint32) for n in whole_rows] + [rng.integers(0, split_rows, size=B).astype(np.uint32)]
    idx[1][::97] = whole_rows[1] + 5                    # beyond a whole table
    idx[2][::89] = N * per + 11                         # beyond the last shard
    d_idx = [torch.from_numpy(i.view(np.int32)).to(dev) for i in idx]
    n_desc = 2 + N
    L = pel.lib.load()
    lanes, stride = 64, 256
    ctr = torch.zeros((n_desc, lanes * stride // 4), dtype=torch.int32, device=dev)
    expect = [int((idx[0] < whole_rows[0]).sum()), int((idx[1] < whole_rows[1]).sum())] + \
             [int(((idx[2] >= d * per) & (idx[2] < min((d + 1) * per, split_rows))).sum()) for d in range(N)]
    assert sum(expect[2:]) == B - int((idx[2] >= split_rows).sum()) < B and expect[1] < B
    descs = (pel.lib.EmbLookupDesc * n_desc)()
    lo = (C.c_uint64 * n_desc)()
    served = (C.c_void_p * n_desc)()
    ref = None
    for prepared in (False, True):
        outs = [torch.full((B, dim), float("nan"), device=dev) for _ in range(3)]
        for i in range(n_desc):
            t = min(i, 2)
            descs[i] = pel.lib.EmbLookupDesc(i, 1, d_idx[t].data_ptr(), None, B, B, outs[t].data_ptr())
            lo[i] = 0 if i < 2 else (i - 2) * per
            served[i] = ctr[i].data_ptr()
        served[3] = None                                # the shard d = 1: not counted
        ctr.zero_()
        for rep_ in range(2):
            if prepared:
                plan = C.c_void_p()
                pel.lib.check(L.emb_plan_create_ranged_counted(eng._h, descs, lo, served, n_desc, C.byref(plan)))
                pel.lib.check(L.emb_plan_launch(plan, None))
                torch.cuda.synchronize()
                pel.lib.check(L.emb_plan_destroy(plan))
            else:
                pel.lib.check(L.emb_lookup_ranged_counted(eng._h, descs, lo, served, n_desc, None))
            torch.cuda.synchronize()
            got = ctr.view(n_desc, lanes, stride // 4)[:, :, 0].sum(dim=1).cpu().numpy().astype(np.int64)
            want = np.array([e * (rep_ + 1) for e in expect], dtype=np.int64)
            want[3] = 0
            assert np.array_equal(got, want), (prepared, rep_, got, want)
            assert int(ctr.view(n_desc, lanes, stride // 4)[:, :, 1:].abs().sum()) == 0        # nothing but the lane words is touched
        rows = [o.cpu().numpy() for o in outs]
        if ref is None:         # the uncounted launch over the same descriptors: the same rows, the same untouched bags
            outs2 = [torch.full((B, dim), float("nan"), device=dev) for _ in range(3)]
            for i in range(n_desc):
                descs[i].pooled = outs2[min(i, 2)].data_ptr()
            pel.lib.check(L.emb_lookup_ranged(eng._h, descs, lo, n_desc, None))
            torch.cuda.synchronize()
            ref = [o.cpu().numpy() for o in outs2]
        for t in range(3):
            assert np.array_equal(rows[t], ref[t], equal_nan=True), (prepared, t)
        assert np.isnan(rows[1][::97]).all() and np.isnan(rows[2][::89]).all() and not np.isnan(rows[0]).any()
    eng.close()


@pytest.mark.gpu
def test_shard_objects_from_two_threads_share_an_engine(pel, oracle):
    """include/pimemb.h: one caller thread per shard object, several shard objects may share an engine.  Two threads, each with
    its own ShardedEmbeddingBags (world of one rank: replicated / whole / row-split tables) and its own stream on ONE engine,
    run routed and direct batches at different depths at the same time; every table of every batch equals the oracle's."""
    import threading
    from importlib import import_module
    import torch
    sh = import_module("pim-embedding-lookup_amd.sharding")
    dev = torch.device("cuda", 0)
    rows, dim = [700, 30_000, 9_000, 20_000, 50], 16
    kinds = [sh.REPLICATED, sh.ROW_SPLIT, sh.WHOLE, sh.ROW_SPLIT, sh.REPLICATED]
    units = [sh.Unit(t, -1 if k == sh.REPLICATED else 0, 0, rows[t], t) for t, k in enumerate(kinds)]
    plan = sh.ShardPlan(1, rows, dim, 4, kinds, units, [[t] for t in range(len(rows))])
    tabs = [(np.random.default_rng(7 + t).standard_normal((n, dim)) * 0.1).astype(np.float32) for t, n in enumerate(rows)]
    eng = pel.EmbeddingEngine(device=0, max_tables=len(rows) + 1)
    for u in units:
        eng.load_table(u.uid, tabs[u.table])
    errors = []

    def worker(tid):
        try:
            rng = np.random.default_rng(100 + tid)
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                for depth in (0, 3, 1):
                    S = sh.ShardedEmbeddingBags(plan, eng, 0, None, depth=depth, check=False)
                    pending = []
                    for j in range(30):
                        nb = int(rng.integers(1, 4000))
                        one_hot = j % 2 == tid % 2
                        idx, off = [], []
                        for n in rows:
                            if one_hot:
                                o, ni = np.arange(nb, dtype=np.int64), nb
                            else:
                                lens = rng.integers(0, 5, size=nb)
                                o = np.zeros(nb, np.int64)
                                o[1:] = np.cumsum(lens)[:-1]
                                ni = int(lens.sum())
                            off.append(o)
                            idx.append(rng.integers(0, n, size=ni).astype(np.int64))
                        d_i = [torch.from_numpy(i.astype(np.int32)).to(dev) for i in idx]
                        d_o = [torch.from_numpy(o.astype(np.int32)).to(dev) for o in off]
                        h = stream.cuda_stream
                        if one_hot:
                            seq, outs = S.submit(d_i, None, fixed_pooling=1, stream=h)
                        else:
                            seq, outs = S.submit(d_i, d_o, stream=h)
                        pending.append((seq, outs, idx, off, (d_i, d_o)))
                        if len(pending) > depth:
                            q, o_, i_, f_, _keep = pending.pop(0)
                            S.wait(q, h)
                            stream.synchronize()
                            for t in range(len(rows)):
                                assert np.array_equal(o_[t].cpu().numpy(), oracle.c_bag_sum(tabs[t], i_[t], f_[t])), (tid, depth, j, t)
                    S.flush()
                    for q, o_, i_, f_, _keep in pending:
                        S.wait(q, stream.cuda_stream)
                        stream.synchronize()
                        for t in range(len(rows)):
                            assert np.array_equal(o_[t].cpu().numpy(), oracle.c_bag_sum(tabs[t], i_[t], f_[t])), (tid, depth, "drained", t)
                    S.close()
        except Exception:  # noqa: BLE001
            import traceback
            errors.append(traceback.format_exc())

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    eng.close()
    assert not errors, errors[0]


@pytest.mark.gpu
def test_deferred_verdict_of_checked_calls(pel, oracle):
    """check="deferred" (emb_lookup_batched_checked_deferred / EMB_FLAG_DEFER_CHECK): the call does not wait for its verdict.
    (1) clean calls -- more of them back to back than the engine has verdict slots -- give the oracle's bits; (2) a bad index:
    the call itself returns, its outputs stay untouched (the validation kernel disarms the lookup on the GPU), and the
    IndexError comes out of a LATER call / check_report() -- once, naming the call; calls made in between ran; (3) two streams
    at once, one finding each side attributed to its own call; (4) the engine flag; (5) the torch modules; (6) close() raises
    a verdict nobody met."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(61)
    sizes = (700, 90_000, 33)
    tabs = [pel.workloads.dlrm_table(rng, n, 16) for n in sizes]
    e = pel.EmbeddingEngine(device=0, max_tables=4)
    for t, w in enumerate(tabs):
        e.load_table(t, w)
    ids = [0, 1, 2]

    def batch(seed, B=512, L=3):
        r = np.random.default_rng(seed)
        idx = [torch.from_numpy(r.integers(0, n, size=B * L)).to(dev) for n in sizes]
        off = [torch.arange(0, B * L, L, dtype=torch.int64, device=dev) for _ in sizes]
        return idx, off, [torch.full((B, 16), 7.0, device=dev) for _ in sizes]

    def want(idx, off):
        return [oracle.c_bag_sum(tabs[t], idx[t].cpu().numpy(), off[t].cpu().numpy()) for t in range(3)]

    # (1) 150 clean calls, no synchronisation in between (64 verdict slots)
    work = [batch(100 + i) for i in range(6)]
    for i in range(150):
        idx, off, outs = work[i % 6]
        e.lookup_batched(ids, idx, off, outs, check="deferred")
    e.check_report()
    for idx, off, outs in work:
        for t in range(3):
            assert np.array_equal(outs[t].cpu().numpy(), want(idx, off)[t])
    # (2) one bad call among clean ones
    st0 = e.stats()
    bad = batch(7)
    bad[0][1][1234] = 90_000
    clean = [batch(8), batch(9)]
    e.lookup_batched(ids, *bad, check="deferred")              # returns: nobody waited
    raised = 0
    for idx, off, outs in clean:
        try:
            e.lookup_batched(ids, idx, off, outs, check="deferred")
        except IndexError as ex:
            raised += 1
            assert "EARLIER" in str(ex) and "1 out-of-range" in str(ex)
    try:
        e.check_report()
    except IndexError as ex:
        raised += 1
        assert "1 out-of-range" in str(ex)
    assert raised == 1
    e.check_report()                                           # once
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in bad[2])         # the refused call wrote nothing
    for idx, off, outs in clean:                               # the calls around it ran (also the one that raised)
        for t in range(3):
            assert np.array_equal(outs[t].cpu().numpy(), want(idx, off)[t])
    st1 = e.stats()
    e.lookup_batched(ids, *clean[0], check="deferred")
    e.check_report()
    per_call = e.stats()["n_kernel_launches"] - st1["n_kernel_launches"]
    # three calls counted, two of them launched lookup kernels that did something
    assert st1["n_lookup_calls"] - st0["n_lookup_calls"] == 3 and st1["n_kernel_launches"] - st0["n_kernel_launches"] == 2 * per_call
    # a synchronous checked call meets an earlier deferred finding
    e.lookup_batched(ids, *bad, check="deferred")
    with pytest.raises(IndexError, match="EARLIER"):
        e.lookup_batched(ids, *clean[0], check=True)
    e.lookup_batched(ids, *clean[0], check=True)
    # (3) two streams, each with its own bad call
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    findings = []
    for rnd in range(40):
        for k, st in enumerate((s1, s2)):
            idx, off, outs = work[(rnd + 3 * k) % 6]
            use = bad if (rnd == 11 and k == 0) or (rnd == 29 and k == 1) else (idx, off, outs)
            try:
                e.lookup_batched(ids, *use, stream=st.cuda_stream, check="deferred")
            except IndexError as ex:
                findings.append(str(ex))
    try:
        e.check_report()
    except IndexError as ex:
        findings.append(str(ex))
    torch.cuda.synchronize()
    assert len(findings) in (1, 2) and all("1 out-of-range" in f or "2 out-of-range" in f for f in findings), findings
    assert sum(int(f.split(" ")[0]) for f in findings) == 2
    assert all(bool((o == 7.0).all()) for o in bad[2])
    e.check_report()
    # (6) close() raises what nobody met
    e.lookup_batched(ids, *bad, check="deferred")
    with pytest.raises(IndexError):
        e.close()

    # (4) the engine flag: every plan-less call is checked, none waits
    e = pel.EmbeddingEngine(device=0, max_tables=4, check_inputs="deferred")
    for t, w in enumerate(tabs):
        e.load_table(t, w)
    for _ in range(4):
        e.lookup_batched(ids, *clean[1])
    assert e.plan_cache_hits == 0
    e.lookup_batched(ids, *bad)
    raised = 0
    for _ in range(3):                       # (the verdict has arrived by the next call, or by one after it: nobody waits)
        try:
            e.lookup_batched(ids, *clean[1])
        except pel.PimembError as ex:
            assert ex.code == pel.lib.EMB_ERR_RANGE and "EARLIER" in str(ex)
            raised += 1
    try:
        e.check_report()
    except IndexError:
        raised += 1
    assert raised == 1
    e.check_report()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in bad[2])
    for t in range(3):
        assert np.array_equal(clean[1][2][t].cpu().numpy(), want(*clean[1][:2])[t])
    e.close()

    # (5) the torch modules
    from importlib import import_module
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    bags = [tm.EmbeddingBag.from_pretrained(torch.from_numpy(tabs[t]), engine=e, table_id=t, deferred_check=True) for t in range(3)]
    fused = tm.FusedEmbeddingBags(bags)
    assert fused.deferred_check and not fused.trusted_inputs
    idx, off, _ = clean[0]
    got = fused(off, idx)
    for t in range(3):
        assert np.array_equal(got[t].cpu().numpy(), want(idx, off)[t])
    fused(bad[1], bad[0])
    with pytest.raises(IndexError):
        for _ in range(3):
            bags[0](idx[0], off[0])
            torch.cuda.synchronize()
    e.check_report()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("itype", ["u32", "i64"])
def test_validation_kernel_counts_exactly(pel, itype):
    """The validation kernel (16-byte loads, two-level tickets that carry the findings, one verdict word) against a numpy count:
    lengths around every boundary of its layout (the vector width, a workgroup's share, the 32-counter threshold, the cap of
    1 024 workgroups per descriptor -> the grid-stride loop), arrays that start at ANY element (views: 4- / 8-byte aligned only),
    descriptors of very different lengths in one launch, bad values at the head, in the remainder, on vector boundaries, in the
    last bag; broken offsets of every kind.  Device and host buffers."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77 if itype == "u32" else 78)
    npt = np.uint32 if itype == "u32" else np.int64
    tdt = torch.int32 if itype == "u32" else torch.int64
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    rows = [50, 1000, 1 << 20, 7]
    for t, n in enumerate(rows):
        e.alloc_table(t, n, 16, pel.EMB_F32)

    def want(idx, off, n_rows):
        i = idx.astype(np.int64) if itype == "i64" else idx.astype(np.uint64)
        bad = int(((i < 0) | (i >= n_rows)).sum()) if itype == "i64" else int((i >= n_rows).sum())
        o = off.astype(np.int64) if itype == "i64" else off.astype(np.uint64).astype(np.int64)
        nxt = np.append(o[1:], len(idx))
        ou = o.astype(np.uint64) if itype == "i64" else o.astype(np.uint64)
        nu = nxt.astype(np.uint64)
        bad += int(((ou > nu) | (nu > np.uint64(len(idx)))).sum())
        return bad

    def make(n_idx, n_bags, n_rows, spoil):
        idx = rng.integers(0, n_rows, size=n_idx).astype(npt)
        cuts = np.sort(rng.integers(0, n_idx + 1, size=n_bags)) if n_bags else np.zeros(0, np.int64)
        if n_bags:
            cuts[0] = 0
        off = cuts.astype(npt)
        if spoil and n_idx:
            k = min(n_idx, int(rng.integers(1, 9)))
            pos = set(int(x) for x in rng.integers(0, n_idx, size=k))
            pos |= {0, n_idx - 1, (n_idx // 4) * 4 - 1 if n_idx >= 4 else 0, max(0, n_idx - n_idx % 4)}
            for p in pos:
                p = min(max(p, 0), n_idx - 1)
                idx[p] = n_rows + int(rng.integers(0, 5)) if (itype == "u32" or rng.integers(0, 2)) else -1 - int(rng.integers(0, 5))
        if spoil and n_bags >= 2:
            for _ in range(int(rng.integers(1, 4))):
                b = int(rng.integers(0, n_bags))
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    off[b] = n_idx + 1 + int(rng.integers(0, 3))          # beyond the indices
                elif kind == 1 and itype == "i64":
                    off[b] = -3
                else:
                    off[b] = (int(off[b - 1]) + int(off[b]) + 1) if b else off[b]    # may break monotony
            off[n_bags - 1] = n_idx + 2                                  # the last bag: its end is n_idx
        return idx, off

    lengths = [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096 + 3, 33 * 1024 + 1, 70_001, 1024 * 1024 * 2 + 5]
    checked = 0
    for spoil in (False, True):
        for n_idx in lengths:
            for shift in (0, 1, 3):
                n_bags = min(n_idx, int(rng.integers(1, 2 + n_idx))) if n_idx else 1
                idx, off = make(n_idx, n_bags, rows[1], spoil)
                w = want(idx, off, rows[1])
                assert spoil or w == 0
                # device buffers that start `shift` elements into an allocation
                di = torch.empty(n_idx + shift + 4, dtype=tdt, device=dev)[shift:shift + n_idx]
                do = torch.empty(n_bags + shift + 4, dtype=tdt, device=dev)[shift:shift + n_bags]
                di.copy_(torch.from_numpy(idx.view(np.int32) if itype == "u32" else idx))
                do.copy_(torch.from_numpy(off.view(np.int32) if itype == "u32" else off))
                got = e.validate([1], [di], [do])
                assert got == w, (n_idx, n_bags, shift, spoil, got, w)
                if shift == 0:
                    got = e.validate([1], [idx], [off])                   # host buffers (staged by the library)
                    assert got == w, ("host", n_idx, n_bags, spoil, got, w)
                checked += 1
    # descriptors of very different lengths in one launch, each with its own findings
    parts = [make(n, max(1, n // 3), rows[t], True) for t, n in enumerate((5, 40_000, 3_000_000, 17))]
    total = sum(want(i, o, rows[t]) for t, (i, o) in enumerate(parts))
    got = e.validate([0, 1, 2, 3], [p[0] for p in parts], [p[1] for p in parts])
    assert got == total and total > 8
    as_t = (lambda a: torch.from_numpy(a.view(np.int32)).to(dev)) if itype == "u32" else (lambda a: torch.from_numpy(a).to(dev))
    d = [(as_t(i), as_t(o)) for i, o in parts]
    assert e.validate([0, 1, 2, 3], [x[0] for x in d], [x[1] for x in d]) == total
    # fixed pooling: n_idx must be n_bags * L
    idx = rng.integers(0, 50, size=96).astype(npt)
    assert e.validate([0], [idx], [None], fixed_pooling=4) == 0
    idx[95] = 50
    assert e.validate([0], [idx], [None], fixed_pooling=4) == 1
    assert checked > 100
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,bags", [(16, [40_000, 39_292, 65_536, 30_000, 50_000]), (64, [40_000, 30_000]), (128, [20_000, 16_384, 24_000, 16_384])])
def test_big_host_pointer_call_in_two_parts(pel, oracle, dim, bags):
    """A host-pointer call whose rows go back table by table at link speed (every table >= 1.5 MB of rows) with >= 1 MB of
    indices: copy-in + lookup in two parts, the second on the engine's own stream next to the first part's copy-out
    (lookup_host_split).  Ragged and one-index tables, uint32 and int64, the default stream and a stream of the caller's with
    work queued on it, the call repeated (the staging buffer and the second stream are reused): the oracle's bits every time."""
    import torch
    rng = np.random.default_rng(dim + len(bags))
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    tabs = [rng.standard_normal((5000 + 1000 * t, dim)).astype(np.float32) for t in range(len(bags))]
    for t, w in enumerate(tabs):
        e.load_table(t, w)
    ids = list(range(len(bags)))
    st = torch.cuda.Stream()
    for rep, itype in enumerate((np.uint32, np.int64, np.uint32)):
        idx, off = [], []
        for t, b in enumerate(bags):
            if t % 2:
                o, n = pel.workloads.ragged_offsets(rng, b, 12, dtype=itype)
            else:
                o, n = np.arange(b).astype(itype) * 6, b * 6
            off.append(o)
            idx.append(rng.integers(0, tabs[t].shape[0], size=n).astype(itype))
        assert sum(i.nbytes + o.nbytes for i, o in zip(idx, off)) >= 1 << 20
        if rep == 2:           # behind work of the caller's on its own stream
            with torch.cuda.stream(st):
                junk = torch.rand((4096, 4096), device="cuda") @ torch.rand((4096, 4096), device="cuda")
            outs = e.lookup_batched(ids, idx, off, stream=st.cuda_stream)
            del junk
        else:
            outs = e.lookup_batched(ids, idx, off)
        for t in range(len(bags)):
            assert np.array_equal(outs[t], oracle.c_bag_sum(tabs[t], idx[t], off[t])), (dim, t, itype)
    e.close()


@pytest.mark.gpu
def test_bench_plain_run_dumps_what_the_last_step_computed(tmp_path):
    """`bench.py --gpus 1`: a plain run launches exactly K timed steps after its W warm-up ones and checks nothing; the outputs
    of its last step (--dump-outputs) are the rows of the batch that step used -- gathered here from the same seeded tables and
    indices, bit for bit -- and equal those of a --full run, whose timed outputs bench.py itself checked.  The plain run spends
    well under 30 s outside its steps."""
    import argparse
    import json
    import subprocess
    import sys
    import time
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import pim_embedding_lookup_amd as pel
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PIMEMB_FORCE_DIST"):
        env.pop(k, None)
    K, W, B, NB = 5, 2, 4096, 3
    common = ["--gpus", "1", "--steps", str(K), "--warmup", str(W), "--batch", str(B), "--nbatch", str(NB), "--prewarm-ms", "20"]
    lines, walls = {}, {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        t0 = time.perf_counter()
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + extra + ["--dump-outputs", str(tmp_path / mode)],
                             env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        walls[mode] = time.perf_counter() - t0
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        lines[mode] = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    p, f = lines["plain"], lines["full"]
    assert p["steps"] == K and p["ms_per_step"] > 0 and p["unit"] == "pooled-lookups/s" and p["dtype"] == "f32"
    assert p["verified"] is None and p["value_cold"] is None and "cpu_baseline" not in p
    assert f["verified"] is True and f["verify"]["bags_bit_exact_vs_torch_gather"] == 26 * B * NB and f["value_cold"] is not None
    # every lookup launch of the process: the pre-warm, then W + K (plain) -- and the cold W + K before the pre-warm (--full)
    assert sum(p["config"]["launches_by_kind"]) == p["config"]["prewarm_launches"] + W + K
    assert sum(f["config"]["launches_by_kind"]) == f["config"]["prewarm_launches"] + 2 * (W + K)
    assert walls["plain"] - (W + K) * p["ms_per_step"] / 1000.0 < 30.0, walls
    # the last step's batch (step i uses batch i % NB), its rows gathered from the tables bench.py generates
    spec = bench.workload_spec(pel, argparse.Namespace(workload="c2", batch=B, index_dist=None, index_order="drawn"))
    idx = bench.make_batches(pel, spec, NB)[(K - 1) % NB][0]
    others = [bench.make_batches(pel, spec, NB)[j][0] for j in range(NB) if j != (K - 1) % NB]
    want, other_rows = {}, {}

    class Gather:                 # stands in for the engine: keeps the rows the batches name, not the 2 GB of tables
        def load_table(self, t, w):
            want[t] = w[torch.from_numpy(idx[t].astype(np.int64)).to(w.device)].cpu().numpy()
            other_rows[t] = [w[torch.from_numpy(o[t].astype(np.int64)).to(w.device)].cpu().numpy() for o in others]

    bench.make_tables_on_gpu(torch, Gather(), spec["rows"], spec["dim"], torch.device("cuda", 0))
    for t in range(26):
        a = np.load(tmp_path / "plain" / ("table_%02d.npy" % t))
        b = np.load(tmp_path / "full" / ("table_%02d.npy" % t))
        assert a.dtype == np.float32 and a.shape == (B, 16) and np.array_equal(a, b), t
        assert np.array_equal(a, want[t]), t
        assert not any(np.array_equal(a, o) for o in other_rows[t]), t
