"""GPU: pooled lookups (emb_lookup_pooled / emb_plan_create_pooled, the bag_pool_* kernels) against torch's CPU
F.embedding_bag, bit for bit: mean / max / weighted sum, padding_idx, fp32 and fp16 tables, uint32 and int64 ids, the
wave-batch (one-hot), lane-group (ragged) and any-dim paths, both memspaces, plans and graph capture, checking, and the
torch modules over them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


def torch_ref(table, idx, off, mode, w=None, pad=None):
    """torch CPU on the fp32 view of the table (fp16 tables: table.float())."""
    t = torch.as_tensor(np.asarray(table)).float()
    return F.embedding_bag(torch.as_tensor(np.asarray(idx)).long(), t, torch.as_tensor(np.asarray(off)).long(), mode=mode,
                           per_sample_weights=None if w is None else torch.as_tensor(np.asarray(w)), padding_idx=pad)


def same(got, want):
    got = got.detach().cpu() if torch.is_tensor(got) else torch.from_numpy(np.asarray(got))
    return torch.equal(got, want)


SHAPES = {
    # name: (rows, dim, bags, max pooling): one-hot big enough for the wave-batch path, ragged 0..40, two any-dim widths
    "onehot": (5000, 16, 140000, 1),
    "ragged": (3000, 64, 3000, 40),
    "anydim3": (700, 3, 2000, 12),
    "anydim30": (700, 30, 1500, 12),
}


def make(shape, seed, table_dtype=np.float32):
    rows, dim, B, L = SHAPES[shape]
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((rows, dim)).astype(table_dtype)
    lens = np.ones(B, np.int64) if L == 1 else rng.integers(0, L + 1, B)
    idx = rng.integers(0, rows, int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    w = rng.standard_normal(len(idx)).astype(np.float32)
    pad = 11
    idx[::7] = pad                            # padding entries, some bags of padding only
    return table, idx, off, w, pad


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["sum", "mean", "max", "weighted"])
@pytest.mark.parametrize("table_dtype", [np.float32, np.float16])
@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("use_pad", [False, True])
def test_pooled_modes_match_torch(eng, shape, mode, table_dtype, id_dtype, use_pad):
    table, idx, off, w, pad = make(shape, sum(map(ord, shape + mode)))
    table = table.astype(table_dtype)
    eng.load_table(0, table)
    pad = pad if use_pad else None
    if mode == "sum" and not use_pad:
        pad = 0 if shape == "onehot" else None   # (a plain sum spec is the sum path itself: give it something to skip)
    weighted = mode == "weighted"
    m = "sum" if weighted else mode
    i = torch.as_tensor(idx).to(id_dtype).to(DEV)
    o = torch.as_tensor(off).to(id_dtype).to(DEV)
    wt = torch.as_tensor(w).to(DEV) if weighted else None
    got = eng.lookup_pooled([0], [i], [o], m, per_sample_weights=None if wt is None else [wt], padding_idx=pad)[0]
    torch.cuda.synchronize()
    want = torch_ref(table.astype(np.float32), idx, off, m, w if weighted else None, pad)
    assert same(got, want)


def test_paths_taken(eng, pel):
    """The shapes above do reach the three kernel families (kind 0 wave-batch, 1 lane-group, 3 any-dim)."""
    from pim_embedding_lookup_amd import codeobj
    kinds = {}
    for shape in ("onehot", "ragged", "anydim3", "anydim30"):
        table, idx, off, w, pad = make(shape, 1)
        eng.load_table(1, table)
        i, o = torch.as_tensor(idx).to(DEV), torch.as_tensor(off).to(DEV)
        p = eng.plan_pooled([1], [i], [o], "sum", per_sample_weights=[torch.as_tensor(w).to(DEV)])
        recs = p.describe()
        assert len(recs) == 1 and recs[0]["pool"] == 0 and recs[0]["weighted"] == 1 and recs[0]["padding"] == 0
        kinds[shape] = recs[0]["kind"]
        sym, _ = codeobj.kernel_of_launch(pel.LIB_PATH, recs[0])
        assert "bag_pool_" in sym
        # algorithmic bytes: the sum plan's + 4 per weight
        q = eng.plan([1], [i], [o])
        assert p.bytes()[0] == q.bytes()[0] + 4 * len(idx)
        p.destroy()
        q.destroy()
    assert kinds == {"onehot": 0, "ragged": 1, "anydim3": 3, "anydim30": 3}


def test_mixed_modes_same_table_twice_one_call(eng):
    table, idx, off, w, pad = make("ragged", 5)
    eng.load_table(2, table)
    i, o, wt = torch.as_tensor(idx).to(DEV), torch.as_tensor(off).to(DEV), torch.as_tensor(w).to(DEV)
    modes = ["mean", "max", "sum", "sum"]
    outs = eng.lookup_pooled([2, 2, 2, 2], [i] * 4, [o] * 4, modes, per_sample_weights=[None, None, wt, None],
                             padding_idx=[pad, None, pad, None])
    torch.cuda.synchronize()
    assert same(outs[0], torch_ref(table, idx, off, "mean", None, pad))
    assert same(outs[1], torch_ref(table, idx, off, "max"))
    assert same(outs[2], torch_ref(table, idx, off, "sum", w, pad))
    assert same(outs[3], torch_ref(table, idx, off, "sum"))


def test_host_memspace(eng):
    table, idx, off, w, pad = make("ragged", 6)
    eng.load_table(3, table)
    for dt in (np.uint32, np.int64):
        outs = eng.lookup_pooled([3, 3, 3], [idx.astype(dt)] * 3, [off.astype(dt)] * 3, ["sum", "mean", "max"],
                                 per_sample_weights=[w, None, None], padding_idx=[None, pad, pad])
        assert isinstance(outs[0], np.ndarray)
        assert same(outs[0], torch_ref(table, idx, off, "sum", w))
        assert same(outs[1], torch_ref(table, idx, off, "mean", None, pad))
        assert same(outs[2], torch_ref(table, idx, off, "max", None, pad))


def test_pooled_plan_in_a_cuda_graph(eng):
    table, idx, off, w, pad = make("onehot", 7)
    eng.load_table(4, table)
    i, o, wt = torch.as_tensor(idx).to(DEV), torch.as_tensor(off).to(DEV), torch.as_tensor(w).to(DEV)
    out = torch.empty((len(off), table.shape[1]), device=DEV)
    plan = eng.plan_pooled([4], [i], [o], "sum", per_sample_weights=[wt], outs=[out])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.launch(s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s.cuda_stream)
    wt.mul_(0.5)                                  # new values in the same buffers: the replay reads them
    out.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert same(out, torch_ref(table, idx, off, "sum", (w * np.float32(0.5)).astype(np.float32)))
    plan.destroy()


def test_hot_rows_table_takes_the_pooled_kernel(eng):
    table, idx, off, w, pad = make("ragged", 8)
    eng.load_table(5, table)
    eng.set_hot_rows(5, np.arange(0, 64, dtype=np.uint64))
    i, o = torch.as_tensor(idx).to(DEV), torch.as_tensor(off).to(DEV)
    p = eng.plan_pooled([5], [i], [o], "mean", padding_idx=pad)
    assert [r["kind"] for r in p.describe()] == [1]
    p.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert same(p.outputs[0], torch_ref(table, idx, off, "mean", None, pad))
    p.destroy()
    q = eng.plan([5], [i], [o])                   # (the sum path keeps its hot-row kernel)
    assert [r["kind"] for r in q.describe()] == [4]
    q.destroy()


@pytest.mark.parametrize("check", [True, "deferred"])
def test_checked_calls_refuse_a_bad_index(eng, check):
    table, idx, off, w, pad = make("ragged", 9)
    eng.load_table(6, table)
    bad = idx.copy()
    bad[17] = table.shape[0] + 5
    i, o = torch.as_tensor(bad).to(DEV), torch.as_tensor(off).to(DEV)
    out = torch.full((len(off), table.shape[1]), 3.0, device=DEV)
    with pytest.raises(IndexError):
        eng.lookup_pooled([6], [i], [o], "max", padding_idx=pad, outs=[out], check=check)
        if check == "deferred":
            eng.check_report()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())               # nothing gathered
    good = torch.as_tensor(idx).to(DEV)
    res = eng.lookup_pooled([6], [good], [o], "max", padding_idx=pad, check=check)[0]
    if check == "deferred":
        eng.check_report()
    torch.cuda.synchronize()
    assert same(res, torch_ref(table, idx, off, "max", None, pad))


def test_all_sum_specs_are_the_sum_plan(eng):
    table, idx, off, w, pad = make("onehot", 10)
    eng.load_table(7, table)
    i, o = torch.as_tensor(idx).to(DEV), torch.as_tensor(off).to(DEV)
    out = torch.empty((len(off), table.shape[1]), device=DEV)
    a = eng.plan([7, 7], [i, i], [o, o], outs=[out, out])
    b = eng.plan_pooled([7, 7], [i, i], [o, o], "sum", outs=[out, out])
    assert a.signature() == b.signature()
    assert a.describe() == b.describe() and "pool" not in b.describe()[0]
    c = eng.plan_pooled([7, 7], [i, i], [o, o], ["sum", "mean"], outs=[out, out])
    assert c.signature() != a.signature()
    for p in (a, b, c):
        p.destroy()


def test_sum_and_pooled_calls_alternate_on_the_same_tensors(pel):
    """The per-call plan cache never replays a sum plan for a pooled call or the other way round.  (An engine of its own:
    the module's engine has its cache filled by the calls above.)"""
    eng = pel.EmbeddingEngine(device=0, max_tables=16)
    table, idx, off, w, pad = make("ragged", 11)
    eng.load_table(8, table)
    i, o, wt = torch.as_tensor(idx).to(DEV), torch.as_tensor(off).to(DEV), torch.as_tensor(w).to(DEV)
    out = torch.empty((len(off), table.shape[1]), device=DEV)
    want_sum = torch_ref(table, idx, off, "sum")
    want = {"mean": torch_ref(table, idx, off, "mean", None, pad), "max": torch_ref(table, idx, off, "max", None, pad),
            "w": torch_ref(table, idx, off, "sum", w)}
    hits0 = eng.plan_cache_hits
    for _ in range(4):
        eng.lookup_batched([8], [i], [o], outs=[out])
        torch.cuda.synchronize()
        assert same(out, want_sum)
        for k in ("mean", "max"):
            eng.lookup_pooled([8], [i], [o], k, padding_idx=pad, outs=[out])
            torch.cuda.synchronize()
            assert same(out, want[k])
        eng.lookup_pooled([8], [i], [o], "sum", per_sample_weights=[wt], outs=[out])
        torch.cuda.synchronize()
        assert same(out, want["w"])
    assert eng.plan_cache_hits > hits0            # (the cache was in play)
    eng.close()


def test_refusals(eng, pel):
    table, idx, off, w, pad = make("ragged", 12)
    eng.load_table(9, table)
    eng.load_table(10, np.zeros((100, 16), np.int32))
    i, o, wt = torch.as_tensor(idx).to(DEV), torch.as_tensor(off).to(DEV), torch.as_tensor(w).to(DEV)
    with pytest.raises(pel.lib.PimembError) as ex:
        eng.lookup_pooled([9], [i], [o], "mean", per_sample_weights=[wt])
    assert ex.value.code == pel.lib.EMB_ERR_INVALID
    with pytest.raises(pel.lib.PimembError) as ex:
        eng.lookup_pooled([9], [i], [o], "max", padding_idx=table.shape[0])
    assert ex.value.code == pel.lib.EMB_ERR_INVALID
    small = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(pel.lib.PimembError) as ex:
        eng.lookup_pooled([10], [small], [torch.arange(4, device=DEV)], "mean")
    assert ex.value.code == pel.lib.EMB_ERR_UNSUPPORTED


def test_pooling_embedding_bag_from_torch(pel):
    from pim_embedding_lookup_amd.torch_module import PoolingEmbeddingBag
    torch.manual_seed(0)
    for mode, pad, last in (("mean", 3, False), ("max", -2, True), ("sum", None, False), ("sum", 4, True)):
        ref = torch.nn.EmbeddingBag(200, 24, mode=mode, padding_idx=pad, include_last_offset=last)
        mine = PoolingEmbeddingBag.from_torch(ref)
        idx = torch.randint(0, 200, (500,))
        idx[::5] = ref.padding_idx if pad is not None else 0
        off = torch.tensor([0, 0, 7, 40, 41, 300])
        if last:
            off = torch.cat([off, torch.tensor([500])])
        psw = torch.randn(500) if mode == "sum" else None
        want = ref(idx, off, per_sample_weights=psw).detach()
        got = mine(idx.to(DEV), off.to(DEV), per_sample_weights=None if psw is None else psw.to(DEV))
        assert same(got, want), (mode, pad, last)
        if not last:       # 2-D input
            x2 = idx[:480].reshape(40, 12)
            w2 = None if psw is None else psw[:480].reshape(40, 12)
            assert same(mine(x2.to(DEV), per_sample_weights=None if w2 is None else w2.to(DEV)),
                        ref(x2, per_sample_weights=w2).detach())
        if mode != "sum":
            with pytest.raises(NotImplementedError):
                mine(idx.to(DEV), off.to(DEV), per_sample_weights=torch.ones(500, device=DEV))
    # checkpoints: the same key and shape as nn.EmbeddingBag
    sd = mine.state_dict()
    assert list(sd) == ["weight"] and torch.equal(sd["weight"].cpu(), ref.weight.detach())
    other = PoolingEmbeddingBag(200, 24, mode="sum", padding_idx=-196)
    assert other.padding_idx == 4                 # negative padding_idx counts from the end, as in torch
    other.load_state_dict(sd)
    assert torch.equal(other.weight.cpu(), ref.weight.detach())


def test_fused_pooling_bags_mixed_modes(pel):
    from pim_embedding_lookup_amd.torch_module import FusedPoolingEmbeddingBags
    torch.manual_seed(1)
    refs = [torch.nn.EmbeddingBag(300, 16, mode="sum"), torch.nn.EmbeddingBag(50, 16, mode="mean", padding_idx=2),
            torch.nn.EmbeddingBag(80, 32, mode="max"), torch.nn.EmbeddingBag(90, 16, mode="sum", padding_idx=0)]
    fused = FusedPoolingEmbeddingBags.from_torch(refs)
    lS_i = [torch.randint(0, r.num_embeddings, (400,)) for r in refs]
    lS_o = [torch.sort(torch.randint(0, 400, (64,))).values.clamp(max=399) for _ in refs]
    for o in lS_o:
        o[0] = 0
    lS_w = [torch.randn(400), None, None, torch.randn(400)]
    want = [r(i, o, per_sample_weights=w).detach() for r, i, o, w in zip(refs, lS_i, lS_o, lS_w)]
    got = fused([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i], [None if w is None else w.to(DEV) for w in lS_w])
    for g, w in zip(got, want):
        assert same(g, w)


def test_c2_weighted_and_c3_mean_in_full(eng):
    """C2: 26 Kaggle-sized tables, dim 16, B = 39 292, one index per bag, weighted (DLRM --weighted-pooling); a C3-like
    shape: dim 128, pooling 32, mean.  Every output checked."""
    from pim_embedding_lookup_amd import workloads
    rng = np.random.default_rng(2)
    rows = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306, 10,
            5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]
    B = 39292
    ids, idxs, offs, ws, tabs = [], [], [], [], []
    for t, n in enumerate(rows):
        n = min(n, 200000)                            # (row counts capped: the check is about the arithmetic)
        tabs.append(rng.standard_normal((n, 16)).astype(np.float32))
        eng.load_table(20 + t, tabs[-1])
        ids.append(20 + t)
        idxs.append(rng.integers(0, n, B))
        offs.append(np.arange(B))
        ws.append(rng.standard_normal(B).astype(np.float32))
    got = eng.lookup_pooled(ids, [torch.as_tensor(x).to(DEV) for x in idxs], [torch.as_tensor(x).to(DEV) for x in offs],
                            "sum", per_sample_weights=[torch.as_tensor(x).to(DEV) for x in ws])
    torch.cuda.synchronize()
    for t in range(len(rows)):
        assert same(got[t], torch_ref(tabs[t], idxs[t], offs[t], "sum", ws[t])), t
    table = rng.standard_normal((100000, 128)).astype(np.float32)
    eng.load_table(50, table)
    Bc, L = 4096, 32
    idx = rng.integers(0, 100000, Bc * L)
    off = np.arange(0, Bc * L, L)
    got = eng.lookup_pooled([50, 50], [torch.as_tensor(idx).to(DEV)] * 2, [torch.as_tensor(off).to(DEV)] * 2, "mean",
                            padding_idx=[None, int(idx[5])])
    torch.cuda.synchronize()
    assert same(got[0], torch_ref(table, idx, off, "mean"))
    assert same(got[1], torch_ref(table, idx, off, "mean", None, int(idx[5])))
    _ = workloads


def test_harness_weighted_pooling_learned_from_checkpoint(tmp_path):
    from importlib import import_module
    hz = import_module("pim-embedding-lookup_amd.dlrm_harness")
    formats = import_module("pim-embedding-lookup_amd.formats")
    rng = np.random.default_rng(3)
    ln = [300, 1000, 50]
    tables = [rng.standard_normal((n, 16)).astype(np.float32) for n in ln]
    v_W = [rng.standard_normal(n).astype(np.float32) for n in ln]
    path = str(tmp_path / "weighted.pt")
    formats.save_dlrm_embedding_weights(path, tables, pooling_weights=v_W)
    ebc = hz.EmbeddingBagCollection.from_checkpoint(path, weighted_pooling="learned")
    lS_i = [torch.as_tensor(rng.integers(0, n, 200)) for n in ln]
    lS_o = [torch.as_tensor(np.sort(rng.integers(0, 200, 32))) for _ in ln]
    for o in lS_o:
        o[0] = 0
    ly = ebc.apply_emb([o.to(DEV) for o in lS_o], [i.to(DEV) for i in lS_i])
    for k in range(len(ln)):        # torch-CPU apply_emb with DLRM's weighted pooling
        w = torch.as_tensor(v_W[k]).gather(0, lS_i[k])
        want = F.embedding_bag(lS_i[k], torch.as_tensor(tables[k]), lS_o[k], mode="sum", per_sample_weights=w)
        assert same(ly[k], want), k
    ebc.close()
    assert hz.main([f"--load-model={path}", "--weighted-pooling=learned", "--mini-batch-size=8", "--num-batches=2",
                    "--inference-only"]) == 0
