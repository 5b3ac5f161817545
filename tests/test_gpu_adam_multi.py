"""GPU: the multi-table Adam steps (emb_grad_adam_step_multi, include/pimemb_grad.h), bit for bit.  One adam_step(multi=True) steps tables
A; adam_step without it steps twin tables B loaded with the same bytes; whole tables, whole exp_avg and whole exp_avg_sq are compared with
each other and with tests/adam_ref.py over tests/grad_ref.py (position order) or tests/grad_seg_ref.py (segmented).  The batch is
tests/grad_cases.py's, laid over tables of 3001, 257 and 4099 rows as tests/test_gpu_grad_multi.py lays it.  No tolerance anywhere."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as ar  # noqa: E402
import grad_cases as gc  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
from grad_gpu import DEV, F, check_state, check_table, host, load_bytes, table_bytes  # noqa: E402
from test_gpu_adam import check  # noqa: E402
from test_gpu_grad_multi import A0, B0, Desc, init_table, once  # noqa: E402

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, S = 0.05, (0.9, 0.99), 1e-6, 8
ROWS, KINDS = (3001, 257, 4099), ("f32", "bf16", "f16")      # key bases 3001 and 3258: no multiples of 256; one group, three dtypes


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["position", "segmented"])
def ctx(eng, request):
    kw = dict(order="segmented", segment=S, max_dim=512) if request.param == "segmented" else {}
    c = eng.grad_context(8192, 1024, **kw)      # (c.segment: S, or None in the position order)
    yield c
    c.close()


def fresh(eng, kinds, descs, tables, rowwise):
    """Tables A and their twins B loaded with the same bytes; ([inits], [(M, V) of A], [(M, V) of B]), the moments zeros."""
    first = [tables.index(t) for t in range(max(tables) + 1)]
    inits = [init_table(kinds[t], descs[j].nr, descs[j].dim) for t, j in enumerate(first)]
    for t, init in enumerate(inits):
        load_bytes(eng, A0 + t, kinds[t], init)
        load_bytes(eng, B0 + t, kinds[t], init)
    zeros = lambda: [(torch.zeros((descs[j].nr, descs[j].dim), device=DEV), torch.zeros((descs[j].nr,) if rowwise else (descs[j].nr, descs[j].dim), device=DEV))  # noqa: E731
                     for j in first]
    return inits, zeros(), zeros()


def adam(c, base, tables, dev, descs, st, t, rowwise, multi, **kw):
    idx, off, G, w = ([x[j] for x in dev] for j in range(4))
    c.adam_step([base + k for k in tables], idx, off, G, [st[k][0] for k in tables], [st[k][1] for k in tables], LR, betas=BETAS, eps=EPS, step=t,
                rowwise=rowwise, modes=[d.mode for d in descs], per_sample_weights=w, padding_idx=[d.pad for d in descs], multi=multi, **kw)


def twins_equal(eng, sA, sB, what):
    for t in range(len(sA)):
        check_table(table_bytes(eng, A0 + t), table_bytes(eng, B0 + t), (what, t))
        check_state(sA[t][0], host(sB[t][0]), (what, t, "exp_avg"))
        check_state(sA[t][1], host(sB[t][1]), (what, t, "exp_avg_sq"))


def sparse_of(d, segment):
    if not segment:
        return d.sparse()
    return once(("seg", segment) + d.key, lambda: sr.seg_sparse_grad(d.nr, d.ids, d.offsets, d.G, segment, d.mode, d.w, d.pad, n_bags=d.n_bags))


@pytest.mark.parametrize("width", ["u32", "i64"])
@pytest.mark.parametrize("dim", [12, 128, 320])        # three pieces on four lanes; a full half wavefront; two pieces for 16 of 64 lanes
@pytest.mark.parametrize("rowwise", [False, True])
def test_multi_equals_the_single_calls_and_the_definition_over_two_steps(eng, ctx, rowwise, dim, width):
    descs = [Desc(3001, "sum", width, dim, overflow=False), Desc(257, "weighted+pad", width, dim, lead=True, overflow=False),
             Desc(4099, "mean", width, dim, overflow=False)]
    assert descs[1].offsets[0] == 3 and descs[0].ids.count(gc.HOT) > S + 1
    tables = [0, 1, 2]
    inits, sA, sB = fresh(eng, KINDS, descs, tables, rowwise)
    want = [(inits[t], host(sA[t][0]), host(sA[t][1])) for t in tables]
    dev = [d.on_device() for d in descs]
    ctx.report()
    ref_rows = 0
    for t in (1, 2):                                   # (the second step meets non-zero moments)
        adam(ctx, A0, tables, dev, descs, sA, t, rowwise, True)
        adam(ctx, B0, tables, dev, descs, sB, t, rowwise, False)
        twins_equal(eng, sA, sB, (rowwise, dim, width, t))
        for k, d in enumerate(descs):
            rows, grads, _ = sparse_of(d, ctx.segment)
            want[k] = ar.adam_step(KINDS[k], *want[k], rows, grads, LR, BETAS, EPS, t, rowwise=rowwise)
            ref_rows += len(rows)
            assert (want[k][0] != inits[k]).any()
            check(eng, A0 + k, *sA[k], want[k], (rowwise, dim, width, t, k), nan_kind=KINDS[k])
    assert ref_rows > 2 * 1000 and ctx.report() == 4 * sum(d.sparse()[2] for d in descs)
    assert ctx.multi_groups([A0, A0 + 1, A0 + 2], [len(d.ids) for d in descs], [d.n_bags for d in descs]) == [0, 0, 0]


def tiny(t):
    rng = np.random.default_rng(170 + t)
    off = np.concatenate([[0], np.sort(rng.integers(0, 50, size=9))]).astype(np.int64)
    return Desc(64, "sum", "i64", 16, G=rng.standard_normal((10, 16)).astype(F), ids=rng.integers(0, 64, size=50).tolist(), offsets=off)


def plain(nr, mode, dim=16, **kw):
    return Desc(nr, mode, "i64", dim, overflow=False, **kw)


# name -> (descriptors, the table of each, rowwise, lane_group of each, the expected groups)
EDGES = {
    "twice": (lambda: [plain(3001, "sum"), plain(257, "sum"), plain(3001, "mean+pad")], [0, 1, 0], False, True, [0, 0, 1]),
    "other dim": (lambda: [plain(3001, "sum"), plain(257, "mean", 8), plain(4099, "sum")], [0, 1, 2], True, True, [0, 1, 2]),
    "empty": (lambda: [plain(3001, "sum"), plain(257, "sum", ids=[], offsets=np.zeros(4, np.int64), G=np.zeros((4, 16), F)), plain(4099, "mean")],
              [0, 1, 2], True, True, [0, None, 0]),
    "seventeen": (lambda: [tiny(t) for t in range(17)], list(range(17)), False, True, [0] * 16 + [1]),
    "dim 6": (lambda: [plain(3001, "sum"), plain(257, "weighted", 6), plain(4099, "sum")], [0, 1, 2], False, [True, False, True], [0, 1, 2]),
    "dim 6 row-wise": (lambda: [plain(3001, "sum"), plain(257, "weighted", 6), plain(4099, "sum")], [0, 1, 2], True, [True, False, True], None),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_grouping_edges_split_as_stated_and_equal_the_single_calls(eng, ctx, pel, edge):
    make, tables, rowwise, lane, groups = EDGES[edge]
    descs = make()
    kinds = [KINDS[t % 3] for t in range(max(tables) + 1)]
    inits, sA, sB = fresh(eng, kinds, descs, tables, rowwise)
    dev = [d.on_device() for d in descs]
    if groups is None:                                 # refused as a whole: every table and state as it was
        with pytest.raises(pel.PimembError, match="lane-group shape") as ei:
            adam(ctx, A0, tables, dev, descs, sA, 1, rowwise, True)
        assert ei.value.code == pel.lib.EMB_ERR_UNSUPPORTED
        twins_equal(eng, sA, sB, edge)
        return
    assert ctx.multi_groups([A0 + t for t in tables], [len(d.ids) for d in descs], [d.n_bags for d in descs], lane_group=lane) == groups
    adam(ctx, A0, tables, dev, descs, sA, 1, rowwise, True)
    adam(ctx, B0, tables, dev, descs, sB, 1, rowwise, False)
    twins_equal(eng, sA, sB, edge)
    assert all((table_bytes(eng, A0 + t) != inits[t]).any() for t in set(tables) if len(descs[tables.index(t)].ids))
    ctx.report()


def test_a_captured_multi_step_replays_with_new_gradients_and_step_sizes(eng, ctx):
    """Row-wise, three tables, ONE captured multi step replayed for t = 1, 2, 3 against three eager per-table steps on the twins."""
    dim, tables = 16, [0, 1, 2]
    descs = [plain(nr, m) for nr, m in zip(ROWS, ("sum", "weighted+pad", "mean"))]
    _inits, sA, sB = fresh(eng, KINDS, descs, tables, True)
    dev = [d.on_device() for d in descs]
    Gs = [[(x[2] * s).contiguous() for x in dev] for s in (1.0, -0.5, 3.0)]
    ss_dev, stream = torch.zeros(1, dtype=torch.float32, device=DEV), torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        adam(ctx, A0, tables, dev, descs, sA, 1, True, True, step_size_dev=ss_dev, stream=stream.cuda_stream)
    for t in (1, 2, 3):
        with torch.cuda.stream(stream):
            for x, G in zip(dev, Gs[t - 1]):
                x[2].copy_(G)
            ss_dev.fill_(ctx.adam_constants(LR, BETAS, EPS, t)[2])
            graph.replay()
        torch.cuda.synchronize()
        adam(ctx, B0, tables, dev, descs, sB, t, True, False)
        twins_equal(eng, sA, sB, ("replay", t))
    assert sA[1][1].any()
    ctx.report()


tm = import_module("pim-embedding-lookup_amd.torch_module")


def test_fused_module_with_multi_table_equals_the_module_without(eng):
    names = ["sum", "mean", "sum+pad"]
    batches = [gc.exact_batch(gc.MODES[m][2]) for m in names]
    lS_i, lS_o = [torch.from_numpy(b[0]).to(DEV) for b in batches], [torch.from_numpy(b[1]).to(DEV) for b in batches]
    wide = torch.from_numpy(np.concatenate([batches[0][2], batches[1][2] * 3, -batches[2][2]], axis=1) * F(0.37)).to(DEV)
    results = []
    for multi, base in ((True, 40), (False, 44)):
        bags = [tm.PoolingEmbeddingBag(gc.EXACT_ROWS, 8, mode=gc.MODES[m][0], padding_idx=gc.PAD if gc.MODES[m][2] else None,
                                       _weight=torch.from_numpy(gc.exact_table().copy()), engine=eng, table_id=base + k,
                                       dtype=torch.float32 if k != 1 else torch.bfloat16) for k, m in enumerate(names)]
        fused = tm.FusedPoolingEmbeddingBags(bags, concat=True).enable_fused_adam(LR, betas=BETAS, eps=EPS, multi_table=multi)
        for _ in range(2):
            (fused(lS_o, lS_i) * wide).sum().backward()
        torch.cuda.synchronize()
        results.append([(b.weight.cpu().contiguous().view(torch.uint8).numpy().copy(), host(b.adam_exp_avg), host(b.adam_exp_avg_sq), b.adam_step)
                        for b in fused.bags])
    for a, b in zip(*results):
        assert np.array_equal(a[0], b[0]) and a[3] == b[3] == 2 and a[1].any()
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    with pytest.raises(ValueError):
        fused.enable_fused_adam(LR, multi_table=True, master_weights=True)


def test_harness_runs_adam_with_the_multi_table_step():
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    assert h.main(["--arch-sparse-feature-size=16", "--arch-embedding-size=1000-2000-300", "--mini-batch-size=64", "--num-batches=2",
                   "--num-indices-per-lookup=4", "--fused-adam", "0.01", "--multi-table-step"]) == 0
