"""GPU: the multi-table sparse gradient (emb_grad_sparse_multi, include/pimemb_grad.h), bit for bit.  The raw call writes into buffers filled
with a sentinel; rows, gradients and counts are compared with the loop references (tests/grad_ref.py, position order; tests/grad_seg_ref.py,
segmented) or with a loop of emb_grad_sparse calls, and everything beyond |U_k| must still hold the sentinel.  No tolerance anywhere."""
import ctypes as C
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
from grad_gpu import CODE, DEV, F, bits, host, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu
S, SENT = 8, -77
_refs, _tables = {}, {}


@pytest.fixture(scope="module", params=["position", "segmented"])
def ctx(pel, request):      # a context of either order on an engine of its own (ctx.engine), which the tables below are allocated on
    eng = pel.EmbeddingEngine(device=0, max_tables=64)
    _tables.clear()
    yield eng.grad_context(8192, 1024, **(dict(order="segmented", segment=S, max_dim=512) if request.param == "segmented" else {}))
    eng.close()


class Batch:
    """One table's share of a call, on the host.  Every row occurs at most ceil(n / nr) + 1 times, but `hot`, which gets 25 good positions:
    three segments of S and one of one.  Positions before offsets[0] = lead have no bag; some ids are bad (uint32: the NEXT table's row 3 in
    key space; int64: row 3 plus 2^32); dead: only bad and padding positions.  Batches of one (nr, dim, kind, tag) name one table."""

    def __init__(self, nr, mode, dim, width, n, B, seed, weighted=False, pad=None, hot=None, dead=False, lead=3, tag=None, kind="f32"):
        rng = np.random.default_rng(seed)
        self.nr, self.mode, self.dim, self.B, self.pad, self.key, self.name = nr, mode, dim, B, pad, (nr, mode, dim, width, n, B, seed), (nr, dim, kind, tag)
        ids, bad = rng.permutation(np.arange(n) % nr).astype(np.int64), nr + 3 if width == "u32" else (1 << 32) + 3
        if dead:
            ids[:] = np.where(rng.random(n) < 0.5, bad, pad)
        elif n:
            ids[lead], ids[lead + 1], ids[lead + 5::41] = 0, nr - 1, bad
            if hot is not None:
                free = np.flatnonzero((ids != hot) & (ids > 0) & (ids < nr - 1) & (np.arange(n) > lead + 1))
                ids[free[7::3][:25 - int((ids[lead:] == hot).sum())]] = hot
                assert (ids[lead:] == hot).sum() == 25 and pad != hot
        self.ids = ids.astype(np.uint32 if width == "u32" else np.int64)
        self.off = np.concatenate([[lead], np.sort(rng.integers(lead, n, size=B - 1))]).astype(np.int64) if n else np.zeros(B, np.int64)
        self.G = rng.standard_normal((B, dim)).astype(F)
        self.w = rng.standard_normal(n).astype(F) if weighted else None

    def ref(self, segment):
        if self.key + (segment,) not in _refs:
            args = (self.nr, [int(i) for i in self.ids], self.off, self.G)
            _refs[self.key + (segment,)] = (sr.seg_sparse_grad(*args, segment, self.mode, self.w, self.pad, n_bags=self.B) if segment else
                                            gr.sparse_grad(*args, self.mode, self.w, self.pad, n_bags=self.B))
        return _refs[self.key + (segment,)]

    def table(self, eng):      # (allocated once; the call reads none of its bytes)
        if self.name not in _tables:
            _tables[self.name] = len(_tables)
            eng.alloc_table(_tables[self.name], self.nr, self.dim, CODE.get(self.name[2], 2))      # (2: EMB_FIXED32)
        return _tables[self.name]

    def on_device(self):
        return to_dev(self.ids), to_dev(self.off.astype(self.ids.dtype)), to_dev(self.G), None if self.w is None else to_dev(self.w)


def base(dim, width):      # 7, 300 and 70 000 rows: a composite key of 17 bits, three radix passes; a dead and an empty descriptor between them
    return [Batch(7, "sum", dim, width, 40, 8, 1, weighted=True), Batch(50, "sum", dim, width, 60, 10, 2, pad=1, dead=True),
            Batch(300, "mean", dim, width, 1500, 200, 3, pad=2, hot=150), Batch(11, "sum", dim, width, 0, 4, 4), Batch(70000, "sum", dim, width, 800, 100, 5)]


def fresh(bs):      # output buffers two rows longer than the capacity the call is told, and the counts, all holding the sentinel
    outs = [(torch.full((len(b.ids) + 2,), SENT, dtype=torch.int64, device=DEV), torch.full((len(b.ids) + 2, b.dim), float(SENT), device=DEV)) for b in bs]
    return outs, torch.full((len(bs),), SENT, dtype=torch.int64, device=DEV)


def enqueue(ctx, tables, bs, dev, outs, counts, caps=None, stream=None):      # the raw call over device tensors, a pure enqueue; returns its code
    idx, off, G, w = ([x[j] for x in dev] for j in range(4))
    arr, n, itype, on_dev, stream = ctx._step_descs(tables, idx, off, G, [b.mode for b in bs], w, [b.pad for b in bs], 0, stream, [])
    ptrs = lambda j: (C.c_void_p * n)(*[o[j].data_ptr() for o in outs])  # noqa: E731
    return ctx._G.emb_grad_sparse_multi(ctx._h, arr, n, itype, ptrs(0), ptrs(1), (C.c_uint64 * n)(*(caps or [len(b.ids) for b in bs])), counts.data_ptr(), stream)


def check(outs, counts, want, what):
    torch.cuda.synchronize()
    for k, ((rows, grads), (want_rows, want_grads)) in enumerate(zip(outs, want)):
        u = int(counts[k])
        assert u == len(want_rows), (what, k, u, len(want_rows))
        assert np.array_equal(host(rows[:u]), host(want_rows)) and (host(rows[u:]) == SENT).all(), (what, k, "rows")
        assert np.array_equal(bits(host(grads[:u])), bits(host(want_grads))) and (host(grads[u:]) == SENT).all(), (what, k, "grads")


def singles(ctx, tables, bs, dev):      # the per-table loop of emb_grad_sparse on the GPU
    return [ctx.sparse_grad(t, x[0], x[1], x[2], mode=b.mode, per_sample_weights=x[3], padding_idx=b.pad) for t, b, x in zip(tables, bs, dev)]


@pytest.mark.parametrize("width", ["u32", "i64"])
@pytest.mark.parametrize("dim", [4, 48, 128, 320])         # one lane; lanes without a piece; half a wavefront; two pieces per lane
def test_one_group_equals_the_definition(ctx, dim, width):
    bs = base(dim, width)
    tables, dev = [b.table(ctx.engine) for b in bs], [b.on_device() for b in bs]
    assert ctx.multi_groups(tables, [len(b.ids) for b in bs], [b.B for b in bs]) == [0, 0, 0, None, 0]
    want = [b.ref(ctx.segment) for b in bs]      # the key ranges touch: row 0 and the last row of every live table occur
    assert [len(w[0]) for w in want][1::2] == [0, 0] and all(w[0][0] == 0 and w[0][-1] == b.nr - 1 for w, b in zip(want[::2], bs[::2]))
    ctx.report()
    outs, counts = fresh(bs)
    assert enqueue(ctx, tables, bs, dev, outs, counts) == 0
    check(outs, counts, [w[:2] for w in want], (dim, width))
    assert ctx.report() == sum(w[2] for w in want) > 40      # every bad position counted once


def tiny(t, dim=16, nr=64, mode="sum", **kw):
    return Batch(nr, mode, dim, "i64", 50, 10, 100 + t, tag=t, **kw)


EDGES = {      # name -> (the descriptors, lane_group of each, the expected groups)
    "seventeen": (lambda: [tiny(t) for t in range(17)], True, [0] * 16 + [1]),
    "mixed dims": (lambda: [tiny(0, nr=300), tiny(1, dim=8, mode="mean"), tiny(2, nr=70000)], True, [0, 1, 2]),
    "dim 6": (lambda: [tiny(0, nr=300), tiny(4), tiny(1, dim=6, weighted=True), tiny(2), tiny(3, mode="mean")], [True, True, False, True, True], [0, 0, 1, 2, 2]),
    "twice": (lambda: [tiny(0, nr=300), tiny(1), Batch(300, "mean", 16, "i64", 50, 10, 9, pad=2, tag=0)], True, [0, 0, 1]),
    "dtypes": (lambda: [tiny(0, dim=32), tiny(1, dim=32, nr=300, kind="bf16"), tiny(2, dim=32, mode="mean", kind="mxfp4")], True, [0, 0, 0]),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_grouping_edges_split_as_stated_and_equal_a_loop_of_single_calls(ctx, edge):
    make, lane, groups = EDGES[edge]
    bs = make()
    tables, dev = [b.table(ctx.engine) for b in bs], [b.on_device() for b in bs]
    assert ctx.multi_groups(tables, [len(b.ids) for b in bs], [b.B for b in bs], lane_group=lane) == groups
    outs, counts = fresh(bs)
    assert enqueue(ctx, tables, bs, dev, outs, counts) == 0
    check(outs, counts, singles(ctx, tables, bs, dev), edge)
    assert int(counts.min()) > 0


@pytest.mark.parametrize("fault", ["fixed32 last", "capacity one short"])
def test_a_refused_call_writes_nothing(ctx, pel, fault):
    bs = [tiny(0, nr=300), tiny(1), tiny(2, kind="fixed32" if fault == "fixed32 last" else "f32")]
    outs, counts = fresh(bs)
    rc = enqueue(ctx, [b.table(ctx.engine) for b in bs], bs, [b.on_device() for b in bs], outs, counts, caps=None if fault == "fixed32 last" else [50, 49, 50])
    assert rc == (pel.lib.EMB_ERR_UNSUPPORTED if fault == "fixed32 last" else pel.lib.EMB_ERR_INVALID)
    torch.cuda.synchronize()
    assert (host(counts) == SENT).all() and all((host(r) == SENT).all() and (host(g) == SENT).all() for r, g in outs)


def test_a_captured_call_replays_with_new_gradients(ctx):
    bs = base(4, "i64")      # (a mean table: cnt is cleared; an empty descriptor: its count is cleared)
    tables, dev = [b.table(ctx.engine) for b in bs], [b.on_device() for b in bs]
    outs, counts = fresh(bs)
    assert enqueue(ctx, tables, bs, dev, outs, counts) == 0      # (every kernel of the chain has run once before the capture)
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        assert enqueue(ctx, tables, bs, dev, outs, counts, stream=stream.cuda_stream) == 0
    for scale in (-0.5, 3.0):
        with torch.cuda.stream(stream):
            for x, (rows, grads) in zip(dev, outs):
                x[2].mul_(scale), rows.fill_(SENT), grads.fill_(SENT)
            counts.fill_(SENT)
            graph.replay()
        torch.cuda.synchronize()
        check(outs, counts, singles(ctx, tables, bs, dev), ("replay", scale))
    assert int(counts[2]) > 200 and int(counts[3]) == 0


def test_the_python_layers_return_what_the_per_table_calls_return(ctx):
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    bs = [Batch(300, "sum", 16, "i64", 400, 60, 21, lead=0, weighted=True), Batch(7, "mean", 16, "i64", 400, 60, 22, pad=2, lead=0),
          Batch(5000, "sum", 8, "i64", 400, 60, 23, lead=0)]
    tables, dev = [b.table(ctx.engine) for b in bs], [b.on_device() for b in bs]
    same = lambda got, want: all(np.array_equal(host(g[0]), host(w[0])) and np.array_equal(bits(host(g[1])), bits(host(w[1]))) for g, w in zip(got, want))  # noqa: E731
    with ctx.engine.grad_context(2048, 256) as c:      # (the position order, as the module's own context)
        want, eng, kw = singles(c, tables, bs, dev), ctx.engine, dict(modes=[b.mode for b in bs], padding_idx=[b.pad for b in bs])
        assert same(c.sparse_grads(tables, *[[x[j] for x in dev] for j in range(3)], per_sample_weights=[x[3] for x in dev], **kw), want)
        assert same(c.sparse_grads(tables, [b.ids for b in bs], [b.off for b in bs], [b.G for b in bs], per_sample_weights=[b.w for b in bs], **kw), want)
        bags = [tm.PoolingEmbeddingBag(b.nr, b.dim, mode=b.mode, padding_idx=b.pad, engine=eng, table_id=60 + k) for k, b in enumerate(bs)]
        wide = torch.randn(60, 4 + 16 + 16 + 8, device=DEV)      # the [B, T*dim] gradient inside a wider buffer, read in place from column 4
        got = tm.FusedPoolingEmbeddingBags(bags, concat=True).sparse_grads([x[1] for x in dev], [x[0] for x in dev], wide, col=4)
        cols = [wide[:, 4:20], wide[:, 20:36], wide[:, 36:44]]
        assert same(got, [c.sparse_grad(60 + k, x[0], x[1], cols[k], mode=b.mode, padding_idx=b.pad) for k, (b, x) in enumerate(zip(bs, dev))])
    bags[1] = tm.PoolingEmbeddingBag(7, 16, mode="max", engine=eng, table_id=63)
    with pytest.raises(ValueError):
        tm.FusedPoolingEmbeddingBags(bags, concat=True).sparse_grads([x[1] for x in dev], [x[0] for x in dev], wide, col=4)
