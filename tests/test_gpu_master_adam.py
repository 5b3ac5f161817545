"""GPU: the fused master-weight Adam steps (include/pimemb_grad.h, THE MASTER-WEIGHT ADAM STEPS; GradContext.master_adam_step) bit for bit
against tests/master_adam_ref.py, over the whole table, master, exp_avg and exp_avg_sq, three steps (t = 1, 2, 3) each.
One engine, a position-order context and a segmented one (S = 8), one stream.  Tables of 300 rows, train_ref's batches (ragged and empty
bags, padding, weights, mean, three bad ids of full width, row HOT 21 times: more than S + 1).  Both reports are asserted."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import master_adam_ref as mar  # noqa: E402
import rows_cases as rc  # noqa: E402
import train_ref as tr  # noqa: E402
from grad_gpu import DEV, F, bits, check_table, in_place, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

N, T, S = tr.N_ROWS, 0, 8
LR, BETAS, EPS = 0.05, (0.5, 0.9), 1e-6     # betas far from 1: the moments of t = 1 weigh visibly in t = 2 and 3
UNSUPPORTED = -4                             # EMB_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctxs(eng):
    c = {"position": eng.grad_context(2048, 512), "segmented": eng.grad_context(2048, 512, order="segmented", segment=S, max_dim=512)}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream()


@pytest.fixture(autouse=True)
def counts_start_at_zero(ctxs):
    for c in ctxs.values():
        c.report()
        c.master_report()


def same_bits(got, want, what):
    got = got.cpu().numpy().reshape(want.shape)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, (what, "rows", bad[:8], got[bad[0]], want[bad[0]])


def misaligned(x):
    """The same values in a contiguous tensor whose address is 4 bytes past a 16-byte boundary."""
    buf = torch.empty((x.numel() + 8,), dtype=torch.float32, device=DEV)
    at = 1 + ((-buf.data_ptr() // 4) % 4)
    out = buf[at:at + x.numel()].view(x.shape)
    out.copy_(x)
    assert out.data_ptr() % 16 == 4
    return out


class Trained:
    """One table with its master and moments on the device, and the same four as the reference holds them."""

    def __init__(self, eng, kind, dim, rowwise, t=T, table=None, master=None):
        st = tr.initial_state(kind, dim)
        self.eng, self.t, self.kind, self.rowwise, self.steps = eng, t, kind, rowwise, 0
        self.table = st.table if table is None else table
        self.master = st.master if master is None else master
        self.m, self.v = mar.initial_moments(N, dim, rowwise)
        load_bytes(eng, t, kind, self.table)
        self.d_master, self.d_m, self.d_v = to_dev(self.master), to_dev(self.m), to_dev(self.v)

    def step(self, c, stream, idx, off, G, lr=LR, step=None, ss_dev=None, **kw):
        with torch.cuda.stream(stream):
            c.master_adam_step([self.t], [idx], [off], [G], [self.d_master], [self.d_m], [self.d_v], lr, betas=BETAS, eps=EPS,
                               step=self.steps + 1 if step is None else step, rowwise=self.rowwise, step_size_dev=ss_dev, stream=stream.cuda_stream, **kw)

    def advance(self, host, G, segment=None, lr=LR):
        ids, off, mode, w, pad = host
        self.steps += 1
        self.table, self.master, self.m, self.v, rows, n_bad, unenc = mar.master_adam_step(
            self.kind, self.table, self.master, self.m, self.v, ids, off, G, mode, w, pad, lr, BETAS, EPS, self.steps, self.rowwise, segment)
        return rows, n_bad, unenc

    def check(self, what):
        torch.cuda.synchronize()
        check_table(table_bytes(self.eng, self.t), self.table, what)
        for got, want, name in ((self.d_master, self.master, "master"), (self.d_m, self.m, "exp_avg"), (self.d_v, self.v, "exp_avg_sq")):
            same_bits(got, want, (what, name))


def dev_batch(b, G, mode_name, width):
    host = b.args(mode_name, width)
    _ids, _off, mode, w, pad = host
    kw = dict(modes=mode, per_sample_weights=None if w is None else [to_dev(w)], padding_idx=pad)
    return host, to_dev(b.ids_array(width)), to_dev(b.offsets_array(width)), to_dev(G), kw


# (kind, dim, rowwise, order, mode, id width): every dtype with both kinds in both orders.  Dims: 32 one MXFP4 block and 8 lanes; 96 idle
# lanes in the butterflies and a scale piece with padding; 320 two pieces per lane (MXFP4: the flag before the first table store); 512 the
# 16 scale bytes exactly; 4 and 48 the small groups of tests/test_gpu_master_step.py's table.
MAIN = (
    ("f16", 4, False, "position", "sum", "i64"), ("f16", 48, True, "position", "mean+pad", "u32"), ("f16", 320, False, "segmented", "weighted+pad", "u32"),
    ("f16", 96, True, "segmented", "sum", "i64"),
    ("bf16", 320, False, "position", "mean+pad", "u32"), ("bf16", 512, True, "position", "sum", "i64"), ("bf16", 48, False, "segmented", "sum", "i64"),
    ("bf16", 320, True, "segmented", "weighted+pad", "u32"),
    ("e4m3", 96, False, "position", "weighted+pad", "i64"), ("e4m3", 320, True, "position", "sum", "u32"), ("e4m3", 512, False, "segmented", "mean+pad", "i64"),
    ("e4m3", 32, True, "segmented", "mean+pad", "i64"),
    ("e5m2", 512, False, "position", "sum", "u32"), ("e5m2", 96, True, "position", "weighted+pad", "i64"), ("e5m2", 32, False, "segmented", "mean+pad", "u32"),
    ("e5m2", 320, True, "segmented", "sum", "i64"),
    ("mxfp4", 32, False, "position", "sum", "i64"), ("mxfp4", 96, True, "position", "mean+pad", "u32"), ("mxfp4", 320, False, "position", "weighted+pad", "i64"),
    ("mxfp4", 512, True, "position", "sum", "u32"), ("mxfp4", 320, True, "segmented", "mean+pad", "i64"), ("mxfp4", 512, False, "segmented", "sum", "u32"),
    ("mxfp4", 96, False, "segmented", "weighted+pad", "u32"), ("mxfp4", 32, True, "segmented", "sum", "i64"),
)


@pytest.mark.parametrize("kind,dim,rowwise,order,mode,width", MAIN, ids=["-".join(map(str, c)) for c in MAIN])
def test_master_adam_step_equals_the_reference(eng, ctxs, stream, kind, dim, rowwise, order, mode, width):
    tab = Trained(eng, kind, dim, rowwise)
    c = ctxs[order]
    start = [x.copy() for x in (tab.table, tab.master, tab.m, tab.v)]
    named = set()
    for b, G in tr.train_batches(kind, dim, 3):
        host, idx, off, dG, kw = dev_batch(b, G, mode, width)
        tab.step(c, stream, idx, off, dG, **kw)
        rows, n_bad, unenc = tab.advance(host, G, S if order == "segmented" else None)
        tab.check((kind, dim, rowwise, order, mode, width, b.k))
        named |= set(int(r) for r in rows)
        assert len(rows) > 60 and unenc == 0 and c.report() == n_bad == 3 and c.master_report() == 0
    out = np.array(sorted(set(range(N)) - named))            # rows outside U: all four arrays keep their bytes (the reference's and so the GPU's)
    assert len(out) > 20 and all(np.array_equal(a[out], b[out]) for a, b in zip(start, (tab.table, tab.master, tab.m, tab.v)))
    assert np.array_equal(tab.table[sorted(named)], rc.host_encode(kind, tab.master)[sorted(named)]) and tab.steps == 3


ELEM = (("e4m3", 7, "plain"), ("bf16", 5, "plain"), ("e5m2", 16, "grad view"), ("f16", 16, "master"), ("bf16", 16, "exp_avg_sq"))


@pytest.mark.parametrize("order", ["position", "segmented"])
@pytest.mark.parametrize("kind,dim,how", ELEM, ids=[f"{k}-{d}-{h}" for k, d, h in ELEM])
def test_the_element_wise_kernel(eng, ctxs, stream, kind, dim, how, order):
    """Off the lane-group shape: an odd dim, a gradient view, or a master or a V that is not 16-byte aligned -- EMB_ADAM, the same bits."""
    tab = Trained(eng, kind, dim, False)
    if how == "master":
        tab.d_master = misaligned(tab.d_master)
    if how == "exp_avg_sq":
        tab.d_v = misaligned(tab.d_v)
    for b, G in tr.train_batches(kind, dim, 3):
        host, idx, off, dG, kw = dev_batch(b, G, "mean+pad" if order == "position" else "sum", "i64")
        if how == "grad view":
            dG = in_place(dG, 20, 1)                           # ld 20, column 1: 4 bytes past a 16-byte boundary
        tab.step(ctxs[order], stream, idx, off, dG, **kw)
        tab.advance(host, G, S if order == "segmented" else None)
        tab.check((kind, dim, how, order, b.k))
        assert ctxs[order].report() == 3 and ctxs[order].master_report() == 0


@pytest.mark.parametrize("kind,dim,rowwise,how", [("e4m3", 7, True, "plain"), ("bf16", 16, True, "master"), ("mxfp4", 32, False, "master"),
                                                  ("mxfp4", 32, False, "grad view"), ("mxfp4", 32, False, "exp_avg_sq"), ("f16", 16, True, "grad view")])
def test_off_the_lane_group_shape_rowwise_and_mxfp4_are_refused_and_write_nothing(pel, eng, ctxs, stream, kind, dim, rowwise, how):
    tab = Trained(eng, kind, dim, rowwise)
    if how == "master":
        tab.d_master = misaligned(tab.d_master)
    if how == "exp_avg_sq":
        tab.d_v = misaligned(tab.d_v)
    b, G = tr.train_batches(kind, dim, 1)[0]
    _host, idx, off, dG, kw = dev_batch(b, G, "sum", "i64")
    if how == "grad view":
        dG = in_place(dG, dim + 4, 1)
    with pytest.raises(pel.lib.PimembError) as ei:
        tab.step(ctxs["position"], stream, idx, off, dG, **kw)
    assert ei.value.code == UNSUPPORTED and "lane-group shape" in str(ei.value)
    tab.check((kind, dim, rowwise, how, "refused"))
    assert ctxs["position"].report() == 0 and ctxs["position"].master_report() == 0


@pytest.mark.parametrize("dim,rowwise", [(96, False), (320, False), (320, True)])
def test_an_mxfp4_row_whose_new_master_overflows_keeps_its_bytes(eng, ctxs, stream, dim, rowwise):
    """Five one-position bags at t = 1 with a huge lr: SparseAdam moves every element by lr * sign(g) = 1e38, row-wise Adam by lr * g / rms(g[r]),
    at most about 4e37 for the ordinary gradients and 1.2e38 for the crafted element.  Row 9 holds 3e38 in an element of its LAST block and
    a gradient of -4 there (the others are about 0.25): P' = inf in that row alone.  Its table bytes are kept, its P', M' and V' are
    stored, and it is counted; the other four rows are written."""
    kind, lr = "mxfp4", 1.0e37 if rowwise else 1.0e38
    master = tr.initial_master(kind, dim).copy()
    ids = np.array([5, 9, 11, 13, 20], dtype=np.int64)
    off = np.arange(5, dtype=np.int64)
    G = (np.random.default_rng(77).standard_normal((5, dim)) * 0.25).astype(F)
    master[9, dim - 3], G[1, dim - 3] = F(3.0e38), F(-4.0)
    table = rc.host_encode(kind, master)
    tab = Trained(eng, kind, dim, rowwise, table=table, master=master)
    tab.step(ctxs["position"], stream, to_dev(ids), to_dev(off), to_dev(G), lr=lr)
    rows, n_bad, unenc = tab.advance((list(ids), off, "sum", None, None), G, lr=lr)
    assert list(rows) == list(ids) and n_bad == 0 and unenc == 1              # the reference alone: exactly one such row
    assert np.isinf(tab.master[9, dim - 3]) and np.isfinite(np.delete(tab.master, 9, axis=0)).all()
    tab.check((kind, dim, rowwise, "overflow"))
    got = table_bytes(eng, T)
    assert np.array_equal(got[9], table[9]) and not np.array_equal(got[5], table[5])
    assert tab.m[9].any() and tab.v[9].any() and ctxs["position"].report() == 0 and ctxs["position"].master_report() == 1


@pytest.mark.parametrize("kind,dim,rowwise,mode", [("mxfp4", 64, False, "mean+pad"), ("e4m3", 16, True, "sum")])
def test_a_captured_step_replays_with_a_new_step_size(eng, ctxs, stream, kind, dim, rowwise, mode):
    """One step captured with step_size_dev (torch's default capture error mode: an allocation, a copy or a wait inside the call fails the
    capture), replayed three times with a new gradient in the same buffer and the step size of t = 1, 2, 3 written between the replays:
    the bytes of three eager steps on a second table, and the reference's."""
    c = ctxs["position"]
    graphed, eager = Trained(eng, kind, dim, rowwise, t=T), Trained(eng, kind, dim, rowwise, t=1)
    Gs = tr.graph_grads(dim)
    b = tr.train_batches(kind, dim, 1)[0][0]
    host, idx, off, dG, kw = dev_batch(b, Gs[0], mode, "i64")
    ss_dev = torch.zeros((1,), dtype=torch.float32, device=DEV)
    warm = Trained(eng, kind, dim, rowwise, t=2)
    warm.step(c, stream, idx, off, dG, ss_dev=ss_dev, **kw)              # uncaptured, on a table of its own: the code objects are loaded
    torch.cuda.synchronize()
    assert c.report() == 3
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        graphed.step(c, stream, idx, off, dG, step=1000, ss_dev=ss_dev, **kw)      # (step's own size is not read: ss_dev is)
    graphed.check("the capture itself ran nothing")
    for t in (1, 2, 3):
        dG.copy_(to_dev(Gs[t]))
        ss_dev.fill_(c.adam_constants(LR, BETAS, EPS, t)[2])
        graph.replay()
        eager.step(c, stream, idx, off, dG, **kw)
        for tab in (graphed, eager):
            tab.advance(host, Gs[t])
            tab.check((kind, "replay" if tab is graphed else "eager", t))
        check_table(table_bytes(eng, T), table_bytes(eng, 1), ("graph against eager", t))
        assert c.report() == 6 and c.master_report() == 0


def test_a_pooling_bag_trains_an_fp8_table_with_master_weight_adam(pel, eng):
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    kind, dim, t = "e4m3", 16, 4
    bag = tm.PoolingEmbeddingBag(N, dim, mode="sum", _weight=torch.from_numpy(tr.initial_master(kind, dim).copy()), engine=eng, table_id=t,
                                 dtype=torch.float8_e4m3fn)
    bag.enable_fused_master_adam(LR, BETAS, EPS)
    table = table_bytes(eng, t)
    master = tr.decode(kind, table)
    same_bits(bag.master_weight, master, "the master starts as the decoded table")
    m, v = mar.initial_moments(N, dim, False)
    lb = tr.lookup_batch()
    idx, off = to_dev(lb.ids), to_dev(lb.offsets)
    for r in range(3):
        G = (np.random.default_rng(9400 + r).standard_normal((lb.B, dim)) * 0.5).astype(F)
        (bag(idx, off) * to_dev(G)).sum().backward()
        table, master, m, v, rows, n_bad, unenc = mar.master_adam_step(kind, table, master, m, v, lb.ids, lb.offsets, G, "sum", None, None, LR, BETAS, EPS, r + 1)
        torch.cuda.synchronize()
        check_table(table_bytes(eng, t), table, ("module", r))
        for got, want, name in ((bag.master_weight, master, "master"), (bag.adam_exp_avg, m, "exp_avg"), (bag.adam_exp_avg_sq, v, "exp_avg_sq")):
            same_bits(got, want, ("module", name, r))
        assert n_bad == 0 and unenc == 0 and len(rows) > 60 and bag.adam_step == r + 1
    assert np.array_equal(rc.host_encode(kind, bag.master_weight.cpu().numpy()), table_bytes(eng, t))      # enc(master_weight) == weight
    sd = bag.state_dict()
    assert set(sd) == {"weight", "master_weight", "adam_exp_avg", "adam_exp_avg_sq", "adam_step"} and int(sd["adam_step"]) == 3
    other = tm.PoolingEmbeddingBag(N, dim, mode="sum", engine=eng, table_id=5, dtype=torch.float8_e4m3fn)
    other.load_state_dict(sd)
    check_table(table_bytes(eng, 5), table, "loaded table")
    for got, want in ((other.master_weight, master), (other.adam_exp_avg, m), (other.adam_exp_avg_sq, v)):
        same_bits(got, want, "loaded")
    assert other.adam_step == 3
    bag.enable_fused_adam(LR)                                            # one fused optimizer at a time, in both directions
    assert bag._fused_master_adam is None and bag.master_weight is None
    assert bag.enable_fused_master_adam(LR)._fused_adam is None and bag.master_weight is not None
    with pytest.raises(ValueError, match="mode='max'"):
        tm.PoolingEmbeddingBag(N, dim, mode="max", engine=eng, table_id=6).enable_fused_master_adam(LR)
    with pytest.raises(ValueError, match="its own master"):
        tm.PoolingEmbeddingBag(N, dim, mode="sum", engine=eng, table_id=7).enable_fused_master_adam(LR)
