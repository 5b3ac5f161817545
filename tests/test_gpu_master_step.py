"""GPU: the fused master-weight steps (include/pimemb_grad.h, THE MASTER-WEIGHT STEPS; GradContext.master_step) bit for bit against
tests/master_ref.py -- the suite's loop-form references put behind one another: the sparse gradient, the step on the fp32 master,
formats.py's encoders for the table row.
  1  every dtype and optimizer on the lane-group kernel, three iterations (the list MAIN)
  2  the same bytes as the documented recipe run on the GPU: emb_grad_sparse, two torch ops, the row writer
  3  a segmented context (S = 8) against the position order, on the witness gradients
  4  the element-wise kernel: odd dims, a gradient view or a master that is not 16-byte aligned; what it refuses
  5  the table is not read
  6  special values: overflow to inf, rows of zeros, subnormal results, ties of the stored format
  7  refusals that leave everything as it was
  8  stream order with a prepared plan, and the step captured in a graph
  9  the modules
One engine, a position-order context and a segmented one (S = 8), one stream.  Tables of 300 rows, batches of about 190 positions
(train_ref.Batch: ragged and empty bags, padding, bad ids of full width, positions before offsets[0], row HOT 21 times).  Whole
tables, masters and states are compared by their bytes; both reports are asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import master_ref as mr  # noqa: E402
import rows_cases as rc  # noqa: E402
import train_ref as tr  # noqa: E402
from grad_gpu import CODE, DEV, F, bits, check_state, check_table, in_place, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

N = tr.N_ROWS
LR, EPS = float(tr.LR), float(tr.EPS)
T = 0
UNSUPPORTED = -4                             # EMB_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.grad_context(2048, 512)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seg(eng):
    c = eng.grad_context(2048, 512, order="segmented", segment=8, max_dim=512)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream()


@pytest.fixture(autouse=True)
def counts_start_at_zero(ctx, seg):
    for c in (ctx, seg):
        c.report()
        c.master_report()


def same_bits(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    got = got.reshape(want.shape)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, (what, "rows", bad[:8], got[bad[0]], want[bad[0]])


class DevBatch:
    def __init__(self, b, G, mode_name, width="i64"):
        self.host = b.args(mode_name, width)
        _ids, _off, self.mode, w, self.pad = self.host
        self.idx, self.off, self.G = to_dev(b.ids_array(width)), to_dev(b.offsets_array(width)), to_dev(G)
        self.w = None if w is None else to_dev(w)
        self.G_host, self.n_bad = G, b.n_bad

    def kw(self):
        return dict(modes=self.mode, per_sample_weights=None if self.w is None else [self.w], padding_idx=self.pad)


class Trained:
    """One table with its master and optimizer state on the device, and the same three as the reference holds them."""

    def __init__(self, eng, kind, dim, optimizer, t=T, table=None, master=None):
        st = tr.initial_state(kind, dim)
        self.eng, self.t, self.kind, self.dim, self.optimizer = eng, t, kind, dim, optimizer
        self.table = st.table if table is None else table
        self.master = st.master if master is None else master
        self.opt = mr.initial_opt(optimizer, N, dim)
        load_bytes(eng, t, kind, self.table)
        self.d_master = to_dev(self.master)
        self.d_opt = None if self.opt is None else to_dev(self.opt)

    def step(self, c, b, stream, lr=LR):
        with torch.cuda.stream(stream):
            c.master_step([self.t], [b.idx], [b.off], [b.G], [self.d_master], lr, optimizer=self.optimizer,
                          states=None if self.d_opt is None else [self.d_opt], eps=EPS, stream=stream.cuda_stream, **b.kw())

    def advance(self, b, segment=None, lr=LR):
        ids, off, mode, w, pad = b.host
        self.table, self.master, self.opt, rows, n_bad, unenc = mr.master_step(self.kind, self.table, self.master, self.opt, ids, off, b.G_host, mode, w, pad,
                                                                              self.optimizer, lr=F(lr), segment=segment)
        return rows, n_bad, unenc

    def check(self, what):
        torch.cuda.synchronize()
        check_table(table_bytes(self.eng, self.t), self.table, what)
        same_bits(self.d_master, self.master, (what, "master"))
        if self.opt is not None:
            check_state(self.d_opt, self.opt, what)


# ---- 1: every dtype and optimizer on the lane-group kernel ----------------------------------------------------------------------------
# (kind, dim, optimizer, mode, id width).  Every dim with SGD and with row-wise on one dtype; every dtype at dims 48 and 288 (MXFP4: 96
# and 288); every dtype with every optimizer; the three modes and both widths spread over them.
MAIN = (
    ("f16", 4, "sgd", "sum", "i64"), ("f16", 4, "rowwise", "mean+pad", "u32"), ("f16", 48, "adagrad", "weighted+pad", "i64"),
    ("f16", 288, "rowwise", "sum", "u32"),
    ("bf16", 16, "sgd", "mean+pad", "u32"), ("bf16", 16, "rowwise", "weighted+pad", "i64"), ("bf16", 48, "sgd", "sum", "i64"),
    ("bf16", 48, "rowwise", "mean+pad", "i64"), ("bf16", 288, "adagrad", "sum", "u32"),
    ("e4m3", 256, "sgd", "weighted+pad", "i64"), ("e4m3", 256, "rowwise", "sum", "u32"), ("e4m3", 48, "adagrad", "mean+pad", "i64"),
    ("e4m3", 288, "sgd", "sum", "i64"), ("e4m3", 288, "rowwise", "weighted+pad", "u32"), ("e4m3", 512, "rowwise", "mean+pad", "u32"),
    ("e4m3", 512, "sgd", "sum", "i64"),
    ("e5m2", 16, "sgd", "mean+pad", "i64"), ("e5m2", 48, "rowwise", "sum", "i64"), ("e5m2", 288, "adagrad", "weighted+pad", "u32"),
    ("mxfp4", 32, "sgd", "sum", "i64"), ("mxfp4", 32, "rowwise", "weighted+pad", "u32"), ("mxfp4", 64, "sgd", "mean+pad", "u32"),
    ("mxfp4", 64, "rowwise", "sum", "i64"), ("mxfp4", 96, "sgd", "weighted+pad", "i64"), ("mxfp4", 96, "rowwise", "mean+pad", "u32"),
    ("mxfp4", 96, "adagrad", "sum", "i64"), ("mxfp4", 128, "sgd", "sum", "u32"), ("mxfp4", 128, "rowwise", "sum", "i64"),
    ("mxfp4", 288, "sgd", "mean+pad", "i64"), ("mxfp4", 288, "rowwise", "weighted+pad", "u32"), ("mxfp4", 288, "adagrad", "sum", "i64"),
    ("mxfp4", 512, "sgd", "sum", "i64"), ("mxfp4", 512, "rowwise", "mean+pad", "u32"),
)


def test_the_thinned_list_covers_what_it_has_to():
    for dims, kinds in (((4, 16, 48, 256, 288, 512), ("f16", "bf16", "e4m3", "e5m2")), ((32, 64, 96, 128, 288, 512), ("mxfp4",))):
        for dim in dims:
            assert any({(k, dim, "sgd"), (k, dim, "rowwise")} <= {c[:3] for c in MAIN} for k in kinds), dim
    for k in mr.KINDS:
        assert {o for kk, _d, o, _m, _w in MAIN if kk == k} == set(mr.OPTIMIZERS), k
        assert {96 if k == "mxfp4" else 48, 288} <= {d for kk, d, *_ in MAIN if kk == k}, k
    assert {m for *_, m, _w in MAIN} == {"sum", "mean+pad", "weighted+pad"} and {w for *_, w in MAIN} == {"u32", "i64"}


@pytest.mark.parametrize("kind,dim,optimizer,mode,width", MAIN, ids=["-".join(map(str, c)) for c in MAIN])
def test_master_step_equals_the_reference(eng, ctx, stream, kind, dim, optimizer, mode, width):
    tab = Trained(eng, kind, dim, optimizer)
    for b, G in tr.train_batches(kind, dim):
        db = DevBatch(b, G, mode, width)
        tab.step(ctx, db, stream)
        rows, n_bad, unenc = tab.advance(db)
        tab.check((kind, dim, optimizer, mode, width, b.k))
        assert len(rows) > 60 and unenc == 0
        assert ctx.report() == n_bad == 3 and ctx.master_report() == 0
    assert np.array_equal(tab.table, rc.host_encode(kind, tab.master))


# ---- 2: the same bytes as the recipe on the GPU ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,mode", [("e4m3", 16, "sum"), ("mxfp4", 32, "weighted+pad")])
def test_master_step_leaves_the_bytes_of_the_recipe(eng, ctx, stream, kind, dim, mode):
    """The README's no-wait recipe through the existing API, on a table and a master of its own: rows_out filled with -1,
    emb_grad_sparse (the raw call: |U| stays on the device), the -1 slots steered to a spare master row, the two torch ops,
    index_copy_, and the writer over all n slots, which skips and counts the -1 ids."""
    from grad_gpu import SparseCall
    fused = Trained(eng, kind, dim, "sgd", t=T)
    recipe = Trained(eng, kind, dim, "sgd", t=1)
    spare = torch.zeros((N + 1, dim), dtype=torch.float32, device=DEV)              # the recipe's master, with the spare row N
    spare[:N] = recipe.d_master
    n_unique = torch.zeros((1,), dtype=torch.int64, device=DEV)
    h = stream.cuda_stream
    with eng.row_writer(2048) as writer:
        for b, G in tr.train_batches(kind, dim):
            db = DevBatch(b, G, mode)
            n = b.n
            call = SparseCall(ctx, 1, db.idx, db.off, db.G, db.mode, db.w, db.pad)
            rows_out = torch.zeros((n,), dtype=torch.int64, device=DEV)
            grads_out = torch.zeros((n, dim), dtype=torch.float32, device=DEV)
            to_spare = torch.full((n,), N, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            fused.step(ctx, db, stream)
            with torch.cuda.stream(stream):                                         # no wait from here to the comparison
                rows_out.fill_(-1)
                call.enqueue(rows_out, grads_out, n_unique, h)
                r = torch.where(rows_out >= 0, rows_out, to_spare)
                t = grads_out * LR                                                  # two torch ops: two roundings
                new = spare[r] - t
                spare.index_copy_(0, r, new)
                writer.update(1, rows_out, new, stream=h)                           # all n slots
            torch.cuda.synchronize()
            rows, _n_bad, _u = fused.advance(db)
            u = int(n_unique.item())
            assert u == len(rows) < n and np.array_equal(rows_out.cpu().numpy()[:u], rows)
            check_table(table_bytes(eng, T), table_bytes(eng, 1), (kind, "fused against the recipe", b.k))
            same_bits(fused.d_master, spare[:N].cpu().numpy(), (kind, "masters", b.k))
            fused.check((kind, "fused", b.k))
            assert ctx.report() == 6 and ctx.master_report() == 0 and writer.report() == n - u


# ---- 3: the segmented context ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("bf16", 16), ("mxfp4", 32)])
def test_a_segmented_context_follows_its_own_order(eng, ctx, seg, stream, kind, dim):
    ends = {}
    for name, c, S in (("position", ctx, None), ("segmented", seg, 8)):
        tab = Trained(eng, kind, dim, "sgd")
        for b, _G in tr.train_batches(kind, dim, 2):
            db = DevBatch(b, b.witness_grads(dim), "sum")
            tab.step(c, db, stream)
            tab.advance(db, segment=S)
            tab.check((kind, name, b.k))
            assert c.report() == 3 and c.master_report() == 0
        ends[name] = tab.master
    differ = np.argwhere(bits(ends["position"]) != bits(ends["segmented"]))
    # only row HOT occurs more than S + 1 times: the orders differ there alone, and in the witness column for certain (0 against 12 per step)
    assert {int(r) for r, _c in differ} == {tr.HOT} and (tr.HOT, 0) in {(int(r), int(c)) for r, c in differ}, differ
    assert ends["position"][tr.HOT, 0] - ends["segmented"][tr.HOT, 0] > 1.0


# ---- 4: the element-wise kernel ---------------------------------------------------------------------------------------------------------------
def misaligned(x):
    """The same values in a contiguous tensor whose address is 4 bytes past a 16-byte boundary."""
    buf = torch.empty((x.numel() + 8,), dtype=torch.float32, device=DEV)
    at = 1 + ((-buf.data_ptr() // 4) % 4)
    out = buf[at:at + x.numel()].view(x.shape)
    out.copy_(x)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


ELEM = (("e4m3", 7, "plain"), ("bf16", 5, "plain"), ("e5m2", 16, "grad view"), ("f16", 16, "master"))


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("kind,dim,how", ELEM, ids=[f"{k}-{d}-{h}" for k, d, h in ELEM])
def test_the_element_wise_kernel(eng, ctx, seg, stream, kind, dim, how, optimizer):
    for name, c, S in (("position", ctx, None), ("segmented", seg, 8)):
        tab = Trained(eng, kind, dim, optimizer)
        if how == "master":
            tab.d_master = misaligned(tab.d_master)
        for b, G in tr.train_batches(kind, dim, 2):
            db = DevBatch(b, G if S is None else b.witness_grads(dim), "sum" if S else "mean+pad")
            db.G_host = G if S is None else b.witness_grads(dim)
            if how == "grad view":
                db.G = in_place(db.G, 20, 1)                                        # ld 20, column 1: 4 bytes past a 16-byte boundary
                assert db.G.data_ptr() % 16 == 4
            tab.step(c, db, stream)
            tab.advance(db, segment=S)
            tab.check((kind, dim, how, optimizer, name, b.k))
            assert c.report() == 3 and c.master_report() == 0


@pytest.mark.parametrize("kind,dim,optimizer,how", [("e4m3", 7, "rowwise", "plain"), ("bf16", 16, "rowwise", "master"), ("mxfp4", 32, "sgd", "master"),
                                                    ("mxfp4", 32, "adagrad", "grad view"), ("f16", 16, "rowwise", "grad view")])
def test_what_the_element_wise_kernel_does_not_run_is_refused_and_writes_nothing(pel, eng, ctx, stream, kind, dim, optimizer, how):
    tab = Trained(eng, kind, dim, optimizer)
    if how == "master":
        tab.d_master = misaligned(tab.d_master)
    b, G = tr.train_batches(kind, dim, 1)[0]
    db = DevBatch(b, G, "sum")
    if how == "grad view":
        db.G = in_place(db.G, dim + 4, 1)
    with pytest.raises(pel.lib.PimembError) as ei:
        tab.step(ctx, db, stream)
    assert ei.value.code == UNSUPPORTED and "lane-group shape" in str(ei.value)
    tab.check((kind, dim, optimizer, how, "refused"))                               # canaries: table, master and state as they were
    assert ctx.report() == 0 and ctx.master_report() == 0


# ---- 5: the table is not read ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,optimizer", [("e4m3", 48, "sgd"), ("mxfp4", 96, "rowwise"), ("bf16", 7, "adagrad")])
def test_the_table_row_is_not_read(eng, ctx, stream, kind, dim, optimizer):
    b, G = tr.train_batches(kind, dim, 1)[0]
    named = b.named_rows("sum")
    st = tr.initial_state(kind, dim)
    garbage = st.table.copy()
    garbage[named[[0, len(named) // 2, -1]]] = 0xA5
    tab = Trained(eng, kind, dim, optimizer, table=garbage)
    db = DevBatch(b, G, "sum")
    tab.step(ctx, db, stream)
    tab.table = st.table                                                            # the reference starts from the clean table
    rows, _n_bad, _u = tab.advance(db)
    assert np.isin(named[[0, len(named) // 2, -1]], rows).all()
    tab.check((kind, dim, "garbage rows"))
    assert np.array_equal(tab.table[rows], rc.host_encode(kind, tab.master[rows]))
    assert ctx.report() == 3 and ctx.master_report() == 0


# ---- 6: special values -----------------------------------------------------------------------------------------------------------------------
SUBNORMAL = {"f16": 1.25 * 2.0 ** -20, "bf16": 1.5 * 2.0 ** -130, "e4m3": 3 * 2.0 ** -9, "e5m2": 2.0 ** -16, "mxfp4": 0.5}
SUBNORMAL_TIE = {"f16": 2.5 * 2.0 ** -24, "bf16": 2.5 * 2.0 ** -133, "e4m3": 2.5 * 2.0 ** -9, "e5m2": 1.5 * 2.0 ** -16, "mxfp4": 0.25}
TIE = {"f16": 1 + 2.0 ** -11, "bf16": 1 + 2.0 ** -8, "e4m3": 1 + 2.0 ** -4, "e5m2": 1 + 2.0 ** -3, "mxfp4": 2.5}


@pytest.mark.parametrize("kind", mr.KINDS)
def test_special_values(eng, ctx, stream, kind):
    """Five one-position bags with lr = 1, so that M' = M - G in one exact or once-rounded subtraction of crafted values.
      rows 5, 9   one element overflows to +inf / -inf
      row 11      M' is all zeros, of both signs
      row 13      a result in the subnormal range of the stored format, a tie there, a tie at half an ulp of a normal value
                  (MXFP4: under a block amax of 4, scale 2^0: 0.5 is the smallest code, 0.25 and 2.5 are ties)
      row 20      ordinary values"""
    dim = 32
    rng = np.random.default_rng(31)
    master = tr.initial_master(kind, dim).copy()
    G = (rng.standard_normal((5, dim)) * 0.25).astype(F)
    ids = np.array([5, 9, 11, 13, 20], dtype=np.int64)
    big = F(3.0e38)
    master[5, 2], G[0, 2] = big, -big                                                # 3e38 + 3e38: +inf
    master[9, 31], G[1, 31] = -big, big
    master[11, 0::2], G[2, 0::2] = F(1.5), F(1.5)                                    # x - x = +0
    master[11, 1::2], G[2, 1::2] = F(-0.0), F(0.0)                                   # -0 - +0 = -0
    master[13], G[3] = F(0.0), F(0.0)
    master[13, 0], master[13, 1], master[13, 2], master[13, 3] = F(4.0), F(SUBNORMAL[kind]), F(SUBNORMAL_TIE[kind]), F(TIE[kind])
    master[13, 4:8] = -master[13, 0:4]
    table = rc.host_encode(kind, master)
    tab = Trained(eng, kind, dim, "sgd", table=table, master=master)

    class B:
        host = (list(ids), np.arange(5, dtype=np.int64), "sum", None, None)
        mode, w, pad, G_host = "sum", None, None, G
        idx, off = to_dev(ids), to_dev(np.arange(5, dtype=np.int64))

        @staticmethod
        def kw():
            return dict(modes="sum", per_sample_weights=None, padding_idx=None)
    B.G = to_dev(G)
    tab.step(ctx, B, stream, lr=1.0)
    rows, n_bad, unenc = tab.advance(B, lr=1.0)
    tab.check((kind, "special values"))
    assert list(rows) == [5, 9, 11, 13, 20] and n_bad == 0
    got = table_bytes(eng, T)
    m = tab.d_master.cpu().numpy()
    assert m[5, 2] == np.inf and m[9, 31] == -np.inf                                # the master holds the inf in every case
    assert ctx.report() == 0 and ctx.master_report() == unenc == (2 if kind == "mxfp4" else 0)
    if kind == "mxfp4":
        assert np.array_equal(got[5], table[5]) and np.array_equal(got[9], table[9])            # the rows keep their old bytes
        assert got[11, 16] == 127 and (got[11, :16] == 0x80).all() and not got[11, 17:].any()    # zeros of both signs: scale 127
        assert got[13, 16] == 127 and got[13, 0] == 0x16 and got[13, 1] == 0x40                  # 4 -> 6, 0.5 -> 1 | 0.25 -> 0 (tie to even), 2.5 -> 2 = code 4
    elif kind == "f16":
        assert got[5].view(np.uint16)[2] == 0x7C00 and got[9].view(np.uint16)[31] == 0xFC00
    elif kind == "e5m2":
        assert got[5, 2] == 0x7C and got[9, 31] == 0xFC
    elif kind == "e4m3":
        assert got[5, 2] == 0x7F and got[9, 31] == 0xFF
    else:
        assert got[5].view(np.uint16)[2] == 0x7F80 and got[9].view(np.uint16)[31] == 0xFF80
    stored = tr.decode(kind, got[13:14])[0]
    assert stored[1] != 0 and stored[1] == F(SUBNORMAL[kind])                       # the subnormal result survives, exactly


# ---- 7: refusals that leave everything as it was ---------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(pel, eng, ctx, stream):
    kind, dim = "bf16", 16
    good = [Trained(eng, kind, dim, "sgd", t=T), Trained(eng, "e4m3", dim, "sgd", t=1)]
    b, G = tr.train_batches(kind, dim, 1)[0]
    db = DevBatch(b, G, "sum")
    h = stream.cuda_stream
    w32 = tr.initial_master("f32", dim)
    eng.load_table(2, w32.copy())                                                   # an EMB_F32 table
    m32 = to_dev(w32)
    big = np.zeros((8, 1024), F)
    eng.load_table(3, rc.host_encode("mxfp4", big), dtype=CODE["mxfp4"])            # MXFP4 dim 1024
    mbig = to_dev(big)
    ids8, off8, G8 = to_dev(np.arange(8, dtype=np.int64)), to_dev(np.arange(8, dtype=np.int64)), to_dev(np.ones((8, 1024), F))

    def refused(code, text, tables, idx, off, grads, masters, **kw):
        with pytest.raises(pel.lib.PimembError) as ei:
            ctx.master_step(tables, idx, off, grads, masters, LR, stream=h, **kw)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    refused(UNSUPPORTED, "its own master", [2], [db.idx], [db.off], [db.G], [m32])
    refused(UNSUPPORTED, "dim 512", [3], [ids8], [off8], [G8], [mbig])
    refused(UNSUPPORTED, "EMB_POOL_MAX", [T], [db.idx], [db.off], [db.G], [good[0].d_master], modes="max")
    eng.set_hot_rows(T, [3, 8, 30])
    try:
        refused(UNSUPPORTED, "hot set", [T], [db.idx], [db.off], [db.G], [good[0].d_master])
    finally:
        eng.set_hot_rows(T, [])
    # a bad descriptor behind two good ones in one call: nothing is enqueued
    refused(UNSUPPORTED, "its own master", [T, 1, 2], [db.idx] * 3, [db.off] * 3, [db.G] * 3, [good[0].d_master, good[1].d_master, m32])
    for g in good:
        g.check((g.kind, "after the refusals"))
    same_bits(m32, w32, "the fp32 table's master")
    assert np.array_equal(table_bytes(eng, 2).view(F), w32)
    assert ctx.report() == 0 and ctx.master_report() == 0
    # ... and the same two good descriptors alone run, table after table
    ctx.master_step([T, 1], [db.idx] * 2, [db.off] * 2, [db.G] * 2, [good[0].d_master, good[1].d_master], LR, stream=h)
    for g in good:
        g.advance(db)
        g.check((g.kind, "two descriptors in one call"))
    assert ctx.report() == 6 and ctx.master_report() == 0


# ---- 8: stream order and capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,mode,optimizer", [("mxfp4", 64, "mean+pad", "rowwise"), ("mxfp4", 64, "sum", "rowwise"), ("mxfp4", 64, "mean+pad", "sgd"),
                                                     ("e4m3", 16, "sum", "sgd")])
def test_a_prepared_plan_reads_the_new_bytes_and_the_step_replays_in_a_graph(eng, ctx, stream, kind, dim, mode, optimizer):
    """A plan prepared before the loop, launched before and behind the step with no synchronize between; then {lookup, row-wise master
    step on MXFP4, lookup} captured in torch's default capture error mode -- an allocation, a copy or a wait inside the call makes
    the capture fail -- and replayed three times with a new gradient in the same buffer."""
    tab = Trained(eng, kind, dim, optimizer)
    Gs = tr.graph_grads(dim)
    b = tr.train_batches(kind, dim, 1)[0][0]
    db = DevBatch(b, Gs[0], mode)
    lb = tr.lookup_batch()
    l_ids, l_off, l_mode, l_w, l_pad = lb.args(mode)
    plan = eng.plan_pooled([T], [to_dev(lb.ids)], [to_dev(lb.offsets)], l_mode, None if l_w is None else [to_dev(l_w)], l_pad)
    first = torch.zeros_like(plan.outputs[0])
    h = stream.cuda_stream

    def enqueue():
        plan.launch(h)
        first.copy_(plan.outputs[0])
        tab.step(ctx, db, stream)
        plan.launch(h)

    def check(j, what):
        before = tr.forward(kind, tab.table, l_ids, l_off, l_mode, l_w, l_pad)
        db.G_host = Gs[j]
        _rows, n_bad, unenc = tab.advance(db)
        tab.check(what)
        same_bits(first, before, (what, "lookup before the step"))
        same_bits(plan.outputs[0], tr.forward(kind, tab.table, l_ids, l_off, l_mode, l_w, l_pad), (what, "lookup behind the step"))
        assert ctx.report() == n_bad == 3 and ctx.master_report() == unenc == 0

    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue()                                                               # uncaptured: the code objects are loaded
        check(0, "uncaptured")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            enqueue()
        tab.check("the capture itself ran nothing")
        assert ctx.report() == 0
        for j in (1, 2, 3):
            db.G.copy_(to_dev(Gs[j]))
            graph.replay()
            check(j, ("replay", j))
    finally:
        torch.cuda.synchronize()
        plan.destroy()


def test_master_of_widens_exactly(eng):
    for kind, dim in (("e4m3", 16), ("mxfp4", 64), ("bf16", 5), ("f16", 8), ("e5m2", 48)):
        st = tr.initial_state(kind, dim)
        load_bytes(eng, T, kind, st.table)
        m = eng.master_of(T)
        assert m.dtype == F and m.shape == (N, dim)
        assert np.array_equal(bits(m), bits(tr.decode(kind, st.table))) and np.array_equal(rc.host_encode(kind, m), st.table), kind
        assert torch.equal(eng.master_of(T, DEV).cpu(), torch.from_numpy(m))


# ---- 9: the modules ------------------------------------------------------------------------------------------------------------------------
def module_batch(dim, seed):
    """train_ref.lookup_batch() -- valid ids only, a module's checked lookup reads them -- with a gradient of its own."""
    lb = tr.lookup_batch()
    rng = np.random.default_rng(9300 + seed + dim)
    G = (rng.standard_normal((lb.B, dim)) * np.exp2(rng.integers(-4, 4, size=(lb.B, 1)))).astype(F)
    return lb, G


def test_a_pooling_bag_trains_an_fp8_table_on_master_weights(pel, eng):
    tm = __import__("importlib").import_module("pim-embedding-lookup_amd.torch_module")
    kind, dim, t = "e4m3", 16, 4
    bag = tm.PoolingEmbeddingBag(N, dim, mode="sum", _weight=torch.from_numpy(tr.initial_master(kind, dim).copy()), engine=eng, table_id=t,
                                 dtype=torch.float8_e4m3fn)
    assert bag.master_weight is None and "master_weight" not in bag.state_dict()
    bag.enable_fused_sgd(LR, master_weights=True)
    table = table_bytes(eng, t)
    master = tr.decode(kind, table)
    same_bits(bag.master_weight, master, "the master starts as the decoded table")
    assert np.array_equal(rc.host_encode(kind, master), table)
    lb, _G = module_batch(dim, 0)
    idx, off = to_dev(lb.ids), to_dev(lb.offsets)
    for r in range(2):
        _lb, G = module_batch(dim, r)
        out = bag(idx, off)
        (out * to_dev(G)).sum().backward()
        table, master, _o, rows, n_bad, unenc = mr.master_step(kind, table, master, None, lb.ids, lb.offsets, G, "sum", None, None, "sgd")
        torch.cuda.synchronize()
        check_table(table_bytes(eng, t), table, ("module", r))
        same_bits(bag.master_weight, master, ("module master", r))
        assert n_bad == 0 and unenc == 0 and len(rows) > 60
        if r == 0:                                                                  # update_rows_ moves table and master together
            ids, new = tr.written_rows(rows, dim)
            bag.update_rows_(ids, new)
            table, master, skipped = tr.write_rows(kind, table, master, ids, new)
            torch.cuda.synchronize()
            assert skipped == 0
            check_table(table_bytes(eng, t), table, "update_rows_")
            same_bits(bag.master_weight, master, "update_rows_: the master")
    assert eng._module_grad.report() == 0 and eng._module_grad.master_report() == 0
    sd = bag.state_dict()
    assert set(sd) == {"weight", "master_weight"}
    same_bits(sd["master_weight"], master, "state_dict")
    other = tm.PoolingEmbeddingBag(N, dim, mode="sum", engine=eng, table_id=5, dtype=torch.float8_e4m3fn)
    other.load_state_dict(sd)
    same_bits(other.master_weight, master, "loaded master")
    check_table(table_bytes(eng, 5), table, "loaded table")
    bag.enable_fused_sgd(LR)                                                         # off again: the key leaves, and the master with it
    assert bag.master_weight is None and "master_weight" not in bag.state_dict()
    ids, new = tr.written_rows(rows, dim, seed=3)
    bag.update_rows_(ids, new)                                                       # the table moves while master weights are off ...
    torch.cuda.synchronize()
    table, _m, skipped = tr.write_rows(kind, table, None, ids, new)
    check_table(table_bytes(eng, t), table, "update_rows_ with master weights off")
    bag.enable_fused_sgd(LR, master_weights=True)                                    # ... and on again: no stale master
    same_bits(bag.master_weight, tr.decode(kind, table), "the master is derived anew from the table")
    assert not np.array_equal(bits(tr.decode(kind, table)), bits(master))


def test_fused_pooling_bags_train_two_dtypes_with_adagrad_on_master_weights(pel, eng):
    tm = __import__("importlib").import_module("pim-embedding-lookup_amd.torch_module")
    specs = (("bf16", 16, torch.bfloat16, 4), ("mxfp4", 32, "mxfp4", 5))
    bags = [tm.PoolingEmbeddingBag(N, dim, mode="sum", _weight=torch.from_numpy(tr.initial_master(kind, dim).copy()), engine=eng, table_id=t, dtype=dt)
            for kind, dim, dt, t in specs]
    model = tm.FusedPoolingEmbeddingBags(bags)
    with pytest.raises(ValueError) as ei:
        model.enable_fused_adagrad(LR, eps=EPS, multi_table=True, master_weights=True)
    assert "no multi-table master step" in str(ei.value)
    model.enable_fused_adagrad(LR, eps=EPS, master_weights=True)
    ref = []
    for (kind, dim, _dt, t), m in zip(specs, model.master_weight):
        table = table_bytes(eng, t)
        master = tr.decode(kind, table)
        same_bits(m, master, (kind, "the master starts as the decoded table"))
        ref.append([table, master, np.zeros((N, dim), F)])
    lb = tr.lookup_batch()
    idx, off = to_dev(lb.ids), to_dev(lb.offsets)
    for r in range(2):
        Gs = [module_batch(dim, r)[1] for _k, dim, _dt, _t in specs]
        outs = model([off, off], [idx, idx])
        sum((o * to_dev(G)).sum() for o, G in zip(outs, Gs)).backward()
        torch.cuda.synchronize()
        for k, (kind, dim, _dt, t) in enumerate(specs):
            table, master, opt, _rows, n_bad, unenc = mr.master_step(kind, *ref[k], lb.ids, lb.offsets, Gs[k], "sum", None, None, "adagrad")
            ref[k] = [table, master, opt]
            check_table(table_bytes(eng, t), table, (kind, "fused module", r))
            same_bits(model.master_weight[k], master, (kind, "fused module master", r))
            check_state(model.adagrad_sum[k], opt, (kind, "fused module state", r))
            assert n_bad == 0 and unenc == 0
    assert eng._module_grad.report() == 0 and eng._module_grad.master_report() == 0
    sd = model.state_dict()
    assert {"bags.0.master_weight", "bags.1.master_weight", "bags.0.adagrad_sum"} <= set(sd)
    # a checkpoint loaded into a fresh model switches the master step on there too: the model reads the flag from its bags
    fresh = tm.FusedPoolingEmbeddingBags([tm.PoolingEmbeddingBag(N, dim, mode="sum", engine=eng, table_id=t + 2, dtype=dt) for _k, dim, dt, t in specs])
    fresh.load_state_dict(sd)
    assert fresh._masters_on()
    Gs = [module_batch(dim, 7)[1] for _k, dim, _dt, _t in specs]
    fresh.adagrad_step_([off, off], [idx, idx], [to_dev(G) for G in Gs], LR, eps=EPS)
    torch.cuda.synchronize()
    for k, (kind, dim, _dt, t) in enumerate(specs):
        table, master, opt, _rows, _b, _u = mr.master_step(kind, *ref[k], lb.ids, lb.offsets, Gs[k], "sum", None, None, "adagrad")
        check_table(table_bytes(eng, t + 2), table, (kind, "loaded model"))
        same_bits(fresh.master_weight[k], master, (kind, "loaded model's master"))
        check_state(fresh.adagrad_sum[k], opt, (kind, "loaded model's state"))
    model.enable_fused_adagrad(LR, eps=EPS)
    assert model.master_weight == [None, None] and not model._masters_on()


def test_the_harness_trains_fp8_and_mxfp4_tables_with_master_weights(pel, capsys):
    """EmbeddingBagCollection with master weights on: two apply_emb / backward rounds against master_ref, per table; then the
    command line once, end to end."""
    h = __import__("importlib").import_module("pim-embedding-lookup_amd.dlrm_harness")
    lb = tr.lookup_batch()
    for dtype, kind, dim, optimizer in (("fp8_e4m3", "e4m3", 16, "sgd"), ("mxfp4", "mxfp4", 32, "rowwise")):
        ebc = h.EmbeddingBagCollection([N, N], dim, dtype=dtype, weights=[tr.initial_master(kind, dim), tr.initial_master(kind, dim)[::-1].copy()])
        try:
            if optimizer == "sgd":
                ebc.enable_fused_sgd(LR, master_weights=True)
            else:
                ebc.enable_fused_adagrad(LR, eps=EPS, rowwise=True, master_weights=True)
            ref = []
            for t, m in zip(ebc._ids, ebc.master_weight):
                table = table_bytes(ebc.engine, t)
                same_bits(m, tr.decode(kind, table), (dtype, "the master starts as the decoded table"))
                ref.append([table, tr.decode(kind, table), mr.initial_opt(optimizer, N, dim)])
            idx, off = to_dev(lb.ids), to_dev(lb.offsets)
            for r in range(2):
                Gs = [module_batch(dim, 20 + r + k)[1] for k in range(2)]
                outs = ebc.apply_emb([off, off], [idx, idx])
                sum((o * to_dev(G)).sum() for o, G in zip(outs, Gs)).backward()
                torch.cuda.synchronize()
                for k, t in enumerate(ebc._ids):
                    table, master, opt, _rows, n_bad, unenc = mr.master_step(kind, *ref[k], lb.ids, lb.offsets, Gs[k], "sum", None, None, optimizer)
                    ref[k] = [table, master, opt]
                    check_table(table_bytes(ebc.engine, t), table, (dtype, "harness", r, k))
                    same_bits(ebc.master_weight[k], master, (dtype, "harness master", r, k))
                    assert n_bad == 0 and unenc == 0
            ebc.enable_fused_sgd(None)
            assert ebc.master_weight is None
        finally:
            close = getattr(ebc, "close", None)
            if close:
                close()
    h.main(["--arch-embedding-size=300-200", "--arch-sparse-feature-size=32", "--mini-batch-size=64", "--num-indices-per-lookup=4", "--num-batches=3",
            "--table-dtype", "mxfp4", "--fused-rowwise-adagrad", "0.05", "--master-weights"])
    assert "ms" in capsys.readouterr().out
