"""GPU: the gradient of per_sample_weights (include/pimemb_grad.h, THE GRADIENT OF PER_SAMPLE_WEIGHTS; emb_grad_weights), bit for bit
against tests/psw_ref.py, the definition as a loop over positions: the lane-group kernel at the dims where it can go wrong, the
fallback kernel, the three table dtypes and both id widths, ragged bags, the edges of a batch, every refusal, the modules'
three forward cases with the order of the two enqueues of a backward, torch parity, the DLRM harness, and stream capture.
Small shapes: tables of 64 rows (the ragged batch of tests/grad_seg_ref.py: 499), batches of a few hundred positions."""
import contextlib
import ctypes as C
import io
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
import optim_ref as orf  # noqa: E402
import psw_ref as pr  # noqa: E402
import rows_cases as rc  # noqa: E402
from grad_gpu import DEV, F, RaggedBatch, bits, in_place, load_bytes, table_bytes, to_dev  # noqa: E402
from test_psw_cpu import exact_inputs, torch_cpu_weights_grad  # noqa: E402

pytestmark = pytest.mark.gpu
tm = import_module("pim-embedding-lookup_amd.torch_module")

ROWS, PAD = 64, 9
LANE_DIMS, FALLBACK_DIMS = (4, 8, 48, 64, 256, 260, 512), (1, 3, 6, 130, 516)
LENS = (0, 1, 7, 8, 9, 17, 70, 0, 5, 0)      # around the in-flight depth of eight; empty bags in the middle and at the end
LEAD = 2                                     # positions before offsets[0]
CANARY = 4321.0


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=32)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.grad_context(2048, 512)
    yield c
    c.close()


_tables = {}


def table(kind, dim, rows=ROWS):
    """uint8 [rows, stride]: values over many binades."""
    key = (kind, dim, rows)
    if key not in _tables:
        rng = np.random.default_rng(dim * 7 + rows)
        w = (rng.standard_normal((rows, dim)) * np.exp2(rng.integers(-6, 7, size=(rows, 1)))).astype(F)
        _tables[key] = gr.encode(kind, w)
        _tables[key].setflags(write=False)
    return _tables[key]


class Batch:
    """LEAD positions without a bag (position 1 holds a bad id that is not counted), then bags of LENS positions: rows repeated
    within a bag, padding entries, four bad ids of full width -- for int64 one >= 2^32 whose low word is a valid row."""

    def __init__(self, width, dim, lens=LENS, lead=LEAD, seed=0):
        rng = np.random.default_rng(seed + len(lens))
        n = lead + sum(lens)
        ids = [int(v) for v in rng.integers(0, ROWS, size=n)]
        starts = lead + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        big = next((k for k, L in enumerate(lens) if L >= 17), None)
        self.bad_at = []
        if big is not None:
            s = int(starts[big])
            ids[s + 1] = ids[s + 3] = ids[s + 12] = ids[s]                                   # a row several times in a bag
            ids[s + 2] = ids[s + 9] = PAD
            bad = [2 ** 32 + 5, -1, ROWS, 2 ** 40 + ROWS - 1] if width == "i64" else [ROWS, ROWS + 7, 2 ** 31 + 5, 2 ** 32 - 1]
            self.bad_at = [s + 4, s + 8, s + 15, s + 16]
            for p, v in zip(self.bad_at, bad):
                ids[p] = v
        if lead > 1:
            ids[1] = ROWS + 3
        self.ids, self.offsets, self.n, self.B, self.width = ids, starts, n, len(lens), width
        self.n_bad = len(self.bad_at)
        self.G = (rng.standard_normal((self.B, dim)) * np.exp2(rng.integers(-6, 7, size=(self.B, 1)))).astype(F)
        np_ids = np.array(ids, dtype=np.int64) if width == "i64" else np.array(ids, dtype=np.uint64).astype(np.uint32)
        self.d_ids, self.d_off = to_dev(np_ids), to_dev(starts.astype(np.int64 if width == "i64" else np.uint32))
        self.d_G = to_dev(self.G)

    def reference(self, kind, raw, pad=PAD, G=None):
        return pr.weights_grad(kind, raw, self.ids, self.offsets, self.G if G is None else G, pad)


def run(ctx, t, b, G=None, pad=PAD, room=16):
    """emb_grad_weights into a buffer with canaries behind dw[n]: (dw as numpy [n], the canaries are intact)."""
    out = torch.full((b.n + room,), CANARY, dtype=torch.float32, device=DEV)
    got = ctx.weights_grad(t, b.d_ids, b.d_off, b.d_G if G is None else G, padding_idx=pad, outs=out[:b.n])
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[b.n:] == CANARY).all(), "entries at and beyond n_indices were written"
    return h[:b.n]


def same(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert bad.size == 0, (what, bad[:8], got[bad[:4]], want[bad[:4]])


def check_batch(eng, ctx, kind, dim, width, what):
    raw = table(kind, dim)
    load_bytes(eng, 0, kind, raw)
    b = Batch(width, dim)
    want, n_bad = b.reference(kind, raw)
    got = run(ctx, 0, b)
    same(got, want, what)
    ids = np.array([v if 0 <= v < ROWS else -1 for v in b.ids])
    not_good = (ids < 0) | (ids == PAD) | (np.arange(b.n) < LEAD)
    assert not_good.sum() >= 8 and (bits(got[not_good]) == 0).all(), what                     # exactly +0
    assert (want[~not_good] != 0).sum() > 90
    assert ctx.report() == n_bad == b.n_bad == 4
    assert np.array_equal(table_bytes(eng, 0), raw)


# ---- the kernels against the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", LANE_DIMS + FALLBACK_DIMS)
def test_every_shape_on_fp32_tables_and_both_id_widths(eng, ctx, dim):
    for width in ("u32", "i64"):
        check_batch(eng, ctx, "f32", dim, width, (dim, width))


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("dim", [4, 48, 260, 512, 3, 130, 516])
def test_half_width_tables(eng, ctx, kind, dim):
    check_batch(eng, ctx, kind, dim, "i64" if dim % 8 else "u32", (kind, dim))


@pytest.mark.parametrize("dim", [8, 260])
def test_gradient_views_in_place_and_misaligned(eng, ctx, dim):
    """G inside a NaN-filled buffer with grad_ld > dim, 16-byte aligned: the lane-group kernel; G as a view that starts at column
    1 of a wider buffer: the fallback kernel -- the same bits as the aligned call."""
    raw = table("bf16", dim)
    load_bytes(eng, 0, "bf16", raw)
    b = Batch("i64", dim)
    want, _ = b.reference("bf16", raw)
    aligned = in_place(b.d_G, dim + 12, 4)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(0) == dim + 12
    same(run(ctx, 0, b, G=aligned), want, ("in place", dim))
    shifted = in_place(b.d_G, dim + 12, 1)
    assert shifted.data_ptr() % 16 == 4
    same(run(ctx, 0, b, G=shifted), want, ("column 1", dim))
    odd = in_place(b.d_G, dim + 13, 0)                                                        # an odd row stride
    same(run(ctx, 0, b, G=odd), want, ("odd stride", dim))
    assert ctx.report() == 3 * b.n_bad


@pytest.mark.parametrize("width", ["u32", "i64"])
@pytest.mark.parametrize("lead", [False, True])
def test_the_ragged_batch(eng, ctx, width, lead):
    """grad_seg_ref.ragged_case: empty bags, a row three times in a bag, padding, positions before offsets[0], bad ids."""
    case = sr.ragged_case(8)
    dim = 16
    raw = table("f16", dim, sr.RAGGED_ROWS)
    load_bytes(eng, 1, "f16", raw)
    rb = RaggedBatch(case, "weighted+pad", width, dim, lead=lead)
    ids, off, _mode, _w, pad = rb.host_args
    want, n_bad = pr.weights_grad("f16", raw, ids, off, case.grads(dim), pad)
    out = torch.full((rb.n + 8,), CANARY, dtype=torch.float32, device=DEV)
    ctx.weights_grad(1, rb.idx, rb.off, rb.G, padding_idx=rb.pad, outs=out[:rb.n])
    h = out.cpu().numpy()
    same(h[:rb.n], want, ("ragged", width, lead))
    assert (h[rb.n:] == CANARY).all()
    assert ctx.report() == n_bad == rb.n_bad
    if lead:
        assert (bits(h[:3]) == 0).all() and want[3:].any()


def test_one_bag_and_fixed_pooling(eng, ctx, pel):
    dim = 64
    raw = table("f32", dim)
    load_bytes(eng, 0, "f32", raw)
    one = Batch("u32", dim, lens=(23,), lead=0)
    assert one.B == 1
    same(run(ctx, 0, one), one.reference("f32", raw)[0], "n_bags = 1")
    # offsets = NULL: bags of 5 positions, the last bag runs to the end (23 = 4 * 5 + 3 positions, 4 bags)
    rng = np.random.default_rng(3)
    G = (rng.standard_normal((4, dim))).astype(F)
    want, n_bad = pr.weights_grad("f32", raw, one.ids, None, G, PAD, n_bags=4, fixed_pooling=5)
    for view in (to_dev(G), in_place(to_dev(G), dim + 1, 1)):                                 # the lane-group kernel, then the fallback
        out = torch.full((one.n + 4,), CANARY, dtype=torch.float32, device=DEV)
        ctx.weights_grad(0, one.d_ids, None, view, padding_idx=PAD, fixed_pooling=5, outs=out[:one.n])
        h = out.cpu().numpy()
        same(h[:one.n], want, "fixed pooling")
        assert (h[one.n:] == CANARY).all()
    assert ctx.report() == one.n_bad + 2 * n_bad


def test_signed_zeros_and_an_infinite_row(eng, ctx):
    """G[b] all -0 and W[r] positive: dw is -0 at dims 4 and 64, +0 at dims 48 and 3 -- the +0 padding is added.  One row with an
    inf: compared by isnan / value."""
    for dim, negative in ((4, True), (64, True), (48, False), (3, False)):
        w = np.abs(gr.decode("f32", table("f32", dim))) + F(0.5)
        w[7, dim // 2] = np.inf
        raw = gr.encode("f32", w)
        load_bytes(eng, 0, "f32", raw)
        ids = np.array([3, 5, 7, 11], dtype=np.int64)
        off = np.array([0, 2], dtype=np.int64)
        G = np.full((2, dim), -0.0, F)
        G[1] = F(1.25)
        got = ctx.weights_grad(0, to_dev(ids), to_dev(off), to_dev(G)).cpu().numpy()
        want, _ = pr.weights_grad("f32", raw, ids, off, G)
        assert (got[:2] == 0).all() and (np.signbit(got[:2]) == negative).all(), (dim, got)
        assert np.isposinf(got[2]) and np.isposinf(want[2]) and bits(got[3]) == bits(want[3])
        G[1, dim // 2] = 0.0                                                                  # 0 * inf
        got = ctx.weights_grad(0, to_dev(ids), to_dev(off), to_dev(G)).cpu().numpy()
        assert np.isnan(got[2]) and np.isnan(pr.weights_grad("f32", raw, ids, off, G)[0][2])


def test_a_segmented_context_gives_the_same_bits_and_a_hot_set_is_served(eng, ctx):
    dim = 48
    raw = table("bf16", dim)
    load_bytes(eng, 0, "bf16", raw)
    b = Batch("u32", dim)
    want, _ = b.reference("bf16", raw)
    with eng.grad_context(2048, 512, order="segmented", segment=8, max_dim=64) as seg:
        same(run(seg, 0, b), want, "segmented")
        assert seg.report() == b.n_bad
    raw = table("f32", 16)
    load_bytes(eng, 3, "f32", raw)
    b = Batch("i64", 16)
    eng.set_hot_rows(3, [1, 2, 3])                                                            # a hot set is a copy; the table's own bytes are read
    try:
        same(run(ctx, 3, b), b.reference("f32", raw)[0], "hot set staged")
    finally:
        eng.set_hot_rows(3, [])
    assert ctx.report() == b.n_bad


def test_refusals_write_nothing(eng, ctx, pel):
    UNS, INV = pel.lib.EMB_ERR_UNSUPPORTED, pel.lib.EMB_ERR_INVALID
    b = Batch("i64", 16)

    def refused(c, t, code, text, dim=16, outs=True, **desc_kw):
        out = torch.full((b.n,), CANARY, dtype=torch.float32, device=DEV)
        G = to_dev(np.ones((b.B, dim), F))
        d, keep = pel.lib.EmbGradDesc(), []
        itype, _dev = c._desc(d, t, b.d_ids, b.d_off, G, desc_kw.get("mode", "sum"), None, PAD, 0, keep)
        ptrs = (C.c_void_p * 1)(out.data_ptr() if outs else None)
        rc_ = c._G.emb_grad_weights(c._h, C.byref(d), ptrs, 1, itype, None)
        torch.cuda.synchronize()
        assert rc_ == code and text in c._G.emb_grad_last_error(), (rc_, c._G.emb_grad_last_error())
        assert (out == CANARY).all().item()

    for kind, dim in (("e4m3", 16), ("e5m2", 16), ("mxfp4", 32)):
        load_bytes(eng, 2, kind, rc.host_encode(kind, np.random.default_rng(2).standard_normal((ROWS, dim)).astype(F)))
        refused(ctx, 2, UNS, b"fp8 or MXFP4", dim=dim)
    eng.load_table(2, np.ones((ROWS, 16), dtype=np.int32))
    refused(ctx, 2, UNS, b"EMB_FIXED32")
    load_bytes(eng, 2, "f32", table("f32", 16))
    refused(ctx, 2, UNS, b"EMB_POOL_SUM only", mode="mean")
    refused(ctx, 2, UNS, b"EMB_POOL_MAX", mode="max")
    refused(ctx, 2, INV, b"NULL or not 4-byte aligned", outs=False)
    with eng.grad_context(64, 512) as small:
        refused(small, 2, INV, b"created for 64")
    with eng.grad_context(2048, 4) as few:
        refused(few, 2, INV, b"created for 4")
    # a refused second descriptor keeps the first one's output unwritten
    out = torch.full((2, b.n), CANARY, dtype=torch.float32, device=DEV)
    eng.load_table(3, np.ones((ROWS, 16), dtype=np.int32))
    with pytest.raises(pel.PimembError) as ei:
        ctx.weights_grad([2, 3], [b.d_ids] * 2, [b.d_off] * 2, [b.d_G] * 2, outs=[out[0], out[1]])
    assert ei.value.code == UNS
    torch.cuda.synchronize()
    assert (out == CANARY).all().item() and ctx.report() == 0


# ---- the modules: the three cases of forward, and the order of a backward's two enqueues ----------------------------------------------------
LR = 0.5


def module_batch(dim, seed=0):
    rng = np.random.default_rng(400 + seed)
    lens = [3, 0, 9, 1, 17, 2]
    ids = rng.integers(0, ROWS, size=sum(lens)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ids[4], ids[20] = PAD, PAD
    w0 = (rng.standard_normal((ROWS, dim)) + np.sign(rng.standard_normal((ROWS, dim))) * 0.5).astype(F)
    G = (rng.standard_normal((len(lens), dim)) + np.sign(rng.standard_normal((len(lens), dim))) * 0.5).astype(F)
    w = (rng.standard_normal(len(ids)) + 2).astype(F)
    return ids, off, w0, G, w


def named_rows(ids):
    return np.unique(ids[ids != PAD])


def backward_through(module_call, G, w):
    """loss = <out, G>: backward hands G itself to the module; returns (out, w.grad)."""
    wt = to_dev(w).requires_grad_(True)
    out = module_call(wt)
    (out * to_dev(G)).sum().backward()
    torch.cuda.synchronize()
    return out, wt


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_backward_enqueues_the_weights_gradient_before_the_fused_step(eng, optimizer):
    """w.grad is the definition over the table bytes read BEFORE the step, the table is the stepped one.  Every named row
    changes in the step, and the definition over the stepped table differs: a backward that stepped first would fail."""
    dim = 12
    ids, off, w0, G, w = module_batch(dim)
    bag = tm.PoolingEmbeddingBag(ROWS, dim, mode="sum", padding_idx=PAD, _weight=torch.from_numpy(w0), trusted_inputs=True, engine=eng, table_id=10)
    before = gr.encode("f32", w0)
    if optimizer == "sgd":
        bag.enable_fused_sgd(LR)
    else:
        bag.enable_fused_adagrad(LR, eps=1e-10)
    out, wt = backward_through(lambda wt: bag(to_dev(ids), to_dev(off), per_sample_weights=wt), G, w)
    assert out.grad_fn is not None
    rows, grads, _ = gr.sparse_grad(ROWS, ids, off, G, "sum", w, PAD)
    if optimizer == "sgd":
        stepped = gr.sgd_step("f32", before, rows, grads, F(LR))
    else:
        stepped, state = orf.adagrad_step("f32", before, np.zeros((ROWS, dim), F), rows, grads, F(LR), F(1e-10))
        assert np.array_equal(bits(bag.adagrad_sum.cpu().numpy()), bits(state))
    assert np.array_equal(rows, named_rows(ids)) and (stepped[rows] != before[rows]).any(axis=1).all()
    want, _ = pr.weights_grad("f32", before, ids, off, G, PAD)
    swapped, _ = pr.weights_grad("f32", stepped, ids, off, G, PAD)
    assert (bits(want) != bits(swapped))[ids != PAD].all()
    assert wt.grad.shape == wt.shape and wt.grad.dtype == torch.float32
    same(wt.grad.cpu().numpy(), want, optimizer)
    assert np.array_equal(bag.weight.cpu().numpy().view(np.uint8).reshape(ROWS, -1), stepped)


def test_fused_concat_backward_reads_the_wide_gradient_in_place_weights_first(eng):
    dims = (8, 16)
    data = [module_batch(d, seed=k) for k, d in enumerate(dims)]
    bags = [tm.PoolingEmbeddingBag(ROWS, d, mode="sum", padding_idx=PAD, _weight=torch.from_numpy(x[2]), trusted_inputs=True, engine=eng, table_id=11 + k)
            for k, (d, x) in enumerate(zip(dims, data))]
    fused = tm.FusedPoolingEmbeddingBags(bags, concat=True).enable_fused_sgd(LR)
    col = 4
    wts = [to_dev(x[4]).requires_grad_(True) for x in data]
    wts[1] = to_dev(data[1][4].astype(np.float64)).requires_grad_(True)                       # a float64 weight: its gradient is cast once
    out = fused([to_dev(x[1]) for x in data], [to_dev(x[0]) for x in data], wts, col=col)
    assert tuple(out.shape) == (6, col + sum(dims))
    Gcat = np.concatenate([x[3] for x in data], axis=1)
    (out[:, col:] * to_dev(Gcat)).sum().backward()
    torch.cuda.synchronize()
    for k, (ids, off, w0, G, w) in enumerate(data):
        before = gr.encode("f32", w0)
        rows, grads, _ = gr.sparse_grad(ROWS, ids, off, G, "sum", w, PAD)
        stepped = gr.sgd_step("f32", before, rows, grads, F(LR))
        want, _ = pr.weights_grad("f32", before, ids, off, G, PAD)
        swapped, _ = pr.weights_grad("f32", stepped, ids, off, G, PAD)
        assert (bits(want) != bits(swapped))[ids != PAD].all()
        assert wts[k].grad.dtype == wts[k].dtype and wts[k].grad.shape == wts[k].shape
        same(wts[k].grad.float().cpu().numpy(), want, ("concat", k))
        assert np.array_equal(bags[k].weight.cpu().numpy().view(np.uint8).reshape(ROWS, -1), stepped)
    # the explicit call, list form, on the stepped tables
    dws = fused.per_sample_weights_grad([x[1] for x in data], [x[0] for x in data], [to_dev(x[3]) for x in data])
    for k, (ids, off, w0, G, w) in enumerate(data):
        same(dws[k].cpu().numpy(), pr.weights_grad("f32", table_bytes_of(bags[k]), ids, off, G, PAD)[0], ("explicit", k))


def table_bytes_of(bag):
    return table_bytes(bag.engine, bag.table_id)


def test_without_a_fused_step_the_table_is_untouched_and_the_output_is_the_plain_forwards(eng):
    dim = 6                                                                                   # the fallback kernel
    ids, off, w0, G, w = module_batch(dim)
    bag = tm.PoolingEmbeddingBag(ROWS, dim, mode="sum", padding_idx=PAD, _weight=torch.from_numpy(w0), dtype=torch.bfloat16, trusted_inputs=True,
                                 engine=eng, table_id=13)
    before = table_bytes_of(bag)
    plain = bag(to_dev(ids), to_dev(off), per_sample_weights=to_dev(w))
    assert plain.grad_fn is None and plain.requires_grad is False                             # weights that do not require grad: as before
    with torch.no_grad():
        quiet = bag(to_dev(ids), to_dev(off), per_sample_weights=to_dev(w).requires_grad_(True))
    assert quiet.grad_fn is None
    out, wt = backward_through(lambda wt: bag(to_dev(ids), to_dev(off), per_sample_weights=wt), G, w)
    assert out.grad_fn is not None
    assert np.array_equal(bits(out.detach().cpu().numpy()), bits(plain.cpu().numpy()))
    want, _ = pr.weights_grad("bf16", before, ids, off, G, PAD)
    same(wt.grad.cpu().numpy(), want, "no step")
    assert np.array_equal(table_bytes_of(bag), before)
    # 2-D input: the gradient has the input's shape; the explicit call agrees
    ids2 = ids[:30].reshape(6, 5)
    w2 = to_dev(w[:30].reshape(6, 5)).requires_grad_(True)
    (bag(to_dev(ids2), per_sample_weights=w2) * to_dev(G)).sum().backward()
    want2, _ = pr.weights_grad("bf16", before, ids2.reshape(-1), None, G, PAD, n_bags=6, fixed_pooling=5)
    assert tuple(w2.grad.shape) == (6, 5)
    same(w2.grad.cpu().numpy().reshape(-1), want2, "2-D")
    explicit = bag.per_sample_weights_grad(ids2, None, G)
    assert tuple(explicit.shape) == (6, 5)
    same(explicit.cpu().numpy().reshape(-1), want2, "explicit")


@pytest.mark.parametrize("dim", [4, 48, 130, 516])
@pytest.mark.parametrize("padded", [False, True])
def test_torch_parity_on_exact_inputs(eng, dim, padded):
    """Against nn.EmbeddingBag's CPU autograd, bit for bit, on inputs whose sums are exact in any order."""
    tab, ids, offsets, G, w = exact_inputs(dim)
    pad = 5 if padded else None
    want = torch_cpu_weights_grad(tab, ids, offsets, G, w, pad)
    bag = tm.PoolingEmbeddingBag(16, dim, mode="sum", padding_idx=pad, _weight=torch.from_numpy(tab), trusted_inputs=True, engine=eng, table_id=14)
    _out, wt = backward_through(lambda wt: bag(to_dev(ids), to_dev(offsets), per_sample_weights=wt), G, w)
    assert np.array_equal(bits(wt.grad.cpu().numpy()), bits(want)), (dim, padded)


# ---- the DLRM harness ---------------------------------------------------------------------------------------------------------------------
def test_dlrm_harness_trains_the_pooling_weights(pel):
    """v_W_l[k].grad is the index-add of the definition's dw (torch's gather backward; exact-valued inputs: any order gives these
    bits), with and without a fused step -- where it is the gradient at the tables the forward read."""
    dh = import_module("pim-embedding-lookup_amd.dlrm_harness")
    dim, ln = 8, [16, 16]
    data = [exact_inputs(dim, seed=k) for k in range(2)]
    vw = [(np.random.default_rng(k).integers(-8, 9, size=16) / 4.0).astype(F) for k in range(2)]
    for fused in (False, True):
        ebc = dh.EmbeddingBagCollection(ln, dim, weights=[x[0] for x in data], weighted_pooling="learned", pooling_weights=vw, trusted_inputs=True)
        try:
            ebc.enable_pooling_weight_grad()
            if fused:
                ebc.enable_fused_sgd(0.25)
            assert all(v.is_leaf and v.requires_grad for v in ebc.v_W_l)
            ly = ebc.apply_emb([to_dev(x[2]) for x in data], [to_dev(x[1]) for x in data])
            sum((y * to_dev(x[3])).sum() for y, x in zip(ly, data)).backward()
            torch.cuda.synchronize()
            for k, (tab, ids, offsets, G, _w) in enumerate(data):
                before = gr.encode("f32", tab)
                dw, _ = pr.weights_grad("f32", before, ids, offsets, G)
                want = np.zeros(16, F)
                np.add.at(want, ids, dw)
                got = ebc.v_W_l[k].grad.cpu().numpy()
                assert np.array_equal(got, want) and want.any(), (fused, k)
                rows, grads, _ = gr.sparse_grad(16, ids, offsets, G, "sum", vw[k][ids], None)
                after = gr.sgd_step("f32", before, rows, grads, F(0.25)) if fused else before
                assert np.array_equal(table_bytes(ebc.engine, k), after)
        finally:
            ebc.close()


def test_dlrm_harness_cli_trains_pooling_weights_for_two_steps(pel):
    dh = import_module("pim-embedding-lookup_amd.dlrm_harness")
    args = ["--arch-embedding-size", "50-60", "--arch-sparse-feature-size", "8", "--mini-batch-size", "4", "--num-indices-per-lookup", "3",
            "--num-batches", "2", "--weighted-pooling", "fixed"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert dh.main(args + ["--train-pooling-weights", "0.1", "--fused-sgd", "0.01"]) == 0
        assert dh.main(args + ["--train-pooling-weights", "0.1"]) == 0
    text = buf.getvalue()
    assert text.count("pooling weights trained by torch.optim.SGD (lr 0.1)") == 2 and "no table step" in text
    with pytest.raises(SystemExit):
        dh.main(["--train-pooling-weights", "0.1"])


# ---- under stream capture -----------------------------------------------------------------------------------------------------------------
def test_a_captured_weights_gradient_replays_with_new_gradients(eng, pel):
    """One graph: a prepared pooled lookup, then emb_grad_weights over two tables (lane-group and fallback) -- a pure enqueue, or
    the capture fails.  Replayed three times with new gradients in the same buffers."""
    dims, kinds = (48, 6), ("f16", "f32")
    c = eng.grad_context(1024, 64)
    batches = [Batch("i64", d, seed=k) for k, d in enumerate(dims)]
    raws = [table(k, d) for k, d in zip(kinds, dims)]
    for t, (k, raw) in enumerate(zip(kinds, raws)):
        load_bytes(eng, 4 + t, k, raw)
    scales = (F(1), F(-0.75), F(1.3))
    outs = [torch.full((b.n + 8,), CANARY, dtype=torch.float32, device=DEV) for b in batches]
    lidx, loff = to_dev(np.arange(40, dtype=np.int64) % ROWS), to_dev(np.arange(0, 40, 4, dtype=np.int64))
    plan = eng.plan([4], [lidx], [loff])
    stream = torch.cuda.Stream()

    def enqueue():
        h = stream.cuda_stream
        plan.launch(h)
        c.weights_grad([4, 5], [b.d_ids for b in batches], [b.d_off for b in batches], [b.d_G for b in batches], padding_idx=PAD,
                       outs=[o[:b.n] for o, b in zip(outs, batches)], stream=h)

    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue()                                                                         # the warm-up, uncaptured
        torch.cuda.synchronize()
        assert c.report() == sum(b.n_bad for b in batches)
        for o in outs:
            o.fill_(CANARY)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            enqueue()
        torch.cuda.synchronize()
        assert all((o == CANARY).all().item() for o in outs)                                  # the capture itself ran nothing
        for s in scales:
            Gs = [(b.G * s).astype(F) for b in batches]
            for b, g in zip(batches, Gs):
                b.d_G.copy_(to_dev(g))
            graph.replay()
            torch.cuda.synchronize()
            for b, g, o, k, raw in zip(batches, Gs, outs, kinds, raws):
                h = o.cpu().numpy()
                same(h[:b.n], b.reference(k, raw, G=g)[0], ("replay", float(s)))
                assert (h[b.n:] == CANARY).all()
        assert c.report() == 3 * sum(b.n_bad for b in batches)
    finally:
        torch.cuda.synchronize()
        plan.destroy()
        c.close()
