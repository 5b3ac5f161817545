"""GPU: the max-mode backward (emb_grad_max_*, include/pimemb_grad.h) against the loops of tests/grad_max_ref.py, bit for bit: the
winners buffer, the sparse gradient, whole tables and states after the fused steps, in a position-order and a segmented (S = 8)
context.  One ragged batch of 41 bags over a 13-row table: long runs, many ties."""
import functools
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_max_ref as mr  # noqa: E402
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402
import rows_cases as rc  # noqa: E402
from grad_gpu import DEV, bits, check_state, check_table, in_place, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu
tm = import_module("pim-embedding-lookup_amd.torch_module")

F = np.float32
ROWS, PAD, LOSER, LR, EPS, S = 13, 11, 10, F(0.25), F(1e-10), 8
LENS = [0, 1, 7, 8, 9, 16, 17] * 5 + [3, 2, 9, 4, 5, 0]          # bags 35 .. 40: padding only, padding first, a row twice, two with a bad id, empty
LEAD = 3                                                           # positions before offsets[0]: no bag
DIMS = [(4, None), (48, None), (128, None), (320, None), (6, None), (16, 17)]      # (dim, grad_ld): the last two run element-wise


def batch(width):
    """(ids, offsets): the ids of both widths name the same rows; the two bad ids differ in how they are bad."""
    rng = np.random.default_rng(11)
    ids = rng.integers(0, ROWS, size=LEAD + sum(LENS)).astype(np.int64)
    off = LEAD + np.concatenate([[0], np.cumsum(LENS)[:-1]])
    ids[off[np.array(LENS) == 1]] = [0, 1, 5, 8, 9]             # (no one-position bag names LOSER: it would win there)
    ids[off[35]:off[35] + 3] = PAD
    ids[off[36]:off[36] + 2] = [PAD, 6]
    ids[off[37]:off[37] + 9] = [4, 7, 4, 2, 3, 3, 2, 9, 4]
    ids[off[38] + 1] = ROWS if width == "u32" else -1
    ids[off[39] + 2] = 0xFFFFFFFF if width == "u32" else (1 << 32) + 5
    return (ids.astype(np.uint32) if width == "u32" else ids), off.astype(np.uint32 if width == "u32" else np.int64)


@functools.lru_cache(maxsize=None)
def table(kind, dim):
    """Table bytes: rows 2 and 3 equal at the even elements, column 1 -0 in even rows and +0 in odd ones, row LOSER below every other
    row everywhere: it is named 20 times and wins nowhere."""
    w = np.random.default_rng(dim).standard_normal((ROWS, dim)).astype(F)
    w[3, 0::2] = w[2, 0::2]
    w[0::2, 1], w[1::2, 1] = F(-0.0), F(0.0)
    w[LOSER] = F(-1000.0)
    raw = gr.encode(kind, w)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def grads(dim):
    """G with magnitudes from 2^-20 to 2^20: the order of a row's additions shows in the bits."""
    rng = np.random.default_rng(100 + dim)
    G = (rng.standard_normal((len(LENS), dim)) * np.exp2(rng.integers(-20, 21, size=(len(LENS), dim)))).astype(F)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def reference(kind, dim, seg):
    ids, off = batch("i64")
    return mr.sparse_grad(kind, table(kind, dim), ids.tolist(), off, grads(dim), PAD, S if seg else None)


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctxs(eng):
    c = {False: eng.grad_context(1024, 64), True: eng.grad_context(1024, 64, order="segmented", segment=S, max_dim=512)}
    yield c
    for x in c.values():
        x.close()


def device_batch(width, dim, ld):
    ids, off = batch(width)
    G = to_dev(grads(dim))
    return to_dev(ids), to_dev(off), G if ld is None else in_place(G, ld, 0)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("width", ["u32", "i64"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("dim,ld", DIMS)
def test_winners_sparse_gradient_and_steps_equal_the_loops(eng, ctxs, dim, ld, kind, width):
    idx, off, G = device_batch(width, dim, ld)
    init = table(kind, dim)
    pos, seg = reference(kind, dim, False), reference(kind, dim, True)
    assert np.array_equal(pos[0], seg[0]) and (bits(pos[1]) != bits(seg[1])).any(), "the two orders are not witnessed"
    hot = np.bincount(batch("i64")[0][LEAD:].clip(0, ROWS - 1), minlength=ROWS).max()
    assert hot > 17 and pos[2] == 2 and (pos[3][35] == mr.NO_WINNER).all() and (pos[3][0] == mr.NO_WINNER).all()
    loser = [k for k in range(len(pos[0])) if not pos[1][k].any()]      # the rows of U that win nowhere
    assert [int(pos[0][k]) for k in loser] == [LOSER]
    for segmented, (rows, g, n_bad, win) in ((False, pos), (True, seg)):
        ctx, what = ctxs[segmented], (dim, ld, kind, width, segmented)
        load_bytes(eng, 1, kind, init)
        assert np.array_equal(u32(ctx.max_winners([1], [idx], [off], padding_idx=PAD)[0]), win), what
        assert ctx.report() == 0
        got_rows, got_g, got_win = ctx.max_sparse_grad(1, idx, off, G, padding_idx=PAD, return_winners=True)
        assert np.array_equal(got_rows.cpu().numpy(), rows) and np.array_equal(bits(got_g.cpu().numpy()), bits(g)), what      # |U| too
        assert np.array_equal(u32(got_win), win) and ctx.report() == n_bad, what
        assert np.array_equal(u32(ctx.max_sgd_step([1], [idx], [off], [G], LR, padding_idx=PAD)[0]), win), what
        after = table_bytes(eng, 1)
        check_table(after, gr.sgd_step(kind, init, rows, g, LR), what)
        outside = np.setdiff1d(np.arange(ROWS), rows)
        assert PAD in outside and np.array_equal(after[outside], init[outside]) and all(np.array_equal(after[rows[k]], init[rows[k]]) for k in loser)
        for rowwise in ((False, True) if ld is None and dim % 4 == 0 else (False,)):
            s0 = np.random.default_rng(5).random((ROWS,) if rowwise else (ROWS, dim)).astype(F)
            load_bytes(eng, 1, kind, init)
            state = to_dev(s0)
            ctx.max_adagrad_step([1], [idx], [off], [G], [state], LR, eps=EPS, rowwise=rowwise, padding_idx=PAD)
            want_t, want_s = orf.adagrad_step(kind, init, s0, rows, g, LR, EPS, rowwise)
            check_table(table_bytes(eng, 1), want_t, what)
            check_state(state, want_s, what)
        assert ctx.report() == n_bad * (2 if ld is None and dim % 4 == 0 else 1) + n_bad


@pytest.mark.parametrize("segmented", [False, True])
def test_a_table_named_twice_is_judged_at_the_bytes_the_forward_read(eng, ctxs, segmented):
    kind, dim = "f32", 48
    idx, off, G = device_batch("i64", dim, None)
    rows, g, _bad, win = reference(kind, dim, segmented)
    load_bytes(eng, 2, kind, table(kind, dim))
    wins = ctxs[segmented].max_sgd_step([2, 2], [idx, idx], [off, off], [G, G], LR, padding_idx=PAD)
    assert np.array_equal(u32(wins[0]), win) and np.array_equal(u32(wins[1]), win)
    once = gr.sgd_step(kind, table(kind, dim), rows, g, LR)
    check_table(table_bytes(eng, 2), gr.sgd_step(kind, once, rows, g, LR), "stepped twice with the pre-step winners")
    ctxs[segmented].report()


def test_refusals_leave_table_state_and_winners_alone(eng, ctxs, pel):
    UNS, INV = pel.lib.EMB_ERR_UNSUPPORTED, pel.lib.EMB_ERR_INVALID
    ctx, G = ctxs[False], pel.lib.load_grad()
    idx, off, g16 = device_batch("i64", 16, None)
    win = torch.full((len(LENS), 16), 7, dtype=torch.int32, device=DEV)
    state = torch.full((ROWS, 16), 0.5, dtype=torch.float32, device=DEV)

    def refused(t, code, text, call):
        before = table_bytes(eng, t)
        with pytest.raises(pel.PimembError) as ei:
            call()
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
        assert np.array_equal(table_bytes(eng, t), before) and (win == 7).all() and (state == 0.5).all()

    def raw_sgd(mode, weights=None, winners=None):
        keep, d = [], pel.lib.EmbGradDesc()
        itype, _dev = ctx._desc(d, 3, idx, off, g16, mode, weights, PAD, 0, keep)
        ptrs = (pel.lib.C.c_void_p * 1)(win.data_ptr() if winners is None else winners)
        pel.lib.check_grad(G.emb_grad_max_sgd(ctx._h, pel.lib.C.byref(d), ptrs, 1, itype, 0.25, None))
    load_bytes(eng, 3, "f32", table("f32", 16))

    def sgd(t, g=g16, c=ctx, own=True):
        c.max_sgd_step([t], [idx], [off], [g], LR, padding_idx=PAD, winners=[win] if own else None)
    refused(3, INV, "takes EMB_POOL_MAX descriptors", lambda: raw_sgd("sum"))
    refused(3, INV, "takes EMB_POOL_MAX descriptors", lambda: raw_sgd("mean"))
    refused(3, INV, "per_sample_weights do not go", lambda: raw_sgd("max", torch.ones(idx.shape[0], device=DEV)))
    refused(3, INV, "NULL or not 4-byte aligned", lambda: raw_sgd("max", winners=0))
    refused(3, INV, "NULL or not 4-byte aligned", lambda: raw_sgd("max", winners=win.data_ptr() + 2))
    eng.set_hot_rows(3, [1, 2])
    refused(3, UNS, "clear the set", lambda: sgd(3))
    eng.set_hot_rows(3, [])
    for kind, dim in (("e4m3", 16), ("e5m2", 16), ("mxfp4", 32)):
        load_bytes(eng, 4, kind, rc.host_encode(kind, np.random.default_rng(2).standard_normal((ROWS, dim)).astype(F)))
        refused(4, UNS, "fp8 or MXFP4", lambda: sgd(4, to_dev(grads(dim)), own=False))
        with pytest.raises(pel.PimembError) as ei:
            ctx.max_sparse_grad(4, idx, off, to_dev(grads(dim)), padding_idx=PAD)
        assert ei.value.code == UNS and "fp8 or MXFP4" in str(ei.value)
    eng.load_table(4, np.ones((ROWS, 16), dtype=np.int32))
    refused(4, UNS, "EMB_FIXED32", lambda: sgd(4))
    refused(3, UNS, "row-wise Adagrad needs the lane-group shape", lambda: ctx.max_adagrad_step(
        [3], [idx], [off], [in_place(g16, 17, 0)], [state[:, 0].contiguous()], LR, rowwise=True, padding_idx=PAD, winners=[win]))
    with eng.grad_context(64, 64) as small:                                      # the batch holds about 300 indices
        refused(3, INV, "created for 64", lambda: sgd(3, c=small))
    load_bytes(eng, 4, "e4m3", rc.host_encode("e4m3", np.ones((ROWS, 16), dtype=F)))                                    # a refused second table
    refused(3, UNS, "fp8 or MXFP4", lambda: ctx.max_sgd_step([3, 4], [idx, idx], [off, off], [g16, g16], LR, padding_idx=PAD, winners=[win, win]))
    with pytest.raises(pel.PimembError, match="EMB_POOL_MAX needs the forward's per-element argmax"):                   # the old calls keep refusing
        ctx.sgd_step([3], [idx], [off], [g16], LR, modes="max")
    assert ctx.report() == 0


def test_a_captured_max_sgd_step_replays_with_new_gradients(eng, ctxs):
    kind, dim = "bf16", 128
    idx, off, G = device_batch("u32", dim, None)
    win = torch.zeros((len(LENS), dim), dtype=torch.int32, device=DEV)
    load_bytes(eng, 5, kind, table(kind, dim))
    ids, offs = batch("i64")
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctxs[True].max_sgd_step([5], [idx], [off], [G], LR, padding_idx=PAD, winners=[win])      # (uncaptured first: nothing lazy is left for the capture)
        with torch.cuda.graph(graph, stream=side):
            ctxs[True].max_sgd_step([5], [idx], [off], [G], LR, padding_idx=PAD, winners=[win])
    torch.cuda.current_stream().wait_stream(side)
    want = gr.sgd_step(kind, table(kind, dim), *reference(kind, dim, True)[:2], LR)
    for scale in (F(-2.0), F(0.5)):                                              # two replays, each with a new G in the captured buffer
        G.copy_(to_dev(grads(dim) * scale))
        graph.replay()
        rows, g, _bad, w = mr.sparse_grad(kind, want, ids.tolist(), offs, grads(dim) * scale, PAD, S)
        want = gr.sgd_step(kind, want, rows, g, LR)
        check_table(table_bytes(eng, 5), want, scale)
        assert np.array_equal(u32(win), w)
    ctxs[True].report()


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def exact_inputs(dim=8):
    """Small integers everywhere: every sum of the backward is exact, so torch's CPU autograd is the reference, order or not."""
    rng = np.random.default_rng(3)
    w = rng.integers(-3, 4, size=(ROWS, dim)).astype(F)
    ids, off = batch("i64")
    ids, off = ids[LEAD:].clip(0, ROWS - 1), off - LEAD
    return w, torch.from_numpy(ids), torch.from_numpy(off), torch.from_numpy(rng.integers(-8, 9, size=(len(LENS), dim)).astype(F))


def torch_cpu_grad(w, ids, off, G, mode="max", pad=PAD):
    wt = torch.from_numpy(w.copy()).requires_grad_(True)
    torch.nn.functional.embedding_bag(ids, wt, off, mode=mode, padding_idx=pad).backward(G)
    return wt.grad.numpy()


def test_module_backward_steps_the_table_and_sparse_grad_equals_torch(eng, pel):
    w, ids, off, G = exact_inputs()
    bag = tm.PoolingEmbeddingBag(ROWS, 8, mode="max", padding_idx=PAD, _weight=torch.from_numpy(w), engine=eng, table_id=6)
    dense = bag.sparse_grad(ids, off, G).to_dense().cpu().numpy()
    want = torch_cpu_grad(w, ids, off, G)
    assert np.array_equal(dense, want)
    for kw in (dict(master_weights=True), dict(stochastic_rounding=True)):
        with pytest.raises(ValueError, match="mode='max'"):
            bag.enable_fused_sgd(0.5, **kw)
    bag.enable_fused_sgd(0.5)
    out = bag(ids.to(DEV), off.to(DEV))
    (out * G.to(DEV)).sum().backward()
    assert np.array_equal(bag.weight.cpu().numpy(), w - F(0.5) * want)           # exact: small integers and a power of two


def test_fused_model_steps_a_max_and_a_sum_table(eng, pel):
    w, ids, off, G = exact_inputs()
    bags = [tm.PoolingEmbeddingBag(ROWS, 8, mode=m, padding_idx=PAD, _weight=torch.from_numpy(w), engine=eng, table_id=7 + k) for k, m in enumerate(("max", "sum"))]
    model = tm.FusedPoolingEmbeddingBags(bags)
    with pytest.raises(ValueError, match="mode='max'"):
        model.enable_fused_sgd(0.5, multi_table=True)
    model.enable_fused_sgd(0.5)
    outs = model([off.to(DEV), off.to(DEV)], [ids.to(DEV), ids.to(DEV)])
    sum((o * G.to(DEV)).sum() for o in outs).backward()
    for b, mode in zip(bags, ("max", "sum")):
        assert np.array_equal(b.weight.cpu().numpy(), w - F(0.5) * torch_cpu_grad(w, ids, off, G, mode)), mode
