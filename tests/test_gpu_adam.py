"""GPU: the fused Adam steps of the backward pass (emb_grad_adam_step, include/pimemb_grad.h, THE ADAM STEPS), bit for bit.  The reference
is tests/adam_ref.py -- the definition as a loop over tests/grad_ref.py's rows, pinned against torch.optim.SparseAdam by
tests/test_adam_cpu.py -- and the inputs are tests/grad_cases.py's batch of about 2 000 positions over 3001 rows (a run of 140, singletons,
rows 0 and 3000, padding, empty bags, bad ids of both widths).  Every test compares the WHOLE table's bytes and both WHOLE states' bits:
untouched rows are covered too.  No tolerance anywhere."""
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
from grad_gpu import DEV, F, check_state, check_table, load_bytes, table_bytes, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

N = gc.NR_ROWS
LR, BETAS, EPS = 0.05, (0.9, 0.99), 1e-6      # (no powers of two: every rounding counts)
S = 8                                          # the segmented context: the run of 140 is 18 segments


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = eng.grad_context(4096, 512)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seg(eng):
    c = eng.grad_context(4096, 512, order="segmented", segment=S, max_dim=512)
    yield c
    c.close()


def batch_on_device(width, mode_name):
    mode, weighted, padded = gc.MODES[mode_name]
    ids, offsets = gc.bad_ids(width)
    arr = gc.ids_array(ids, width)
    return dict(indices=[to_dev(arr)], offsets=[to_dev(offsets.astype(arr.dtype))], modes=mode, per_sample_weights=to_dev(gc.weights()) if weighted else None,
                padding_idx=gc.PAD if padded else None)


_states = {}


def init_state(dim, rowwise):
    """(M, V) before a step.  V: random and non-negative over many magnitudes, every fifth row 0, the run of 140 at 0, row 3000 at 1e30, and
    fp32 DENORMALS on the rows of bags 7 and 8, whose gradients are denormals (grad_cases.grads).  M: signed randoms, zero where V is."""
    key = (dim, rowwise)
    if key not in _states:
        rng = np.random.default_rng(1900 + dim + rowwise)
        ids, offsets, _bad = gc.batch()
        at = [p for b in (7, 8) for p in range(int(offsets[b]), int(offsets[b + 1]))]
        tiny = sorted({ids[p] for p in at if 0 <= ids[p] < N and ids[p] not in (gc.PAD, gc.HOT, 3000)})
        shape = (N,) if rowwise else (N, dim)
        v = (np.abs(rng.standard_normal(shape)) * np.exp2(rng.integers(-12, 12, size=(N,) + (1,) * (len(shape) - 1)))).astype(F)
        m = (rng.standard_normal((N, dim)) * np.exp2(rng.integers(-8, 8, size=(N, 1)))).astype(F)
        v[::5], m[::5] = 0, 0
        v[gc.HOT], m[gc.HOT] = 0, 0
        v[3000] = F(1e30)
        v[tiny] = np.array([1, 0x00400000, 0x007FFFFF], np.uint32).view(F)[np.arange(len(tiny)) % 3].reshape((-1,) + (1,) * (len(shape) - 1))
        m.setflags(write=False), v.setflags(write=False)
        _states[key] = (m, v)
    return _states[key]


_wants = {}


def reference(kind, dim, mode_name, width, rowwise, segment=None):
    """(table bytes, M, V) after ONE step with t = 1 from gc.step_table / init_state, by adam_ref; once per case."""
    key = (kind, dim, mode_name, width, rowwise, segment)
    if key not in _wants:
        rows, grads, n_bad = sr.batch_reference(segment, width, mode_name, dim) if segment else gc.reference(width, mode_name, dim, overflow=False)
        assert n_bad == 5 and gc.HOT in rows and 0 in rows and 3000 in rows
        _wants[key] = ar.adam_step(kind, gc.step_table(kind, dim), *init_state(dim, rowwise), rows, grads, LR, BETAS, EPS, 1, rowwise=rowwise)
    return _wants[key]


def check(eng, t, d_m, d_v, want, what, nan_kind=None):
    what = what if isinstance(what, tuple) else (what,)
    got = table_bytes(eng, t)
    if nan_kind:      # later steps of a row that overflowed: an element that is NaN on both sides is equal (NaN payloads are unspecified)
        both = np.isnan(ar.gr.decode(nan_kind, got)) & np.isnan(ar.gr.decode(nan_kind, want[0]))
        got = np.where(np.repeat(both, got.shape[1] // both.shape[1], axis=1), want[0], got)
    check_table(got, want[0], what)
    check_state(d_m, want[1], what + ("exp_avg",))
    check_state(d_v, want[2], what + ("exp_avg_sq",))


def run_case(eng, c, kind, dim, mode_name, width, rowwise, segment=None):
    want = reference(kind, dim, mode_name, width, rowwise, segment)
    init, (m0, v0) = gc.step_table(kind, dim), init_state(dim, rowwise)
    assert (want[0] != init).any() and (want[1] != m0).any() and (want[2] != v0).any()
    load_bytes(eng, 2, kind, init)
    d_m, d_v = to_dev(m0), to_dev(v0)
    c.adam_step([2], grads=[to_dev(gc.grads(dim, overflow=False))], exp_avgs=[d_m], exp_avg_sqs=[d_v], lr=LR, betas=BETAS, eps=EPS, step=1, rowwise=rowwise,
                **batch_on_device(width, mode_name))
    check(eng, 2, d_m, d_v, want, (kind, dim, mode_name, width, rowwise, segment))
    assert c.report() == 5


@pytest.mark.parametrize("width", ["u32", "i64"])
@pytest.mark.parametrize("mode_name", ["weighted+pad", "mean+pad"])
@pytest.mark.parametrize("dim", [8, 48, 6])            # two lanes; 12 pieces in 16 lanes; the element-wise kernel
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_adam_equals_the_definition_over_the_whole_table_and_states(eng, ctx, kind, dim, mode_name, width):
    run_case(eng, ctx, kind, dim, mode_name, width, rowwise=False)


@pytest.mark.parametrize("mode_name", ["sum", "mean+pad"])
@pytest.mark.parametrize("dim", [4, 48, 256, 320, 512])      # one lane; 12 pieces in 16 lanes; a full wavefront; 16 lanes hold two pieces; all do
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_rowwise_adam_equals_the_definition_over_the_whole_table_and_states(eng, ctx, kind, dim, mode_name):
    run_case(eng, ctx, kind, dim, mode_name, "i64", rowwise=True)


@pytest.mark.parametrize("kind,dim,rowwise", [("bf16", 48, False), ("f32", 6, False), ("f32", 320, True)])
def test_the_segmented_order(eng, seg, kind, dim, rowwise):
    run_case(eng, seg, kind, dim, "weighted+pad" if not rowwise else "sum", "i64", rowwise, segment=S)
    assert not np.array_equal(reference(kind, dim, "sum", "i64", rowwise, S)[1], reference(kind, dim, "sum", "i64", rowwise)[1])      # other bits than the position order


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_a_misaligned_exp_avg_takes_the_elementwise_kernel_with_the_same_bits(eng, ctx, kind):
    """exp_avg one float into its allocation: 4-byte but not 16-byte aligned.  SparseAdam gives the lane-group kernel's bits through the
    element-wise one and writes nothing around the state; row-wise Adam refuses, and leaves everything alone."""
    dim = 8
    want = reference(kind, dim, "weighted+pad", "u32", False)
    init, (m0, v0) = gc.step_table(kind, dim), init_state(dim, False)
    load_bytes(eng, 2, kind, init)
    room = torch.full((m0.size + 8,), float("nan"), device=DEV)
    d_m, d_v = room[1:1 + m0.size], to_dev(v0)
    d_m.copy_(to_dev(m0).reshape(-1))
    assert d_m.data_ptr() % 16 == 4 and d_m.is_contiguous()
    args = dict(grads=[to_dev(gc.grads(dim, overflow=False))], lr=LR, betas=BETAS, eps=EPS, step=1, **batch_on_device("u32", "weighted+pad"))
    with pytest.raises(import_module("pim-embedding-lookup_amd.lib").PimembError, match="lane-group shape"):
        ctx.adam_step([2], exp_avgs=[d_m], exp_avg_sqs=[to_dev(init_state(dim, True)[1])], rowwise=True, **args)
    check(eng, 2, d_m, d_v, (init, m0, v0), (kind, "refused"))
    ctx.adam_step([2], exp_avgs=[d_m], exp_avg_sqs=[d_v], **args)
    check(eng, 2, d_m, d_v, want, (kind, dim, "misaligned"))
    assert torch.isnan(room[0]) and torch.isnan(room[1 + m0.size:]).all()
    ctx.report()


def three_steps(kind, dim, rowwise, Gs):
    """[(table, M, V) after steps t = 1, 2, 3] of the batch in sum mode with the gradients Gs."""
    ids, offsets = gc.bad_ids("i64")
    state, out = (gc.step_table(kind, dim),) + init_state(dim, rowwise), []
    for t, G in enumerate(Gs, 1):
        rows, grads, _ = ar.gr.sparse_grad(N, ids, offsets, G)
        state = ar.adam_step(kind, *state, rows, grads, LR, BETAS, EPS, t, rowwise=rowwise)
        out.append(state)
    return out


@pytest.mark.parametrize("kind,dim,rowwise", [("bf16", 48, False), ("f32", 320, True)])
def test_three_steps_back_to_back_and_as_one_captured_graph(eng, ctx, kind, dim, rowwise):
    """t = 1, 2, 3 without a host wait; then ONE captured step replayed three times, a new gradient in the same buffer and the step size of
    t written into step_size_dev before each replay (the spec's own step stays 1)."""
    Gs = [gc.grads(dim, overflow=False)] + [(gc.grads(dim, overflow=False) * F(s)).astype(F) for s in (-0.5, 3.0)]
    wants = three_steps(kind, dim, rowwise, Gs)
    b = batch_on_device("i64", "sum")
    d_Gs = [to_dev(G) for G in Gs]

    def fresh():
        load_bytes(eng, 2, kind, gc.step_table(kind, dim))
        return [to_dev(s) for s in init_state(dim, rowwise)]
    d_m, d_v = fresh()
    for t in (1, 2, 3):
        ctx.adam_step([2], grads=[d_Gs[t - 1]], exp_avgs=[d_m], exp_avg_sqs=[d_v], lr=LR, betas=BETAS, eps=EPS, step=t, rowwise=rowwise, **b)
    check(eng, 2, d_m, d_v, wants[2], (kind, dim, rowwise, "three steps"), nan_kind=kind)
    ss_dev, G = torch.zeros(1, dtype=torch.float32, device=DEV), d_Gs[0].clone()
    stream = torch.cuda.Stream()
    enqueue = lambda: ctx.adam_step([2], grads=[G], exp_avgs=[d_m], exp_avg_sqs=[d_v], lr=LR, betas=BETAS, eps=EPS, step=1, rowwise=rowwise,  # noqa: E731
                                    step_size_dev=ss_dev, stream=stream.cuda_stream, **b)
    d_m, d_v = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        enqueue()
    torch.cuda.synchronize()
    check(eng, 2, d_m, d_v, (gc.step_table(kind, dim),) + init_state(dim, rowwise), "the capture itself ran nothing")
    for t in (1, 2, 3):
        with torch.cuda.stream(stream):
            G.copy_(d_Gs[t - 1])
            ss_dev.fill_(ctx.adam_constants(LR, BETAS, EPS, t)[2])
            graph.replay()
        torch.cuda.synchronize()
        check(eng, 2, d_m, d_v, wants[t - 1], (kind, dim, rowwise, "replay", t), nan_kind=kind)
    assert ctx.report() == 5 * 6      # (three eager steps and three replays; the capture itself ran nothing)


def test_a_refused_call_leaves_table_and_states_alone(eng, ctx, pel):
    """Two descriptors, the second refused (its exp_avg_sq is NULL): the first, fine one is not stepped either."""
    kind, dim = "f32", 8
    init, (m0, v0) = gc.step_table(kind, dim), init_state(dim, False)
    load_bytes(eng, 2, kind, init)
    load_bytes(eng, 3, kind, init)
    d_m, d_v, b = to_dev(m0), to_dev(v0), batch_on_device("i64", "sum")
    two = dict(indices=b["indices"] * 2, offsets=b["offsets"] * 2, grads=[to_dev(gc.grads(dim, overflow=False))] * 2)
    with pytest.raises(pel.lib.PimembError, match="exp_avg_sq of table 3 is NULL"):
        ctx.adam_step([2, 3], exp_avgs=[d_m, d_m], exp_avg_sqs=[d_v, None], lr=LR, **two)
    with pytest.raises(pel.lib.PimembError, match="EMB_POOL_MAX"):
        ctx.adam_step([2, 3], exp_avgs=[d_m, d_m], exp_avg_sqs=[d_v, d_v], lr=LR, modes=["sum", "max"], **two)
    check(eng, 2, d_m, d_v, (init, m0, v0), "refused")
    assert ctx.report() == 0


@pytest.mark.parametrize("rowwise", [False, True])
def test_module_trains_through_backward_and_its_state_dict_round_trips(eng, pel, rowwise):
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    kind, dim = "f32", 8
    ids, offsets = gc.bad_ids("i64")
    clean = [r if 0 <= r < N else 7 for r in ids]             # (the module checks its inputs: no bad ids here)
    d_ids, d_off = to_dev(np.array(clean, np.int64)), to_dev(offsets)
    w0 = ar.gr.decode(kind, gc.step_table(kind, dim))
    bag = tm.PoolingEmbeddingBag(N, dim, mode="sum", engine=eng, table_id=10, _weight=torch.from_numpy(w0.copy()))
    assert bag.adam_exp_avg is None and list(bag.state_dict()) == ["weight"]
    bag.enable_fused_adam(LR, betas=BETAS, eps=EPS, rowwise=rowwise)
    zeros = (np.zeros((N, dim), F), np.zeros((N,) if rowwise else (N, dim), F))
    want = (gc.step_table(kind, dim),) + zeros
    for t in (1, 2, 3):
        G = (gc.grads(dim, overflow=False) * F(t)).astype(F)
        (bag(d_ids, d_off) * to_dev(G)).sum().backward()
        rows, grads, _ = ar.gr.sparse_grad(N, clean, offsets, G)
        want = ar.adam_step(kind, *want, rows, grads, LR, BETAS, EPS, t, rowwise=rowwise)
    check(eng, bag.table_id, bag.adam_exp_avg, bag.adam_exp_avg_sq, want, ("module", rowwise), nan_kind=kind)
    sd = bag.state_dict()
    assert list(sd) == ["weight", "adam_exp_avg", "adam_exp_avg_sq", "adam_step"] and int(sd["adam_step"]) == 3 == bag.adam_step
    other = tm.PoolingEmbeddingBag(N, dim, mode="sum", engine=eng, table_id=11)
    other.load_state_dict(sd)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731 -- (bits: the overflowed row's states hold NaNs)
    assert other.adam_step == 3 and same(other.adam_exp_avg_sq, bag.adam_exp_avg_sq) and same(other.adam_exp_avg, bag.adam_exp_avg)
    bag.enable_fused_sgd(0.1)                                  # one fused optimizer at a time
    assert bag._fused_adam is None and bag.enable_fused_adam(LR)._fused_lr is None
    for kw in (dict(master_weights=True), dict(stochastic_rounding=True), dict(multi_table=True)):
        with pytest.raises(ValueError, match="no master-weight"):
            bag.enable_fused_adam(LR, **kw)
    with pytest.raises(ValueError, match="no master-weight"):
        tm.PoolingEmbeddingBag(N, dim, mode="max", engine=eng, table_id=12).enable_fused_adam(LR)


@pytest.mark.parametrize("flag", ["--fused-adam", "--fused-rowwise-adam"])
def test_harness_trains_with_each_flag(flag, capsys):
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    assert h.main(["--arch-embedding-size=100-200-50", "--arch-sparse-feature-size=16", "--mini-batch-size=32", "--num-batches=2", flag, "0.01"]) == 0
    assert "the fused %s step" % ("row-wise Adam" if "rowwise" in flag else "Adam") in capsys.readouterr().out
