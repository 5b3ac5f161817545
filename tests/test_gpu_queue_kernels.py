"""GPU: every kernel an emb_queue_flush can choose, bit for bit.  A flush whose pending requests add up to a big one-hot launch
leaves the lane-group kernel its requests were tiled for, re-tiles every descriptor and runs the wave-batch (kind 0) or the
two-batch kernel (kind 2) on the plain 2-D grid of max_tiles x descriptors -- the only multi-descriptor launch of those kernels
that is decoded by blockIdx.x / blockIdx.y instead of an XCD map.  The layouts (tests/queue_cases.py, proven on the CPU by
test_queue_cases_cpu.py) sit right at choose_kernel's thresholds, so these tests depend on them: 131 072 bags for the wave-batch
kernel, 524 288 bags and rows of <= 4 lanes for the two-batch kernel, n_indices <= 2 n_bags for both, and kQueueBlock (1 MiB)
for what a host queue stages.  Who retunes one of them moves the constants at the top of queue_cases.py.

The method of every test: outputs are prefilled with the bit pattern 0x7fc0dead; in device space all outputs of a flush are
carved back to back from ONE tensor with 64 guard words between neighbours and at both ends; after flush and wait every request's
rows equal oracle.c_bag_sum (c_lookup_fixed32 for FIXED32) over that request alone as raw bits, every guard word is untouched,
the flush counted ONE kernel launch, and n_launches_by_kind moved by +1 at the expected kind and nowhere else."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import queue_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NP_IDX = {"u32": np.uint32, "i64": np.int64}
_REFS = {}


def to_dev(a):
    """numpy ids -> CUDA tensor (uint32 bits travel as int32)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def refs_row_bytes(dtype, dim):
    return dim * {"fp32": 4, "fixed32": 4, "fp16": 2, "bf16": 2, "e4m3": 1, "e5m2": 1}[dtype]


def engine_with(pel, dtype, dim):
    """An engine holding the five tables of queue_cases.TABLE_ROWS at this dtype and dim -> (engine, their reference tables)."""
    eng = pel.EmbeddingEngine(device=0, max_tables=16)
    tabs = qc.make_tables(dtype, dim, seed=qc.TABLE_SEED)
    for t, (rows, name, _ref) in enumerate(tabs):
        eng.load_table(t, rows, dtype=None if name is None else getattr(pel, name))
    return eng, [ref for _rows, _name, ref in tabs]


def references(oracle, dtype, dim, refs, lay, key=None):
    """The oracle's rows of every descriptor of a layout; those of the shared layouts -- key = (class, cap): qc.layout(*key), and
    nothing else, over the tables of engine_with -- are computed once per (dtype, dim) while they are small (dim <= 16).  The
    cache key names both seeds, so rows of other tables or another layout never answer for these."""
    if key is None or dim > 16:
        return [qc.reference(oracle, dtype, refs[d.table], d) for d in lay.descs]
    assert lay is qc.layout(*key), "only the shared layout of this class may use the cache"
    k = (dtype, dim, qc.TABLE_SEED, qc.LAYOUT_SEED) + key
    if k not in _REFS:
        _REFS[k] = [qc.reference(oracle, dtype, refs[d.table], d) for d in lay.descs]
    return _REFS[k]


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "%d of %d words differ; first (bag, col, got, want): %s" % (
        len(bad), got.size, [(int(b), int(c), hex(int(got[b, c])), hex(int(want[b, c]))) for b, c in bad[:4]])


def run_flush(pel, eng, q, lay, want, dim, space, ids, kind, n_threads=1):
    """Queue the requests of a layout, flush, wait for every ticket and check the flush as the module's docstring says."""
    npdt = NP_IDX[ids]
    sentinel = np.uint32(qc.SENTINEL)
    host = space == "host"
    if host:
        one = None
        outs = [np.full((d.n_bags, dim), sentinel, np.uint32).view(np.float32) for d in lay.descs]
    else:
        total = qc.GUARD + sum(d.n_bags * dim + qc.GUARD for d in lay.descs)
        one = torch.full((total,), qc.SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        outs, at = [], qc.GUARD
        for d in lay.descs:
            outs.append(one[at:at + d.n_bags * dim].view(d.n_bags, dim))
            at += d.n_bags * dim + qc.GUARD
    args, k = [], 0
    for rq in lay.requests:
        conv = (lambda a: a.astype(npdt)) if host else (lambda a: to_dev(a.astype(npdt)))
        args.append(([d.table for d in rq], [conv(d.idx) for d in rq], [None if d.off is None else conv(d.off) for d in rq],
                     outs[k:k + len(rq)], [d.fixed_pooling for d in rq]))
        k += len(rq)
    before = eng.stats()
    tickets, errors, added = [None] * len(args), [], [0] * n_threads

    def client(r0):
        try:
            for r in range(r0, len(args), n_threads):
                tickets[r] = q.add(*args[r])
                added[r0] += 1
        except Exception as ex:  # noqa: BLE001 -- reported by the test's thread below
            errors.append(ex)

    if n_threads > 1:
        threads = [threading.Thread(target=client, args=(r0,)) for r0 in range(n_threads)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    else:
        client(0)
    assert not errors, errors
    assert sum(added) == len(args) and (n_threads == 1 or min(added) >= 2), "every client thread adds several requests: %s" % added
    assert q.flush() == len(args) and q.flush() == 0
    for t in tickets:
        q.wait(t)
    torch.cuda.synchronize()
    after = eng.stats()
    assert after["n_kernel_launches"] - before["n_kernel_launches"] == 1, "a flush is ONE launch"
    delta = [a - b for a, b in zip(after["n_launches_by_kind"], before["n_launches_by_kind"])]
    assert delta == [int(i == kind) for i in range(len(delta))], (delta, kind)
    if not host:                                          # every guard word still holds the sentinel
        words = one.view(torch.int32)
        guards, at = [words[:qc.GUARD]], qc.GUARD
        for d in lay.descs:
            at += d.n_bags * dim
            guards.append(words[at:at + qc.GUARD])
            at += qc.GUARD
        g = torch.stack(guards).cpu().numpy()
        touched = np.flatnonzero((g != qc.SENTINEL).any(axis=1))
        assert len(touched) == 0, "guard words overwritten behind descriptor(s) %s (-1: before the first)" % [int(i) - 1 for i in touched]
    for i, d in enumerate(lay.descs):
        got = (outs[i] if host else outs[i].cpu().numpy()).view(np.uint32)
        w = want[i].view(np.uint32)
        assert got.shape == w.shape
        if not np.array_equal(got, w):
            kept = np.flatnonzero((got == sentinel).all(axis=1))
            pytest.fail("descriptor %d (table %d, %d bags): %s; %d bags still hold the sentinel (first %s)" % (
                i, d.table, d.n_bags, first_difference(got, w), len(kept), kept[:4].tolist()))
    return outs


def queue_of(pel, eng, ids, space):
    return pel.RequestQueue(eng, pel.EMB_IDX_U32 if ids == "u32" else pel.EMB_IDX_I64,
                            pel.EMB_MEM_HOST if space == "host" else pel.EMB_MEM_DEVICE)


def flush_once(pel, oracle, dtype, dim, lay, key, space, ids, kind, n_threads=1):
    eng, refs = engine_with(pel, dtype, dim)
    q = queue_of(pel, eng, ids, space)
    try:
        run_flush(pel, eng, q, lay, references(oracle, dtype, dim, refs, lay, key), dim, space, ids, kind, n_threads)
    finally:
        q.close()
        eng.close()


# ---- (a) the wave-batch kernel through the queue, device space ---------------------------------------------------------------------
WAVE_CASES = [("fp32", 4, "u32"), ("fp32", 16, "u32"), ("fp32", 16, "i64"), ("fp32", 24, "u32"), ("fp32", 128, "u32"),
              ("fp32", 256, "u32"), ("fp16", 64, "u32"), ("bf16", 64, "u32"), ("bf16", 64, "i64"), ("e4m3", 64, "u32"),
              ("e5m2", 1024, "u32"), ("fixed32", 16, "u32")]


@pytest.mark.parametrize("dtype,dim,ids", WAVE_CASES, ids=["%s-d%d-%s" % c for c in WAVE_CASES])
def test_wave_flush_runs_the_wave_batch_kernel(pel, oracle, dtype, dim, ids):
    """A flush of just over 131 072 bags (choose_kernel's threshold) with n_indices <= 2 n_bags: kind 0 on the 2-D grid, for rows
    of 1 .. 64 lanes (fp32 dim 24: 6 pieces in 8 lanes, two of them dead), every table dtype with a wave-batch kernel, both index
    widths."""
    lay = qc.layout("wave")
    assert qc.expected_kind(lay.B, lay.N, qc.lanes_per_row(refs_row_bytes(dtype, dim))) == 0
    flush_once(pel, oracle, dtype, dim, lay, ("wave", None), "device", ids, 0)


# ---- (b) the two-batch kernel through the queue, device space ----------------------------------------------------------------------
TWO_CASES = [("fp32", 4, 2), ("fp32", 16, 2), ("fp16", 8, 2), ("e4m3", 16, 2), ("fixed32", 16, 2), ("fp32", 128, 0)]


@pytest.mark.parametrize("dtype,dim,kind", TWO_CASES, ids=["%s-d%d-kind%d" % c for c in TWO_CASES])
def test_two_flush_runs_the_two_batch_kernel_for_narrow_rows(pel, oracle, dtype, dim, kind):
    """A flush of just over 524 288 bags: kind 2 for rows of <= 4 lanes (choose_kernel's second threshold), re-tiled to 256 bags
    per tile; the same flush over rows of 32 lanes stays on the wave-batch kernel, which has no two-batch twin that wide."""
    lay = qc.layout("two")
    assert qc.expected_kind(lay.B, lay.N, qc.lanes_per_row(refs_row_bytes(dtype, dim))) == kind
    flush_once(pel, oracle, dtype, dim, lay, ("two", None), "device", "u32", kind)


# ---- (c) host space: indices, offsets and rows in the queue's pinned staging, requests added from four threads ------------------
HOST_CASES = [("wave", "fp32", 16, "u32", 0), ("wave", "fp32", 16, "i64", 0), ("wave", "bf16", 16, "u32", 0), ("two", "fp32", 4, "u32", 2)]


@pytest.mark.parametrize("cls,dtype,dim,ids,kind", HOST_CASES, ids=["%s-%s-d%d-%s" % c[:4] for c in HOST_CASES])
def test_host_queue_flush_switches_kernel(pel, oracle, cls, dtype, dim, ids, kind):
    """The same switch in a HOST queue: every staged buffer is at most kQueueBlock (1 MiB), so the totals are met by many
    descriptors of host_cap(dim) bags.  The flush's 8 requests are added from 4 threads, two each and interleaved (run_flush
    asserts that every thread added its share), every ticket is waited for, and the caller's own arrays receive the oracle's rows
    (the sentinel survives nowhere)."""
    lay = qc.layout(cls, qc.host_cap(dim))
    assert len(lay.requests) == qc.HOST_REQUESTS >= 2 * qc.HOST_THREADS
    assert qc.expected_kind(lay.B, lay.N, qc.lanes_per_row(refs_row_bytes(dtype, dim))) == kind
    flush_once(pel, oracle, dtype, dim, lay, (cls, qc.host_cap(dim)), "host", ids, kind, n_threads=qc.HOST_THREADS)


# ---- (d) both sides of the switch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["just-below", "too-pooled"])
def test_boundary_flush_stays_on_the_lane_group_kernel(pel, oracle, cls):
    """131 071 bags (one short of choose_kernel's threshold), and 131 109 bags with 2 n_bags + 1 indices (one too many): kind 1,
    the same bits."""
    lay = qc.layout(cls)
    assert qc.expected_kind(lay.B, lay.N, 4) == 1
    flush_once(pel, oracle, "fp32", 16, lay, (cls, None), "device", "u32", 1)


# ---- (e) MXFP4 has the lane-group kernel only ---------------------------------------------------------------------------------------
def test_mxfp4_wave_flush_stays_on_the_lane_group_kernel(pel, oracle):
    """The `wave` layout over MXFP4 dim 64 tables: kind 1 whatever the totals say; bits against the dequantised table."""
    flush_once(pel, oracle, "mxfp4", 64, qc.layout("wave"), ("wave", None), "device", "u32", 1)


# ---- (f) nothing of a big flush sticks to the queue ---------------------------------------------------------------------------------
def test_kernel_switch_does_not_leak_between_flushes(pel, oracle):
    """ONE queue: small (kind 1), wave (kind 0), small (kind 1), two (kind 2), small (kind 1) -- five flushes, more than the
    queue's kQueueGens = 4 generations.  The small flushes behind a big one are tiled and launched for the lane-group kernel again."""
    eng, refs = engine_with(pel, "fp32", 16)
    q = queue_of(pel, eng, "u32", "device")
    try:
        for n, (cls, kind) in enumerate([("small", 1), ("wave", 0), ("small", 1), ("two", 2), ("small", 1)]):
            if cls == "small":
                lay, key = qc.ragged_layout(10 + n, bags=(1, 17, 32, 5), max_len=3, tables=(0, 1, 2, 3, 4)), None
            else:
                lay, key = qc.layout(cls), (cls, None)
            run_flush(pel, eng, q, lay, references(oracle, "fp32", 16, refs, lay, key), 16, "device", "u32", kind)
    finally:
        q.close()
        eng.close()


# ---- (g) the header's promise: the bits a lookup of its own would give --------------------------------------------------------------
def test_wave_flush_equals_each_requests_own_lookup(pel, oracle):
    """Every request of a `wave` flush equals eng.lookup_batched over that request's tables bit for bit.  The direct call is far
    below choose_kernel's threshold and runs other kernels, so this compares kernels with each other."""
    lay = qc.layout("wave")
    eng, refs = engine_with(pel, "fp32", 16)
    q = queue_of(pel, eng, "u32", "device")
    try:
        outs = run_flush(pel, eng, q, lay, references(oracle, "fp32", 16, refs, lay, ("wave", None)), 16, "device", "u32", 0)
        assert all(sum(d.n_bags for d in rq) < qc.WAVE_MIN_BAGS for rq in lay.requests)
        k = 0
        for rq in lay.requests:
            live = [(d, outs[k + j]) for j, d in enumerate(rq) if d.n_bags]
            k += len(rq)
            before = eng.stats()["n_launches_by_kind"]
            direct = eng.lookup_batched([d.table for d, _o in live], [to_dev(d.idx.astype(np.uint32)) for d, _o in live],
                                        [None if d.off is None else to_dev(d.off.astype(np.uint32)) for d, _o in live],
                                        fixed_pooling=[d.fixed_pooling for d, _o in live])
            torch.cuda.synchronize()
            assert [a - b for a, b in zip(eng.stats()["n_launches_by_kind"], before)][0] == 0      # not the wave-batch kernel
            for (d, o), got in zip(live, direct):
                assert torch.equal(got.view(torch.int32), o.view(torch.int32)), (d.table, d.n_bags)
    finally:
        q.close()
        eng.close()


# ---- (h) rows that are no 16-byte multiple: the queue's any-dim kernel --------------------------------------------------------------
ANYDIM_CASES = [("fp32", 3), ("fp32", 10), ("fp16", 5), ("e4m3", 36)]


@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("dtype,dim", ANYDIM_CASES, ids=["%s-d%d" % c for c in ANYDIM_CASES])
def test_anydim_queue(pel, oracle, dtype, dim, space):
    """fp32 dim 3 (a lane per element), fp32 dim 10 and e4m3 dim 36 (a lane per 16-byte piece), fp16 dim 5: three ragged requests
    (1, 17 and 300 bags of 0 .. 9 indices) run as ONE launch of kind 3; a table of the same dtype and another dim is refused."""
    assert qc.lanes_per_row(refs_row_bytes(dtype, dim)) == 0
    lay = qc.ragged_layout(dim, bags=(1, 17, 300), max_len=9, tables=(0, 1))
    assert max(int(d.lens.max()) for d in lay.descs) == 9 and any((d.lens == 0).any() for d in lay.descs)
    eng, refs = engine_with(pel, dtype, dim)
    other = qc.make_table(dtype, 100, dim + 1, 1)
    eng.load_table(9, other[0], dtype=None if other[1] is None else getattr(pel, other[1]))
    q = queue_of(pel, eng, "u32", space)
    try:
        want = references(oracle, dtype, dim, refs, lay)
        run_flush(pel, eng, q, lay, want, dim, space, "u32", 3)
        one = np.zeros(1, np.uint32)
        out = np.zeros((1, dim + 1), np.float32)
        with pytest.raises(pel.PimembError) as ex:
            q.add([9], [one if space == "host" else to_dev(one)], [one if space == "host" else to_dev(one)],
                  [out if space == "host" else torch.from_numpy(out).to(DEV)])
        assert ex.value.code == pel.lib.EMB_ERR_UNSUPPORTED
        assert q.flush() == 0                             # the refused request left nothing pending
        run_flush(pel, eng, q, lay, want, dim, space, "u32", 3)
    finally:
        q.close()
        eng.close()


# ---- (i) a table with a hot-row set in a queue --------------------------------------------------------------------------------------
def test_hot_row_table_in_a_queue_takes_the_plain_lane_group_kernel(pel, oracle):
    """An fp32 dim-16 table with set_hot_rows, queued with a small pooled flush (32 Zipf-distributed indices per bag, most of
    them hot): the queue launches the plain lane-group kernel (kind 1, never the hot-row kernel, kind 4); the oracle's bits."""
    lay = qc.pooled_layout(4)
    eng, refs = engine_with(pel, "fp32", 16)
    eng.set_hot_rows(0, lay.hot)
    q = queue_of(pel, eng, "i64", "device")
    try:
        run_flush(pel, eng, q, lay, references(oracle, "fp32", 16, refs, lay), 16, "device", "i64", 1)
    finally:
        q.close()
        eng.close()
