"""CPU: the flush layouts of tests/queue_cases.py are what they claim -- the conditions under which emb_queue_flush switches to
the wave-batch / two-batch kernel (or, for the two boundary layouts, just does not), the descriptor mix, the three step classes
of the wave-batch kernel, the 1-MiB cap of host queues -- and the reference the GPU tests compare with is pinned: the oracle's C
sum equals a plain in-order numpy sum on every layout.  No GPU.

Depends on choose_kernel's thresholds (131 072 bags, 524 288 bags and <= 4 lanes per row, n_indices <= 2 n_bags), the wave-batch
step sizes (64 / 128 bags) and kQueueBlock (1 MiB), as restated at the top of queue_cases.py."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import queue_cases as qc  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pim-embedding-lookup_amd", "csrc")
HOST_DIM = {qc.host_cap(16): 16, qc.host_cap(4): 4}
IDS = ["%s-%s" % (c, "device" if cap is None else "host%d" % HOST_DIM[cap]) for c, cap, _k in qc.GPU_LAYOUTS]


def test_constants_are_the_engines():
    """queue_cases.py restates choose_kernel's thresholds, the wave-batch configurations and kQueueBlock: read them off the
    source, so that a retuned constant fails HERE and names the file to follow it.  A deliberate tripwire on the source TEXT:
    a pattern that no longer matches may mean the source was only reformatted or renamed, with nothing retuned -- then this
    test's pattern is what to update, after checking that the value it used to read still equals the one in queue_cases.py."""
    kern = open(os.path.join(CSRC, "pimemb_kernels.hip")).read()
    eng = open(os.path.join(CSRC, "pimemb_engine.cpp")).read()
    moved = ("%s: this test's pattern no longer matches the source text.  The code may only have been reformatted or renamed "
             "(then update the pattern here), or the constant was retuned (then move it in tests/queue_cases.py, and the layouts follow)")
    retuned = "%s is %s in the source but %s in tests/queue_cases.py: move the constant there, and the layouts follow"
    body = kern[kern.index("KernelKind choose_kernel("):]
    body = body[:body.index("\n}\n")]
    assert "total_indices <= 2 * total_bags" in body, moved % "choose_kernel's one-hot-ish rule (n_indices <= 2 n_bags)"
    m = re.search(r"total_bags / 64u < (\d+)u", body)
    assert m, moved % "choose_kernel's wave-batch threshold"
    assert 64 * int(m.group(1)) == qc.WAVE_MIN_BAGS, retuned % ("the wave-batch threshold", 64 * int(m.group(1)), qc.WAVE_MIN_BAGS)
    m = re.search(r"g\.lanes_per_row <= (\d+) && total_bags / 128u >= (\d+)u", body)
    assert m, moved % "choose_kernel's two-batch rule"
    assert int(m.group(1)) == qc.TWO_MAX_LANES, retuned % ("the two-batch kernel's widest row", m.group(1), qc.TWO_MAX_LANES)
    assert 128 * int(m.group(2)) == qc.TWO_MIN_BAGS, retuned % ("the two-batch threshold", 128 * int(m.group(2)), qc.TWO_MIN_BAGS)
    # BagCfg<BLOCK, UNROLL, ntS, ntM, inflight, minW, BATCHES, ...>: bags per step = 64 x BATCHES, per tile = step x BLOCK / 64
    for name, kind in (("WaveCfg", 0), ("Wave2Cfg", 2)):
        m = re.search(r"using %s = BagCfg<(\d+), (\d+), true, false, \d+, \d+, (\d+)," % name, kern)
        assert m, moved % ("the BagCfg alias " + name)
        block, unroll, batches = (int(v) for v in m.groups())
        assert qc.STEP_BAGS[kind] == 64 * batches, retuned % (name + "'s bags per step", 64 * batches, qc.STEP_BAGS[kind])
        tile = 64 * batches * (block // 64)
        assert qc.TILE_BAGS[kind] == tile, retuned % (name + "'s bags per tile", tile, qc.TILE_BAGS[kind])
        assert unroll in qc.UNROLLS, retuned % (name + "'s unroll", unroll, qc.UNROLLS)
    m = re.search(r"constexpr size_t kQueueBlock = 1u << (\d+);", eng)
    assert m, moved % "kQueueBlock"
    assert 1 << int(m.group(1)) == qc.QUEUE_BLOCK, retuned % ("kQueueBlock", 1 << int(m.group(1)), qc.QUEUE_BLOCK)
    m = re.search(r"constexpr int kQueueGens = (\d+);", eng)
    assert m, moved % "kQueueGens"
    assert int(m.group(1)) < 5, "test_gpu_queue_kernels.py runs five flushes to outlast the queue's generations: it needs more now"


@pytest.mark.parametrize("cls,cap,kinds", qc.GPU_LAYOUTS, ids=IDS)
def test_layout_is_what_it_claims(cls, cap, kinds):
    lay = qc.layout(cls, cap)
    qc.check_layout(lay, HOST_DIM.get(cap))
    for kind in kinds or ():
        counts = qc.step_counts(lay, qc.STEP_BAGS[kind])
        assert all(counts[k] >= 8 for k in ("kept", "dropped", "general")), (kind, counts)
    if cap is not None:                                   # a host layout at the dim it was capped for, and one bag more is refused
        assert max(d.n_bags for d in lay.descs) == cap and (cap + 1) * HOST_DIM[cap] * 4 > qc.QUEUE_BLOCK


def test_expected_kind_by_row_width():
    """The kinds the GPU tests expect for their row widths, from the totals of the layouts they flush."""
    wave, two = qc.layout("wave"), qc.layout("two")
    for row_bytes, lpr in ((16, 1), (64, 4), (96, 8), (512, 32), (1024, 64), (128, 8), (32, 2)):
        assert qc.lanes_per_row(row_bytes) == lpr
        assert qc.expected_kind(wave.B, wave.N, lpr) == 0
        assert qc.expected_kind(two.B, two.N, lpr) == (2 if lpr <= 4 else 0)
    for row_bytes in (12, 40, 10, 36):                    # fp32 dim 3 and 10, fp16 dim 5, e4m3 dim 36: the any-dim kernels
        assert qc.lanes_per_row(row_bytes) == 0 and qc.expected_kind(wave.B, wave.N, 0) == 3
    small = qc.ragged_layout(1)
    assert qc.expected_kind(small.B, small.N, 4) == 1
    pooled = qc.pooled_layout(1)
    assert pooled.N == 32 * pooled.B and np.mean(np.concatenate([d.idx for d in pooled.descs]) < len(pooled.hot)) > 0.5


def test_layouts_are_deterministic():
    a, b = qc.flush_layout("wave", seed=5), qc.flush_layout("wave", seed=5)
    assert all(np.array_equal(x.idx, y.idx) and np.array_equal(x.lens, y.lens) and x.table == y.table
               for x, y in zip(a.descs, b.descs))
    assert qc.layout("wave") is qc.layout("wave", None) and qc.layout("two", qc.host_cap(4)) is qc.layout("two", cap=qc.host_cap(4))
    c = qc.flush_layout("wave", seed=6)
    assert not all(np.array_equal(x.idx, y.idx) for x, y in zip(a.descs, c.descs) if len(x.idx) == len(y.idx) > 0)


@pytest.mark.parametrize("dtype", qc.DTYPES)
def test_tables_widen_exactly(dtype):
    """What load_table gets and what the reference sums over are the same numbers."""
    dim = 64 if dtype == "mxfp4" else 16
    rows, name, ref = qc.make_table(dtype, 583, dim, 3)
    assert ref.shape == (583, dim) and (name is None) == (dtype in ("fp32", "fp16", "fixed32"))
    if dtype == "bf16":
        assert rows.dtype == np.uint16 and np.array_equal(qc.formats.to_bf16_bits(ref), rows)
    elif dtype in ("e4m3", "e5m2"):
        assert rows.dtype == np.uint8 and np.array_equal(qc.formats.to_f8_bits(ref, dtype), rows)
    elif dtype == "mxfp4":
        assert rows.shape == (583, qc.formats.mxfp4_row_stride(dim)) and np.array_equal(qc.formats.to_mxfp4(ref), rows)
    elif dtype == "fixed32":
        assert rows.dtype == np.int32 and rows.min() < -2 ** 30 and rows.max() > 2 ** 30
    assert np.isfinite(ref.astype(np.float64)).all()


@pytest.mark.parametrize("cls,cap,kinds", qc.GPU_LAYOUTS, ids=IDS)
def test_reference_is_pinned(cls, cap, kinds):
    """oracle.c_bag_sum equals the in-order fp32 sum in numpy on every descriptor of every layout (fp32 and fp16 tables), and
    c_lookup_fixed32 equals the oracle's own numpy restatement."""
    lay = qc.layout(cls, cap)
    # skipped only where the C oracle CANNOT be built (it is not there, and make or the C compiler is missing); an import, build
    # or load error of the oracle is a failure, as for conftest's `oracle` fixture
    from oracle import oracle
    if not os.path.exists(os.path.join(os.path.dirname(CSRC), os.pardir, "oracle", "libemb_oracle.so")):
        missing = [tool for tool in ("make", os.environ.get("CC") or "cc") if shutil.which(tool) is None]
        if missing:
            pytest.skip("the C oracle is not built and cannot be: no %s here" % " / ".join(missing))
    oracle.build()
    oracle.lib()
    f32, f16, fix = (qc.make_tables(dt, 16) for dt in ("fp32", "fp16", "fixed32"))
    for d in lay.descs:
        want = qc.np_bag_sum(f32[d.table][2], d)
        got = qc.reference(oracle, "fp32", f32[d.table][2], d)
        assert got.shape == (d.n_bags, 16) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        if d.n_bags <= 4099:
            got = qc.reference(oracle, "fp16", f16[d.table][2], d)
            assert np.array_equal(got.view(np.uint32), qc.np_bag_sum(f16[d.table][2], d).view(np.uint32))
            if d.n_bags:
                got = qc.reference(oracle, "fixed32", fix[d.table][2], d)
                want = oracle.np_lookup_fixed32(fix[d.table][2], d.idx.astype(np.uint32), d.ref_off.astype(np.uint32))
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
