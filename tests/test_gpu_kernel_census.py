"""GPU: the kernel census -- every lookup kernel instantiation the library ships is launched once, through the engine's own
dispatch, and compared bit for bit with a high-precision reference.  The cases, their shapes and inputs are tests/kernel_census.py's
(proved on the CPU by test_kernel_census_cpu.py: one case per bag_*_kernel symbol, none left out).

Per case and row width: a PLAN is built (plan / plan_pooled / emb_plan_create_strided / emb_plan_create_ranged_typed); every launch
record of describe() must be exactly the case's, and codeobj.kernel_of_launch() must resolve it to the case's symbol -- that is what
makes a passing run a proof that the kernel ran.  The plan is launched once into outputs pre-filled with a NaN pattern, with a guard
row before and after (strided: every column the call does not own is a guard too).  References: oracle.c_bag_sum /
c_lookup_fixed32 for sums, pool_cases.reference (torch's CPU embedding_bag over the fp32-widened table) for pooled specs, rounded
once by torch for half-width output, a row gather (the oracle's sum over one-index bags: +0 + x, as every lookup computes it) with
zeros for the open end's ids for ranged launches.  Raw bits equal, NaN positions equal, guards unchanged, served counters equal.
Small cases run once more plan-less: the same bits, and the engine's n_launches_by_kind counter.

One test id is a (family, dtype, id width): at most seven lane counts.  A (family, dtype)'s two id widths run next to each other and
share tables, index sets and references."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census as kc  # noqa: E402
import pool_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x7FC0DEAD                  # fp32 outputs are prefilled with this NaN, which no lookup here produces ...
SENT16 = 0x7FAD                    # ... 2-byte outputs with this one (a NaN as fp16 and as bf16)
COL = 4                            # strided cases: the table's columns start here in a [bags, 3 dim + 8] buffer
GROUPS = kc.groups()
TORCH_HALF = {kc.F16: torch.float16, kc.BF16: torch.bfloat16}
SLOT, HOT_SLOT, SHARD_SLOT = 0, 1, 2
SERVED_WORDS = 64 * 256 // 4       # EMB_SERVED_LANES x EMB_SERVED_STRIDE bytes per counter


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=8)
    e.plan_cache_size = 0          # a plan-less call here is a transient launch, every time
    yield e
    e.close()


@pytest.fixture
def plans():
    """The plans a test made: destroyed when it ends, passing or not (an engine does not close over live plans)."""
    made = []
    yield made
    for p in made:
        p.destroy()


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


# ---- host side: tables, descriptors and references, shared by a (family, dtype)'s cases and id widths --------------------------------
_host = {"key": None, "dims": {}}


def sum_reference(oracle, dtype, ref_table, idx, off):
    if dtype == kc.FIXED32:
        return oracle.c_lookup_fixed32(ref_table, idx.astype(np.uint32), off.astype(np.uint32))
    return oracle.c_bag_sum(ref_table, idx, off)


def out_bits(case, rows32):
    """The reference as the raw bits the output must hold: fp32, or rounded ONCE by torch to the table's 2-byte dtype."""
    if case.record.get("out"):
        return torch.from_numpy(np.ascontiguousarray(rows32, dtype=np.float32)).to(TORCH_HALF[case.dtype]).view(torch.int16).numpy()
    return np.ascontiguousarray(rows32, dtype=np.float32).view(np.int32)


def reference(oracle, case, t, idx, off, w, pad, spec):
    if spec is None:
        return sum_reference(oracle, case.dtype, t.ref, idx, off)
    return pc.reference(t.wide, idx, off, kc.ALL_SPECS[spec], w, pad)


def host_shape(oracle, case, dim):
    """Table and descriptors of a case at one row width.  A descriptor: idx, off (int64), w, pad, spec (None: plain sum), bits
    (the expected output).  Built once per (family, dtype, dim): the big cases keep ONE reference over their whole layout, of which
    both descriptors and both tails are slices."""
    key = (case.family, case.dtype)
    if _host["key"] != key:
        _host["key"], _host["dims"] = key, {}
    h = _host["dims"].get(dim)
    if h is None:
        rows, name, ref, wide = kc.make_table(case.dtype, dim)
        h = _host["dims"][dim] = SimpleNamespace(rows=rows, name=name, ref=ref, wide=wide, small=None, full=None)
    specs = case.specs or (None,)
    if case.size == "small":
        if h.small is None:
            _lpr, _chunks, scalar, _vec = kc.geometry(case.dtype, dim)
            counts = kc.small_bag_counts(case.kind, case.lpr, scalar)[:case.n_descs]
            h.small = []
            for spec in specs:
                for k, n in enumerate(counts):
                    d = kc.small_inputs(n, k)
                    bits = out_bits(case, reference(oracle, case, h, d.idx, d.off, d.w, d.pad, spec))
                    h.small.append(SimpleNamespace(idx=d.idx, off=d.off, w=d.w, pad=d.pad, spec=spec, bits=bits, n_bags=n))
        return h, h.small
    B, ranges = kc.big_descs(case)
    big = kc.big_case(B, kc.big_unroll(case))
    if h.full is None:
        h.full = out_bits(case, reference(oracle, case, h, big.idx, big.off, big.w, big.pad, specs[0]))
    descs = []
    for b0, n in ranges:
        idx, off, w = pc.cut_range(big, b0, n)
        descs.append(SimpleNamespace(idx=idx, off=off, w=w, pad=big.pad, spec=specs[0], bits=h.full[b0:b0 + n], n_bags=n))
    return h, descs


# ---- device side ------------------------------------------------------------------------------------------------------------------
def guarded(n_bags, width, half=None):
    """[1 + n_bags + 1, width] of the NaN pattern: the rows a descriptor owns with a guard row before and after."""
    if half is not None:
        return torch.full((n_bags + 2, width), SENT16, dtype=torch.int16, device=DEV).view(TORCH_HALF[half])
    return torch.full((n_bags + 2, width), SENT, dtype=torch.int32, device=DEV).view(torch.float32)


def refill(buf):
    buf.view(torch.int16 if buf.element_size() == 2 else torch.int32).fill_(SENT16 if buf.element_size() == 2 else SENT)


def check_buffer(buf, bits, col, what, untouched=None):
    """Rows 1 .. n of `buf`, columns col .. col + dim, hold `bits`; every other element is still the NaN pattern.  untouched: a
    bool per bag -- those bags' rows must still be the pattern as well (ranged launches)."""
    torch.cuda.synchronize()
    half = buf.element_size() == 2
    ints = buf.view(torch.int16 if half else torch.int32)
    want = torch.full_like(ints, SENT16 if half else SENT)
    body = torch.from_numpy(np.ascontiguousarray(bits)).to(DEV)
    if untouched is not None:
        body = torch.where(torch.from_numpy(untouched).to(DEV)[:, None], want[1:-1, col:col + body.shape[1]], body)
    want[1:-1, col:col + body.shape[1]] = body
    if torch.equal(ints, want):
        return
    got, exp = ints.cpu().numpy(), want.cpu().numpy()           # slow path: which elements, NaN payloads aside
    inside = np.zeros(got.shape, bool)
    inside[1:-1, col:col + body.shape[1]] = True
    if untouched is not None:
        inside[1:-1][untouched] = False
    guards = np.argwhere(~inside & (got != exp))
    assert len(guards) == 0, "%s: %d guard elements were written; first (row, column, bits): %s" % (
        what, len(guards), [(int(r), int(c), hex(int(got[r, c]) & 0xFFFFFFFF)) for r, c in guards[:6]])
    g, w = np.where(inside, got, 0), np.where(inside, exp, 0)
    ok, text = pc.same_bits16(g, w, bf16=buf.dtype is torch.bfloat16) if half else pc.same_bits(g.view(np.float32), w.view(np.float32))
    assert ok, "%s: %s" % (what, text)


_symbols = {}


def check_records(pel, plan, case, dim, n_launches, n_descs):
    """describe() returns exactly the case's record for every launch, and the record resolves to the case's kernel symbol."""
    from pim_embedding_lookup_amd import codeobj
    recs = plan.describe()
    want = kc.record_at(case, dim)
    assert len(recs) == n_launches and sum(r["descs"] for r in recs) == n_descs, (case.id, dim, recs)
    if case.id not in _symbols:
        _symbols[case.id] = codeobj.kernel_of_launch(pel.LIB_PATH, kc.record_at(case, case.dims[0]))[0]
    for r in recs:
        assert kc.record_of(r) == want, "%s dim %d: the dispatch chose %s, the case is %s" % (case.id, dim, r, want)
        sym = codeobj.kernel_of_launch(pel.LIB_PATH, r)[0]
        assert sym == _symbols[case.id], (case.id, dim, sym, _symbols[case.id])
    if case.specs and n_launches > 1:                                      # one launch per mode: sum, mean, max
        assert sorted(r["pool"] for r in recs) == [0, 1, 2], recs


def kind_delta(eng, before):
    return [a - b for a, b in zip(eng.stats()["n_launches_by_kind"], before)]


def load(eng, pel, slot, h, rows=None):
    eng.load_table(slot, h.rows if rows is None else rows, dtype=None if h.name is None else getattr(pel, h.name))


def run_dense_or_strided(eng, pel, oracle, plans, case, dim):
    h, descs = host_shape(oracle, case, dim)
    n = len(descs)
    half = case.dtype if case.record.get("out") else None
    strided = bool(case.record.get("strided"))
    slot = HOT_SLOT if case.kind == 4 else SLOT
    load(eng, pel, slot, h)
    if case.kind == 4:
        eng.set_hot_rows(slot, kc.hot_hint())
    it = kc.ID_NP[case.itype]
    d_idx, d_off = [to_dev(d.idx.astype(it)) for d in descs], [to_dev(d.off.astype(it)) for d in descs]
    weighted = [d.spec is not None and kc.ALL_SPECS[d.spec][1] for d in descs]
    d_w = [torch.from_numpy(d.w).to(DEV) if wt else None for d, wt in zip(descs, weighted)]
    modes = [kc.ALL_SPECS[d.spec][0] for d in descs] if case.specs else None
    pads = [d.pad if kc.ALL_SPECS[d.spec][2] else None for d in descs] if case.specs else None
    n_launches = len(set(modes)) if case.specs else 1
    width = 3 * dim + 8 if strided else dim
    col = COL if strided else 0
    bufs = [guarded(d.n_bags, width, half) for d in descs]
    outs = [b[1:-1] for b in bufs]
    stream = torch.cuda.current_stream().cuda_stream
    L, lib = eng._L, pel.lib
    if strided:                                                            # what plan_concat makes, with a buffer per descriptor
        arr = (lib.EmbLookupDesc * n)()
        for k, d in enumerate(descs):
            arr[k] = lib.EmbLookupDesc(slot, 0, d_idx[k].data_ptr(), d_off[k].data_ptr(), len(d.idx), d.n_bags,
                                       bufs[k].data_ptr() + 4 * (width + col))
        strides = (C.c_uint64 * n)(*([width] * n))
        pools = eng._pools(n, arr, modes, d_w, pads, lib.EMB_MEM_DEVICE)[0] if case.specs else None
        p = C.c_void_p()
        lib.check(L.emb_plan_create_strided(eng._h, arr, pools, strides, n, case.itype, C.byref(p)))
        plan = pel.Plan(eng, p.value, None, None)
    elif case.specs:
        plan = eng.plan_pooled([slot] * n, d_idx, d_off, modes, per_sample_weights=d_w, padding_idx=pads, outs=outs,
                               out_dtype="table" if half is not None else None)
    else:
        plan = eng.plan([slot] * n, d_idx, d_off, outs=outs, out_dtype="table" if half is not None else None)
    plans.append(plan)
    check_records(pel, plan, case, dim, n_launches, n)
    plan.launch(stream)
    for k, d in enumerate(descs):
        check_buffer(bufs[k], d.bits, col, "%s dim %d, plan, descriptor %d (%s)" % (case.id, dim, k, d.spec or "sum"))
    if case.size != "small":
        return
    for b in bufs:
        refill(b)
    before = eng.stats()["n_launches_by_kind"]
    if strided:
        bad = C.c_uint64()
        lib.check(L.emb_lookup_strided(eng._h, arr, pools, strides, n, case.itype, stream, 0, C.byref(bad)))
    elif case.specs or half is not None:
        eng.lookup_pooled([slot] * n, d_idx, d_off, modes or "sum", per_sample_weights=d_w if case.specs else None,
                          padding_idx=pads, outs=outs, out_dtype="table" if half is not None else None)
    else:
        eng.lookup_batched([slot] * n, d_idx, d_off, outs=outs)
    for k, d in enumerate(descs):
        check_buffer(bufs[k], d.bits, col, "%s dim %d, plan-less, descriptor %d (%s)" % (case.id, dim, k, d.spec or "sum"))
    delta = kind_delta(eng, before)
    assert delta[case.kind] == n_launches and sum(delta) == n_launches, (case.id, dim, delta)


def run_ranged(eng, pel, oracle, plans, case, dim):
    """Three row shards of one table scan ONE index array; the last carries EMB_RANGE_OPEN_END and zeroes the bags nobody holds;
    without the flag those bags stay untouched."""
    key = (case.family, case.dtype)
    if _host["key"] != key:
        _host["key"], _host["dims"] = key, {}
    h = _host["dims"].get(dim)
    small = case.size == "ranged"
    B = kc.RANGED_B if small else kc.TWO_B
    r = kc.ranged_inputs(B)
    if h is None:
        rows, name, ref, wide = kc.make_table(case.dtype, dim)
        rel = np.clip(r.idx, 0, kc.ROWS - 1)
        # the row gather as what it is to every lookup kernel and to torch: the sum of a one-index bag, +0 + x -- a -0 element of the
        # table (fp8 tables hold many) comes out as +0
        gathered = sum_reference(oracle, case.dtype, ref, rel, np.arange(B, dtype=np.int64))
        bits = np.where(r.held[:, None], np.ascontiguousarray(gathered, dtype=np.float32).view(np.int32), np.int32(0))
        h = _host["dims"][dim] = SimpleNamespace(rows=rows, name=name, bits=np.ascontiguousarray(bits))
    N, per = kc.N_SHARDS, kc.PER_SHARD
    for s in range(N):
        load(eng, pel, SHARD_SLOT + s, h, h.rows[s * per:min((s + 1) * per, kc.ROWS)])
    d_idx = to_dev(r.idx if case.itype == 1 else r.idx32)
    lib, L = pel.lib, eng._L
    ctr = torch.zeros((N, SERVED_WORDS), dtype=torch.int32, device=DEV)
    served = (C.c_void_p * N)(*[ctr[s].data_ptr() for s in range(N)])
    stream = torch.cuda.current_stream().cuda_stream
    mine = [int(m.sum()) for m in r.mine]

    def call(buf, open_end, counted, prepared):
        descs = (lib.EmbLookupDesc * N)(*[lib.EmbLookupDesc(SHARD_SLOT + s, 1, d_idx.data_ptr(), None, B, B, buf[1:].data_ptr()) for s in range(N)])
        lo = (C.c_uint64 * N)(*[(s * per) | (lib.EMB_RANGE_OPEN_END if open_end and s == N - 1 else 0) for s in range(N)])
        if not prepared:
            lib.check(L.emb_lookup_ranged_typed(eng._h, descs, lo, served if counted else None, N, case.itype, stream))
            return None
        p = C.c_void_p()
        lib.check(L.emb_plan_create_ranged_typed(eng._h, descs, lo, served if counted else None, N, case.itype, C.byref(p)))
        plan = pel.Plan(eng, p.value, None, None)
        plans.append(plan)
        check_records(pel, plan, case, dim, 1, N)
        plan.launch(stream)
        return plan

    buf = guarded(B, dim)
    call(buf, True, True, True)
    check_buffer(buf, h.bits, 0, "%s dim %d, plan, open end" % (case.id, dim))
    assert ctr.cpu().numpy().astype(np.int64).sum(axis=1).tolist() == mine and sum(mine) == B - len(kc.NOBODY), (case.id, dim)
    # without the open end: the bags nobody holds stay what they were
    refill(buf)
    before = eng.stats()["n_launches_by_kind"]
    call(buf, False, False, not small)
    check_buffer(buf, h.bits, 0, "%s dim %d, no open end" % (case.id, dim), untouched=~r.held)
    if small:
        delta = kind_delta(eng, before)
        assert delta[case.kind] == 1 and sum(delta) == 1, (case.id, dim, delta)
        refill(buf)
        ctr.zero_()
        call(buf, True, True, False)
        check_buffer(buf, h.bits, 0, "%s dim %d, plan-less, open end" % (case.id, dim))
        assert ctr.cpu().numpy().astype(np.int64).sum(axis=1).tolist() == mine, (case.id, dim)


@pytest.mark.parametrize("cases", [cs for _g, cs in GROUPS], ids=[g for g, _cs in GROUPS])
def test_kernel_census(eng, pel, oracle, plans, cases):
    """Every case of one (family, dtype, id width), at every row width it has.  A case that fails does not hide the next one: the
    failures are collected and reported together, each under its case id."""
    failed = []
    for case in cases:
        for dim in case.dims:
            try:
                if case.record["ranged"]:
                    run_ranged(eng, pel, oracle, plans, case, dim)
                else:
                    run_dense_or_strided(eng, pel, oracle, plans, case, dim)
            except AssertionError as ex:
                failed.append("%s dim %d: %s" % (case.id, dim, str(ex)[:800]))
            finally:
                while plans:
                    plans.pop().destroy()
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(cases), "\n".join(failed))


def test_every_case_is_collected():
    """The parametrisation above runs every case of the table, each once."""
    ran = [c.id for _g, cs in GROUPS for c in cs]
    assert sorted(ran) == sorted(c.id for c in kc.CASES) and len(ran) == len(set(ran)) == len(kc.CASES)
