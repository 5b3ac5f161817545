"""GPU: the pooled kernels (bag_pool_*, bag_bf16pool_*, bag_f8pool_*, bag_hpool_*, bag_mx4pool_group_kernel) where random normal
data and one-index bags do not reach: the wave-batch kernel's mixed-length steps (general rounds over pool_walk, the one-hot
step with its speculation rejected), several descriptors under it in one launch, special values (signed zeros, ties, denormals,
infinities, NaN) through every pooled path, and a replayed plan over rewritten weights.  Inputs come from tests/pool_cases.py,
whose conditions tests/test_pooling_reference.py proves on the CPU.

The reference everywhere is torch's CPU F.embedding_bag over the table widened to fp32 (half-width output: rounded once, by
torch, to the table's dtype).  NaN positions must be equal and every other element equal as raw bits.  Every test asserts the
path it took from Plan.describe() and from the kernel symbol the launch record resolves to."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WB_B = 131072 + 5                      # the smallest launch choose_kernel hands to the wave-batch kernel
ID_TYPES = [("u32", np.uint32), ("i64", np.int64)]

# family: (table dtype of pool_cases, emb_dtype value, half-width output, pool_walk's unroll, kernel name prefix)
FAMILIES = {"fp32": ("fp32", 0, False, 4, "bag_pool_"), "fp16": ("fp16", 1, False, 8, "bag_pool_"),
            "bf16": ("bf16", 3, False, 8, "bag_bf16pool_"), "e4m3": ("e4m3", 8, False, 8, "bag_f8pool_"),
            "e5m2": ("e5m2", 9, False, 8, "bag_f8pool_"), "fp16-half": ("fp16", 1, True, 8, "bag_hpool_"),
            "bf16-half": ("bf16", 3, True, 8, "bag_hpool_"), "mxfp4": ("mxfp4", 10, False, 8, "bag_mx4pool_")}
ELEM_BYTES = {"fp32": 4, "fp16": 2, "bf16": 2, "e4m3": 1, "e5m2": 1}


@pytest.fixture(scope="module")
def eng(pel):
    e = pel.EmbeddingEngine(device=0, max_tables=64)
    yield e
    e.close()


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def lanes_of(family, dim):
    chunks = dim * ELEM_BYTES[FAMILIES[family][0]] // 16
    lpr = 1
    while lpr < chunks:
        lpr *= 2
    return lpr, chunks


def normal_table(family, rows, dim, seed):
    """(torch CPU table, its exact fp32 widening): normal values, so that every difference is a path difference."""
    t = torch.randn((rows, dim), generator=torch.Generator().manual_seed(seed)).to(pc.TORCH_DTYPE[FAMILIES[family][0]])
    return t, t.float().numpy()


def load(eng, pel, slot, family, table):
    if family == "mxfp4":
        eng.load_table(slot, table, dtype=pel.EMB_MXFP4)
    else:
        eng.load_table(slot, table)


def references(family, wide, idx, off, w, pad, specs):
    """{spec name: expected rows}: fp32, or for a half-output family the 2-byte patterns of the fp32 reference rounded once."""
    tdt = pc.TORCH_DTYPE.get(FAMILIES[family][0])
    out = {}
    for name, spec in specs.items():
        r = pc.reference(wide, idx, off, spec, w, pad)
        out[name] = torch.from_numpy(r).to(tdt).view(torch.int16).numpy() if FAMILIES[family][2] else r
    return out


def check_rows(family, got, want, what):
    if FAMILIES[family][2]:
        assert got.dtype is pc.TORCH_DTYPE[FAMILIES[family][0]], (what, got.dtype)
        ok, text = pc.same_bits16(got.cpu().contiguous().view(torch.int16).numpy(), want, bf16=FAMILIES[family][0] == "bf16")
    else:
        assert got.dtype is torch.float32, (what, got.dtype)
        ok, text = pc.same_bits(got.cpu().numpy(), want)
    assert ok, "%s: %s" % (what, text)


@pytest.fixture
def plans():
    """The plans a test made: destroyed when it ends, passing or not (an engine does not close over live plans)."""
    made = []
    yield made
    for p in made:
        p.destroy()


def pooled_plan(plans, eng, family, slot, specs, d_idx, d_off, d_w, pad):
    """One plan_pooled call over descriptors (d_idx[k], d_off[k], d_w[k]) with spec specs[k] (a pool_cases.SPECS value)."""
    n = len(specs)
    plan = eng.plan_pooled([slot] * n, d_idx, d_off, [s[0] for s in specs], per_sample_weights=[d_w[k] if s[1] else None for k, s in enumerate(specs)],
                           padding_idx=[pad if s[2] else None for s in specs], out_dtype="table" if FAMILIES[family][2] else None)
    plans.append(plan)
    return plan


_symbols = {}


def check_path(pel, family, recs, kind, lanes=None, n_launches=None, vec=None):
    """Every launch of the plan took `kind`, for the family's dtype / output width, and resolves to one kernel of its name."""
    from pim_embedding_lookup_amd import codeobj
    _t, dt, half, _u, prefix = FAMILIES[family]
    assert n_launches is None or len(recs) == n_launches, recs
    if n_launches == 3:                                                        # one launch per mode: sum, mean, max
        assert sorted(r["pool"] for r in recs) == [0, 1, 2], recs
    path = {0: "wavebatch", 1: "group", 3: "anydim"}[kind]
    syms = []
    for r in recs:
        assert (r["kind"], r["dtype"], int(r.get("out", 0))) == (kind, dt, int(half)) and "pool" in r, r
        if lanes is not None:
            assert (r["lanes_per_row"], r["chunks"]) == lanes, r
        if vec is not None:
            assert r["anydim_vec"] == vec, r
        key = tuple(codeobj.symbol_fragments(r))
        if key not in _symbols:                                                # (one walk of the code object per kernel)
            _symbols[key] = codeobj.kernel_of_launch(pel.LIB_PATH, r)[0]
        sym = _symbols[key]
        assert (prefix + path) in sym and "pool_" + path in sym, sym
        syms.append(sym)
    return syms


def run(plan):
    plan.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


# ---- 1. the pooled wave-batch kernel on mixed-length steps ------------------------------------------------------------------
# one row width per lanes-per-row class with code of its own for fp32 (1; 4; 8 with dead lanes; 32; 64 lanes), a narrow and a
# wide one for every other family (fp16 dim 512: 64 lanes)
WB_SHAPES = [("fp32", 4), ("fp32", 16), ("fp32", 24), ("fp32", 128), ("fp32", 256), ("fp16", 8), ("fp16", 512), ("bf16", 16),
             ("bf16", 256), ("e4m3", 16), ("e4m3", 256), ("e5m2", 48), ("e5m2", 128), ("fp16-half", 24), ("fp16-half", 512),
             ("bf16-half", 8), ("bf16-half", 128)]
_wb_cache = {}


def wb_case(family, dim):
    """(table, case, references) of a wave-batch shape, computed once and shared by the tests and id widths that use it (the
    latest shape only: the references of the widest are 1.3 GB)."""
    key = (family, dim)
    if key not in _wb_cache:
        _wb_cache.clear()
        table, wide = normal_table(family, 3001, dim, 7 * dim)
        # the last, partial step is a general one for the fp32 shapes and a shifted one-hot one for the others
        c = pc.wave_batch_case(3001, WB_B, FAMILIES[family][3], seed=dim, tail="general" if family == "fp32" else "shifted")
        pc.check_wave_batch_case(c, WB_B)
        _wb_cache[key] = (table, c, references(family, wide, c.idx, c.off, c.w, c.pad, pc.SPECS))
    return _wb_cache[key]


@pytest.mark.parametrize("ids", ID_TYPES, ids=[n for n, _ in ID_TYPES])
@pytest.mark.parametrize("family,dim", WB_SHAPES, ids=["%s-%d" % s for s in WB_SHAPES])
def test_wave_batch_mixed_length_steps(eng, pel, plans, family, dim, ids):
    _n, it = ids
    table, c, refs = wb_case(family, dim)
    assert c.counts["general"] >= 8 and c.counts["shifted"] >= 8 and c.counts["spec"] >= 8 and len(c.idx) <= 2 * WB_B
    load(eng, pel, 0, family, table)
    i, o, w = to_dev(c.idx.astype(it)), to_dev(c.off.astype(it)), torch.from_numpy(c.w).to(DEV)
    names = list(pc.SPECS)
    plan = pooled_plan(plans, eng, family, 0, [pc.SPECS[n] for n in names], [i] * 5, [o] * 5, [w] * 5, c.pad)
    # three launches (sum with its three ops in one, mean, max), each of >= 131 072 bags: the wave-batch kernel
    syms = check_path(pel, family, plan.describe(), 0, lanes=lanes_of(family, dim), n_launches=3)
    assert len(set(syms)) == 1 and sorted(r["descs"] for r in plan.describe()) == [1, 1, 3]
    for out in plan.outputs:
        out.fill_(7.0)
    run(plan)
    for name, out in zip(names, plan.outputs):
        check_rows(family, out, refs[name], name)
        if pc.SPECS[name][2]:                                                  # bags made empty by padding: +0
            rows = out[torch.from_numpy(c.emptied).to(DEV)]
            assert not bool(rows.view(torch.int16 if FAMILIES[family][2] else torch.int32).any()), name
    plan.destroy()


# ---- 2. the same kernel over several descriptors in one launch ---------------------------------------------------------------
@pytest.mark.parametrize("family,dim,ids", [("fp32", 16, ID_TYPES[0]), ("fp32", 128, ID_TYPES[1]), ("bf16", 16, ID_TYPES[1]),
                                            ("fp16-half", 24, ID_TYPES[0])], ids=["fp32-16-u32", "fp32-128-i64", "bf16-16-i64", "fp16-half-24-u32"])
def test_wave_batch_several_descriptors_one_launch(eng, pel, plans, family, dim, ids):
    """Six descriptors of one dtype, dim and mode -- plain with padding, weighted, weighted with padding: the kernel reads the op
    per descriptor -- form one launch group; their tiles end mid-wavefront (1, 63, 65 bags), so decode_block and the XCD map
    run under the pooled kernel with partial steps in the middle of the grid."""
    _n, it = ids
    table, c, _refs = wb_case(family, dim)
    wide = table.float().numpy()
    load(eng, pel, 1, family, table)
    first_long = int(c.long_bags[c.long_bags >= 64 * 13][0])                   # step 13: long bags in lanes 0 and 63
    assert first_long == 64 * 13 and c.lens[first_long] >= 2 and c.lens[first_long + 63] == 20
    cuts = [(first_long, 1), (first_long, 63), (first_long, 64), (first_long + 63, 65), (0, 70000), (70000, WB_B - 70000)]
    assert sum(n for _b, n in cuts) >= 131072 and [n for _b, n in cuts[:5]] == [1, 63, 64, 65, 70000]
    ops = ["sum+pad", "weighted", "weighted+pad", "weighted+pad", "sum+pad", "weighted"]
    parts = [pc.cut_range(c, b0, n) for b0, n in cuts]
    for (idx, off, w), (_b0, n) in zip(parts, cuts):
        assert len(off) == n and off[0] == 0 and (n > 1 or len(idx) >= 2)
    plan = pooled_plan(plans, eng, family, 1, [pc.SPECS[n] for n in ops], [to_dev(p[0].astype(it)) for p in parts],
                       [to_dev(p[1].astype(it)) for p in parts], [torch.from_numpy(p[2]).to(DEV) for p in parts], c.pad)
    recs = plan.describe()
    check_path(pel, family, recs, 0, lanes=lanes_of(family, dim), n_launches=1)
    assert (recs[0]["descs"], recs[0]["pool"], recs[0]["weighted"], recs[0]["padding"]) == (6, 0, 4, 4)
    before = eng.stats()["n_launches_by_kind"]
    run(plan)
    assert [a - b for a, b in zip(eng.stats()["n_launches_by_kind"], before)] == [1, 0, 0, 0, 0]
    for k, ((idx, off, w), name) in enumerate(zip(parts, ops)):
        want = references(family, wide, idx, off, w, c.pad, {name: pc.SPECS[name]})[name]
        check_rows(family, plan.outputs[k], want, "descriptor %d (%d bags, %s)" % (k, len(off), name))
    plan.destroy()


# ---- 3. special values on every pooled path ----------------------------------------------------------------------------------
ALL_SPECS = dict(pc.SPECS, **pc.SPECS_NO_PAD)
SP_ROWS, SP_BAGS = 400, 600
SP_DIMS = {"fp32": (16, 128, 36, 10, 3), "mxfp4": (32, 128)}                   # every other family: 16, 128, 36, 10
_sp_cache = {}


def sp_case(family, dim):
    """(special table, special bags, references over all seven specs), once per family and dim."""
    key = (family, dim)
    if key not in _sp_cache:
        tab = pc.special_table(SP_ROWS, dim, FAMILIES[family][0], seed=dim)
        sb = pc.special_bags(tab, SP_BAGS, seed=dim + 1)
        pc.check_special_case(tab, sb, {n: pc.reference(tab.wide, sb.idx, sb.off, s, sb.w, sb.pad) for n, s in ALL_SPECS.items()})
        _sp_cache[key] = (tab, sb, references(family, tab.wide, sb.idx, sb.off, sb.w, sb.pad, ALL_SPECS))
    return _sp_cache[key]


def expected_path(family, dim):
    """(kind, anydim_vec or None): choose_kernel's rule for a ragged launch of this row width."""
    if family == "mxfp4":
        return 1, None
    rb = dim * ELEM_BYTES[FAMILIES[family][0]]
    if rb % 16 == 0 and rb <= 1024:
        return 1, None
    return 3, int(rb % 4 == 0 and rb >= 32)


def test_special_dims_cover_every_path():
    for family in FAMILIES:
        paths = {expected_path(family, d) for d in SP_DIMS.get(family, (16, 128, 36, 10))}
        assert paths == ({(1, None)} if family == "mxfp4" else {(1, None), (3, 1), (3, 0)}), (family, paths)


SP_SHAPES = [(f, d) for f in FAMILIES for d in SP_DIMS.get(f, (16, 128, 36, 10))]


@pytest.mark.parametrize("family,dim", SP_SHAPES, ids=["%s-%d" % s for s in SP_SHAPES])
def test_special_values_ragged_bags(eng, pel, plans, family, dim):
    tab, sb, refs = sp_case(family, dim)
    load(eng, pel, 2, family, tab.table)
    kind, vec = expected_path(family, dim)
    names = list(ALL_SPECS)
    w = torch.from_numpy(sb.w).to(DEV)
    if FAMILIES[family][2]:      # half-width output: an fp32 mean that is a 2-byte denormal, a finite fp32 weighted sum that is a 2-byte inf
        exp, inf = (0x7F80, 0x7F80) if FAMILIES[family][0] == "bf16" else (0x7C00, 0x7C00)
        q = refs["mean+pad"][sb.edges["mean of 3 below the format's normals"]].view(np.uint16)
        assert ((q & exp) == 0).all() and ((q & 0x7FFF) != 0).all()
        b = sb.edges["weighted beyond the format's largest"]
        assert np.isfinite(pc.reference(tab.wide, sb.idx, sb.off, pc.SPECS["weighted"], sb.w, sb.pad)[b]).all()
        assert (refs["weighted"][b].view(np.uint16) == inf).all() and (refs["weighted+pad"][b].view(np.uint16) == inf).all()
    for _n, it in ID_TYPES:
        i, o = to_dev(sb.idx.astype(it)), to_dev(sb.off.astype(it))
        plan = pooled_plan(plans, eng, family, 2, [ALL_SPECS[n] for n in names], [i] * 7, [o] * 7, [w] * 7, sb.pad)
        check_path(pel, family, plan.describe(), kind, n_launches=3, vec=vec)
        for out in plan.outputs:
            out.fill_(7.0)
        run(plan)
        for name, out in zip(names, plan.outputs):
            check_rows(family, out, refs[name], "%s ids, %s" % (_n, name))
        plan.destroy()


SP_WB = [("fp32", 16), ("fp16", 64), ("bf16", 32), ("e4m3", 64), ("e5m2", 16), ("fp16-half", 64), ("bf16-half", 16)]


@pytest.mark.parametrize("family,dim", SP_WB, ids=["%s-%d" % s for s in SP_WB])
def test_special_values_wave_batch(eng, pel, plans, family, dim):
    """The special bags tiled into the mixed-length wave-batch layout: every long bag is one of them, the one-index bags walk
    over every row of the special table."""
    tab = pc.special_table(SP_ROWS, dim, FAMILIES[family][0], seed=dim + 50)
    sb = pc.special_bags(tab, SP_BAGS, seed=dim + 51)
    c = pc.wave_batch_case(SP_ROWS, WB_B, FAMILIES[family][3], seed=dim + 52, fill=sb)
    pc.check_wave_batch_case(c, WB_B)
    refs = references(family, tab.wide, c.idx, c.off, c.w, c.pad, pc.SPECS)
    ref32 = {n: pc.reference(tab.wide, c.idx, c.off, s, c.w, c.pad) for n, s in pc.SPECS.items()}
    assert all(np.isnan(r).mean() <= pc.NAN_CAP for r in ref32.values())
    mx = ref32["max+pad"][c.long_bags]
    assert (mx.view(np.uint32) == 0x80000000).any() and np.isnan(mx).any()      # a -0 and a NaN result of max in general steps
    load(eng, pel, 3, family, tab.table)
    it = np.int64 if dim % 32 == 0 else np.uint32
    i, o, w = to_dev(c.idx.astype(it)), to_dev(c.off.astype(it)), torch.from_numpy(c.w).to(DEV)
    names = list(pc.SPECS)
    plan = pooled_plan(plans, eng, family, 3, [pc.SPECS[n] for n in names], [i] * 5, [o] * 5, [w] * 5, c.pad)
    check_path(pel, family, plan.describe(), 0, lanes=lanes_of(family, dim), n_launches=3)
    run(plan)
    for name, out in zip(names, plan.outputs):
        check_rows(family, out, refs[name], name)
    plan.destroy()


# ---- 4. a plan launched again over rewritten weights -------------------------------------------------------------------------
def test_wave_batch_plan_replay_reads_the_new_weights(eng, pel, plans):
    """The per-sample weights are loaded speculatively, next to the index: a launch that kept anything of the first one's would
    show here."""
    family, dim = "fp32", 16
    table, c, refs = wb_case(family, dim)
    wide = table.float().numpy()
    load(eng, pel, 4, family, table)
    i, o, w = to_dev(c.idx.astype(np.uint32)), to_dev(c.off.astype(np.uint32)), torch.from_numpy(c.w).to(DEV)
    names = ["weighted", "weighted+pad"]
    plan = pooled_plan(plans, eng, family, 4, [pc.SPECS[n] for n in names], [i] * 2, [o] * 2, [w] * 2, c.pad)
    check_path(pel, family, plan.describe(), 0, lanes=lanes_of(family, dim), n_launches=1)
    assert plan.describe()[0]["pool"] == 0 and plan.describe()[0]["weighted"] == 2
    run(plan)
    for name, out in zip(names, plan.outputs):
        check_rows(family, out, refs[name], "first launch, " + name)
    w2 = (np.roll(c.w, 3) * np.float32(-1.75)).astype(np.float32)             # the special weights move to other entries
    assert not np.array_equal(w2.view(np.uint32), c.w.view(np.uint32))
    w.copy_(torch.from_numpy(w2))
    for out in plan.outputs:
        out.fill_(7.0)
    run(plan)
    for name, out in zip(names, plan.outputs):
        want = pc.reference(wide, c.idx, c.off, pc.SPECS[name], w2, c.pad)
        assert not np.array_equal(want.view(np.uint32), refs[name].view(np.uint32))
        check_rows(family, out, want, "second launch, " + name)
    plan.destroy()
