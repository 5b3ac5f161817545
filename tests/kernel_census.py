"""The kernel census: ONE CASE PER LOOKUP KERNEL the library ships (test_kernel_census_cpu.py on the CPU, test_gpu_kernel_census.py on
the GPU).  A plain module like pool_cases.py / queue_cases.py: no GPU code and no test functions; every builder returns its inputs
TOGETHER WITH the facts the tests assert about them.

A CASE is the launch record Plan.describe() must return (kind, dtype, itype, lanes_per_row, chunks, anydim_vec, ranged, and pool /
out / strided where they apply -- what codeobj.symbol_fragments() resolves to exactly one bag_*_kernel symbol) together with the
SHAPE that makes the engine's own dispatch (resolve() / choose_kernel() in csrc/, never PIMEMB_FORCE_KERNEL) pick that kernel:

  size "small"   a few hundred ragged bags in two descriptors of unequal, odd bag counts (more than one tile each): the lane-group
                 kernels (kind 1), the hot-row kernel (kind 4: the same inputs over a table with a hot-row hint) and, with one
                 descriptor, the any-dim kernels (kind 3)
  size "wave"    pool_cases.wave_batch_case at 131 072 + 5 bags plus a second descriptor of 4101 bags: the wave-batch kernels (kind 0)
  size "two"     the same at 524 288 + 5 bags and <= 4 lanes per row: the two-batch kernels (kind 2)
  ranged         one index per bag, three row shards of one table over ONE index array, the last shard with EMB_RANGE_OPEN_END:
                 4099 bags (a ranged launch takes the wave-batch kernel at any size) or 524 288 + 5 (kind 2)

CASES is GENERATED from the rules of the dispatch (cases()), never typed out.  A new template argument of the kernels gets its
cases by one more loop (or one more value in a loop) there; test_kernel_census_cpu.py fails until CASES and the library's
bag_*_kernel symbols are the same set again.

THE CONSTANTS BELOW RESTATE THE ENGINE'S (test_kernel_census_cpu.py reads them off the source text)."""
from __future__ import annotations

import re
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import pool_cases as pc
import queue_cases as qc

WAVE_MIN_BAGS, TWO_MIN_BAGS, TWO_MAX_LANES = qc.WAVE_MIN_BAGS, qc.TWO_MIN_BAGS, qc.TWO_MAX_LANES
GROUP_BLOCK = 256                  # GroupCfg / Mx4GroupCfg::kBlock: bags per lane-group tile = 64 / lanes x kBlock / 64
HOT_BLOCK = 1024                   # HotCfg::kBlock
ANYDIM_BLOCK = 256                 # the any-dim kernels' workgroup: bags per tile = 256 / scalar_lanes
HOT_LDS_BUDGET = 62 << 10          # kHotLdsBudget
HOT_PROBES = 2                     # kHotProbes (pimemb_hot_rows.h: build_hot_set)
MAX_ROW_BYTES = 1024               # geometry_for(): wider rows, and rows that are no 16-byte multiple, run the any-dim kernels

F32, F16, FIXED32, BF16, E4M3, E5M2, MXFP4 = 0, 1, 2, 3, 8, 9, 10
DT_NAME = {F32: "fp32", F16: "fp16", FIXED32: "fixed32", BF16: "bf16", E4M3: "e4m3", E5M2: "e5m2", MXFP4: "mxfp4"}
ELEM_BYTES = {F32: 4, F16: 2, FIXED32: 4, BF16: 2, E4M3: 1, E5M2: 1}
SUM_DTYPES = (F32, F16, FIXED32, BF16, E4M3, E5M2)
POOL_DTYPES = (F32, F16, BF16, E4M3, E5M2)          # (fixed-point tables pool by plain sum only; no strided twin either)
HALF_DTYPES = (F16, BF16)
ID_NAME = {0: "u32", 1: "i64"}
ID_NP = {0: np.uint32, 1: np.int64}
LPRS = (1, 2, 4, 8, 16, 32, 64)

ROWS = 3001                        # rows of every census table
WAVE_B = WAVE_MIN_BAGS + 5
TWO_B = TWO_MIN_BAGS + 5
SECOND_B = 4101                    # bags of the second descriptor of a big launch ...
SECOND_AT = 64 * 12 - 3            # ... cut out of the big case from here: the irregular steps begin in its first 64-bag steps
RANGED_B = 4099
N_SHARDS = 3
ALL_SPECS = dict(pc.SPECS, **pc.SPECS_NO_PAD)
SPEC_NAMES = tuple(ALL_SPECS)

# any-dim row widths (elements) per dtype: (non-vec, vec).  Non-vec: row bytes no multiple of 4, or < 32.  Vec: a multiple of 4 and
# >= 32 that is no 16-byte multiple -- or a row beyond 1 KiB (fp16, fixed32, e5m2 here).
ANYDIM_DIMS = {F32: (5, 10), F16: (5, 514), FIXED32: (3, 260), BF16: (17, 18), E4M3: (7, 36), E5M2: (33, 1028)}


# ---- the case table -----------------------------------------------------------------------------------------------------------------
def dim_of(dtype, chunks):
    return 32 * chunks if dtype == MXFP4 else chunks * 16 // ELEM_BYTES[dtype]


def row_bytes_of(dtype, dim):
    return dim * ELEM_BYTES[dtype]


def geometry(dtype, dim):
    """geometry_for() restated: (lanes_per_row, chunks, scalar_lanes, anydim_vec)."""
    if dtype == MXFP4:
        assert dim % 32 == 0 and 0 < dim <= 2048
        chunks = dim // 32
    else:
        rb = row_bytes_of(dtype, dim)
        if rb % 16 or rb > MAX_ROW_BYTES:
            vec = rb % 4 == 0 and rb >= 32
            units = (rb + 15) // 16 if vec else dim
            lanes = 1
            while lanes < units and lanes < 256:
                lanes *= 2
            return 0, dim, lanes, int(vec)
        chunks = rb // 16
    lpr = 1
    while lpr < chunks:
        lpr *= 2
    return lpr, chunks, 0, 0


def bags_per_tile(kind, lpr, scalar_lanes=0):
    """bags_per_tile() restated."""
    if kind == 3:
        return ANYDIM_BLOCK // scalar_lanes
    if kind == 4:
        return (64 // lpr) * (HOT_BLOCK // 64)
    if kind in (0, 2):
        return qc.TILE_BAGS[kind]
    return (64 // lpr) * (GROUP_BLOCK // 64)


def expected_kind(case, dim, total_bags, total_indices, hot_lds=0):
    """resolve()'s choice for one launch group restated: choose_kernel(), then the overrides for MXFP4, ranged, pooled and hot-row
    launches."""
    r = case.record
    lpr, _chunks, scalar, _vec = geometry(r["dtype"], dim)
    kind = qc.expected_kind(total_bags, total_indices, lpr if not scalar else 0)
    if r["dtype"] == MXFP4:
        kind = 1
    if r.get("ranged") and kind == 1:
        kind = 0
    if r.get("pool") and kind == 2:
        kind = 0
    if kind == 1 and not r.get("pool") and not r.get("out") and not r.get("strided") and hot_lds:
        kind = 4
    return kind


def _widths(lpr, size):
    """Chunks a case runs at: the full width and the one that leaves exactly one dead lane (lanes >= 4) for small launches, the
    dead-lane width alone for big ones (the full widths are the popular dims the other GPU tests run); 1 and 2 lanes: their only one."""
    if lpr < 4:
        return (lpr,)
    return (lpr, lpr - 1) if size == "small" else (lpr - 1,)


def _case(family, kind, dtype, itype, size, lpr=0, vec=None, ranged=0, pool=False, out=0, strided=0, specs=(), n_descs=2):
    if lpr:
        dims = tuple(dim_of(dtype, c) for c in _widths(lpr, size))
        tag = "lpr%d" % lpr
    else:
        dims = (ANYDIM_DIMS[dtype][vec],)
        tag = "vec" if vec else "novec"
    rec = dict(kind=kind, dtype=dtype, itype=itype, lanes_per_row=lpr, anydim_vec=int(bool(vec)), ranged=ranged)
    if pool:
        rec["pool"] = 1
    if out:
        rec["out"] = 1
    if strided:
        rec["strided"] = 1
    group = "%s-%s-%s" % (family, DT_NAME[dtype], ID_NAME[itype])
    # the last, partial step of the big descriptor: "general" under one id width, "shifted" under the other
    tail = ("general", "shifted")[(itype + dtype) % 2]
    return SimpleNamespace(id="%s-%s" % (group, tag), group=group, family=family, record=rec, size=size, dims=dims, specs=tuple(specs),
                           tail=tail, n_descs=n_descs, lpr=lpr, dtype=dtype, itype=itype, kind=kind)


def record_at(case, dim):
    """The case's launch record at one of its row widths, chunks included (any-dim: chunks is the dim)."""
    lpr, chunks, _scalar, vec = geometry(case.dtype, dim)
    assert lpr == case.lpr and vec == case.record["anydim_vec"], (case.id, dim)
    return dict(case.record, chunks=chunks)


def record_of(rec):
    """A Plan.describe() record reduced to the census fields: what names the kernel, not the launch's size or its pooling mode."""
    out = {k: rec[k] for k in ("kind", "dtype", "itype", "lanes_per_row", "chunks", "anydim_vec", "ranged")}
    if "pool" in rec:
        out["pool"] = 1
    for k in ("out", "strided"):
        if rec.get(k):
            out[k] = 1
    return out


def _big_spec(dtype, lpr, dtypes):
    """The one spec a big pooled case runs: rotated over lane counts and dtypes, the same for both id widths (they share a reference),
    so that every spec occurs at some lane count of every (family, dtype)."""
    return SPEC_NAMES[(LPRS.index(lpr) + dtypes.index(dtype)) % len(SPEC_NAMES)]


def cases():
    """Every legal launch record, from the rules of resolve() / launch_bag_sum() / launch_bag_pool() / launch_bag_strided()."""
    out = []
    for itype in (0, 1):
        # -- dense fp32 output, plain sum
        for dt in SUM_DTYPES:
            for lpr in LPRS:
                out.append(_case("sum-group", 1, dt, itype, "small", lpr))
                out.append(_case("sum-hot", 4, dt, itype, "small", lpr))
                out.append(_case("sum-wave", 0, dt, itype, "wave", lpr))
                out.append(_case("ranged-wave", 0, dt, itype, "ranged", lpr, ranged=1, n_descs=N_SHARDS))
                if lpr <= TWO_MAX_LANES:
                    out.append(_case("sum-two", 2, dt, itype, "two", lpr))
                    out.append(_case("ranged-two", 2, dt, itype, "ranged-two", lpr, ranged=1, n_descs=N_SHARDS))
            for vec in (0, 1):
                out.append(_case("sum-anydim", 3, dt, itype, "small", vec=vec, n_descs=1))
        # -- half-width output of fp16 / bf16 tables: the sum kernels' twins (never ranged, never hot) and the bag_hpool_* set
        for dt in HALF_DTYPES:
            for lpr in LPRS:
                out.append(_case("halfsum-group", 1, dt, itype, "small", lpr, out=1))
                out.append(_case("halfsum-wave", 0, dt, itype, "wave", lpr, out=1))
                out.append(_case("hpool-group", 1, dt, itype, "small", lpr, pool=True, out=1, specs=SPEC_NAMES))
                out.append(_case("hpool-wave", 0, dt, itype, "wave", lpr, pool=True, out=1, specs=(_big_spec(dt, lpr, HALF_DTYPES),)))
                if lpr <= TWO_MAX_LANES:
                    out.append(_case("halfsum-two", 2, dt, itype, "two", lpr, out=1))
            for vec in (0, 1):
                out.append(_case("halfsum-anydim", 3, dt, itype, "small", vec=vec, out=1, n_descs=1))
                out.append(_case("hpool-anydim", 3, dt, itype, "small", vec=vec, pool=True, out=1, specs=SPEC_NAMES, n_descs=1))
        # -- pooled (mean / max / weights / padding): one wave-batch geometry, no fixed-point tables
        for dt in POOL_DTYPES:
            for lpr in LPRS:
                out.append(_case("pool-group", 1, dt, itype, "small", lpr, pool=True, specs=SPEC_NAMES))
                out.append(_case("pool-wave", 0, dt, itype, "wave", lpr, pool=True, specs=(_big_spec(dt, lpr, POOL_DTYPES),)))
                # -- strided twins: lane-group, wave-batch and two-batch sums, lane-group and wave-batch pooled
                out.append(_case("strided-sum-group", 1, dt, itype, "small", lpr, strided=1))
                out.append(_case("strided-sum-wave", 0, dt, itype, "wave", lpr, strided=1))
                out.append(_case("strided-pool-group", 1, dt, itype, "small", lpr, pool=True, strided=1, specs=SPEC_NAMES))
                out.append(_case("strided-pool-wave", 0, dt, itype, "wave", lpr, pool=True, strided=1, specs=(_big_spec(dt, lpr, POOL_DTYPES),)))
                if lpr <= TWO_MAX_LANES:
                    out.append(_case("strided-sum-two", 2, dt, itype, "two", lpr, strided=1))
            for vec in (0, 1):
                out.append(_case("pool-anydim", 3, dt, itype, "small", vec=vec, pool=True, specs=SPEC_NAMES, n_descs=1))
        # -- MXFP4: the lane-group kernels only
        for lpr in LPRS:
            out.append(_case("mx4-sum", 1, MXFP4, itype, "small", lpr))
            out.append(_case("mx4-pool", 1, MXFP4, itype, "small", lpr, pool=True, specs=SPEC_NAMES))
            out.append(_case("strided-mx4-sum", 1, MXFP4, itype, "small", lpr, strided=1))
            out.append(_case("strided-mx4-pool", 1, MXFP4, itype, "small", lpr, pool=True, strided=1, specs=SPEC_NAMES))
    return out


CASES = cases()
# kernels no public call can reach: {symbol: reason}; subtracted by the CPU test.  Empty is the expected state.
UNREACHABLE: dict = {}


def groups():
    """[(group id, [cases])] in table order, a (family, dtype)'s two id widths next to each other so that they share what they load."""
    by = {}
    for c in CASES:
        by.setdefault((c.family, c.dtype, c.itype), []).append(c)
    order = sorted(by, key=lambda k: ([c.family for c in CASES].index(k[0]), k[1], k[2]))
    return [(by[k][0].group, by[k]) for k in order]


# The library's other kernels: kernel name -> (C entry point that launches it, GPU test file that drives that entry point, the text
# by which that file names the call: the entry point itself, its Python wrapper, or the variant that takes the path).  A new kernel
# with no home fails test_kernel_census_cpu.py::test_helper_kernels_have_a_home.
_SHARD = "tests/test_gpu_shard.py"
HELPER_KERNELS = {
    "validate_kernel<uint32_t>": ("emb_lookup_batched_checked", "tests/test_gpu_parity.py", "emb_lookup_batched_checked"),
    "validate_kernel<int64_t>": ("emb_lookup_batched_checked", "tests/test_gpu_parity.py", "emb_lookup_batched_checked"),
    "scatter_column_kernel": ("emb_load_table_column", "tests/test_gpu_bf16.py", "load_table_column"),
    "gather_rows_kernel": ("emb_set_hot_rows", "tests/test_gpu_parity.py", "emb_set_hot_rows"),
    "store_word_kernel": ("emb_queue_flush", "tests/test_gpu_queue_kernels.py", "emb_queue_flush"),
    "route_bags_count_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "route_bags_scan_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "route_bags_layout_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "route_bags_place_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "route_onehot_count_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "route_onehot_layout_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "route_onehot_place_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "route_onehot_place_fused_kernel": ("emb_route_bags_typed", "tests/test_gpu_sharding.py", "route_bags"),
    "unroute_bags_kernel": ("emb_unroute_bags", "tests/test_gpu_sharding.py", "unroute_bags"),
    "zero_words_kernel": ("emb_shard_submit", _SHARD, "emb_shard_"),
    "publish_words_kernel": ("emb_shard_submit", _SHARD, "emb_shard_"),
    "served_counts_kernel": ("emb_shard_submit", _SHARD, "one-hot-direct"),
    "widen_words_kernel": ("emb_shard_submit", _SHARD, "int64-ragged"),
    "peer_post_kernel": ("emb_shard_submit", _SHARD, "peer_stores"),
    "peer_done_kernel": ("emb_shard_submit", _SHARD, "peer_stores"),
}


def helper_name(symbol):
    """A mangled non-bag kernel symbol as HELPER_KERNELS names it: the function's own name, with its index type where it has one."""
    assert symbol.startswith("_ZN"), symbol
    at = 3
    while True:                                      # the nested name's <length><name> pieces of the Itanium mangling, in order
        m = re.compile(r"\d+").match(symbol, at)
        assert m, "no kernel name in " + symbol
        name = symbol[m.end():m.end() + int(m.group())]
        at = m.end() + len(name)
        if name.endswith("_kernel"):
            rest = symbol[at:]
            return name + ("<uint32_t>" if rest.startswith("IjE") else "<int64_t>" if rest.startswith("IlE") else "")


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def make_table(dtype, dim, seed=11):
    """(rows to load, name of the EMB_* constant load_table needs or None, what the SUM reference reads, the fp32 widening)."""
    rows, name, ref = qc.make_table(DT_NAME[dtype], ROWS, dim, seed)
    wide = None if dtype == FIXED32 else np.ascontiguousarray(ref, dtype=np.float32)
    return rows, name, ref, wide


# ---- small inputs: the lane-group, hot-row and any-dim kernels ----------------------------------------------------------------------
def hot_hint(rows=ROWS):
    """The hint set_hot_rows gets, hottest first: row 0, the last row, a duplicate, an id beyond the table, then 140 distinct rows --
    more than kHotLdsBudget holds of 1-KiB rows."""
    more = [(17 * k + 3) % rows for k in range(1, 141)]
    return np.array([0, rows - 1, 5, 5, rows + 10, 0] + more, np.uint64)


def hot_accepted(hint, nr_rows, row_bytes, budget=HOT_LDS_BUDGET):
    """build_hot_set() restated: (accepted rows in slot order, log2 of the hash size, LDS bytes)."""
    n = len(hint)
    max_rows = min(budget // (row_bytes + 64), n)
    if n == 0 or row_bytes == 0 or max_rows == 0:
        return [], 0, 0
    log2 = 2
    while (1 << log2) < 4 * max_rows:
        log2 += 1
    while max_rows and max_rows * row_bytes + (8 << log2) > budget:
        max_rows -= 1
    mask = (1 << log2) - 1
    table, rows, seen = {}, [], set()
    for r in (int(v) for v in hint):
        if len(rows) >= max_rows:
            break
        if r >= nr_rows or r >= 0xFFFFFFFF or r in seen:
            continue
        seen.add(r)
        home = ((r * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - log2)
        for p in range(HOT_PROBES):
            if (home + p) & mask not in table:
                table[(home + p) & mask] = r
                rows.append(r)
                break
    return rows, (log2 if rows else 0), (len(rows) * row_bytes + (8 << log2) if rows else 0)


def small_bag_counts(kind, lpr, scalar_lanes=0):
    """Bag counts of a small launch's two descriptors: odd (no multiple of any tile), unequal, more than one tile each."""
    bpt = bags_per_tile(kind, lpr, scalar_lanes)
    return (bpt + 45) | 1, (2 * bpt + 6) | 1


@lru_cache(maxsize=None)
def small_inputs(n_bags, seed, rows=ROWS):
    """One descriptor of ragged bags: empties, a trailing empty bag, a bag of 44 entries with duplicates, row 0 and the last row;
    bag 0 only rows at the head of hot_hint() (hits under every row width), bag 1 only rows the hint does not name (misses), the
    others half from the hint, half from anywhere (mixed).  Returns a namespace: idx, off (int64), lens, w (float32), pad."""
    rng = np.random.default_rng([seed, n_bags])
    hint = hot_hint(rows)
    named = np.unique(hint[hint < rows]).astype(np.int64)
    others = np.setdiff1d(np.arange(rows), named)
    pad = rows // 3
    assert pad not in named
    lens = rng.integers(0, 10, size=n_bags)
    lens[0], lens[1], lens[2], lens[3], lens[-1] = 4, 5, 0, 44, 0
    lens[7] = 0
    off = np.zeros(n_bags, np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    n = int(lens.sum())
    idx = np.where(rng.random(n) < 0.5, rng.choice(named, size=n), rng.integers(0, rows, size=n))
    idx[idx == pad] = pad + 1
    idx[rng.random(n) < 0.1] = pad
    idx[off[0]:off[0] + 4] = [0, rows - 1, 5, 0]
    miss = rng.choice(others[others != pad], size=5)
    idx[off[1]:off[1] + 5] = miss
    long_bag = rng.integers(0, rows, size=44)
    long_bag[:6] = [0, rows - 1, 9, 9, pad, rows - 1]
    long_bag[20:30] = long_bag[10]
    idx[off[3]:off[3] + 44] = long_bag
    w = rng.standard_normal(n).astype(np.float32)
    return SimpleNamespace(idx=idx.astype(np.int64), off=off, lens=lens.astype(np.int64), w=w, pad=pad, n_bags=n_bags)


def hot_bag_classes(d, accepted):
    """Per bag of a small descriptor: "hit" (every entry in the accepted hot set), "miss" (none), "mixed", or "empty"."""
    acc = np.isin(d.idx, np.array(sorted(accepted), np.int64))
    out = []
    for b in range(d.n_bags):
        a = acc[d.off[b]:d.off[b] + d.lens[b]]
        out.append("empty" if len(a) == 0 else "hit" if a.all() else "miss" if not a.any() else "mixed")
    return out


# ---- big inputs: the wave-batch and two-batch kernels -------------------------------------------------------------------------------
def big_unroll(case):
    """The unroll the general step of the case's kernel walks a bag with (WaveCfg 8, Wave2Cfg and fp32's PoolWaveCfg 4)."""
    return 4 if case.kind == 2 or (case.record.get("pool") and case.dtype == F32) else 8


@lru_cache(maxsize=None)
def big_case(B, unroll):
    """THE wave-batch layout of B bags (pool_cases.wave_batch_case, its last step a general one), shared by every dtype and dim."""
    c = pc.wave_batch_case(ROWS, B, unroll, seed=B % 1000 + unroll, tail="general")
    pc.check_wave_batch_case(c, B)
    return c


def big_descs(case):
    """The two descriptors of a big case as (first bag, bags) ranges of big_case(): the whole layout -- without its last, long bag
    where the case's tail is "shifted": the partial step is then bags of <= 1 index with an empty one among them -- and SECOND_B bags
    from SECOND_AT.  Bags are independent, so one reference over the whole layout serves both descriptors and both id widths."""
    B = TWO_B if case.size == "two" else WAVE_B
    return B, [(0, B if case.tail == "general" else B - 1), (SECOND_AT, SECOND_B)]


# ---- ranged inputs ------------------------------------------------------------------------------------------------------------------
NOBODY = {3: ROWS + 100, 11: -1, 500: -(1 << 45), 1000: (1 << 32) + 5, -1: 1 << 62}      # position -> an id no shard holds
PER_SHARD = -(-ROWS // N_SHARDS)


@lru_cache(maxsize=None)
def ranged_inputs(B):
    """One int64 index per bag over the whole table, ids no shard holds among them (beyond the end, negative, beyond 2^32).
    Returns a namespace: idx (int64), idx32 (uint32: the ids nobody holds as ROWS + 7), held, mine (per shard)."""
    rng = np.random.default_rng(B)
    idx = rng.integers(0, ROWS, size=B).astype(np.int64)
    idx[5], idx[6] = 0, ROWS - 1
    idx[20:20 + N_SHARDS] = [(s + 1) * PER_SHARD - 1 for s in range(N_SHARDS - 1)] + [ROWS - 1]     # every shard's last row ...
    idx[30:30 + N_SHARDS] = [s * PER_SHARD for s in range(N_SHARDS)]                                # ... and first
    for p, v in NOBODY.items():
        idx[p] = v
    held = (idx >= 0) & (idx < ROWS)
    mine = [(idx >= s * PER_SHARD) & (idx < min((s + 1) * PER_SHARD, ROWS)) for s in range(N_SHARDS)]
    return SimpleNamespace(idx=idx, idx32=np.where(held, idx, ROWS + 7).astype(np.uint32), held=held, mine=mine, B=B)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def np_sum(table, idx, off):
    """Plain float32 accumulation in index order: step j adds every bag's j-th row."""
    lens = np.append(off[1:], len(idx)) - off
    out = np.zeros((len(off), table.shape[1]), np.float32)
    for j in range(int(lens.max(initial=0))):
        live = np.flatnonzero(lens > j)
        out[live] = out[live] + table[idx[off[live] + j]].astype(np.float32)
    return out
