"""CPU: the kernel census of tests/kernel_census.py is what it claims.  Against the built library: every case resolves to exactly
one bag_*_kernel symbol, no two cases share one, and no lookup kernel is left without a case; every other kernel of the library has
a named home.  Against the source text: the constants kernel_census.py restates.  Against the inputs: every case's shape is on the
side of the dispatch thresholds it relies on, the big layouts hold every class of step, the hot-row inputs hold the hit / miss /
mixed bags promised under every row width, and hot_accepted() equals build_hot_set() compiled from pimemb_hot_rows.h.  The
references the GPU half compares with are pinned against plain numpy accumulation in index order.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census as kc  # noqa: E402
import pool_cases as pc  # noqa: E402
import pool_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
FAMILIES = sorted({c.family for c in kc.CASES})


# ---- 1. one case, one kernel --------------------------------------------------------------------------------------------------------
def test_one_case_one_kernel(pel):
    from pim_embedding_lookup_amd import codeobj
    lookup = {k for k in codeobj.kernel_hashes(pel.LIB_PATH) if "bag_" in k}
    assert all(k.endswith(("PKNS_7DevDescEjPKj", "PKNS_7DevDescEj", "PKNS_7DevDescEjj")) and "_kernelI" in k for k in lookup), \
        "a bag_* symbol that is no lookup kernel template"
    owner = {}
    for c in kc.CASES:
        syms = {codeobj.kernel_of_launch(pel.LIB_PATH, kc.record_at(c, dim))[0] for dim in c.dims}      # raises unless exactly one
        assert len(syms) == 1, "%s: its row widths resolve to different kernels: %s" % (c.id, sorted(syms))
        sym = syms.pop()
        assert sym not in owner, "%s and %s share the kernel %s" % (c.id, owner[sym], sym)
        owner[sym] = c.id
    assert not set(kc.UNREACHABLE) - lookup, "UNREACHABLE names kernels the library does not hold"
    assert not set(kc.UNREACHABLE) & set(owner), "a kernel listed as unreachable has a case"
    missing = lookup - set(owner) - set(kc.UNREACHABLE)
    assert not missing, "%d lookup kernels without a census case (add their loop to kernel_census.cases()): %s" % (len(missing), sorted(missing)[:5])
    assert set(owner) <= lookup and len(owner) == len(kc.CASES) == len(lookup) - len(kc.UNREACHABLE)


def test_case_table_is_well_formed():
    ids = [c.id for c in kc.CASES]
    assert len(set(ids)) == len(ids)
    groups = kc.groups()
    assert sum(len(cs) for _g, cs in groups) == len(kc.CASES) and len({g for g, _cs in groups}) == len(groups)
    for g, cs in groups:
        assert len(cs) <= 7 and len({(c.family, c.dtype, c.itype) for c in cs}) == 1, g
    for a, b in zip(groups[0::2], groups[1::2]):              # a (family, dtype)'s two id widths run next to each other
        assert a[0][:-3] == b[0][:-3] and [c.dims for c in a[1]] == [c.dims for c in b[1]]
    for c in kc.CASES:
        assert (c.kind == 2) <= (c.lpr <= kc.TWO_MAX_LANES) and bool(c.specs) == bool(c.record.get("pool")), c.id
        if c.lpr >= 4:                                        # the width with one dead lane everywhere, the full one on small launches too
            chunks = [kc.geometry(c.dtype, d)[1] for d in c.dims]
            assert chunks == ([c.lpr, c.lpr - 1] if c.size == "small" else [c.lpr - 1]), c.id
        elif c.lpr:
            assert [kc.geometry(c.dtype, d)[1] for d in c.dims] == [c.lpr], c.id
        else:                                                 # any-dim: non-vec rows of < 32 bytes or no 4-byte multiple; vec the rest
            rb, vec = kc.row_bytes_of(c.dtype, c.dims[0]), c.record["anydim_vec"]
            assert rb % 16 or rb > kc.MAX_ROW_BYTES
            assert (rb % 4 != 0 or rb < 32) if not vec else (rb % 4 == 0 and rb >= 32), c.id
    # big pooled cases run one spec each: every spec at some lane count of every (family, dtype), the same under both id widths
    for fam in ("pool-wave", "hpool-wave", "strided-pool-wave"):
        for dt in {c.dtype for c in kc.CASES if c.family == fam}:
            for it in (0, 1):
                assert {c.specs[0] for c in kc.CASES if (c.family, c.dtype, c.itype) == (fam, dt, it)} == set(kc.SPEC_NAMES), (fam, dt)
    for c in kc.CASES:
        if c.size == "small" and c.specs:
            assert c.specs == kc.SPEC_NAMES and set(kc.SPEC_NAMES) == set(pc.SPECS) | set(pc.SPECS_NO_PAD)
    # the two id widths of a big shape take the two tails
    for a, b in zip(groups[0::2], groups[1::2]):
        assert all({x.tail, y.tail} == {"general", "shifted"} for x, y in zip(a[1], b[1]))


# ---- 2. the library's other kernels -------------------------------------------------------------------------------------------------
def test_helper_kernels_have_a_home(pel):
    from pim_embedding_lookup_amd import codeobj
    others = {kc.helper_name(k) for k in codeobj.kernel_hashes(pel.LIB_PATH) if "bag_" not in k}
    assert others == set(kc.HELPER_KERNELS), "kernels without a home in kernel_census.HELPER_KERNELS: %s; names that are no kernel: %s" % (
        sorted(others - set(kc.HELPER_KERNELS)), sorted(set(kc.HELPER_KERNELS) - others))
    header = open(os.path.join(ROOT, "include", "pimemb.h")).read()
    for kernel, (entry, path, mention) in kc.HELPER_KERNELS.items():
        assert re.search(r"\bint %s\(" % entry, header), "%s: %s is no entry point of pimemb.h" % (kernel, entry)
        text = open(os.path.join(ROOT, path)).read()
        assert "pytest.mark.gpu" in text and mention in text, "%s: %s does not mention %s" % (kernel, path, mention)
        src = "".join(open(os.path.join(CSRC, f)).read() for f in ("pimemb_kernels.hip", "pimemb_peer.cpp"))
        assert kernel.split("<")[0] + "(" in src or kernel.split("<")[0] + "<" in src, kernel


# ---- 3. the constants -----------------------------------------------------------------------------------------------------------------
def test_constants_are_the_engines():
    """A tripwire on the source TEXT, as test_queue_cases_cpu.py's: a pattern that no longer matches may mean a reformatted line
    (update the pattern) or a retuned constant (move it in tests/kernel_census.py; the shapes follow).  choose_kernel's own
    thresholds are queue_cases.py's, pinned by test_queue_cases_cpu.py."""
    kern = open(os.path.join(CSRC, "pimemb_kernels.hip")).read()
    eng = open(os.path.join(CSRC, "pimemb_engine.cpp")).read()
    internal = open(os.path.join(CSRC, "pimemb_internal.h")).read()
    hot = open(os.path.join(CSRC, "pimemb_hot_rows.h")).read()
    moved = "%s: this test's pattern no longer matches the source text (reformatted: update the pattern; retuned: move the constant in tests/kernel_census.py)"
    for name, want in (("GroupCfg", kc.GROUP_BLOCK), ("Mx4GroupCfg", kc.GROUP_BLOCK), ("HotCfg", kc.HOT_BLOCK)):
        m = re.search(r"using %s = BagCfg<(\d+)," % name, kern)
        assert m, moved % name
        assert int(m.group(1)) == want, (name, m.group(1), want)
    m = re.search(r"constexpr size_t kHotLdsBudget = (\d+)u << (\d+);", internal)
    assert m, moved % "kHotLdsBudget"
    assert int(m.group(1)) << int(m.group(2)) == kc.HOT_LDS_BUDGET
    m = re.search(r"for \(uint32_t p = 0; p < (\d+); p\+\+\) \{\s+// kHotProbes", hot)
    assert m, moved % "kHotProbes"
    assert int(m.group(1)) == kc.HOT_PROBES
    assert "size_t max_rows = lds_budget / ((size_t)row_bytes + 64);" in hot and "(key * 0x9E3779B1u) >> (32u - log2)" in hot, moved % "build_hot_set"
    m = re.search(r"if \(row_bytes % 16 != 0 \|\| row_bytes > (\d+)\) \{", kern)
    assert m, moved % "geometry_for's any-dim rule"
    assert int(m.group(1)) == kc.MAX_ROW_BYTES
    assert "g->anydim_vec = row_bytes % 4 == 0 && row_bytes >= 32;" in kern, moved % "geometry_for's vec rule"
    assert "if (kind == KERNEL_ANYDIM) return %du / g.scalar_lanes;" % kc.ANYDIM_BLOCK in kern, moved % "bags_per_tile(KERNEL_ANYDIM)"
    assert "if (kind == KERNEL_HOT) return (64u / g.lanes_per_row) * (HotCfg::kBlock / 64);" in kern, moved % "bags_per_tile(KERNEL_HOT)"
    # resolve()'s overrides of choose_kernel, as kernel_census.expected_kind() restates them
    for line in ("if (g.dtype == pimemb::kMXFP4) g.kind = pimemb::KERNEL_GROUP;",
                 "if (g.ranged && g.kind == pimemb::KERNEL_GROUP) g.kind = pimemb::KERNEL_WAVEBATCH;",
                 "if (g.pool && g.kind == pimemb::KERNEL_WAVEBATCH2) g.kind = pimemb::KERNEL_WAVEBATCH;",
                 "if (g.kind == pimemb::KERNEL_GROUP && !g.pool && !g.out_half && !g.strided) {",
                 "if (g.hot_lds) g.kind = pimemb::KERNEL_HOT;"):
        assert line in eng, moved % line
    assert kc.TWO_B == kc.TWO_MIN_BAGS + 5 and kc.WAVE_B == kc.WAVE_MIN_BAGS + 5 and kc.WAVE_B + kc.SECOND_B < kc.TWO_MIN_BAGS


# ---- 4. shapes reach their kernels --------------------------------------------------------------------------------------------------
def launch_totals(c, dim):
    """(descriptors, bags, indices) of the LARGEST launch group the case's call forms at this row width."""
    if c.size in ("ranged", "ranged-two"):
        B = kc.RANGED_B if c.size == "ranged" else kc.TWO_B
        return kc.N_SHARDS, kc.N_SHARDS * B, kc.N_SHARDS * B
    if c.size == "small":
        _lpr, _chunks, scalar, _vec = kc.geometry(c.dtype, dim)
        counts = kc.small_bag_counts(c.kind, c.lpr, scalar)[:c.n_descs]
        descs = [kc.small_inputs(n, k) for k, n in enumerate(counts)]
        k = max(1, len(c.specs))                         # (an upper bound: the specs of one mode form one group)
        return k * len(descs), k * sum(counts), k * sum(len(d.idx) for d in descs)
    B, ranges = kc.big_descs(c)
    big = kc.big_case(B, kc.big_unroll(c))
    n_idx = sum(len(pc.cut_range(big, b0, n)[0]) for b0, n in ranges)
    return len(ranges), sum(n for _b0, n in ranges), n_idx


@pytest.mark.parametrize("family", FAMILIES)
def test_shapes_reach_their_kernels(family):
    hint = kc.hot_hint()
    for c in (c for c in kc.CASES if c.family == family):
        for dim in c.dims:
            lpr, chunks, scalar, _vec = kc.geometry(c.dtype, dim)
            n, bags, idx = launch_totals(c, dim)
            hot_lds = 0
            if c.kind == 4:
                rows, _log2, hot_lds = kc.hot_accepted(hint, kc.ROWS, chunks * 16)
                assert 0 < hot_lds <= kc.HOT_LDS_BUDGET and len(rows) >= 3, c.id
                if chunks * 16 >= 1008:                  # ~1-KiB rows: the hint is more than the budget holds
                    assert len(rows) < len(np.unique(hint[hint < kc.ROWS])), c.id
            assert kc.expected_kind(c, dim, bags, idx, hot_lds) == c.kind, (c.id, dim, bags, idx)
            assert n == c.n_descs * max(1, len(c.specs) if c.size == "small" else 1), c.id
            if c.size == "small":
                assert kc.expected_kind(c, dim, bags // max(1, len(c.specs)), idx // max(1, len(c.specs)), hot_lds) == c.kind
                bpt = kc.bags_per_tile(c.kind, lpr, scalar)
                counts = kc.small_bag_counts(c.kind, lpr, scalar)
                assert counts[0] != counts[1] and all(nb > bpt and nb % bpt for nb in counts), (c.id, counts, bpt)
            elif c.size in ("wave", "two"):
                floor = kc.TWO_MIN_BAGS if c.size == "two" else kc.WAVE_MIN_BAGS
                assert floor <= bags and idx <= 2 * bags and (c.size == "two" or bags < kc.TWO_MIN_BAGS or lpr > kc.TWO_MAX_LANES), c.id
                assert kc.expected_kind(c, dim, floor - 1, idx, 0) != c.kind, "the threshold is not where the shape thinks it is"
            elif c.size == "ranged-two":
                assert bags >= kc.TWO_MIN_BAGS and lpr <= kc.TWO_MAX_LANES
            else:
                assert bags < kc.WAVE_MIN_BAGS           # ranged: the wave-batch kernel although choose_kernel says lane-group


# ---- 5. the inputs --------------------------------------------------------------------------------------------------------------------
def test_big_inputs_are_sound():
    used = {(kc.big_descs(c)[0], kc.big_unroll(c)) for c in kc.CASES if c.size in ("wave", "two")}
    assert used == {(kc.WAVE_B, 8), (kc.WAVE_B, 4), (kc.TWO_B, 4)}
    for B, unroll in used:
        big = kc.big_case(B, unroll)
        pc.check_wave_batch_case(big, B)                                     # (also run when the case is built)
        assert big.tail_class == "general" and big.lens[B - 1] >= 2
        cut = pc.step_classes(big.lens[:B - 1], big.off[:B - 1])            # without the last bag: a shifted partial step
        assert cut[-1] == "shifted" and (B - 1) % 64 and cut[:-1] == big.classes[:-1]
        assert kc.SECOND_AT % 64 and (kc.SECOND_AT + kc.SECOND_B) % 64 and kc.SECOND_AT + kc.SECOND_B < B
        idx, off, _w = pc.cut_range(big, kc.SECOND_AT, kc.SECOND_B)
        lens = np.append(off[1:], len(idx)) - off
        second = pc.step_classes(lens, off)
        assert np.array_equal(lens, big.lens[kc.SECOND_AT:kc.SECOND_AT + kc.SECOND_B])
        assert second.count("general") >= 2 and len(second) == -(-kc.SECOND_B // 64) and len(set(second)) >= 2, second
        assert big.idx.min() >= 0 and big.idx.max() < kc.ROWS and 0 <= big.pad < kc.ROWS
        assert big.idx.max() == kc.ROWS - 1 and big.idx.min() == 0, "row 0 and the last row are not among the ids"


def test_small_and_hot_inputs_are_sound():
    hint = kc.hot_hint()
    assert hint[0] == 0 and hint[1] == kc.ROWS - 1 and (hint >= kc.ROWS).any() and len(np.unique(hint)) < len(hint)
    seen = set()
    for c in kc.CASES:
        if c.size != "small":
            continue
        for dim in c.dims:
            lpr, chunks, scalar, _vec = kc.geometry(c.dtype, dim)
            key = (c.kind, lpr, scalar, chunks if c.kind == 4 else 0)
            if key in seen:
                continue
            seen.add(key)
            accepted = kc.hot_accepted(hint, kc.ROWS, chunks * 16)[0] if c.kind == 4 else None
            for k, n in enumerate(kc.small_bag_counts(c.kind, lpr, scalar)[:c.n_descs]):
                d = kc.small_inputs(n, k)
                assert d.n_bags == n == len(d.off) == len(d.lens) and np.array_equal(np.diff(np.append(d.off, len(d.idx))), d.lens)
                assert d.lens[-1] == 0 and (d.lens[:-1] == 0).sum() >= 2 and d.lens.max() >= 40 and len(d.w) == len(d.idx)
                assert d.idx.min() == 0 and d.idx.max() == kc.ROWS - 1 and (d.idx == d.pad).sum() >= 3
                long_bag = d.idx[d.off[3]:d.off[3] + d.lens[3]]
                assert len(np.unique(long_bag)) < len(long_bag)
                if accepted is not None:
                    cls = kc.hot_bag_classes(d, accepted)
                    assert cls[0] == "hit" and cls[1] == "miss" and cls.count("mixed") >= n // 4, (c.id, dim, cls[:8])
                    assert set(accepted) >= {0, kc.ROWS - 1, 5}


def test_ranged_inputs_are_sound():
    for B in (kc.RANGED_B, kc.TWO_B):
        r = kc.ranged_inputs(B)
        assert len(r.idx) == B and (~r.held).sum() == len(kc.NOBODY) and (r.idx < 0).sum() == 2 and (r.idx > 1 << 32).sum() == 2
        assert (r.idx32[~r.held] >= kc.ROWS).all() and np.array_equal(r.idx32[r.held], r.idx[r.held])
        assert sum(int(m.sum()) for m in r.mine) == B - len(kc.NOBODY) and all(m.sum() > B // 4 for m in r.mine)
        for s in range(kc.N_SHARDS):                      # first and last row of every shard
            lo, hi = s * kc.PER_SHARD, min((s + 1) * kc.PER_SHARD, kc.ROWS) - 1
            assert (r.idx == lo).any() and (r.idx == hi).any()
        assert ((r.idx & 0xFFFFFFFF)[~r.held] < kc.ROWS).any(), "no id that a 32-bit truncation would turn into a held row"


_HOT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "pimemb_hot_rows.h"
int main(int argc, char **argv) {      // hot_check <nr_rows> <row_bytes> <budget> <id>...: the accepted rows, log2size, LDS bytes
    std::vector<uint64_t> ids;
    for (int i = 4; i < argc; i++) ids.push_back(strtoull(argv[i], nullptr, 10));
    const uint32_t row_bytes = (uint32_t)atoi(argv[2]);
    pimemb::HotSet hs = pimemb::build_hot_set(ids.data(), (uint32_t)ids.size(), strtoull(argv[1], nullptr, 10), row_bytes, (size_t)atol(argv[3]));
    for (uint64_t r : hs.rows) printf("%llu ", (unsigned long long)r);
    printf("\n%u %zu\n", hs.log2size, hs.rows.empty() ? (size_t)0 : hs.lds_bytes(row_bytes));
    return 0;
}
"""


def test_hot_accepted_mirrors_build_hot_set(tmp_path):
    """kernel_census.hot_accepted() against build_hot_set() itself, compiled from pimemb_hot_rows.h (a host-only header), at every
    row width the hot cases run and with a hint that fills the hash's two probes."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler here")
    src, exe = tmp_path / "hot_check.cpp", tmp_path / "hot_check"
    src.write_text(_HOT_PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])
    widths = sorted({kc.geometry(c.dtype, d)[1] * 16 for c in kc.CASES if c.kind == 4 for d in c.dims})
    assert widths[0] == 16 and widths[-1] == 1024 and len(widths) == 12
    # fewer ids than 16-byte rows fit, drawn at random: the ones left out missed both probes
    crowded = np.random.default_rng(1).choice(kc.ROWS, size=780, replace=False).astype(np.uint64)
    for hint in (kc.hot_hint(), crowded):
        for rb in widths:
            out = subprocess.check_output([str(exe), str(kc.ROWS), str(rb), str(kc.HOT_LDS_BUDGET)] + [str(int(v)) for v in hint], text=True)
            rows_line, tail = out.split("\n")[:2]
            rows, log2, lds = kc.hot_accepted(hint, kc.ROWS, rb)
            assert [int(v) for v in rows_line.split()] == rows, rb
            assert [int(v) for v in tail.split()] == [log2, lds], rb
    dropped = kc.hot_accepted(crowded, kc.ROWS, 16)[0]
    assert len(crowded) < kc.HOT_LDS_BUDGET // (16 + 64) and len(dropped) < len(crowded), "no row of the crowded hint missed both probes"


# ---- 6. the references ----------------------------------------------------------------------------------------------------------------
def test_references_are_pinned(oracle):
    """oracle.c_bag_sum, c_lookup_fixed32 and pool_cases.reference (torch's CPU embedding_bag) against plain numpy float32
    accumulation in index order, once, on a small instance: sum, weighted (with and without padding) and fixed-point."""
    d = kc.small_inputs(301, 0)
    _rows, _name, ref, wide = kc.make_table(kc.F32, 12)
    want = kc.np_sum(wide, d.idx, d.off)
    assert np.array_equal(oracle.c_bag_sum(ref, d.idx, d.off).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(pc.reference(wide, d.idx, d.off, ("sum", False, False), d.w, d.pad).view(np.uint32), want.view(np.uint32))
    _rows, _name, h, hwide = kc.make_table(kc.F16, 24)
    assert np.array_equal(oracle.c_bag_sum(h, d.idx, d.off).view(np.uint32), kc.np_sum(hwide, d.idx, d.off).view(np.uint32))
    for name in ("weighted", "weighted+pad", "sum+pad", "mean+pad", "max+pad", "mean", "max"):
        mode, weighted, padded = kc.ALL_SPECS[name]
        got = pc.reference(wide, d.idx, d.off, kc.ALL_SPECS[name], d.w, d.pad)
        plain = pool_ref.embedding_bag(wide, d.idx, d.off, mode=mode, per_sample_weights=d.w if weighted else None,
                                       padding_idx=d.pad if padded else None)
        ok, text = pc.same_bits(got, plain)
        assert ok, "%s: %s" % (name, text)
    _rows, _name, fix, _none = kc.make_table(kc.FIXED32, 8)
    i32, o32 = d.idx.astype(np.uint32), d.off.astype(np.uint32)
    assert np.array_equal(oracle.c_lookup_fixed32(fix, i32, o32).view(np.uint32), oracle.np_lookup_fixed32(fix, i32, o32).view(np.uint32))
