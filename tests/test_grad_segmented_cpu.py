"""CPU: the segmented order of additions of the backward pass (EMB_GRAD_ORDER_SEGMENTED, include/pimemb_grad.h).  The reference
of its GPU tests (tests/grad_seg_ref.py) is what it has to be: the position order wherever every run has at most S + 1
occurrences, another sum on the witnesses; the +-FLT_MAX witness keeps its properties inside segments and across them; the absorb
column tells the orders, the segment lengths and the two ways of counting segments apart.  The additions to the C ABI are
declared, exported, bound and refuse bad configs; the slot numbering of the partial sums (csrc/pimemb_grad_segments.h, the very text
the kernels compile) is collision-free over enumerated run layouts.  No GPU work is called."""
import ctypes as C
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_order_cases as oc  # noqa: E402
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402

F = np.float32
ROOT = gr.ROOT
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
build = import_module("pim-embedding-lookup_amd.build")
codeobj = import_module("pim-embedding-lookup_amd.codeobj")


def seg_cases(S):
    return [sr.lengths_case(S, True), sr.lengths_case(S, False), sr.placement_case(S, "bad"), sr.placement_case(S, "end"), sr.one_row_case(S),
            sr.short_case(S)] + sr.multi_cases(S)


def order_cases():
    """The cases of the position order's tests (they carry no absorb column: Case.fold and sr.fold read the same gradients)."""
    return [oc.run_case(L, b) for L, b in oc.RUN_CASES] + [oc.edge_case(n) for n in (257, 1025)] + [oc.pass_case(255), oc.small_case(), oc.long_case()]


# ---- the reference against the position order --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 16, 64, 256])
def test_reference_is_the_position_order_where_every_run_has_at_most_S_plus_1_occurrences(S):
    seen = 0
    for case in order_cases() + (seg_cases(S) if S in sr.SEGMENTS else [c for c in seg_cases(16) if c.n < 1000]):
        longest = max(case.run_lengths().values())
        if longest > S + 1:
            continue
        seen += 1
        for dim, path, narrow in ((4, "sum", False), (5, "weighted", False), (8, "mean", False), (8, "sum", True)):
            got = sr.fold(case, S, dim, path, narrow)
            oc.check_sparse(got[0], got[1], case.fold(dim, path, narrow), (case.name, S, dim, path))
            assert got[2] == case.n_bad
    assert seen >= {8: 1, 16: 1, 64: 5, 256: 10}[S], seen


@pytest.mark.parametrize("S", sr.SEGMENTS)
def test_a_last_segment_of_one_element_adds_that_element_itself(S):
    """k = S + 1 is the edge of the identity: the runs of S + 1 of the cases give the position order's bits, the runs of S + 2 do
    not (on the absorb column)."""
    case = sr.lengths_case(S, False)
    runs = case.run_lengths()
    rows, seg, _ = case.seg_reference(S, 4)
    _, pos, _ = case.fold(4, "sum")
    for k, r in enumerate(rows.tolist()):
        same = np.array_equal(oc.bits(seg[k]), oc.bits(pos[k]))
        assert same == (runs[r] <= S + 1), (r, runs[r])


@pytest.mark.parametrize("S", sr.SEGMENTS)
def test_reference_differs_from_the_position_order_on_the_witnesses(S):
    for case in (sr.lengths_case(S, True), sr.placement_case(S, "bad"), sr.one_row_case(S), sr.multi_cases(S)[1]):
        for dim, path in ((4, "sum"), (6, "weighted"), (8, "mean")):
            rows, seg, _ = sr.fold(case, S, dim, path)
            _, pos, _ = case.fold(dim, path)
            differs = (oc.bits(seg) != oc.bits(pos)).any(axis=1)
            long = np.array([case.run_lengths()[r] > S + 1 for r in rows.tolist()])
            assert long.any() and np.array_equal(differs, long), (case.name, dim, path)
            with pytest.raises(AssertionError):
                oc.check_sparse(rows, pos, (rows, seg), "the position order is rejected")


def test_the_three_coefficient_paths_give_the_same_bits():
    for S in sr.SEGMENTS:
        for case in (sr.lengths_case(S, True), sr.placement_case(S, "end")):
            want = case.seg_reference(S, 8)
            for path in ("weighted", "mean"):
                got = sr.fold(case, S, 8, path)
                oc.check_sparse(got[0], got[1], want, (case.name, path))
            assert not np.array_equal(oc.bits(case.grads(8, weighted=True)[case.good]), oc.bits(case.grads(8)[case.good]))


# ---- the +-FLT_MAX witness under the segmented order ---------------------------------------------------------------------------------
def partial_sums(case, S, row, order=None):
    """Every intermediate value of columns 0 and 1 of one row in the segmented order: inside the segments, then across them."""
    C2 = case.contributions(4, "sum")[:, :2]
    ps = [int(p) for p in (case.order() if order is None else order) if case.ids[p] == row]
    seen, partials = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for at in range(0, len(ps), S):
            t = np.zeros(2, F)
            for p in ps[at:at + S]:
                t = t + C2[p]
                seen.append(t)
            partials.append(t)
        g = partials[0]
        for t in partials[1:]:
            g = g + t
            seen.append(g)
    return np.array(seen), g


@pytest.mark.parametrize("S", sr.SEGMENTS)
def test_the_witness_stays_finite_in_the_right_order_inside_segments_and_across_them(S):
    """For even S a segment starts at an odd ordinal: column 0 runs +M, 0, +M, ... inside every segment and adds zeros and at most
    one +M across them; column 1 (grad_seg_ref's, which follows the segments) runs 0, s M, 0, s M, ... inside segment m and
    +M, 0, +M, ... across them."""
    for case in (sr.lengths_case(S, False), sr.placement_case(S, "bad"), sr.one_row_case(S)):
        for row, k in case.run_lengths().items():
            seen, g = partial_sums(case, S, row)
            assert np.isfinite(seen).all(), (case.name, row, k)
            assert set(np.unique(np.abs(seen)).tolist()) <= {0.0, float(oc.M)}
        rows, grads, _ = sr.fold(case, S, 4, "sum")
        assert np.isfinite(grads).all()
        # column 2 is the exact sum of p + 1 over the row's positions, in this order too
        want = np.bincount(case.ids[case.good], weights=np.flatnonzero(case.good) + 1.0)
        assert np.array_equal(grads[:, 2].astype(np.float64), want[rows]) and want.max() < 2 ** 24


def test_grad_order_cases_own_column_1_would_leave_half_of_the_later_segments_exchanges_unseen():
    """Why grad_seg_ref changes column 1: with the position order's pattern both witness columns stand at 0 after an even number of
    a later segment's elements, and the exchange behind it overflows nothing."""
    S = 8
    j = np.arange(1, 3 * S + 1)
    c0 = np.where(j % 2 == 1, oc.M, -oc.M).astype(F)
    c1 = np.where(j == 1, F(0), np.where(j % 2 == 0, oc.M, -oc.M)).astype(F)
    seg = slice(S, 2 * S)                                # segment 1
    with np.errstate(over="ignore"):
        for col in (c0, c1):
            x = col[seg].copy()
            x[[2, 3]] = x[[3, 2]]                        # its third and fourth element
            assert np.isfinite(np.cumsum(x, dtype=F)).all()
    case = sr.lengths_case(S, False)                     # ... and the column used here sees that exchange
    row = max(case.run_lengths(), key=case.run_lengths().get)
    wrong = sr.fold(case, S, 4, "sum", order=exchanged(case, row, S + 3))
    assert not np.isfinite(wrong[1][int(np.flatnonzero(wrong[0] == row)[0])][:2]).all()


def test_a_batch_built_for_segments_of_16_stays_finite_in_segments_of_8():
    """The GPU tests sum one batch with S = 8 and with S = 16: its reference has to be finite for both."""
    case = sr.lengths_case(16, True)
    for S in (8, 16):
        for row in case.run_lengths():
            assert np.isfinite(partial_sums(case, S, row)[0]).all(), (S, row)
    a8, a16 = (sr.fold(case, S, 4, "sum")[1][:, sr.ABSORB] for S in (8, 16))
    assert (a8 != a16).any()


def exchanged(case, row, j):
    """case.order() with the occurrences j and j + 1 (1-based) of `row` exchanged."""
    order = case.order().copy()
    at = np.flatnonzero(case.ids[order] == row)
    order[[at[j - 1], at[j]]] = order[[at[j], at[j - 1]]]
    return order


@pytest.mark.parametrize("S", sr.SEGMENTS)
def test_exchanging_two_neighbours_inside_a_segment_gives_inf(S):
    """Wrong orders are applied to the list the reference folds, as tests/test_grad_order_cpu.py does: every exchange of the
    occurrences j and j + 1 that lie in one segment overflows column 0 or column 1, and the comparison the GPU tests use rejects
    the result.  The first pair of a SEGMENT is exempt as the first pair of a run is in the position order: a segment starts from
    +0, and 0 + a + b = 0 + b + a in IEEE arithmetic -- that exchange is no other sum."""
    case = sr.lengths_case(S, False)
    ref = case.seg_reference(S, 4)
    for row, k in case.run_lengths().items():
        if k > 4 * S:
            continue                                     # (the long ones: sampled below)
        for j in range(2, k):
            if (j - 1) // S != j // S or j % S == 1:
                continue                                 # j and j + 1 lie in two segments, or are the first pair of one
            wrong = sr.fold(case, S, 4, "sum", order=exchanged(case, row, j))
            at = int(np.flatnonzero(wrong[0] == row)[0])
            assert not np.isfinite(wrong[1][at][:2]).all(), (row, k, j)
            with pytest.raises(AssertionError):
                oc.check_sparse(wrong[0], wrong[1], ref, (row, j))
    row = max(case.run_lengths(), key=case.run_lengths().get)
    for j in (2, S - 1, S + 2, 2 * S - 1, 9 * S + 2, 64 * S + 3):
        wrong = sr.fold(case, S, 4, "sum", order=exchanged(case, row, j))
        assert not np.isfinite(wrong[1][int(np.flatnonzero(wrong[0] == row)[0])][:2]).all(), j
    first_pair = sr.fold(case, S, 4, "sum", order=exchanged(case, row, S + 1))      # the first pair of segment 1 commutes
    oc.check_sparse(first_pair[0], first_pair[1], ref, "the first pair of a segment")
    right = sr.fold(case, S, 4, "sum", order=case.order())
    oc.check_sparse(right[0], right[1], ref, "the right order")


# ---- the absorb column -----------------------------------------------------------------------------------------------------------
def by_sorted_place(case, S, dim):
    """A WRONG order: segments cut at the S-aligned sorted places of the whole batch instead of at the row's own ordinals."""
    C = case.contributions(dim, "sum")
    acc, place = {}, 0
    for r, _head, _k in sr.sorted_layout(case):
        ps = [int(p) for p in case.order() if case.ids[p] == r]
        parts, t = [], None
        for p in ps:
            if t is None or place % S == 0:
                if t is not None:
                    parts.append(t)
                t = np.zeros(dim, F)
            t = t + C[p]
            place += 1
        parts.append(t)
        g = parts[0]
        for t in parts[1:]:
            g = g + t
        acc[r] = g
    rows = np.array(sorted(acc), dtype=np.int64)
    return rows, np.stack([acc[int(r)] for r in rows])


def test_the_absorb_column_tells_orders_segment_lengths_and_ordinals_from_places_apart():
    for S in (16, 32, 64):
        case = sr.lengths_case(16, False)
        rows, pos, _ = case.fold(4, "sum")
        assert (pos[:, sr.ABSORB] == F(1)).all()          # the position order absorbs every 2^-24: exactly 1.0
        _, seg, _ = sr.fold(case, S, 4, "sum")
        for k, r in enumerate(rows.tolist()):
            n = case.run_lengths()[r]
            later = max(n - S, 0)                         # occurrences in the segments 1, 2, ...
            got = float(seg[k, sr.ABSORB])
            if later < 2:
                assert got == 1.0, (S, n)
            elif later % 2 == 0:
                assert got == 1.0 + later * 2.0 ** -24, (S, n, got)      # sums of an even number of 2^-24 above 1.0 are exact
            else:
                assert got > 1.0, (S, n)
    case = sr.lengths_case(16, False)
    a8, a16, a32 = (sr.fold(case, S, 4, "sum")[1][:, sr.ABSORB] for S in (8, 16, 32))
    assert (a8 != a16).any() and (a16 != a32).any() and (a8 != a32).any()      # the wrong S shows
    for S in sr.SEGMENTS:                                 # segments by sorted place show (the runs do not start on multiples of S)
        case = sr.placement_case(S, "end")
        rows, wrong = by_sorted_place(case, S, 4)
        with pytest.raises(AssertionError):
            oc.check_sparse(rows, wrong, case.seg_reference(S, 4), "by sorted place")
        assert (wrong[:, sr.ABSORB] != case.seg_reference(S, 4)[1][:, sr.ABSORB]).any()


# ---- the cases hold what their names say ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sr.SEGMENTS)
def test_cases_hold_their_runs(S):
    case = sr.lengths_case(S, True)
    assert sorted(case.run_lengths().values()) == sorted(sr.run_lengths(S)) and case.n_bad == 3 and case.n <= 4097
    assert int((case.ids == sr.LENGTH_PAD).sum()) == 5 and sr.LENGTH_PAD not in case.run_lengths()
    assert np.isnan(case.grads(4)[~case.good]).all() and not np.isnan(case.grads(4)[case.good]).any()
    assert 8 * S + 3 in sr.run_lengths(S) and -(-(8 * S + 3) // S) == 9 and -(-(65 * S + 1) // S) == 66
    for tail in ("bad", "end"):
        case = sr.placement_case(S, tail)
        lay = {r: (h, k) for r, h, k in sr.sorted_layout(case)}
        assert case.run_lengths() == sr.placement_lengths(S) and case.n_bad == (3 if tail == "bad" else 0)
        last = sr.PLACE_ROWS - 1
        assert lay[last][1] > S and lay[last][0] + lay[last][1] == case.n - case.n_bad      # the long run ends the good positions / the array
        assert lay[5][1] > S and lay[6][1] <= S and lay[7][1] > S                             # a short run between two long ones
        h7, k7 = lay[7]
        assert k7 == 2 * S + 3 and lay[8] == (h7 + k7, 2 * S)                                 # directly followed by a long run
        assert (h7 + 2 * S) // S == lay[8][0] // S                                            # two segment starts in one S-aligned block
    one = sr.one_row_case(S)
    assert one.n == 4097 and one.run_lengths() == {sr.ONE_ROW: 4097}
    assert max(sr.short_case(S).run_lengths().values()) == S + 1 and sr.short_case(S).n_bad == 1
    cases = sr.multi_cases(S)
    assert len(cases) == 3 and sum(c.n for c in cases) <= 4097
    for c in cases:
        runs = c.run_lengths()
        assert runs[0] > S + 1 and runs[c.nr_rows - 1] > S + 1 and c.n_bad == 1


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
HEADER = os.path.join(ROOT, "include", "pimemb_grad.h")


def test_header_states_the_definition():
    text = open(HEADER).read()
    for needle in ("EMB_GRAD_ORDER_SEGMENTED", "starting FROM t_0", "k <= S + 1", "emb_grad_scratch_bytes_ex", "emb_grad_create_ex", "emb_grad_config_of"):
        assert needle in text, needle


def test_header_compiles_as_c_and_cxx_and_the_config_record_matches(pel, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pimemb_grad.h"\nint main(void){emb_grad_config c = {EMB_GRAD_ORDER_SEGMENTED, 16, 128, 0};\n'
                   'printf("%zu %zu %zu %zu %zu %u %u\\n", sizeof(emb_grad_config), offsetof(emb_grad_config, order), offsetof(emb_grad_config, segment), '
                   'offsetof(emb_grad_config, max_dim), offsetof(emb_grad_config, reserved), (unsigned)EMB_GRAD_ORDER_POSITION, c.order);\nreturn 0;}\n')
    K = pel.lib.EmbGradConfig
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
        assert got == [C.sizeof(K), K.order.offset, K.segment.offset, K.max_dim.offset, K.reserved.offset, pel.lib.EMB_GRAD_ORDER_POSITION,
                       pel.lib.EMB_GRAD_ORDER_SEGMENTED]
    assert C.sizeof(K) == 16


def test_new_functions_are_exported_and_bound(pel):
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("emb_grad_scratch_bytes_ex", "emb_grad_create_ex", "emb_grad_config_of"):
        assert name in exported and name in pel.lib.GRAD_SIGNATURES, name


def cfg(pel, order, segment=0, max_dim=0, reserved=0):
    return pel.lib.EmbGradConfig(order, segment, max_dim, reserved)


def test_scratch_bytes_ex_equals_the_old_function_for_the_position_order_and_is_monotone(pel):
    G = pel.lib.load_grad()
    POS, SEG = pel.lib.EMB_GRAD_ORDER_POSITION, pel.lib.EMB_GRAD_ORDER_SEGMENTED
    sizes = (1, 2, 255, 1024, 1025, 4097, 65537, 1 << 20, 1 << 30)
    for n in sizes:
        for b in sizes:
            assert G.emb_grad_scratch_bytes_ex(n, b, C.byref(cfg(pel, POS))) == G.emb_grad_scratch_bytes(n, b)
    dims = (1, 3, 4, 5, 16, 128, 320, 511, 512, 513, 4096)
    for S in (8, 64, 1024):
        table = [[[G.emb_grad_scratch_bytes_ex(n, b, C.byref(cfg(pel, SEG, S, d))) for d in dims] for b in sizes] for n in sizes]
        a = np.array(table, dtype=np.uint64)
        assert (np.diff(a.astype(np.float64), axis=0) >= 0).all() and (np.diff(a.astype(np.float64), axis=1) >= 0).all() and (np.diff(a.astype(np.float64), axis=2) >= 0).all()
        for i, n in enumerate(sizes):
            base = G.emb_grad_scratch_bytes(n, sizes[0])
            for k, d in enumerate(dims):
                want = 2 * -(-n // S) * (-(-min(d, 512) // 4)) * 16            # what the header states
                assert int(a[i, 0, k]) == base + -(-want // 256) * 256, (S, n, d)
    # a shorter segment needs more slots
    assert G.emb_grad_scratch_bytes_ex(4097, 4097, C.byref(cfg(pel, SEG, 8, 128))) > G.emb_grad_scratch_bytes_ex(4097, 4097, C.byref(cfg(pel, SEG, 16, 128)))


def test_bad_configs_are_refused_without_a_gpu(pel):
    G = pel.lib.load_grad()
    POS, SEG, INV = pel.lib.EMB_GRAD_ORDER_POSITION, pel.lib.EMB_GRAD_ORDER_SEGMENTED, pel.lib.EMB_ERR_INVALID
    bad = [(cfg(pel, 2, 16, 16), b"unknown order"), (cfg(pel, SEG, 0, 16), b"segment must be"), (cfg(pel, SEG, 4, 16), b"segment must be"),
           (cfg(pel, SEG, 24, 16), b"segment must be"), (cfg(pel, SEG, 2048, 16), b"segment must be"), (cfg(pel, SEG, 16, 0), b"max_dim must be"),
           (cfg(pel, SEG, 16, 16, 1), b"reserved field"), (cfg(pel, POS, 0, 0, 7), b"reserved field"), (cfg(pel, POS, 16, 0), b"with EMB_GRAD_ORDER_POSITION"),
           (cfg(pel, POS, 0, 16), b"with EMB_GRAD_ORDER_POSITION")]
    for c, word in bad:
        h = C.c_void_p()
        assert G.emb_grad_create_ex(None, 16, 16, C.byref(c), C.byref(h)) == INV and not h.value
        assert word in G.emb_grad_last_error(), (word, G.emb_grad_last_error())
        assert G.emb_grad_scratch_bytes_ex(16, 16, C.byref(c)) == 0
    h = C.c_void_p()
    assert G.emb_grad_create_ex(None, 16, 16, None, C.byref(h)) == INV and b"NULL" in G.emb_grad_last_error()
    assert G.emb_grad_scratch_bytes_ex(16, 16, None) == 0
    for good in (cfg(pel, POS), cfg(pel, SEG, 8, 1), cfg(pel, SEG, 1024, 2 ** 32 - 1)):      # a good config gets as far as the engine
        assert G.emb_grad_create_ex(None, 16, 16, C.byref(good), C.byref(h)) == INV and b"engine or out is NULL" in G.emb_grad_last_error()
        assert G.emb_grad_scratch_bytes_ex(16, 16, C.byref(good)) > 0
    out = pel.lib.EmbGradConfig()
    assert G.emb_grad_config_of(None, C.byref(out)) == INV


def test_python_surface_takes_and_checks_the_order(pel):
    import inspect
    sig = inspect.signature(pel.EmbeddingEngine.grad_context)
    assert [sig.parameters[k].default for k in ("order", "segment", "max_dim")] == ["position", None, None]
    assert pel.GradContext.DEFAULT_SEGMENT in (16, 32, 64, 128, 256)
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    for cls in (tm.PoolingEmbeddingBag, tm.FusedPoolingEmbeddingBags):
        for name in ("enable_fused_sgd", "enable_fused_adagrad", "sgd_step_", "adagrad_step_"):
            assert inspect.signature(getattr(cls, name)).parameters["order"].default == "position", (cls, name)
    assert inspect.signature(tm.PoolingEmbeddingBag.sparse_grad).parameters["order"].default == "position"
    with pytest.raises(ValueError):
        tm._order("sorted")


def test_harness_refuses_segmented_sums_without_a_fused_step():
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    with pytest.raises(SystemExit) as ei:
        h.main(["--arch-embedding-size=10-10", "--segmented-sums", "16"])
    assert "--segmented-sums goes with" in str(ei.value)


# ---- the kernels and the slot numbering ---------------------------------------------------------------------------------------------------
def test_new_kernels_are_in_the_code_object_without_spills_or_scratch(pel):
    res = codeobj.kernel_resources(build.GRAD_LIB_PATH)
    seg = {k: v for k, v in res.items() if "grad_seg_" in k}
    for want, count in (("grad_seg_partials", 1), ("grad_seg_multi_partials", 1), ("grad_seg_rows_group", 4), ("grad_seg_multi_rows", 3), ("grad_seg_rows_elem", 3)):
        assert sum(want in k for k in seg) == count, (want, sorted(seg))
    for k, v in seg.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
    assert all("grad_" in k for k in res)


def test_slot_numbering_is_collision_free_over_enumerated_layouts(tmp_path):
    exe = tmp_path / "grad_segments_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "grad_segments_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out[0] == "ok" and int(out[1]) > 10 ** 6 and int(out[3]) > 10 ** 6, out


def test_slot_numbering_holds_on_the_test_cases_layouts():
    """The same formula in Python over the sorted layouts of the GPU cases: unique, below 2 * ceil(n / S)."""
    for S in sr.SEGMENTS:
        for case in seg_cases(S):
            n, used = int(case.good.sum()), set()
            for _r, head, k in sr.sorted_layout(case):
                if k <= S:
                    continue
                for start in range(head, head + k, S):
                    slot = 2 * (start // S) + (start == head)
                    assert slot not in used and slot < 2 * -(-n // S), (case.name, S, start)
                    used.add(slot)
            assert used
