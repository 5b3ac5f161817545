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
import grad_cases as gc  # noqa: E402
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
    for S in sr.SEGMENTS + sr.WIDE_SEGMENTS + sr.MID_SEGMENTS:
        for case in seg_cases(S) if S <= 64 else [sr.reduced_case(S)]:
            n, used = int(case.good.sum()), set()
            for _r, head, k in sr.sorted_layout(case):
                if k <= S:
                    continue
                for start in range(head, head + k, S):
                    slot = 2 * (start // S) + (start == head)
                    assert slot not in used and slot < 2 * -(-n // S), (case.name, S, start)
                    used.add(slot)
            assert used


# ---- the general reference: bags of any shape ----------------------------------------------------------------------------------------------
from grad_gpu import check_state, check_table  # noqa: E402  (the assertions of the GPU tests; nothing in that module touches a GPU on import)

FOREVER = 1 << 20                    # a segment longer than any run


def seg_general(case, S, dim, path, narrow=False):
    """seg_sparse_grad on a one-index case, fed what the kernels are fed."""
    return sr.seg_sparse_grad(case.nr_rows, case.ids, case.offsets, case.grads(dim, narrow, weighted=path == "weighted"), S, "mean" if path == "mean" else "sum",
                              case.weights() if path == "weighted" else None, case.pad)


def test_seg_sparse_grad_is_fold_on_the_one_index_cases():
    for S, case in ((8, sr.lengths_case(8, True)), (8, sr.placement_case(8, "bad")), (16, sr.placement_case(16, "end")), (16, sr.multi_cases(16)[2]),
                    (8, sr.short_case(8))):
        for dim, path, narrow in ((4, "sum", False), (5, "weighted", False), (8, "mean", False), (8, "sum", True)):
            got = seg_general(case, S, dim, path, narrow)
            oc.check_sparse(got[0], got[1], sr.fold(case, S, dim, path, narrow), (case.name, S, dim, path))
            assert got[2] == case.n_bad
    case = sr.placement_case(8, "bad")                    # ... and with bags of fixed_pooling = 1 in place of offsets
    got = sr.seg_sparse_grad(case.nr_rows, case.ids, None, case.grads(4), 8, n_bags=case.n, fixed_pooling=1)
    oc.check_sparse(got[0], got[1], case.seg_reference(8, 4), "fixed pooling")


@pytest.mark.parametrize("mode_name", list(gc.MODES))
def test_seg_sparse_grad_with_one_segment_per_run_is_grad_ref(mode_name):
    for lead in (False, True):
        got = sr.batch_reference(FOREVER, "i64", mode_name, 4, lead)
        want = gc.reference("i64", mode_name, 4, lead, overflow=False)
        oc.check_sparse(got[0], got[1], want, ("batch", mode_name, lead))
        assert got[2] == want[2] == (4 if lead else 5)
        case = sr.ragged_case(8)
        got, want = case.reference(FOREVER, mode_name, "u32", 6, lead), case.reference(None, mode_name, "u32", 6, lead)
        oc.check_sparse(got[0], got[1], want, (case.name, mode_name, lead))
        assert got[2] == want[2] == case.n_bad(lead)
    longest = max(sr.ragged_runs(8).values())             # S = the longest run and S + 1 = longest: still the position order
    for S in (longest, longest - 1):
        got = sr.ragged_case(8).reference(S, mode_name, "i64", 4)
        oc.check_sparse(got[0], got[1], sr.ragged_case(8).reference(None, mode_name, "i64", 4), (S, mode_name))


@pytest.mark.parametrize("S", sr.RAGGED_SEGMENTS)
def test_on_grad_cases_batch_only_the_hot_row_differs_from_the_position_order(S):
    for mode_name in gc.MODES:
        rows, seg, _ = sr.batch_reference(S, "i64", mode_name, 4)
        _, pos, _ = gc.reference("i64", mode_name, 4, overflow=False)
        differs = (oc.bits(seg) != oc.bits(pos)).any(axis=1)
        assert rows[differs].tolist() == [gc.HOT], (S, mode_name, rows[differs])


# ---- the ragged case ------------------------------------------------------------------------------------------------------------------------
def differing(a, b):
    """The rows whose gradients differ in bits between two references of one batch."""
    assert np.array_equal(a[0], b[0])
    return a[0][(oc.bits(a[1]) != oc.bits(b[1])).any(axis=1)].tolist()


@pytest.mark.parametrize("S", sr.RAGGED_SEGMENTS)
def test_ragged_case_holds_what_its_docstring_says(S):
    case, runs = sr.ragged_case(S), sr.ragged_runs(S)
    ids, off, lens = case.bad_ids("i64"), case.offsets(), case.lens
    assert abs(case.n - (16 * S + 300)) <= 120 and case.nr_rows == 499 and case.B & (case.B - 1) and len(off) == case.B
    assert lens.min() == 0 and lens.max() == 13 and len(set(lens.tolist())) >= 13 and int(lens.sum()) == case.n
    assert all(lens[b] == 0 and 0 < b < case.B - 1 for b in case.EMPTY) and lens[-1] == 0 and off[-1] == case.n      # empty bags inside, a trailing one
    assert len(runs) >= 5 and {S + 2, 2 * S + 1, 3 * S + 5, 8 * S + 3, 2 * S} <= set(runs.values()) and {0, case.nr_rows - 1} <= set(runs)
    bag_of = np.repeat(np.arange(case.B), lens)
    for r, k in runs.items():
        at = [p for p, v in enumerate(ids) if v == r]
        assert len(at) == k and len(set(bag_of[at].tolist())) >= min(k, case.B) // 3, (r, k)      # spread over many bags
        with_pad = [b for b in case.PAD_BAGS if r in ids[off[b]:off[b] + lens[b]]]
        assert with_pad and all(case.pad in ids[off[b]:off[b] + lens[b]] for b in with_pad), r        # cnt != the bag's length
    triple = ids[off[case.TRIPLE_BAG]:off[case.TRIPLE_BAG] + lens[case.TRIPLE_BAG]]
    assert triple.count(sr.RAGGED_TRIPLE) == 3
    assert ids[off[case.PAD_ONLY]:off[case.PAD_ONLY] + lens[case.PAD_ONLY]] == [case.pad] * 3
    # the lead variant: positions 0 .. 2 without a bag; a long-run row and a bad id among them
    assert case.offsets(True)[0] == 3 and ids[0] == 123 and case.bad_at[0] == 1 and len(case.bad_at) == 5
    full, lead = case.reference(S, "sum", "i64", 4), case.reference(S, "sum", "i64", 4, lead=True)
    assert full[2] == 5 and lead[2] == 4 and 123 in differing(full, (full[0], lead[1][np.searchsorted(lead[0], full[0])]))
    for width in ("i64", "u32"):
        bad = [case.bad_ids(width)[p] for p in case.bad_at]
        assert all(v < 0 or v >= case.nr_rows for v in bad)
        assert (min(bad) < 0 and max(bad) >= 2 ** 32 and {v % 2 ** 32 for v in bad} & set(runs)) if width == "i64" else max(bad) == 2 ** 32 - 1
        assert case.ids_array(width).dtype == (np.int64 if width == "i64" else np.uint32)
    G, w = case.grads(4), case.weights()
    assert np.signbit(G[G == 0]).any() and ((G != 0) & (np.abs(G) < np.finfo(F).tiny)).any() and np.isfinite(G).all()
    assert len(set(np.frexp(np.abs(G[G != 0]))[1].tolist())) > 16 and (w == 0).any() and (w < 0).any()
    assert np.abs(case.grads(4, narrow=True)[9:]).max() < 2 ** 6


@pytest.mark.parametrize("S", sr.RAGGED_SEGMENTS)
def test_ragged_case_tells_the_orders_the_segment_lengths_cnt_and_the_weights_apart(S):
    """What the batch has to show of the REFERENCE ALONE, so that a kernel with the wrong order, S, cnt or weight index cannot
    pass: in every mode at least four rows differ from the position order, from S / 2, from 2 S and from segments cut by sorted
    place; with every cnt replaced by the bag's length (mean + padding) and with w[bag(p)] for w[p] every long-run row differs.
    Each wrong reference is rejected by the assertions the GPU tests call: check_sparse, and check_table / check_state behind a
    step."""
    case = sr.ragged_case(S)
    long_rows = sorted(sr.ragged_runs(S))
    for dim in (4, 6):
        for mode_name in gc.MODES:
            ref = case.reference(S, mode_name, "i64", dim)
            wrongs = {"position": case.reference(None, mode_name, "i64", dim), "S/2": case.reference(S // 2, mode_name, "i64", dim),
                      "2S": case.reference(2 * S, mode_name, "i64", dim), "by place": case.reference(S, mode_name, "i64", dim, by_place=True)}
            for name, wrong in wrongs.items():
                assert len(differing(ref, wrong)) >= 4, (S, dim, mode_name, name, differing(ref, wrong))
                with pytest.raises(AssertionError):
                    oc.check_sparse(wrong[0], wrong[1], ref, name)
        ref = case.reference(S, "mean+pad", "u32", dim)
        wrong = case.reference(S, "mean+pad", "u32", dim, cnt_of=lambda cnt, bags, p: int(case.lens[bags[p]]))
        assert set(long_rows) <= set(differing(ref, wrong)), (S, dim, "cnt", differing(ref, wrong))
        with pytest.raises(AssertionError):
            oc.check_sparse(wrong[0], wrong[1], ref, "cnt")
        for mode_name in ("weighted", "weighted+pad"):
            ref = case.reference(S, mode_name, "u32", dim)
            wrong = case.reference(S, mode_name, "u32", dim, weight_at=lambda p, bags: bags[p])
            assert set(long_rows) <= set(differing(ref, wrong)), (S, dim, mode_name, differing(ref, wrong))
            with pytest.raises(AssertionError):
                oc.check_sparse(wrong[0], wrong[1], ref, "weights")
    # behind a step, on the narrow gradients: the GPU tests call check_table AND check_state, a wrong sum has to fail one of them
    dim = 4
    init = case.step_table("f32", dim)
    wrongs = lambda: (("position", case.reference(None, "mean+pad", "i64", dim, narrow=True)),  # noqa: E731
                      ("S/2", case.reference(S // 2, "mean+pad", "i64", dim, narrow=True)), ("2S", case.reference(2 * S, "mean+pad", "i64", dim, narrow=True)),
                      ("cnt", case.reference(S, "mean+pad", "i64", dim, narrow=True, cnt_of=lambda cnt, bags, p: int(case.lens[bags[p]]))))
    ref = case.reference(S, "mean+pad", "i64", dim, narrow=True)
    check_table(sr.sgd_table("f32", init, ref), sr.sgd_table("f32", init, ref).copy(), "the right table")
    for name, wrong in wrongs():
        assert rejects(check_table, sr.sgd_table("f32", init, wrong), sr.sgd_table("f32", init, ref)), (S, name, "sgd")
    for rowwise in (False, True):
        s0 = oc.init_state(case.nr_rows, dim, rowwise)
        want_table, want_state = sr.adagrad_tables("f32", init, s0, ref, rowwise)
        check_table(want_table, want_table.copy(), "the right table")
        check_state(want_state, want_state.copy(), "the right state")
        for name, wrong in wrongs():
            got_table, got_state = sr.adagrad_tables("f32", init, s0, wrong, rowwise)
            assert rejects(check_table, got_table, want_table) or rejects(check_state, got_state, want_state), (S, name, rowwise)


def rejects(check, got, want):
    try:
        check(got, want, "a wrong reference")
    except AssertionError:
        return True
    return False


# ---- the wider segment lengths ------------------------------------------------------------------------------------------------------------------
def wide_cases(S):
    if S == 64:
        return [sr.lengths_case(S, True), sr.placement_case(S, "bad"), sr.placement_case(S, "end"), sr.one_row_case(S), sr.short_case(S), sr.reduced_case(S)] + sr.multi_cases(S)
    return [sr.reduced_case(S)]


@pytest.mark.parametrize("S", sr.WIDE_SEGMENTS + sr.MID_SEGMENTS)
def test_the_wider_cases_stay_finite_in_columns_0_to_2_in_the_right_order(S):
    for case in wide_cases(S):
        assert case.S == S and case.n <= 16384
        for row in case.run_lengths():
            seen, _g = partial_sums(case, S, row)
            assert np.isfinite(seen).all() and set(np.unique(np.abs(seen)).tolist()) <= {0.0, float(oc.M)}, (case.name, row)
        rows, grads, _ = case.seg_reference(S, 4)
        assert np.isfinite(grads[:, :3]).all() and np.isfinite(grads).all(), case.name
        if max(case.run_lengths().values()) > S + 1:
            assert differing((rows, grads), case.fold(4, "sum")), case.name
    if S == 64:                                           # what the cases promise for S = 8 and 16 holds here
        case = sr.lengths_case(64, True)
        assert case.n == 5523 and sorted(case.run_lengths().values()) == sorted(sr.run_lengths(64))
        assert len(differing(case.seg_reference(64, 4), case.fold(4, "sum"))) == 7
        lay = {r: (h, k) for r, h, k in sr.sorted_layout(sr.placement_case(64, "bad"))}
        assert lay[7][0] + 2 * 64 == 328 and lay[8][0] == 331 and 328 // 64 == 331 // 64      # two segment starts in one 64-aligned block
    else:
        case = sr.reduced_case(S)
        assert sorted(case.run_lengths().values()) == sorted(sr.reduced_run_lengths(S)) and case.n == 15 * S + 14 and case.n_bad == 3
        assert -(-(9 * S + 3) // S) == 10
    if S == 1024:                                         # column 2 is NOT exact in any order here: a run's sum of p + 1 passes 2^24
        case = sr.reduced_case(S)
        exact = np.bincount(case.ids[case.good], weights=np.flatnonzero(case.good) + 1.0)
        assert exact.max() > 2 ** 24


def row_partials(C, ps, S):
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for at in range(0, len(ps), S):
            t = np.zeros(C.shape[1], F)
            for p in ps[at:at + S]:
                t = t + C[p]
            out.append(t)
    return out


def row_with_exchange(C, ps, S, partials, j):
    """The row's gradient with its occurrences j and j + 1 (1-based) exchanged: the fold of grad_seg_ref, with the segments the
    exchange does not touch taken from `partials` (their sums are what they were)."""
    ps = list(ps)
    ps[j - 1], ps[j] = ps[j], ps[j - 1]
    parts = list(partials)
    for m in {(j - 1) // S, j // S}:
        parts[m] = row_partials(C, ps[m * S:(m + 1) * S], S)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        g = parts[0]
        for t in parts[1:]:
            g = g + t
    return g


def exchange_proof(case, S, js_of):
    """For every row and every j of js_of(k): the exchange of the occurrences j and j + 1 makes column 0 or 1 infinite, and
    check_sparse rejects the result.  Returns the number of exchanges tried."""
    ref = case.seg_reference(S, 4)
    C = case.contributions(4, "sum")
    tried = 0
    for row, k in case.run_lengths().items():
        ps = [int(p) for p in case.order() if case.ids[p] == row]
        partials = row_partials(C, ps, S)
        at = int(np.flatnonzero(ref[0] == row)[0])
        assert np.array_equal(oc.bits(row_with_exchange(C, ps, S, partials, 1)), oc.bits(ref[1][at]))      # (the first pair commutes: the fold is grad_seg_ref's)
        for j in js_of(k):
            g = row_with_exchange(C, ps, S, partials, j)
            assert not np.isfinite(g[:2]).all(), (row, k, j)
            wrong = ref[1].copy()
            wrong[at] = g
            with pytest.raises(AssertionError):
                oc.check_sparse(ref[0], wrong, ref, (row, j))
            tried += 1
    return tried


def test_every_exchange_inside_a_segment_of_64_gives_inf():
    """As test_exchanging_two_neighbours_inside_a_segment_gives_inf, over EVERY run of lengths_case(64), the run of 65 S + 1
    included: every j with j and j + 1 in one segment, but the first pair of a segment."""
    S = 64
    inside = lambda k: [j for j in range(2, k) if (j - 1) // S == j // S and j % S != 1]  # noqa: E731
    tried = exchange_proof(sr.lengths_case(S, False), S, inside)
    assert tried == sum(len(inside(k)) for k in sr.run_lengths(S)) > 5000
    full = sr.fold(sr.lengths_case(S, False), S, 4, "sum", order=exchanged(sr.lengths_case(S, False), max(sr.lengths_case(S, False).run_lengths(), key=sr.lengths_case(S, False).run_lengths().get), 9 * S + 2))
    assert not np.isfinite(full[1][:, :2]).all()          # (one of them through grad_seg_ref.fold itself)


def test_sampled_exchanges_around_the_boundaries_of_segments_of_1024_give_inf():
    """The quadratic proof is too slow at S = 1024.  THE SAMPLE: in every run of reduced_case(1024), every exchange (j, j + 1)
    within two places of a segment boundary -- j mod S in {S - 2, S - 1, 0, 2, 3}: the two before it, the one across it, the two
    behind the first pair of the next segment (that pair commutes and is no other sum) -- plus 40 seeded others per run, 240 in
    all.  Every one of them changes the reference."""
    S = 1024
    rng = np.random.default_rng(1024)

    def sample(k):
        near = [j for j in range(2, k) if j % S in (S - 2, S - 1, 0, 2, 3)]
        rest = [j for j in range(2, k) if j % S not in (S - 2, S - 1, 0, 1, 2, 3)]
        return near + sorted(int(j) for j in rng.choice(rest, size=40, replace=False))

    tried = exchange_proof(sr.reduced_case(S), S, sample)
    assert tried >= 240 + 5 * 13
