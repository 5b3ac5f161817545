"""CPU: the inputs of the order tests of the backward pass (tests/grad_order_cases.py) are what they have to be.  The WITNESS
CONDITION: in every case, for every row with at least three occurrences, every exchange of two neighbouring occurrences beyond
the first pair changes the bits of the reference -- all of them, not most.  The reference is finite where it must be, equals
tests/grad_ref.py bit for bit wherever that quadratic loop can be afforded (n <= 600), and is the same on the three coefficient
paths.  Every case holds what its name says.  And the proof that the witness works is here, not in a broken kernel: wrong orders
of the list the reference folds are rejected by the very assertion helper the GPU tests use.  No GPU work is called."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_order_cases as oc  # noqa: E402
import grad_ref as gr  # noqa: E402

F = np.float32


def witness_cases():
    """Every case that carries the witness columns."""
    return [oc.run_case(L, b) for L, b in oc.RUN_CASES] + [oc.edge_case(n) for n in oc.EDGE_NS] + [oc.pass_case(r) for r in oc.PASS_ROWS] + \
        [oc.long_case(), oc.small_case()]


def all_cases():
    return witness_cases() + [oc.nothing_case(w) for w in oc.NOTHING]


def ids_of(cases):
    return [c.name for c in cases]


# ---- the witness condition ----------------------------------------------------------------------------------------------------------
def fold_terms(X):
    """X: float32 [T, L, k], T sequences of L terms: (((+0 + x_1) + x_2) + ...) per sequence and column."""
    acc = np.zeros((X.shape[0], X.shape[2]), dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        for l in range(X.shape[1]):
            acc = acc + X[:, l]
    return acc


def transpositions_witnessed(C):
    """C: float32 [L, k], the contributions of one row in position order.  bool [L - 2]: whether the exchange of occurrences j and
    j + 1 changes a bit of the sum, for j = 2 .. L - 1."""
    L = C.shape[0]
    base = oc.bits(fold_terms(C[None]))[0]
    out = np.zeros(L - 2, dtype=bool)
    for t0 in range(0, L - 2, 256):
        T = min(256, L - 2 - t0)
        at = np.arange(t0, t0 + T) + 1                   # 0-based place of occurrence j
        idx = np.tile(np.arange(L), (T, 1))
        idx[np.arange(T), at], idx[np.arange(T), at + 1] = at + 1, at
        out[t0:t0 + T] = (oc.bits(fold_terms(C[idx])) != base).any(axis=1)
    return out


_shares = {"witness": [0, 0], "random, dim 4": [0, 0], "random, dim 8": [0, 0]}


@pytest.mark.parametrize("case", witness_cases(), ids=ids_of(witness_cases()))
def test_every_adjacent_transposition_beyond_the_first_pair_changes_the_reference(case):
    """The required share is 100 %.  Printed as well: the share the random columns alone witness (one of them at dim 4, five at
    dim 8) -- for information, nothing is required of it."""
    order = case.order()
    C4, C8 = case.contributions(4, "sum"), case.contributions(8, "sum")
    seen = dict((k, [0, 0]) for k in _shares)
    for row, length in case.run_lengths().items():
        if length < 3:
            continue
        at = order[case.ids[order] == row]
        for key, C in (("witness", C4[at][:, :2]), ("random, dim 4", C4[at][:, 3:]), ("random, dim 8", C8[at][:, 3:])):
            hit = transpositions_witnessed(C)
            assert len(hit) == length - 2
            seen[key][0] += int(hit.sum())
            seen[key][1] += len(hit)
            if key == "witness":
                assert hit.all(), (case.name, row, length, "exchanges not witnessed at j =", (np.flatnonzero(~hit) + 2)[:8])
    for key in seen:
        _shares[key][0] += seen[key][0]
        _shares[key][1] += seen[key][1]
    if seen["witness"][1]:
        print(case.name, {k: "%d of %d" % tuple(v) for k, v in seen.items()},
              "-- so far:", {k: "%.1f %%" % (100.0 * v[0] / max(v[1], 1)) for k, v in _shares.items()})
    assert seen["witness"][0] == seen["witness"][1]


def test_the_first_pair_is_exempt_because_it_commutes():
    case = oc.run_case(9, False)
    order = case.order().copy()
    first_two = np.flatnonzero(case.ids[order] == oc.LAST_ROW)[:2]
    order[first_two] = order[first_two[::-1]]
    oc.check_sparse(*case.fold(8, "sum", order=order)[:2], case.reference(8), "first pair")


# ---- the reference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", witness_cases(), ids=ids_of(witness_cases()))
def test_reference_is_finite_in_the_witness_columns_and_the_same_on_the_three_paths(case):
    for dim in (4, 5):
        rows, grads, n_bad = case.reference(dim)
        assert len(rows) == len(case.run_lengths()) and np.isfinite(grads[:, :3]).all(), case.name
        assert np.isfinite(grads).all()
        assert set(np.unique(grads[:, :2]).tolist()) <= {0.0, float(oc.M)}
        for path in ("weighted", "mean"):
            oc.check_sparse(*case.fold(dim, path)[:2], (rows, grads), (case.name, dim, path))
    # column 2 is the exact sum of p + 1 over the row's positions: nothing dropped, doubled or foreign
    rows, grads, _ = case.reference(4)
    want = np.bincount(case.ids[case.good], weights=np.flatnonzero(case.good) + 1.0, minlength=0)
    assert np.array_equal(grads[:, 2].astype(np.float64), want[rows]) and want.max() < 2 ** 24
    # the weighted path's G really differs from the plain one: a kernel that ignores w shows
    if case.n > 8:
        assert not np.array_equal(oc.bits(case.grads(4, weighted=True)[case.good]), oc.bits(case.grads(4)[case.good]))
    # the narrow variant (for the steps with a state): no +-M anywhere, squares stay finite
    rows_n, grads_n, _ = case.reference(8, narrow=True)
    assert np.array_equal(rows_n, rows) and np.isfinite(grads_n * grads_n).all() and np.abs(case.grads(8, narrow=True)[case.good][:, :2]).max() < 10


@pytest.mark.parametrize("case", [c for c in all_cases() if c.n <= 600], ids=ids_of([c for c in all_cases() if c.n <= 600]))
def test_reference_equals_grad_ref_bit_for_bit(case):
    assert case.n <= 600
    for dim, path, fixed in ((4, "sum", False), (5, "weighted", False), (8, "mean", False), (4, "mean", True), (8, "sum", True)):
        if fixed and not case.one_index:
            continue
        G = case.grads(dim, weighted=path == "weighted")
        kw = dict(n_bags=case.n, fixed_pooling=1) if fixed else {}
        want = gr.sparse_grad(case.nr_rows, case.ids.tolist(), None if fixed else case.offsets, G, "mean" if path == "mean" else "sum",
                              case.weights() if path == "weighted" else None, case.pad, **kw)
        got = case.fold(dim, path)
        assert got[2] == want[2] == case.n_bad
        oc.check_sparse(got[0], got[1], want, (case.name, dim, path, fixed))
    got = case.fold(8, "sum", narrow=True)
    oc.check_sparse(got[0], got[1], gr.sparse_grad(case.nr_rows, case.ids.tolist(), case.offsets, case.grads(8, narrow=True), padding_idx=case.pad), "narrow")


@pytest.mark.parametrize("B", oc.BAG_COUNTS)
def test_bag_search_cases_hold_their_edges_and_equal_grad_ref(B):
    case = oc.bag_case(B)
    assert len(case.offsets) == B and case.offsets[0] == 0 and (np.diff(case.offsets) >= 0).all() and case.n >= 1
    if B >= 3:
        assert case.lens[0] == 0 and case.offsets[-1] == case.n          # a leading and a trailing empty bag
    if B >= 7:
        assert (case.offsets == 0).sum() >= 3 and (case.offsets == case.n).sum() >= 2      # several offsets are 0; several equal n
        runs = np.flatnonzero(case.lens[2:-2] == 0)
        assert runs.size >= 1
    if B >= 10:
        z = case.lens[3:-3] == 0
        assert (z[:-1] & z[1:]).any()                                     # a run of empty bags inside
    assert case.n < 20 or (case.ids == 11).sum() >= 3                     # a row named from many bags
    for dim in (4, 5):
        for mode in ("sum", "mean"):
            want = gr.sparse_grad(case.nr_rows, case.ids.tolist(), case.offsets, case.grads(dim), mode)
            got = case.reference(dim, mode)
            assert want[2] == 0
            oc.check_sparse(got[0], got[1], want, (B, dim, mode))


# ---- inventory --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last_len,with_bad", oc.RUN_CASES)
def test_run_length_cases_hold_their_runs(last_len, with_bad):
    case = oc.run_case(last_len, with_bad)
    runs = case.run_lengths()
    rows = sorted(runs)
    assert case.nr_rows == 600 and case.n <= 600 and case.one_index
    assert rows[-1] == oc.LAST_ROW == case.nr_rows - 1 and runs[oc.LAST_ROW] == last_len          # the last run of the sorted order
    assert sorted(runs[r] for r in rows[:-1]) == sorted(oc.RUN_LENGTHS) == sorted(oc.RUN_ROW_ORDER)
    assert [runs[r] for r in rows[:-1]] == list(oc.RUN_ROW_ORDER) and oc.RUN_ROW_ORDER[:2] == (129, 1)      # 129 next to 1
    assert int((~case.good).sum()) == case.n_bad == (1 if with_bad else 0)                         # what follows the last run
    assert case.n == sum(oc.RUN_LENGTHS) + last_len + case.n_bad
    # interleaved: no row's positions are all consecutive (but the singletons')
    order = case.order()
    for r in rows:
        at = order[case.ids[order] == r]
        assert len(at) < 3 or at[-1] - at[0] >= 2 * len(at), (r, at[:4])


@pytest.mark.parametrize("n", oc.EDGE_NS)
def test_boundary_cases_hold_their_runs_and_singletons(n):
    case = oc.edge_case(n)
    runs = case.run_lengths()
    assert case.n == n and case.nr_rows == 70001 and case.n_bad == oc.EDGE_BAD and int((~case.good).sum()) == oc.EDGE_BAD
    hot = sum(runs.get(r, 0) for r in oc.EDGE_HOT)
    assert 0.6 * n <= hot <= 0.9 * n, (hot, n)                            # three quarters, as drawn
    assert all(runs.get(r, 0) >= 3 for r in oc.EDGE_HOT)
    assert all(v == 1 for r, v in runs.items() if r not in oc.EDGE_HOT)  # the rest are singletons
    for s in range(n // 64):                                              # every full slice holds several positions of one row
        ids = case.ids[64 * s:64 * s + 64]
        assert max((ids == r).sum() for r in oc.EDGE_HOT) >= 3, s
    single = np.array([r for r in runs if r not in oc.EDGE_HOT])
    assert {r >> 16 for r in oc.EDGE_HOT} == {0, 1} and len({r & 255 for r in oc.EDGE_HOT}) == 5
    if n >= 255:
        assert set((single >> 16).tolist()) == {0, 1} and len(set((single & 255).tolist())) > 30 and len(set(((single >> 8) & 255).tolist())) > 30


@pytest.mark.parametrize("nr_rows", oc.PASS_ROWS)
def test_sort_pass_cases_hold_their_rows(nr_rows):
    case = oc.pass_case(nr_rows)
    runs = case.run_lengths()
    assert oc.passes_of(nr_rows) == oc.PASSES[nr_rows]
    # at a byte boundary the key nr_rows of a position that is not good needs one more pass than the largest row id
    assert (oc.passes_of(nr_rows) == oc.passes_of(nr_rows - 1) + 1) == (nr_rows in (1, 256, 65536, 2 ** 24))
    assert 0 in runs and nr_rows - 1 in runs and min(runs.values()) >= 4 and max(runs) == nr_rows - 1
    assert 250 <= case.n <= 350 and case.n_bad == 3 and {nr_rows, nr_rows + 1} <= set(case.ids.tolist())
    for d in (256, 65536, 2 ** 24):
        assert (5 + d in runs) == (5 + d < nr_rows)
    if nr_rows > 2 ** 24:
        assert {0, 256, 65536, 2 ** 24} <= set(runs)                       # (2^24 is the last row of 2^24 + 1)
    order = case.order()
    at = order[case.ids[order] == 0]
    assert len(runs) <= 2 or at[-1] - at[0] > 2 * len(at)                 # interleaved


def test_the_other_cases_hold_what_their_names_say():
    long = oc.long_case()
    assert long.n == 4096 and long.run_lengths() == {oc.LONG_ROW: 4096} and long.n_bad == 0
    for which, n_bad in zip(oc.NOTHING, (300, 0, 0)):
        case = oc.nothing_case(which)
        assert case.n == 300 and not case.good.any() and case.n_bad == n_bad, which
        assert np.isnan(case.grads(8)).all() and len(case.fold(8, "sum")[0]) == 0
    assert oc.nothing_case("nobag").B == 1 and (oc.nothing_case("nobag").bag == -1).all()
    assert (oc.nothing_case("padding").ids == oc.NOTHING_PAD).all()
    small = oc.small_case()
    assert small.n == 65 and small.nr_rows == 255 and oc.passes_of(255) == 1 and small.n_bad == 1 and max(small.run_lengths().values()) >= 9
    # positions that are not good hold NaN in every column, on every path's G
    edge = oc.edge_case(257)
    for weighted in (False, True):
        G = edge.grads(8, weighted=weighted)
        assert np.isnan(G[~edge.good]).all() and not np.isnan(G[edge.good]).any()


# ---- the proof that the witness works: wrong orders are rejected -------------------------------------------------------------------
def neighbours(case, want):
    """(place of occurrence j in case.order(), place of occurrence j + 1) of some row, j >= 2, chosen by want(j, p, q)."""
    order = case.order()
    for row, length in sorted(case.run_lengths().items(), key=lambda kv: -kv[1]):
        places = np.flatnonzero(case.ids[order] == row)
        for k in range(1, length - 1):                                    # occurrence j = k + 1
            if want(k + 1, int(order[places[k]]), int(order[places[k + 1]])):
                return int(places[k]), int(places[k + 1])
    return None


EXCHANGES = {
    "inside a slice": lambda j, p, q: j != 8 and p // 64 == q // 64,
    "across a slice boundary": lambda j, p, q: j != 8 and p // 64 != q // 64,
    "across the 8th / 9th occurrence": lambda j, p, q: j == 8,
}


@pytest.mark.parametrize("what", list(EXCHANGES))
@pytest.mark.parametrize("case", [oc.edge_case(257), oc.edge_case(4097), oc.run_case(9, False), oc.run_case(16, True)],
                         ids=["edge-257", "edge-4097", "runs-last9", "runs-last16-bad"])
def test_the_assertion_helper_rejects_a_wrong_order(case, what):
    pair = neighbours(case, EXCHANGES[what])
    assert pair is not None, (case.name, what)
    order = case.order().copy()
    order[[pair[0], pair[1]]] = order[[pair[1], pair[0]]]
    for dim in (4, 8, 5):
        for path in oc.PATHS:
            wrong = case.fold(dim, path, order=order)
            with pytest.raises(AssertionError):
                oc.check_sparse(wrong[0], wrong[1], case.reference(dim), (case.name, what, dim, path))
            # ... and on the witness columns alone: the random columns and column 2 are not what rejects it
            assert not np.array_equal(oc.bits(wrong[1][:, :2]), oc.bits(case.reference(dim)[1][:, :2]))
            assert np.array_equal(oc.bits(wrong[1][:, 2]), oc.bits(case.reference(dim)[1][:, 2]))
    right = case.fold(8, "sum", order=case.order())
    oc.check_sparse(right[0], right[1], case.reference(8), "the right order")


def test_the_assertion_helper_rejects_a_dropped_a_doubled_and_a_foreign_position():
    case = oc.edge_case(257)
    order, ref = case.order(), case.reference(4)
    hot_at = np.flatnonzero(case.ids[order] == oc.EDGE_HOT[0])
    for name, wrong_order in (("dropped", np.delete(order, hot_at[4])), ("doubled", np.insert(order, hot_at[4], order[hot_at[4]])),
                              ("last dropped", np.delete(order, hot_at[-1]))):
        wrong = case.fold(4, "sum", order=wrong_order)
        with pytest.raises(AssertionError):
            oc.check_sparse(wrong[0], wrong[1], ref, name)
        assert wrong[1][list(wrong[0]).index(oc.EDGE_HOT[0]), 2] != ref[1][list(ref[0]).index(oc.EDGE_HOT[0]), 2]      # column 2 shows it
    # a position that is not good, read: NaN
    wrong = case.fold(4, "sum", order=np.sort(np.append(order, np.flatnonzero(~case.good)[0])))
    with pytest.raises(AssertionError):
        oc.check_sparse(wrong[0], wrong[1], ref, "foreign")
