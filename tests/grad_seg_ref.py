"""EMB_GRAD_ORDER_SEGMENTED of include/pimemb_grad.h restated as a plain loop, and the inputs of its tests
(tests/test_grad_segmented_cpu.py, tests/test_gpu_grad_segmented.py).  Nothing here runs the code under test.

THE REFERENCE.  fold(case, S, ...): for every row, its good positions in position order are cut into segments of S by their
ORDINAL within the row; a segment is folded from +0.0f in position order, and the row's gradient is the fold of the segments'
sums in segment order, starting FROM the first sum -- float32, one rounding per addition.  sgd_table / adagrad_tables apply
grad_ref's and optim_ref's steps to that g.

THE INPUTS.  SegCase is grad_order_cases.Case (one-index bags, the +-FLT_MAX witness in columns 0 and 1, the exact column 2, NaN
wherever a position is not good), built for one segment length S, with two changes.
COLUMN 1 follows the segments.  grad_order_cases' column 1 (0 at ordinal 1, then +M at even and -M at odd ordinals) is finite under
the segmented order, but in every segment behind the first it runs -M, 0, -M, 0, ... in step with column 0's +M, 0, +M, 0, ...:
after an even number of a segment's elements BOTH columns stand at 0, and the exchange of the next two elements overflows neither
-- half of the exchanges inside the segments 1, 2, ... would pass unseen.  Here, with i = 0, 1, ... the place of an occurrence
inside its segment m:  column 1 = 0 at i = 0, else s_m * (+M for odd i, -M for even i), s_m = +1 for even m and -1 for odd m.
Segment 0 is grad_order_cases' pattern.  Inside every segment column 0 stands at +M after an odd number of elements and column 1
at s_m * M after an even number (>= 2): every exchange of two neighbours inside a segment, but its first pair (0 + a + b is
0 + b + a), adds M to M in one of the two.  A full segment sums to 0 in column 0 and to s_m * M in column 1, so across the
segments column 1 runs +M, 0, +M, 0, ...: every partial sum is finite in the right order.
ONE MORE COLUMN, the ABSORB column 3: 1.0f at ordinal 1 of a row and 2^-24 at every other ordinal.  In the position order every
2^-24 is absorbed by the 1.0 before it (a tie, rounded to even): the sum is exactly 1.0.
In the segmented order the segments 1, 2, ... sum their own 2^-24s first, and those sums are not absorbed: the result is above
1.0, by an amount that depends on S -- so the column tells a kernel that ignores the order from one that follows it, one S from
another, and segments counted by ordinal from segments counted by sorted place."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_order_cases as oc  # noqa: E402
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402

F = np.float32
M = oc.M
TINY = F(2.0 ** -24)
ABSORB = 3
SEGMENTS = (8, 16)
LR, EPS = oc.LR, F(1e-10)


class SegCase(oc.Case):
    """A grad_order_cases.Case for segment length S: column 1 follows the segments, column 3 is the absorb column."""

    def __init__(self, name, nr_rows, ids, S, pad=None):
        super().__init__(name, nr_rows, ids, pad=pad)
        self.S = int(S)

    def grads(self, dim, narrow=False, weighted=False):
        key = ("G", dim, narrow, weighted)
        if key not in self._cache:
            assert dim >= 4 and self.one_index
            G = np.random.default_rng(self.seed + 2 + dim).standard_normal((self.n, dim)).astype(F)
            G[G == 0] = F(1)
            j = self.ordinals()
            if not narrow:
                G[:, 0] = np.where(j % 2 == 1, M, -M)
                m, i = (j - 1) // self.S, (j - 1) % self.S
                G[:, 1] = np.where(i == 0, F(0), np.where(m % 2 == 0, F(1), F(-1)) * np.where(i % 2 == 1, M, -M))
            G[:, 2] = np.arange(1, self.n + 1, dtype=F)
            G[:, ABSORB] = np.where(j == 1, F(1), TINY)
            if weighted:
                G = G * self.weights()[:, None]
            G[~self.good] = np.nan
            G.setflags(write=False)
            self._cache[key] = G
        return self._cache[key]

    def seg_reference(self, S, dim, narrow=False):
        """fold() of the plain sum in the segmented order, once per (S, dim, narrow)."""
        key = ("seg", S, dim, narrow)
        if key not in self._cache:
            self._cache[key] = fold(self, S, dim, "sum", narrow)
        return self._cache[key]


def fold(case, S, dim, path, narrow=False, order=None):
    """(rows int64 ascending, grads float32 [|U|, dim], n_bad): the definition.  `order` (default: the good positions in
    position order) is the list the ordinals are counted in -- a wrong list is a wrong order."""
    assert S >= 1
    C = case.contributions(dim, path, narrow)
    runs = {}
    for p in (case.order() if order is None else order):
        runs.setdefault(int(case.ids[p]), []).append(int(p))
    acc = {}
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for r, ps in runs.items():
            partials = []
            for at in range(0, len(ps), S):               # segment j: ordinals jS + 1 .. min((j + 1)S, k)
                t = np.zeros(dim, dtype=F)                # +0.0f
                for p in ps[at:at + S]:                   # position order inside the segment
                    t = t + C[p]
                partials.append(t)
            g = partials[0]                               # starting FROM t_0
            for t in partials[1:]:                        # segment order
                g = g + t
            acc[r] = g
    rows = np.array(sorted(acc), dtype=np.int64)
    grads = np.stack([acc[int(r)] for r in rows]) if len(rows) else np.zeros((0, dim), F)
    return rows, grads, case.n_bad


def sgd_table(kind, init, ref, lr=LR):
    return gr.sgd_step(kind, init, ref[0], ref[1], lr)


def adagrad_tables(kind, init, s0, ref, rowwise, lr=LR, eps=EPS):
    return orf.adagrad_step(kind, init, s0, ref[0], ref[1], lr, eps, rowwise=rowwise)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
_cases = {}


def _once(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def run_lengths(S):
    """On both sides of one segment, of two, a short last segment, nine partials (t_0 and one full round of eight loads), 66."""
    return (S - 1, S, S + 1, S + 2, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 5, 8 * S + 3, 65 * S + 1)


LENGTH_ROWS = 500
LENGTH_PAD = 77


def lengths_case(S, dirty=True):
    """The runs of run_lengths(S) over ten rows spread over 500, interleaved by a seeded permutation.  dirty: three bad ids and
    five occurrences of the padding id in between."""
    def make():
        rows = np.sort(np.random.default_rng(S).choice(np.setdiff1d(np.arange(LENGTH_ROWS), [LENGTH_PAD]), size=len(run_lengths(S)), replace=False))
        ids = np.concatenate([np.full(L, r) for L, r in zip(run_lengths(S), rows)])
        if dirty:
            ids = np.concatenate([ids, [LENGTH_ROWS, LENGTH_ROWS + 1, 2 ** 31 + 5], np.full(5, LENGTH_PAD)])
        ids = ids[np.random.default_rng(200 + S).permutation(len(ids))]
        return SegCase(f"seg-lengths-S{S}-{'dirty' if dirty else 'clean'}", LENGTH_ROWS, ids, S, pad=LENGTH_PAD if dirty else None)
    return _once(("lengths", S, dirty), make)


PLACE_ROWS = 300


def placement_lengths(S):
    """{row: run length} in sorted order: a long run, a short run between two long ones, a run of 2S + 3 directly followed by a
    run of 2S (row 7's head lies at sorted place 3S + 8, so its last segment starts at 5S + 8 and row 8's head at 5S + 11: one
    S-aligned block for S = 8 and S = 16), some short runs, and a long run on the last row."""
    return {5: 3 * S + 5, 6: 3, 7: 2 * S + 3, 8: 2 * S, 100: 2, 200: S, PLACE_ROWS - 1: 4 * S + 1}


def placement_case(S, tail):
    """tail "bad": three bad ids -- the last row's long run ends the good positions and the keys of the positions that are not
    good follow it directly; tail "end": none -- the long run ends the array."""
    def make():
        ids = np.concatenate([np.full(L, r) for r, L in placement_lengths(S).items()])
        if tail == "bad":
            ids = np.concatenate([ids, [PLACE_ROWS, PLACE_ROWS + 7, 2 ** 31 + 3]])      # (every id fits uint32: the cases run at both widths)
        ids = ids[np.random.default_rng(300 + S).permutation(len(ids))]
        return SegCase(f"seg-places-S{S}-{tail}", PLACE_ROWS, ids, S)
    return _once(("places", S, tail), make)


ONE_ROW_N, ONE_ROW = 4097, 123


def one_row_case(S):
    """One row holds every position: 4097 occurrences, 513 segments of 8."""
    return _once(("one-row", S), lambda: SegCase(f"seg-one-row-S{S}", LENGTH_ROWS, np.full(ONE_ROW_N, ONE_ROW), S))


def short_case(S):
    """Every run has at most S + 1 occurrences: the segmented order IS the position order."""
    def make():
        lengths = (1, 2, 3, 7, S - 1, S, S + 1, S + 1, S, 5)
        rows = np.sort(np.random.default_rng(50 + S).choice(LENGTH_ROWS, size=len(lengths), replace=False))
        ids = np.concatenate([np.full(L, r) for L, r in zip(lengths, rows)] + [[LENGTH_ROWS + 2]])
        return SegCase(f"seg-short-S{S}", LENGTH_ROWS, ids[np.random.default_rng(60 + S).permutation(len(ids))], S)
    return _once(("short", S), make)


MULTI_ROWS = (40, 40, 40)


def multi_cases(S):
    """Three tables' batches: row 0 and the last row of each carry long runs, so that in the composite keys of a group the long
    run of table k's last row lies directly before the long run of table k + 1's row 0; short runs in between, a bad id each."""
    def make():
        out = []
        for k, nr in enumerate(MULTI_ROWS):
            lengths = {0: 2 * S + 1 + k, nr - 1: 3 * S + 2 + k, 7: S, 9: 3, 20 + k: S + 1}
            ids = np.concatenate([np.full(L, r) for r, L in lengths.items()] + [[nr + k]])
            out.append(SegCase(f"seg-multi-S{S}-t{k}", nr, ids[np.random.default_rng(400 + 10 * S + k).permutation(len(ids))], S))
        return out
    return _once(("multi", S), make)


def sorted_layout(case):
    """[(row, head place, length)] of the runs in the sorted order of the good positions."""
    out, at = [], 0
    for r, L in sorted(case.run_lengths().items()):
        out.append((r, at, L))
        at += L
    return out
