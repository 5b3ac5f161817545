"""EMB_GRAD_ORDER_SEGMENTED of include/pimemb_grad.h restated as a plain loop, and the inputs of its tests
(tests/test_grad_segmented_cpu.py, tests/test_gpu_grad_segmented.py, tests/test_gpu_grad_segmented_ragged.py,
tests/test_gpu_grad_graph.py).  Nothing here runs the code under test.

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
another, and segments counted by ordinal from segments counted by sorted place.

RAGGED BAGS.  seg_sparse_grad is grad_ref.sparse_grad with the segmented fold, for bags of any shape, modes, weights, padding and
offsets[0] > 0; ragged_case(S) is the batch built for it (RaggedCase), batch_reference runs grad_cases.batch() through it.
tests/test_grad_segmented_cpu.py pins seg_sparse_grad to fold() on the one-index cases and to grad_ref where S covers every run.
WIDER SEGMENTS.  WIDE_SEGMENTS and MID_SEGMENTS: the cases above generalise to S = 64; reduced_case(S) holds a shorter set of runs
for the lengths up to 1024."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as gc  # noqa: E402
import grad_order_cases as oc  # noqa: E402
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402

F = np.float32
M = oc.M
TINY = F(2.0 ** -24)
ABSORB = 3
SEGMENTS = (8, 16)
MODES = gc.MODES
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


_bags = {}


def _bags_and_kinds(nr_rows, indices, offsets, padding_idx, n_bags, fixed_pooling):
    """grad_ref.bags_of and grad_ref.classify, remembered per batch (the plain scan costs n * B steps)."""
    ids = tuple(int(r) for r in indices)
    off = None if offsets is None else tuple(int(o) for o in offsets)
    key = (nr_rows, hash(ids), len(ids), off, padding_idx, n_bags, fixed_pooling)
    if key not in _bags:
        B = len(off) if off is not None else n_bags
        bags = gr.bags_of(len(ids), off, B, fixed_pooling)
        _bags[key] = (ids, B, bags, gr.classify(nr_rows, ids, bags, padding_idx))
    assert _bags[key][0] == ids
    return _bags[key][1:]


def seg_sparse_grad(nr_rows, indices, offsets, grad, S, mode="sum", per_sample_weights=None, padding_idx=None, n_bags=None, fixed_pooling=0,
                    cnt_of=None, weight_at=None, by_place=False):
    """grad_ref.sparse_grad with the segmented fold, for bags of any shape: (rows int64 ascending, grads float32 [|U|, dim], number
    of bad positions).  Positions are classified and cnt is counted as grad_ref does (its bags_of and classify); each row's
    contributions are collected in position order, cut into segments of S by ordinal, every segment folded from +0.0f, and the
    segment sums folded in segment order starting FROM t_0 -- float32, one rounding per operation.
    The last three arguments make WRONG references for tests/test_grad_segmented_cpu.py: cnt_of(cnt, bags, p) replaces cnt[bag(p)]
    in the mean, weight_at(p, bags) the index of w[p], by_place cuts the segments at the S-aligned sorted places of the whole
    batch instead of at the row's own ordinals."""
    assert S >= 1
    G = np.asarray(grad, dtype=F)
    n = len(indices)
    B, bags, kinds = _bags_and_kinds(nr_rows, indices, offsets, padding_idx, n_bags, fixed_pooling)
    cnt = [0] * max(B, 1)
    for p in range(n):
        if kinds[p] in ("good", "bad"):
            cnt[bags[p]] += 1
    w = None if per_sample_weights is None else np.asarray(per_sample_weights, dtype=F)
    runs = {}
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for p in range(n):                                # position order
            if kinds[p] != "good":
                continue
            g = G[bags[p]]
            if mode == "mean":
                c = g / F(cnt[bags[p]] if cnt_of is None else cnt_of(cnt, bags, p))
            elif mode == "sum":
                c = g if w is None else w[p if weight_at is None else weight_at(p, bags)] * g
            else:
                raise ValueError(mode)
            runs.setdefault(int(indices[p]), []).append(c)
        acc, place = {}, 0
        for r in sorted(runs):
            cs = runs[r]
            if by_place:                                  # (wrong) a new segment wherever the sorted place is a multiple of S
                cuts = [0] + [i for i in range(1, len(cs)) if (place + i) % S == 0] + [len(cs)]
            else:                                         # segment j: ordinals jS + 1 .. min((j + 1)S, k)
                cuts = list(range(0, len(cs), S)) + [len(cs)]
            place += len(cs)
            partials = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                t = np.zeros(G.shape[1], dtype=F)         # +0.0f
                for c in cs[a:b]:
                    t = t + c
                partials.append(t)
            g = partials[0]                               # starting FROM t_0
            for t in partials[1:]:
                g = g + t
            acc[r] = g
    rows = np.array(sorted(acc), dtype=np.int64)
    grads = np.stack([acc[int(r)] for r in rows]).astype(F) if len(rows) else np.zeros((0, G.shape[1]), F)
    return rows, grads, sum(k == "bad" for k in kinds)


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


# ---- wider segment lengths --------------------------------------------------------------------------------------------------------
WIDE_SEGMENTS = (64, 1024)           # 64: GradContext.DEFAULT_SEGMENT, with every case of S = 8 and 16; 1024: the maximum, reduced runs
MID_SEGMENTS = (32, 128, 256, 512)   # the reduced runs at one dim


def reduced_run_lengths(S):
    """On both sides of one segment, two segments and a tail, and ten partials: t_0, one full round of eight loads, one more."""
    return (S - 1, S, S + 1, S + 2, 2 * S + 1, 9 * S + 3)


def reduced_case(S):
    """The runs of reduced_run_lengths(S) over six rows of 500, interleaved by a seeded permutation, three bad ids and five
    occurrences of the padding id in between: 15 S + 14 positions, 15 374 for S = 1024.
    COLUMN 2.  grad_order_cases calls its column 2, float(p + 1), "exact in any order while n <= 4097".  That does not hold for
    the longer of these batches: from about 5 790 positions on (2^24 ~ n^2 / 2) the sum of a run's p + 1 can pass 2^24 and is
    rounded, so the column's value depends on the order like any other -- at S = 1024 the run of 9 S + 3 does
    (tests/test_grad_segmented_cpu.py asserts it).  The reference is a loop in the definition's order and stays right; the column
    still shows a dropped, doubled or foreign position, it is just no longer order-free.  (lengths_case(64), n = 5523, stays
    below 2^24.)"""
    def make():
        lengths = reduced_run_lengths(S)
        rows = np.sort(np.random.default_rng(S + 1).choice(np.setdiff1d(np.arange(LENGTH_ROWS), [LENGTH_PAD]), size=len(lengths), replace=False))
        ids = np.concatenate([np.full(L, r) for L, r in zip(lengths, rows)] + [[LENGTH_ROWS, LENGTH_ROWS + 1, 2 ** 31 + 5], np.full(5, LENGTH_PAD)])
        ids = ids[np.random.default_rng(700 + S).permutation(len(ids))]
        return SegCase(f"seg-reduced-S{S}", LENGTH_ROWS, ids, S, pad=LENGTH_PAD)
    return _once(("reduced", S), make)


# ---- ragged bags ----------------------------------------------------------------------------------------------------------------------
RAGGED_ROWS = 499
RAGGED_PAD = 17
RAGGED_SEGMENTS = (8, 16, 64)
RAGGED_TRIPLE = 250                  # the long-run row that one bag holds three times


def ragged_runs(S):
    """{long-run row: occurrences}: row 0 and the last row among them."""
    return {0: S + 2, 123: 3 * S + 5, RAGGED_TRIPLE: 8 * S + 3, 300: 4 * S + 3, 377: 2 * S, RAGGED_ROWS - 1: 2 * S + 1}


class RaggedCase:
    """One batch of about 16 S + 300 positions over a table of 499 rows, built for the segmented kernels the way
    grad_cases.batch() was built for the position order.  Bags of 0 to 13 positions (empty bags in the middle, a trailing empty
    bag, a bag of padding only); the five long-run rows of ragged_runs(S) spread over many bags, row 250 three times within bag
    TRIPLE_BAG; every long-run row also in a bag that holds a padding position (cnt != the bag's length); five bad ids of full
    width per id width (bad_ids), one of them at position 1; position 0 holds long-run row 123.  offsets(lead=True): offsets[0] = 3
    -- positions 0 .. 2 have no bag: row 123 loses an occurrence and the bad id of position 1 is NOT counted.
    grads / weights: as grad_cases makes them (many magnitudes, -0.0, denormals; weights with 0 and negatives); narrow: magnitudes
    within 2^-3 .. 2^3 for the steps that keep a state."""

    EMPTY, PAD_ONLY, TRIPLE_BAG = (3, 20, 33), 10, 25
    # the binades of a bag's gradient row: sixteen, not grad_cases' forty -- with forty one bag dominates a run's sum at dim 4 and
    # absorbs what the segment length changes (tests/test_grad_segmented_cpu.py asserts what the batch has to show)
    WIDE, NARROW = (-8, 8), (-3, 4)
    PAD_BAGS = [40, 41, 42, 43, 44, 45]                   # each holds a padding position and a long-run row

    def __init__(self, S, attempt=0):
        self.S, self.nr_rows, self.pad = int(S), RAGGED_ROWS, RAGGED_PAD
        self.name = f"ragged-S{S}"
        rng = np.random.default_rng(3000 + S + 1000 * attempt)
        runs = ragged_runs(S)
        B = -(-(16 * S + 300) * 2 // 13) | 1             # about (16 S + 300) / 6.5 bags, an odd count
        lens = rng.integers(1, 14, size=B)
        lens[list(self.EMPTY) + [B - 1]] = 0
        lens[0], lens[self.PAD_ONLY], lens[self.TRIPLE_BAG] = 5, 3, 13
        pad_bags = self.PAD_BAGS
        lens[pad_bags] = [4, 7, 11, 9, 6, 5]
        self.B, self.lens = B, lens
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        n = int(lens.sum())
        start = lambda b: int(off[b])  # noqa: E731
        common = np.setdiff1d(np.arange(RAGGED_ROWS), list(runs) + [RAGGED_PAD])
        ids = [int(v) for v in rng.choice(common[::3], size=n)]      # about 160 rows for the rest: repeats and singletons
        taken = set(range(0, 5))
        for k in range(3):
            ids[start(self.PAD_ONLY) + k] = RAGGED_PAD
            taken.add(start(self.PAD_ONLY) + k)
        placed = {r: 0 for r in runs}

        def put(p, r):
            assert p not in taken
            ids[p] = r
            taken.add(p)
            if r in placed:
                placed[r] += 1

        taken.discard(0)
        put(0, 123)                                       # (without a bag under offsets(lead=True))
        for k in (0, 5, 12):
            put(start(self.TRIPLE_BAG) + k, RAGGED_TRIPLE)
        for b, r in zip(pad_bags, list(runs)):
            put(start(b) + 1, RAGGED_PAD)
            put(start(b) + 2, r)
            if r == RAGGED_TRIPLE:
                put(start(b) + 0, RAGGED_PAD)             # two padding positions and two occurrences of row 250 in one bag
                put(start(b) + 9, r)
        for b in [self.TRIPLE_BAG] + pad_bags:            # what these bags hold of the long-run rows is what was put there
            taken.update(range(start(b), start(b) + int(lens[b])))
        free = [p for p in range(5, n) if p not in taken]
        bad_at = [1] + [int(p) for p in rng.choice(free, size=4, replace=False)]
        taken.update(bad_at)
        free = [p for p in free if p not in taken]
        spots = rng.permutation(free)
        at = 0
        for r, k in runs.items():
            need = k - placed[r]
            for p in spots[at:at + need]:
                put(int(p), r)
            at += need
        assert all(ids.count(r) == k for r, k in runs.items()) and at <= len(spots)
        self.n, self._ids, self._offsets, self.bad_at = n, ids, off, bad_at
        self._offsets.setflags(write=False)
        self._cache = {}

    def heads(self, padded, lead):
        """{long-run row: the sorted place of its first occurrence} among the good positions."""
        ids = np.array(self._ids)
        good = np.ones(self.n, bool)
        good[self.bad_at] = False
        if padded:
            good &= ids != self.pad
        if lead:
            good[:3] = False
        g = np.sort(ids[good])
        return {r: int(np.searchsorted(g, r)) for r in ragged_runs(self.S)}

    def bad_ids(self, width):
        """The ids as Python ints with the bad positions filled, per id width as grad_cases.bad_ids does: int64 -> two negative ids,
        two ids >= 2^32 whose low 32 bits name rows that carry long runs (0 and the last), and nr_rows itself."""
        ids = list(self._ids)
        nr = self.nr_rows
        vals = [-1, 2 ** 32, -(2 ** 40), 2 ** 32 + nr - 1, nr] if width == "i64" else [nr, nr + 7, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 1]
        for p, v in zip(self.bad_at, vals):
            ids[p] = v
        return ids

    def n_of(self, bags=None):
        """The positions of the first `bags` bags (None: all): a smaller batch with shorter long runs."""
        return self.n if bags is None else int(self._offsets[bags])

    def clean_ids(self, bags=None):
        """int64 ids with row 1 at the bad positions: for callers whose lookup reads the table unchecked."""
        ids = np.array(self._ids[:self.n_of(bags)], dtype=np.int64)
        ids[[p for p in self.bad_at if p < len(ids)]] = 1
        return ids

    def ids_array(self, width, bags=None):
        ids = self.bad_ids(width)[:self.n_of(bags)]
        return np.array(ids, dtype=np.int64) if width == "i64" else np.array(ids, dtype=np.uint64).astype(np.uint32)

    def offsets(self, lead=False, bags=None):
        if not lead and bags is None:
            return self._offsets
        off = self._offsets[:bags].copy()
        if lead:
            off[0] = 3
        return off

    def offsets_array(self, width, lead=False, bags=None):
        return self.offsets(lead, bags).astype(np.int64 if width == "i64" else np.uint32)

    def n_bad(self, lead=False, bags=None):
        return sum(p < self.n_of(bags) for p in self.bad_at) - (1 if lead else 0)

    def grads(self, dim, narrow=False):
        key = ("G", dim, narrow)
        if key not in self._cache:
            rng = np.random.default_rng(dim * 31 + self.S)
            lo, hi = self.NARROW if narrow else self.WIDE
            G = (rng.standard_normal((self.B, dim)) * np.exp2(rng.integers(lo, hi, size=(self.B, 1)))).astype(F)
            G[self.PAD_BAGS] = (rng.standard_normal((len(self.PAD_BAGS), dim)) * 2.0 ** (hi - 1)).astype(F)      # a wrong cnt there is not absorbed
            G[5] = -0.0
            G[6, ::2] = -0.0
            G[7] = np.array([1, 0x007FFFFF, 0x80000001, 0x00400000], dtype=np.uint32).view(F)[np.arange(dim) % 4]      # denormals
            G[8] = F(1e-39)
            G.setflags(write=False)
            self._cache[key] = G
        return self._cache[key]

    def weights(self):
        if "w" not in self._cache:
            rng = np.random.default_rng(99 + self.S)
            w = rng.choice(np.array([0.0, -1.5, 0.3, 1.7, -0.7, 2.0, 1.0, 0.1], dtype=F), size=self.n)
            w[::3] = rng.standard_normal(len(w[::3])).astype(F)
            w.setflags(write=False)
            self._cache["w"] = w
        return self._cache["w"]

    def step_table(self, kind, dim):
        """uint8 [499, stride]: the table before a step.  Small values (about 2^-10), and 0 on the long-run rows: the step's product
        is not absorbed by the weight, so the table shows the bits of the gradient that the fold decides."""
        key = ("table", kind, dim)
        if key not in self._cache:
            w = (np.random.default_rng(500 + dim).standard_normal((self.nr_rows, dim)) * 2.0 ** -10).astype(F)
            w[list(ragged_runs(self.S))] = 0
            self._cache[key] = gr.encode(kind, w)
            self._cache[key].setflags(write=False)
        return self._cache[key]

    def args(self, mode_name, width, lead=False, bags=None):
        """(ids, offsets, mode, weights or None, padding id or None) of one of grad_cases.MODES."""
        mode, weighted, padded = MODES[mode_name]
        n = self.n_of(bags)
        return self.bad_ids(width)[:n], self.offsets(lead, bags), mode, self.weights()[:n] if weighted else None, self.pad if padded else None

    def reference(self, S, mode_name, width, dim, lead=False, narrow=False, bags=None, **wrong):
        """seg_sparse_grad of the batch, once per case (S None: grad_ref.sparse_grad, the position order)."""
        key = ("ref", S, mode_name, width, dim, lead, narrow, bags) + tuple(sorted(wrong))
        if wrong or key not in self._cache:
            ids, off, mode, w, pad = self.args(mode_name, width, lead, bags)
            G = self.grads(dim, narrow)[:bags]
            if S is None:
                ref = gr.sparse_grad(self.nr_rows, ids, off, G, mode, w, pad)
            else:
                ref = seg_sparse_grad(self.nr_rows, ids, off, G, S, mode, w, pad, **wrong)
            if wrong:
                return ref
            self._cache[key] = ref
        return self._cache[key]


def ragged_case(S):
    """The first of the seeded batches in which no long-run row but row 0 starts on a multiple of S in sorted order, with and
    without padding and the leading positions: a kernel that cuts segments by sorted place then shows on every one of them."""
    def make():
        for attempt in range(100):
            case = RaggedCase(S, attempt)
            if all(h % S for padded in (False, True) for lead in (False, True) for r, h in case.heads(padded, lead).items() if r):
                return case
        raise AssertionError(S)
    return _once(("ragged", S), make)


def batch_reference(S, width, mode_name, dim, lead=False):
    """seg_sparse_grad of grad_cases.batch() -- the project's own adversarial ragged batch, one row of 140 occurrences -- once per
    case, without the overflow bags (a sum of +inf is the same in any order)."""
    def make():
        mode, weighted, padded = MODES[mode_name]
        ids, offsets = gc.bad_ids(width)
        if lead:
            offsets = gc.offsets_lead()
        return seg_sparse_grad(gc.NR_ROWS, ids, offsets, gc.grads(dim, overflow=False), S, mode, gc.weights() if weighted else None, gc.PAD if padded else None)
    return _once(("batch", S, width, mode_name, dim, lead), make)


def sorted_layout(case):
    """[(row, head place, length)] of the runs in the sorted order of the good positions."""
    out, at = [], 0
    for r, L in sorted(case.run_lengths().items()):
        out.append((r, at, L))
        at += L
    return out
