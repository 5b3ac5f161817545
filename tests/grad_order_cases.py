"""Inputs and references of the order tests of the backward pass (tests/test_grad_order_cpu.py, tests/test_gpu_grad_order.py).
Nothing here runs the code under test.

THE ORDER WITNESS.  A batch of ONE-INDEX BAGS (offsets = arange(n), or offsets None with fixed_pooling = 1): the contribution of
position p is G[p], fully under the generator's control.  With j = 1, 2, ... the ordinal of p among the good positions of its row,
in position order, and M = FLT_MAX:
    column 0    +M, -M, +M, ...                   (odd j: +M)
    column 1    0 for j = 1, then +M for even j and -M for odd j
    column 2    float(p + 1): every sum exact in any order while n <= 4097 -- a dropped, doubled or foreign position shows
    columns 3+  narrow-magnitude randoms: the net for rotations and gross scrambles
In the right order every partial sum of columns 0 and 1 is 0 or +M.  Exchange the neighbouring occurrences j and j + 1, j >= 2:
for even j column 0 adds +M to +M, for odd j column 1 does; the sum is +inf and stays.  (The first pair commutes: 0 + a + b.)
Positions that are not good -- a bad id, the padding id -- hold NaN in every column: one of them read as a contribution shows.
The three coefficient paths have the same expected bits: plain sum; weighted sum with w[p] from {+1, -1} and G[p] pre-multiplied
by the same sign (a kernel that ignores w shows); mean, whose cnt is 1.
The step kernels with a state cannot carry +-M (the squares overflow): narrow=True replaces columns 0 and 1 by randoms.

The reference is fold(): a plain ordered loop acc[row] = acc[row] + c_p in float32 from +0.0f, over the list of good positions
in position order.  tests/test_grad_order_cpu.py pins it to grad_ref.sparse_grad bit for bit where n <= 600, and applies wrong
orders to that list to show that check_sparse rejects them."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402

F = np.float32
M = np.finfo(F).max
PATHS = ("sum", "weighted", "mean")
LR = F(0.1)
_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def passes_of(nr_rows):
    """Passes of the 8-bit LSD sort: the keys run up to nr_rows itself (the key of every position that is not good)."""
    return (int(nr_rows).bit_length() + 7) // 8


class Case:
    """ids int64 [n]; offsets int64 [B] (one-index bags: arange(n)); pad: the padding id or None."""

    def __init__(self, name, nr_rows, ids, offsets=None, pad=None):
        self.name, self.nr_rows, self.pad = name, int(nr_rows), pad
        self.ids = np.asarray(ids, dtype=np.int64)
        self.n = len(self.ids)
        self.one_index = offsets is None
        self.offsets = np.arange(self.n, dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
        self.B = len(self.offsets)
        self.ids.setflags(write=False)
        self.offsets.setflags(write=False)
        self.bag = np.searchsorted(self.offsets, np.arange(self.n), side="right").astype(np.int64) - 1      # -1: no bag
        in_table = (self.ids >= 0) & (self.ids < self.nr_rows)
        padding = np.zeros(self.n, bool) if pad is None else self.ids == pad
        self.good = (self.bag >= 0) & in_table & ~padding
        self.n_bad = int(((self.bag >= 0) & ~in_table & ~padding).sum())
        self.cnt = np.bincount(self.bag[(self.bag >= 0) & ~padding], minlength=self.B)
        self.seed = zlib.crc32(name.encode())
        self._cache = {}

    def order(self):
        """The good positions in position order: the list the reference folds."""
        return np.flatnonzero(self.good)

    def ordinals(self):
        """j per position: 1, 2, ... among the good positions of its row, in position order; 0 where not good."""
        j = np.zeros(self.n, dtype=np.int64)
        seen = {}
        for p in self.order():
            r = int(self.ids[p])
            seen[r] = seen.get(r, 0) + 1
            j[p] = seen[r]
        return j

    def run_lengths(self):
        """{row: number of good positions}."""
        rows, counts = np.unique(self.ids[self.good], return_counts=True)
        return dict(zip(rows.tolist(), counts.tolist()))

    def ids_array(self, width):
        return self.ids.copy() if width == "i64" else self.ids.astype(np.uint64).astype(np.uint32)

    def offsets_array(self, width):
        return self.offsets.copy() if width == "i64" else self.offsets.astype(np.uint32)

    # ---- inputs --------------------------------------------------------------------------------------------------------------
    def weights(self):
        """float32 [n] from {+1, -1}."""
        if "w" not in self._cache:
            w = np.random.default_rng(self.seed + 1).choice(np.array([1, -1], F), size=self.n)
            w.setflags(write=False)
            self._cache["w"] = w
        return self._cache["w"]

    def grads(self, dim, narrow=False, weighted=False):
        """G: float32 [B, dim] as the module's docstring says.  weighted: every row multiplied by its position's w (one-index bags).
        A case that is not of one-index bags has no good position here, and holds NaN throughout."""
        key = ("G", dim, narrow, weighted)
        if key not in self._cache:
            assert dim >= 4
            if not self.one_index:
                assert not self.good.any()
                G = np.full((self.B, dim), np.nan, dtype=F)
            else:
                G = np.random.default_rng(self.seed + 2 + dim).standard_normal((self.n, dim)).astype(F)
                G[G == 0] = F(1)
                if not narrow:
                    j = self.ordinals()
                    G[:, 0] = np.where(j % 2 == 1, M, -M)
                    G[:, 1] = np.where(j == 1, F(0), np.where(j % 2 == 0, M, -M))
                G[:, 2] = np.arange(1, self.n + 1, dtype=F)
                if weighted:
                    G = G * self.weights()[:, None]
                G[~self.good] = np.nan
            G.setflags(write=False)
            self._cache[key] = G
        return self._cache[key]

    # ---- the reference -------------------------------------------------------------------------------------------------------
    def contributions(self, dim, path, narrow=False):
        """c_p for every position, float32 [n, dim], one rounding per element (rows of positions that are not good mean nothing)."""
        assert path in PATHS
        G = self.grads(dim, narrow, weighted=path == "weighted")
        rows = G[np.clip(self.bag, 0, self.B - 1)]
        with np.errstate(**_QUIET):
            if path == "weighted":
                return self.weights()[:, None] * rows
            if path == "mean":
                return rows / self.cnt[np.clip(self.bag, 0, self.B - 1)].astype(F)[:, None]
        return rows

    def fold(self, dim, path, narrow=False, order=None):
        """(rows int64 ascending, grads float32 [|U|, dim], n_bad): acc[row] = acc[row] + c_p over `order` (default: the good
        positions in position order), from +0.0f."""
        C = self.contributions(dim, path, narrow)
        acc = {}
        with np.errstate(**_QUIET):
            for p in (self.order() if order is None else order):
                r = int(self.ids[p])
                if r not in acc:
                    acc[r] = np.zeros(dim, dtype=F)
                acc[r] = acc[r] + C[p]
        rows = np.array(sorted(acc), dtype=np.int64)
        grads = np.stack([acc[int(r)] for r in rows]) if len(rows) else np.zeros((0, dim), F)
        return rows, grads, self.n_bad

    def reference(self, dim, narrow=False):
        """fold() of the plain sum, once per (dim, narrow).  The other two paths give the same bits (test_grad_order_cpu)."""
        key = ("ref", dim, narrow)
        if key not in self._cache:
            self._cache[key] = self.fold(dim, "sum", narrow)
        return self._cache[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def check_sparse(got_rows, got_grads, want, what):
    """The assertion of every sparse comparison: |U|, the rows, and every gradient bit."""
    w_rows, w_grads = want[0], want[1]
    rows, grads = np.asarray(got_rows), np.asarray(got_grads)
    assert rows.dtype == np.int64 and grads.dtype == F, (what, rows.dtype, grads.dtype)
    assert len(rows) == len(w_rows), (what, "|U|", len(rows), len(w_rows))
    assert np.array_equal(rows, w_rows), (what, "rows")
    assert grads.shape == w_grads.shape, (what, grads.shape, w_grads.shape)
    bad = np.flatnonzero((bits(grads) != bits(w_grads)).any(axis=1))
    assert bad.size == 0, (what, "rows", rows[bad[:4]], "got", grads[bad[0]][:8], "want", w_grads[bad[0]][:8])


_cases = {}


def _once(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


# ---- run lengths around the look-ahead of eight --------------------------------------------------------------------------------
RUN_ROWS = 600
RUN_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 129)
# the lengths in ascending order of their rows: the run of 129 lies next to the run of 1 in sorted order
RUN_ROW_ORDER = (129, 1, 2, 64, 3, 7, 65, 8, 9, 63, 15, 16, 25, 17, 23, 24)
LAST_ROW = RUN_ROWS - 1
LAST_LENGTHS = (1, 7, 8, 9, 16)


def run_rows():
    """The 16 rows of RUN_ROW_ORDER, ascending, all below LAST_ROW."""
    return np.sort(np.random.default_rng(41).choice(LAST_ROW, size=len(RUN_ROW_ORDER), replace=False))


def run_case(last_len, with_bad):
    """Runs of RUN_LENGTHS over 16 rows and a run of last_len on row 599, interleaved by a seeded permutation.  without a bad id
    the run of row 599 ends exactly at n in sorted order; with_bad puts exactly one bad id behind it."""
    def make():
        ids = np.concatenate([np.full(L, r) for L, r in zip(RUN_ROW_ORDER, run_rows())] + [np.full(last_len, LAST_ROW)])
        ids = ids[np.random.default_rng(100 + last_len).permutation(len(ids))]
        if with_bad:
            ids = np.insert(ids, len(ids) // 3, RUN_ROWS)
        return Case(f"runs-last{last_len}-{'bad' if with_bad else 'clean'}", RUN_ROWS, ids)
    return _once(("run", last_len, with_bad), make)


RUN_CASES = [(L, b) for L in LAST_LENGTHS for b in (False, True)]


# ---- n on the structural boundaries --------------------------------------------------------------------------------------------
EDGE_ROWS = 70001
EDGE_NS = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)
EDGE_HOT = (7, 255, 300, 65545, 70000)      # five rows hold three quarters of the positions
EDGE_BAD = 3


def edge_case(n):
    """Five rows hold three quarters of the n positions -- their runs cross slices, wavefronts, rounds and tiles, and every slice
    holds several positions of one row; the rest are singletons spread over all id bytes of 70001 rows; three bad ids."""
    def make():
        rng = np.random.default_rng(7000 + n)
        singles = rng.choice(np.setdiff1d(np.arange(EDGE_ROWS), EDGE_HOT), size=n, replace=False)
        ids = np.where(rng.random(n) < 0.75, rng.choice(np.array(EDGE_HOT), size=n), singles)
        ids[rng.choice(n, size=EDGE_BAD, replace=False)] = [EDGE_ROWS, EDGE_ROWS + 1, 2 ** 31 + 5]
        return Case(f"edge-n{n}", EDGE_ROWS, ids)
    return _once(("edge", n), make)


# ---- sort passes ---------------------------------------------------------------------------------------------------------------
PASS_ROWS = (1, 2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1)
PASSES = {1: 1, 2: 1, 255: 1, 256: 2, 257: 2, 65535: 2, 65536: 3, 65537: 3, 2 ** 24 - 1: 3, 2 ** 24: 4, 2 ** 24 + 1: 4}


def pass_rows(nr_rows):
    """Rows 0 and nr_rows - 1, and groups that differ in one byte only, where they fit."""
    rows = {0, nr_rows - 1}
    for r in (0, 5, 200):
        rows |= {r + d for d in (0, 256, 65536, 2 ** 24) if r + d < nr_rows}
    return sorted(rows)


def pass_case(nr_rows):
    """About 300 positions: every row of pass_rows at least four times, interleaved; bad ids nr_rows and nr_rows + 1."""
    def make():
        rows = pass_rows(nr_rows)
        ids = np.tile(np.array(rows, dtype=np.int64), max(4, 296 // len(rows)))
        ids = ids[np.random.default_rng(300 + nr_rows % 1000).permutation(len(ids))]
        ids = np.insert(ids, [len(ids) // 4, len(ids) // 2, len(ids) - 1], [nr_rows, nr_rows + 1, nr_rows])
        return Case(f"passes-{nr_rows}", nr_rows, ids)
    return _once(("pass", nr_rows), make)


# ---- one long run, nothing good, a small batch --------------------------------------------------------------------------------------
LONG_N, LONG_ROW = 4096, 77


def long_case():
    return _once("long", lambda: Case("long-run", RUN_ROWS, np.full(LONG_N, LONG_ROW)))


NOTHING_N, NOTHING_PAD = 300, 17
NOTHING = ("bad", "padding", "nobag")


def nothing_case(which):
    """300 positions, none of them good: (case, what report() says)."""
    def make():
        if which == "bad":
            ids = np.random.default_rng(1).choice(np.array([RUN_ROWS, RUN_ROWS + 1, 2 ** 31, 2 ** 32 - 1]), size=NOTHING_N)
            return Case("nothing-bad", RUN_ROWS, ids)
        if which == "padding":
            return Case("nothing-padding", RUN_ROWS, np.full(NOTHING_N, NOTHING_PAD), pad=NOTHING_PAD)
        ids = np.random.default_rng(2).integers(0, RUN_ROWS + 50, size=NOTHING_N)      # good and bad ids, all before offsets[0]
        return Case("nothing-nobag", RUN_ROWS, ids, offsets=[NOTHING_N])
    return _once(("nothing", which), make)


SMALL_ROWS, SMALL_N = 255, 65


def small_case():
    """65 positions over a table of 255 rows (one pass of the sort): four rows hold most of them, one bad id."""
    def make():
        rng = np.random.default_rng(65)
        ids = np.where(rng.random(SMALL_N) < 0.7, rng.choice(np.array([0, 3, 128, 254]), size=SMALL_N), rng.integers(0, SMALL_ROWS, size=SMALL_N))
        ids[40] = SMALL_ROWS
        return Case("small-255", SMALL_ROWS, ids)
    return _once("small", make)


# ---- tables and states of the steps ---------------------------------------------------------------------------------------------
_tables = {}


def step_table(kind, nr_rows, dim):
    """uint8 [nr_rows, stride]: the host encoding of finite randoms."""
    key = (kind, nr_rows, dim)
    if key not in _tables:
        w = (np.random.default_rng(500 + dim).standard_normal((nr_rows, dim)) * 3).astype(F)
        _tables[key] = gr.encode(kind, w)
        _tables[key].setflags(write=False)
    return _tables[key]


def init_state(nr_rows, dim, rowwise):
    """Random and non-negative over some magnitudes, every fifth row 0."""
    key = ("state", nr_rows, dim, rowwise)
    if key not in _tables:
        rng = np.random.default_rng(900 + dim + rowwise)
        shape = (nr_rows,) if rowwise else (nr_rows, dim)
        s = (np.abs(rng.standard_normal(shape)) * np.exp2(rng.integers(-6, 6, size=(nr_rows,) + (1,) * (len(shape) - 1)))).astype(F)
        s[::5] = 0
        s.setflags(write=False)
        _tables[key] = s
    return _tables[key]


# ---- bag search ------------------------------------------------------------------------------------------------------------------
BAG_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257)


class BagCase:
    """B bags of seeded lengths over 600 rows: runs of empty bags, leading empty bags (several offsets are 0: position 0 belongs
    to the LAST of them) and trailing empty bags (offsets equal n).  G[b, :] = cnt(b) * (b + 1): the contributions of sum and of
    mean are small integers, exact in any order; the reference is numpy's bincount."""

    def __init__(self, B):
        rng = np.random.default_rng(8000 + B)
        lens = rng.integers(1, 5, size=B)
        if B >= 3:
            lens[0] = 0                                  # a leading empty bag
            lens[-1] = 0                                 # a trailing one
        if B >= 7:
            lens[[1, B - 2]] = 0                         # two of each
            k = 3 if B < 10 else int(rng.integers(3, B - 6))
            lens[k:k + (3 if B > 9 else 1)] = 0          # a run of empty bags inside
        if B >= 255:
            for k in rng.integers(3, B - 10, size=12):
                lens[k:k + int(rng.integers(1, 6))] = 0
            lens[[0, 1, 2, B - 3, B - 2, B - 1]] = 0
        if lens.sum() == 0:
            lens[B // 2] = 3
        self.B, self.nr_rows, self.lens = B, RUN_ROWS, lens
        self.n = int(lens.sum())
        self.offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.ids = rng.integers(0, RUN_ROWS, size=self.n).astype(np.int64)
        self.ids[rng.integers(0, self.n, size=max(1, self.n // 3))] = 11      # a row named from many bags
        self.ids[0], self.ids[-1] = 0, RUN_ROWS - 1
        self.bag = np.repeat(np.arange(B), lens)

    def grads(self, dim):
        return np.repeat((self.lens * np.arange(1, self.B + 1)).astype(F)[:, None], dim, axis=1)

    def reference(self, dim, mode):
        per_pos = (self.lens[self.bag] * (self.bag + 1)) if mode == "sum" else (self.bag + 1)
        dense = np.bincount(self.ids, weights=per_pos, minlength=self.nr_rows)
        assert dense.max() < 2 ** 24
        rows = np.unique(self.ids).astype(np.int64)
        return rows, np.repeat(dense[rows].astype(F)[:, None], dim, axis=1), 0


def bag_case(B):
    return _once(("bags", B), lambda: BagCase(B))
