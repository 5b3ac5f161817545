"""Inputs of the backward-pass tests (tests/test_grad_cpu.py, tests/test_gpu_grad.py) and their references, computed once each by
tests/grad_ref.py and never changed.  One batch of about 2 000 positions in 301 bags over a table of 3001 rows, built to break
the kernels (see batch()); a second, EXACT batch for the comparison with torch, in which every sum, product and quotient is
exact in fp32 in any order.  Nothing here runs the code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import rows_cases as rc  # noqa: E402

NR_ROWS = rc.NR_ROWS     # 3001
N_BAGS = 301
PAD = 17                 # the padding row
HOT = 1234               # the row that occurs 140 times
N_HOT = 140
LR = np.float32(0.1)     # no power of two: every rounding counts
MODES = {                # name -> (mode, weighted, padding)
    "sum": ("sum", False, False), "weighted": ("sum", True, False), "sum+pad": ("sum", False, True),
    "weighted+pad": ("sum", True, True), "mean": ("mean", False, False), "mean+pad": ("mean", False, True)}
# special rows: each occurs exactly once, alone in a bag of its own, with a gradient crafted (sum and mean mode: g = G) so that
# the step on the table value of step_table() lands on a rounding tie of the dtype, in its subnormal range, beyond its largest
# finite value
SPECIAL = {("f16", "tie"): 2001, ("f16", "sub"): 2002, ("f16", "over"): 2003, ("bf16", "tie"): 2004, ("bf16", "sub"): 2005,
           ("bf16", "over"): 2006}
_F16_MAX, _BF16_MAX = 65504.0, float(np.uint32(0x7F7F0000).view(np.float32))
# (table value, the product lr * g wanted): W - product is the tie 1 + half an ulp; 1.5 quanta of the subnormal range; the
# largest finite value plus three quarters of its ulp
_SPECIAL_W_P = {("f16", "tie"): (1.0, -(2.0 ** -11)), ("f16", "sub"): (0.0, -1.5 * 2.0 ** -24), ("f16", "over"): (_F16_MAX, -24.0),
                ("bf16", "tie"): (1.0, -(2.0 ** -8)), ("bf16", "sub"): (0.0, -1.5 * 2.0 ** -133), ("bf16", "over"): (_BF16_MAX, -(2.0 ** 119) * 1.5)}


def grad_for_product(product, lr=LR):
    """An fp32 g with fl(lr * g) == product exactly (lr < 1: the map is onto; the quotient's neighbours are searched)."""
    want = np.float32(product)
    g = np.float32(np.float64(want) / np.float64(lr))
    for _ in range(64):
        got = np.float32(lr) * g
        if got == want:
            return g
        g = np.nextafter(g, np.float32(np.inf) if got < want else np.float32(-np.inf))
    raise AssertionError(product)


_cache = {}


def batch():
    """(ids as Python ints [n], offsets int64 [301], positions of the bad ids).  Holds: empty bags (3, 77, 150) and a trailing
    empty bag (300); a bag of padding only (10) and two more padding positions; rows 0 and 3000; row HOT 140 times, over many
    bags and five times within bag 40; rows that occur exactly once (the special rows among them); five positions for bad ids
    (bad_ids() fills them per id width), one of them position 1, which offsets_lead() leaves without a bag."""
    if "batch" in _cache:
        return _cache["batch"]
    rng = np.random.default_rng(2024)
    lens = rng.integers(1, 14, size=N_BAGS)
    lens[[3, 77, 150, 300]] = 0
    lens[0] = 4
    lens[10] = 3
    lens[40] = 12
    special_bags = list(range(200, 200 + len(SPECIAL)))
    lens[special_bags] = 1
    lens[[20, 21]] = 4
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    n = int(lens.sum())
    common = np.setdiff1d(np.arange(NR_ROWS), [0, 3000, PAD, HOT, 5, 2999] + list(SPECIAL.values()) + list(range(2100, 2110)))
    ids = [int(v) for v in rng.choice(common[:900], size=n)]          # 900 rows for ~2 000 positions: repeats and singletons
    start = lambda b: int(offsets[b])
    for k in range(3):
        ids[start(10) + k] = PAD
    ids[start(30) + 0], ids[start(55)] = PAD, PAD
    for k, (_key, row) in enumerate(SPECIAL.items()):
        ids[start(special_bags[k])] = row
    # bags 20 and 21 (the overflow bags of grads()): row 5 once each, and rows that occur nowhere else
    for b, base in ((20, 2100), (21, 2104)):
        ids[start(b)] = 5
        for k in range(1, 4):
            ids[start(b) + k] = base + k
    ids[start(1)], ids[start(299)], ids[start(2)] = 0, 3000, 2999
    free = [p for b in range(N_BAGS) if b not in (10, 20, 21, 40, 30, 55, 1, 2, 299) and b not in special_bags for p in range(start(b), start(b) + int(lens[b]))]
    hot_at = [int(p) for p in rng.choice(free[8:], size=N_HOT - 5, replace=False)]
    for p in hot_at:
        ids[p] = HOT
    for k in (0, 3, 4, 7, 11):
        ids[start(40) + k] = HOT
    bad_at = [1] + [p for p in free[8:] if p not in hot_at][100:900:200]
    assert len(bad_at) == 5 and ids.count(HOT) == N_HOT and ids.count(2999) == 1 and 1900 <= n <= 2200, (len(bad_at), ids.count(HOT), n)
    _cache["batch"] = (ids, offsets, bad_at)
    return _cache["batch"]


def bad_ids(width):
    """The batch with its bad positions filled: int64 -> two negative ids, two ids >= 2^32 whose low 32 bits name held rows (5 and
    3000), and nr_rows itself; uint32 -> nr_rows, nr_rows + 7, two ids near 2^31 and 2^32 - 1."""
    ids, offsets, bad_at = batch()
    ids = list(ids)
    vals = [-1, 2 ** 32 + 5, -(2 ** 40), 2 ** 32 + 3000, NR_ROWS] if width == "i64" else [NR_ROWS, NR_ROWS + 7, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 1]
    for p, v in zip(bad_at, vals):
        ids[p] = v
    return ids, offsets


def ids_array(ids, width):
    return np.array(ids, dtype=np.int64) if width == "i64" else np.array(ids, dtype=np.uint64).astype(np.uint32)


def offsets_lead():
    """The variant with offsets[0] > 0: positions 0 .. 2 belong to no bag (position 1 holds a bad id, which is then NOT counted)."""
    off = batch()[1].copy()
    off[0] = 3
    return off


def grads(dim, overflow=True):
    """G: float32 [301, dim].  Randoms over many magnitudes, -0.0, fp32 denormals; bags 20 and 21 hold 3e38 in column 0, so row 5
    (once in each, with nothing else) sums to +inf; the special bags hold the crafted values.  No infinity, no NaN."""
    key = ("grads", dim, overflow)
    if key not in _cache:
        rng = np.random.default_rng(dim * 31 + 7)
        G = (rng.standard_normal((N_BAGS, dim)) * np.exp2(rng.integers(-20, 20, size=(N_BAGS, 1)))).astype(np.float32)
        G[5] = -0.0
        G[6, ::2] = -0.0
        G[7] = np.array([1, 0x007FFFFF, 0x80000001, 0x00400000], dtype=np.uint32).view(np.float32)[np.arange(dim) % 4]      # denormals
        G[8] = np.float32(1e-39)
        if overflow:
            G[20, 0] = G[21, 0] = np.float32(3e38)
        for k, key2 in enumerate(SPECIAL):
            G[200 + k] = grad_for_product(_SPECIAL_W_P[key2][1])
        G.setflags(write=False)
        _cache[key] = G
    return _cache[key]


def weights():
    """float32 [n]: 0, negatives, non-powers of two; the two positions of row 5 in the overflow bags keep a positive weight."""
    if "weights" not in _cache:
        ids, offsets, _ = batch()
        rng = np.random.default_rng(99)
        w = rng.choice(np.array([0.0, -1.5, 0.3, 1.7, -0.7, 2.0, 1.0, 0.1], dtype=np.float32), size=len(ids))
        w[::3] = rng.standard_normal(len(w[::3])).astype(np.float32)
        w[int(offsets[20])] = w[int(offsets[21])] = np.float32(1.3)
        w.setflags(write=False)
        _cache["weights"] = w
    return _cache["weights"]


def step_table(kind, dim):
    """uint8 [3001, stride]: the table before a step -- the host encoding of finite randoms, the special rows holding the
    values their crafted gradients go with."""
    key = ("table", kind, dim)
    if key not in _cache:
        rng = np.random.default_rng(500 + dim)
        w = (rng.standard_normal((NR_ROWS, dim)) * 3).astype(np.float32)
        for (k, _cls), row in SPECIAL.items():
            if k == kind:
                w[row] = np.float32(_SPECIAL_W_P[(k, _cls)][0])
        _cache[key] = gr.encode(kind, w)
        _cache[key].setflags(write=False)
    return _cache[key]


def reference(width, mode_name, dim, lead=False, overflow=True):
    """(rows, grads, n_bad) of the batch by grad_ref, once per case."""
    key = ("ref", width, mode_name, dim, lead, overflow)
    if key not in _cache:
        mode, weighted, padded = MODES[mode_name]
        ids, offsets = bad_ids(width)
        if lead:
            offsets = offsets_lead()
        _cache[key] = gr.sparse_grad(NR_ROWS, ids, offsets, grads(dim, overflow), mode, weights() if weighted else None, PAD if padded else None)
    return _cache[key]


# ---- the exact batch ---------------------------------------------------------------------------------------------------------
EXACT_ROWS, EXACT_BAGS = 257, 64


def exact_batch(padded):
    """(ids int64 [n], offsets int64 [64], G float32 [64, dim = 8], weights float32 [n]): small-integer gradients, power-of-two
    weights, 1 / 2 / 4 / 8 non-padding positions per bag (padded: plus padding positions, and a bag of padding only), ids drawn
    from 40 rows so that rows repeat.  Every sum, product and quotient is exact in fp32, in any order.  No gradient is zero: a
    contribution of -0.0 is the one value on which an order shows even here (the definition's sum starts from +0.0f and gives +0.0,
    a lone -0.0 copied through stays -0.0)."""
    key = ("exact", padded)
    if key not in _cache:
        rng = np.random.default_rng(5)
        ids, offsets = [], []
        for b in range(EXACT_BAGS):
            offsets.append(len(ids))
            k = int(rng.choice([1, 2, 4, 8]))
            bag = [int(v) for v in rng.choice(np.setdiff1d(np.arange(40) * 6, [PAD]), size=k)]
            if padded and b % 5 == 0:
                bag.insert(int(rng.integers(0, k + 1)), PAD)
            if padded and b == 7:
                bag = [PAD, PAD]
            ids += bag
        ids[0], ids[-1] = 0, EXACT_ROWS - 1
        G = (rng.integers(1, 9, size=(EXACT_BAGS, 8)) * rng.choice([-1, 1], size=(EXACT_BAGS, 8))).astype(np.float32)
        w = np.exp2(rng.integers(-2, 3, size=len(ids))).astype(np.float32) * rng.choice(np.array([-1, 1], np.float32), size=len(ids))
        _cache[key] = (np.array(ids, dtype=np.int64), np.array(offsets, dtype=np.int64), G, w)
    return _cache[key]


def exact_table():
    """float32 [257, 8]: small integers (so that w - 0.5 * g is exact)."""
    if "exact_table" not in _cache:
        _cache["exact_table"] = np.random.default_rng(6).integers(-64, 65, size=(EXACT_ROWS, 8)).astype(np.float32)
    return _cache["exact_table"]
