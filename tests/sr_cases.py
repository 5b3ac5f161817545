"""Inputs of the tests of the stochastically rounded steps (tests/test_gpu_grad_sr.py) and their references, computed once each and
never changed.  One ragged batch of 40 bags and about 290 positions over a table of 97 rows, in grad_cases' conventions (its MODES, its
id widths): empty bags, padding positions, three ids outside the table at full width, weights with zeros and negatives, and row HOT 21
times -- at S = 8 a run of two full segments and a tail, 2S + 5 -- three of them side by side in one bag.  Nothing here runs the
code under test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as gc  # noqa: E402
import grad_ref as gr  # noqa: E402
import grad_seg_ref as gs  # noqa: E402

F = np.float32
N_ROWS, N_BAGS, PAD, HOT, N_HOT, S = 97, 40, 17, 50, 21, 8
MODES = gc.MODES
LR, EPS = F(0.1), F(1e-10)
_cache = {}


def batch():
    """(ids as Python ints [n], offsets int64 [40], positions of the bad ids)."""
    if "batch" not in _cache:
        rng = np.random.default_rng(4242)
        lens = rng.integers(3, 13, size=N_BAGS)
        lens[[5, 39]] = 0
        lens[12] = 14
        offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        n = int(lens.sum())
        common = np.setdiff1d(np.arange(N_ROWS), [PAD, HOT])
        ids = [int(v) for v in rng.choice(common, size=n)]
        in_12 = set(range(int(offsets[12]), int(offsets[12]) + 3))
        free = [p for p in range(1, n - 1) if p not in in_12]
        picked = [int(p) for p in rng.choice(free, size=N_HOT - 3 + 4 + 3, replace=False)]
        for p in sorted(in_12) + picked[:N_HOT - 3]:
            ids[p] = HOT
        for p in picked[N_HOT - 3:N_HOT + 1]:
            ids[p] = PAD
        bad_at = picked[N_HOT + 1:]
        ids[0], ids[n - 1] = 0, N_ROWS - 1
        assert ids.count(HOT) == N_HOT >= 2 * S + 3 and len(bad_at) == 3 and 0 not in bad_at and n - 1 not in bad_at and 250 <= n <= 350, (ids.count(HOT), n)
        _cache["batch"] = (ids, offsets, bad_at)
    return _cache["batch"]


def ids_of(width):
    ids, _off, bad_at = batch()
    ids = list(ids)
    for p, v in zip(bad_at, [-1, 2 ** 32 + 5, N_ROWS] if width == "i64" else [N_ROWS, 2 ** 31 + 3, 2 ** 32 - 1]):
        ids[p] = v
    return ids


def weights():
    if "weights" not in _cache:
        rng = np.random.default_rng(77)
        w = rng.choice(np.array([0.0, -1.5, 0.3, 1.7, -0.7, 2.0, 1.0], F), size=len(batch()[0])).astype(F)
        w.setflags(write=False)
        _cache["weights"] = w
    return _cache["weights"]


def args(mode_name, width):
    """(ids, offsets, mode, weights or None, padding_idx or None) as the references take them."""
    mode, weighted, padded = MODES[mode_name]
    return ids_of(width), batch()[1], mode, weights() if weighted else None, PAD if padded else None


def grads(dim, seed=0):
    """G: float32 [40, dim] over ten binades, a bag of -0.0; `seed` makes other gradients of the same shape."""
    key = ("grads", dim, seed)
    if key not in _cache:
        rng = np.random.default_rng(dim * 13 + 5 + 1000 * seed)
        G = (rng.standard_normal((N_BAGS, dim)) * np.exp2(rng.integers(-6, 4, size=(N_BAGS, 1)))).astype(F)
        G[7] = -0.0
        G.setflags(write=False)
        _cache[key] = G
    return _cache[key]


def table(kind, dim, seed=0):
    """uint8 [97, 2 * dim]: finite randoms in the table's dtype; row 3 deep in (fp16) or near (bf16) the subnormal range, row 4 near
    the largest finite value -- steps on them reach the subnormal branch of enc_sr and the carry into infinity."""
    key = ("table", kind, dim, seed)
    if key not in _cache:
        rng = np.random.default_rng(300 + dim + 1000 * seed)
        w = (rng.standard_normal((N_ROWS, dim)) * 2).astype(F)
        w[3] = w[3] * F(2.0 ** -22 if kind == "f16" else 2.0 ** -125)
        w[4] = np.sign(w[4]) * F(65504.0 if kind == "f16" else 3.3e38)      # (fp16: the largest finite value itself)
        _cache[key] = gr.encode(kind, w)
        _cache[key].setflags(write=False)
    return _cache[key]


def state(optimizer, dim):
    key = ("state", optimizer, dim)
    if key not in _cache:
        if optimizer == "sgd":
            return None
        rng = np.random.default_rng(600 + dim)
        s = np.abs(rng.standard_normal((N_ROWS,) if optimizer == "rowwise" else (N_ROWS, dim))).astype(F)
        s[::5] = 0
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def sparse(width, mode_name, dim, segment=None, seed=0):
    """(rows, grads, n_bad) of the batch: grad_ref in the position order, grad_seg_ref with segment length `segment`."""
    key = ("sparse", width, mode_name, dim, segment, seed)
    if key not in _cache:
        ids, off, mode, w, pad = args(mode_name, width)
        if segment is None:
            _cache[key] = gr.sparse_grad(N_ROWS, ids, off, grads(dim, seed), mode, w, pad)
        else:
            _cache[key] = gs.seg_sparse_grad(N_ROWS, ids, off, grads(dim, seed), segment, mode, w, pad)
    return _cache[key]
