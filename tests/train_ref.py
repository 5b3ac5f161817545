"""A training loop over one table as a list of events, composed from the references the suite already has: the reference of
tests/test_train_loop_cpu.py and tests/test_gpu_train_loop.py, which run lookups (include/pimemb.h), the backward pass
(include/pimemb_grad.h) and the row writer (include/pimemb_rows.h) back to back on shared tables.  Every piece is another module's
definition -- grad_ref.sparse_grad / sgd_step, grad_seg_ref.seg_sparse_grad, optim_ref.adagrad_step, psw_ref.weights_grad,
pool_ref.embedding_bag, rows_cases.host_encode / sequential_update, formats.py's decoders -- and only their ORDER is new.  Nothing here
runs the code under test.

THE STATE.  State(kind, table, master, opt): the table as it lies in HBM (uint8 [N, row stride]), the fp32 master rows [N, dim] of
the master-row recipe (None for a table that is stepped in place), the optimizer state (float32 [N, dim], [N] row-wise, or None).

THE MASTER-ROW RECIPE (include/pimemb_grad.h: "keep fp32 master rows, take emb_grad_sparse, and write rows with emb_rows_update"):
    rows, g = sparse_grad(batch);  t = float32(lr) * g;  master[rows] = master[rows] - t;  table[rows] = enc(master[rows])
The product and the subtraction are two fp32 operations, each rounded on its own, never one FMA.

THE BATCHES.  train_batches(kind, dim) makes K = 3 batches over a table of 300 rows; lookup_batch() the pooled lookup that
reads the table between the steps.  What they hold is listed at Batch and asserted by tests/test_train_loop_cpu.py."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as gc  # noqa: E402
import grad_ref as gr  # noqa: E402
import grad_seg_ref as sr  # noqa: E402
import optim_ref as orf  # noqa: E402
import pool_ref  # noqa: E402
import psw_ref as pr  # noqa: E402
import rows_cases as rc  # noqa: E402

formats = rc.formats
F = np.float32
MODES = gc.MODES                     # name -> (mode, weighted, padding)
N_ROWS, N_BAGS, K = 300, 40, 3
PAD = 17
HOT, N_HOT = 123, 21                 # the row that occurs 21 times in every batch, three times inside bag TRIPLE_BAG
TRIPLE_BAG = 10
EMPTY_BAGS = (6, 21, N_BAGS - 1)     # in the middle and at the end
LEAD_ROWS = (298, 299)               # the rows of the two positions before offsets[0] of batch 0: no other position names them
# the 16 rows every batch names and the lookup batch reads most often (eight times each): the hot set of the hot-set dance
TOP = (3, 8, 30, 57, 84, 111, HOT, 138, 150, 165, 192, 201, 219, 246, 273, 290)
LR = F(0.05)                         # no power of two: every rounding counts
EPS = F(1e-10)
WRITE_ROWS = 64

State = namedtuple("State", "kind table master opt")


def decode(kind, raw):
    """uint8 [n, stride] table bytes of any of the six dtypes -> float32 [n, dim], exactly."""
    raw = np.ascontiguousarray(raw)
    if kind in ("e4m3", "e5m2"):
        return formats.from_f8_bits(raw, kind).astype(F)
    if kind == "mxfp4":
        return formats.from_mxfp4(raw, formats.mxfp4_dim_of_stride(raw.shape[1])).astype(F)
    return gr.decode(kind, raw)


# ---- the events ---------------------------------------------------------------------------------------------------------------------
def forward(kind, table_bytes, ids, off, mode="sum", w=None, pad=None):
    """The pooled lookup: pool_ref.embedding_bag over the decoded bytes, float32 [B, dim]."""
    return pool_ref.embedding_bag(decode(kind, table_bytes), ids, off, mode, w, pad)


def master_step(kind, table_bytes, master, ids, off, G, mode="sum", w=None, pad=None, lr=LR, contract=False):
    """The documented recipe: (table bytes, master, rows int64 [|U|], n_bad).  contract=True is a WRONG recipe for
    tests/test_train_loop_cpu.py: master - lr * g in one rounding."""
    rows, g, n_bad = gr.sparse_grad(master.shape[0], ids, off, G, mode, w, pad)
    master = np.array(master, dtype=F, copy=True)
    if len(rows):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            if contract:
                master[rows] = pool_ref.fma32(-F(lr), g, master[rows])
            else:
                t = F(lr) * g
                master[rows] = master[rows] - t
    table, skipped = rc.sequential_update(table_bytes, rows, rc.host_encode(kind, master[rows]))
    assert skipped == 0
    return table, master, rows, n_bad


def fused_step(kind, table_bytes, opt, ids, off, G, mode="sum", w=None, pad=None, optimizer="sgd", lr=LR, eps=EPS, segment=None):
    """The fused steps of include/pimemb_grad.h, dispatched: optimizer "sgd" / "adagrad" / "rowwise"; segment None: the position
    order (grad_ref), else the segmented order with that S (grad_seg_ref).  (table bytes, optimizer state, rows, n_bad)."""
    n = table_bytes.shape[0]
    if segment is None:
        rows, g, n_bad = gr.sparse_grad(n, ids, off, G, mode, w, pad)
    else:
        rows, g, n_bad = sr.seg_sparse_grad(n, ids, off, G, segment, mode, w, pad)
    if optimizer == "sgd":
        return gr.sgd_step(kind, table_bytes, rows, g, F(lr)), opt, rows, n_bad
    if optimizer not in ("adagrad", "rowwise"):
        raise ValueError(optimizer)
    table, opt = orf.adagrad_step(kind, table_bytes, opt, rows, g, F(lr), F(eps), rowwise=optimizer == "rowwise")
    return table, opt, rows, n_bad


def write_rows(kind, table_bytes, master, ids, rows_f32, first_wins=False):
    """emb_rows_update of fp32 rows: (table bytes, master, rows skipped).  The last occurrence of an id wins; a master follows the
    write.  first_wins=True is a WRONG writer for tests/test_train_loop_cpu.py."""
    ids = [int(i) for i in ids]
    order = range(len(ids))
    if first_wins:
        order = list(reversed(order))
    enc = rc.host_encode(kind, rows_f32)
    table, skipped = rc.sequential_update(table_bytes, [ids[p] for p in order], enc[list(order)])
    if master is not None:
        master = np.array(master, dtype=F, copy=True)
        for p in order:
            if 0 <= ids[p] < master.shape[0]:
                master[ids[p]] = rows_f32[p]
    return table, master, skipped


def run(events, state):
    """Apply the events in order: [(state after the event, what the event gives)].  An event is
      ("lookup", ids, off, mode, w, pad)                                    -> the pooled rows
      ("master_step", ids, off, G, mode, w, pad, lr)                        -> (rows, n_bad)
      ("fused_step", ids, off, G, mode, w, pad, optimizer, lr, eps, segment) -> (rows, n_bad)
      ("write_rows", ids, rows_f32)                                         -> rows skipped
      ("weights_grad", ids, off, G, pad)                                    -> (dw, n_bad)"""
    out = []
    for ev in events:
        what, a = ev[0], ev[1:]
        if what == "lookup":
            res = forward(state.kind, state.table, *a)
        elif what == "master_step":
            table, master, rows, n_bad = master_step(state.kind, state.table, state.master, *a)
            state, res = state._replace(table=table, master=master), (rows, n_bad)
        elif what == "fused_step":
            table, opt, rows, n_bad = fused_step(state.kind, state.table, state.opt, *a)
            state, res = state._replace(table=table, opt=opt), (rows, n_bad)
        elif what == "write_rows":
            table, master, res = write_rows(state.kind, state.table, state.master, *a)
            state = state._replace(table=table, master=master)
        elif what == "weights_grad":
            ids, off, G, pad = a
            res = pr.weights_grad(state.kind, state.table, ids, off, G, pad)
        else:
            raise ValueError(what)
        out.append((state, res))
    return out


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class Batch:
    """One training batch over the 300 rows.  40 ragged bags of 0 - 9 positions, EMPTY_BAGS empty (in the middle and the last one);
    row HOT 21 times, three of them inside bag TRIPLE_BAG and the others at the head of 18 bags before and behind it; every row of
    TOP at least once; two padding entries; three bad ids of full width (bad_values: for int64 one >= 2^32 whose low word is
    HOT, and one negative); batch 0 alone has two positions before offsets[0], which name LEAD_ROWS.  The other ids come from a
    window of 150 rows that moves by 60 rows per batch: the row sets of consecutive batches overlap and differ.  G: float32
    [40, dim] over eight binades, no zeros; weights without zeros."""

    def __init__(self, k):
        rng = np.random.default_rng(9000 + k)
        self.k, self.lead = k, 2 if k == 0 else 0
        lens = rng.integers(1, 10, size=N_BAGS)
        lens[list(EMPTY_BAGS)] = 0
        lens[TRIPLE_BAG] = 9
        self.lens, self.B = lens, N_BAGS
        self.n = n = self.lead + int(lens.sum())
        self.offsets = (self.lead + np.concatenate([[0], np.cumsum(lens)[:-1]])).astype(np.int64)
        self.offsets.setflags(write=False)
        window = np.setdiff1d((np.arange(150) + 60 * k) % 296, (PAD,) + TOP)
        ids = [int(v) for v in rng.choice(window, size=n)]
        taken = set(range(self.lead))
        for p, r in zip(range(self.lead), LEAD_ROWS):
            ids[p] = r

        def put(p, r):
            assert p not in taken
            ids[p] = r
            taken.add(p)

        start = lambda b: int(self.offsets[b])  # noqa: E731
        for s in (0, 4, 8):
            put(start(TRIPLE_BAG) + s, HOT)
        others = [b for b in range(N_BAGS) if lens[b] and b != TRIPLE_BAG]
        self.hot_bags = [others[i] for i in np.linspace(0, len(others) - 1, N_HOT - 3).round().astype(int)]
        assert len(set(self.hot_bags)) == N_HOT - 3 and self.hot_bags[0] < TRIPLE_BAG < self.hot_bags[-1]
        for b in self.hot_bags:
            put(start(b), HOT)
        free = [int(p) for p in rng.permutation([p for p in range(self.lead, n) if p not in taken])]
        for r in TOP:
            if r != HOT:
                put(free.pop(), r)
        self.pad_at = [free.pop(), free.pop()]
        for p in self.pad_at:
            put(p, PAD)
        self.bad_at = [free.pop(), free.pop(), free.pop()]
        taken.update(self.bad_at)
        self._ids, self.n_bad = ids, 3
        w = rng.choice(np.array([-1.5, 0.3, 1.7, -0.7, 2.0, 1.0, 0.1], dtype=F), size=n)
        w[::3] = (rng.standard_normal(len(w[::3])) + np.sign(rng.standard_normal(len(w[::3]))) * 0.25).astype(F)
        assert (w != 0).all()
        w.setflags(write=False)
        self.weights = w
        self._G = {}

    @staticmethod
    def bad_values(width):
        return [2 ** 32 + HOT, -1, N_ROWS] if width == "i64" else [N_ROWS, N_ROWS + 7, 2 ** 32 - 1]

    def ids(self, width="i64"):
        """The ids as Python ints (full width) with the bad positions filled."""
        ids = list(self._ids)
        for p, v in zip(self.bad_at, self.bad_values(width)):
            ids[p] = v
        return ids

    def ids_array(self, width="i64"):
        return np.array(self.ids(width), dtype=np.int64) if width == "i64" else np.array(self.ids(width), dtype=np.uint64).astype(np.uint32)

    def offsets_array(self, width="i64"):
        return self.offsets.astype(np.int64 if width == "i64" else np.uint32)

    def named_rows(self, mode_name="sum"):
        """The rows with at least one good position, ascending."""
        padded = MODES[mode_name][2]
        ids = np.array(self._ids[self.lead:])
        good = np.ones(len(ids), bool)
        good[[p - self.lead for p in self.bad_at]] = False
        if padded:
            good &= ids != PAD
        return np.unique(ids[good])

    def grads(self, dim):
        if dim not in self._G:
            rng = np.random.default_rng(9100 + 10 * dim + self.k)
            G = (rng.standard_normal((self.B, dim)) * np.exp2(rng.integers(-4, 4, size=(self.B, 1)))).astype(F)
            G[G == 0] = F(1)
            G.setflags(write=False)
            self._G[dim] = G
        return self._G[dim]

    def witness_grads(self, dim):
        """grads(dim) with column 0 made a witness of the order of additions on row HOT (mode "sum", no weights): 2^24 in the bag
        of its first occurrence, -2^24 in the bag of its last, 1 in the bags between.  In the position order every 1 is absorbed by
        the 2^24 before it (a tie, rounded to even) and the sum is 0; in the segmented order with S = 8 the second segment sums
        eight 1s and the third four of them before the -2^24: the sum is 12."""
        G = self.grads(dim).copy()
        G[self.hot_bags + [TRIPLE_BAG], 0] = F(1)
        G[self.hot_bags[0], 0], G[self.hot_bags[-1], 0] = F(2.0 ** 24), F(-(2.0 ** 24))
        G.setflags(write=False)
        return G

    def args(self, mode_name, width="i64"):
        """(ids, offsets, mode, weights or None, padding id or None) as the references take them."""
        mode, weighted, padded = MODES[mode_name]
        return self.ids(width), self.offsets, mode, self.weights if weighted else None, PAD if padded else None


def train_batches(kind, dim, k=K):
    """K batches for one table of 300 rows of `kind` and `dim`: [(Batch, G float32 [40, dim])].  The ids do not depend on kind or
    dim, the gradients on dim alone."""
    assert kind in rc.KINDS and k >= 1
    return [(b, b.grads(dim)) for b in (_once(("batch", j), lambda j=j: Batch(j)) for j in range(k))]


class LookupBatch:
    """The pooled lookup that reads the table between the steps: 48 bags of 0 - 7 positions (more than two per bag on average),
    valid ids only -- a lookup reads the table unchecked -- Zipf-like: every row of TOP eight times, two padding entries, the rest
    uniform over the other rows (none of them more than five times)."""

    def __init__(self):
        rng = np.random.default_rng(9500)
        lens = rng.integers(1, 8, size=48)
        lens[[7, 47]] = 0
        n = int(lens.sum())
        assert n > 8 * len(TOP) + 20
        rest = np.setdiff1d(np.arange(N_ROWS), (PAD,) + TOP)
        while True:
            cold = rng.choice(rest, size=n - 8 * len(TOP) - 2)
            if np.bincount(cold).max() <= 5:
                break
        ids = np.concatenate([np.repeat(np.array(TOP), 8), cold, [PAD, PAD]])
        self.ids = ids[rng.permutation(n)].astype(np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.weights = (rng.standard_normal(n) + np.sign(rng.standard_normal(n)) * 0.25).astype(F)
        self.n, self.B = n, len(lens)
        for a in (self.ids, self.offsets, self.weights):
            a.setflags(write=False)

    def args(self, mode_name):
        mode, weighted, padded = MODES[mode_name]
        return self.ids, self.offsets, mode, self.weights if weighted else None, PAD if padded else None


def lookup_batch():
    return _once("lookup", LookupBatch)


def initial_master(kind, dim):
    """float32 [300, dim]: the master rows (and, encoded, the table) every case starts from.  Values about 1/2."""
    def make():
        w = (np.random.default_rng(9700 + dim).standard_normal((N_ROWS, dim)) * 0.5).astype(F)
        w.setflags(write=False)
        return w
    return _once(("master", dim), make)


def initial_state(kind, dim, master=True, optimizer=None):
    w = initial_master(kind, dim)
    opt = None if optimizer in (None, "sgd") else np.zeros((N_ROWS, dim) if optimizer == "adagrad" else (N_ROWS,), F)
    return State(kind, rc.host_encode(kind, w), w.copy() if master else None, opt)


def written_rows(after, dim, seed=0, n=WRITE_ROWS):
    """(ids int64 [64], rows float32 [64, dim]) of a writer update between two steps: half of the ids are rows of `after` (the
    rows a step just changed), the others any rows; eight ids occur twice, positions apart, with different sources."""
    rng = np.random.default_rng(9800 + seed + dim)
    after = np.asarray(after, dtype=np.int64)
    ids = np.concatenate([rng.choice(after, size=n // 2, replace=False), rng.choice(np.setdiff1d(np.arange(N_ROWS), after), size=n // 2, replace=False)])
    ids = ids[rng.permutation(n)]
    ids[n - 8:] = ids[:8]
    rows = (rng.standard_normal((n, dim)) * 0.5).astype(F)
    return ids.astype(np.int64), rows


# ---- the sequences both test files run ------------------------------------------------------------------------------------------------
# (kind, dim, mode): the master-row recipe with a host wait; e4m3 at dim 7 runs the element-wise writer and the any-dim lookup
RECIPE_CASES = (("e4m3", 16, "sum"), ("e4m3", 7, "mean+pad"), ("e5m2", 48, "weighted+pad"), ("mxfp4", 32, "mean+pad"), ("mxfp4", 96, "sum"),
                ("bf16", 24, "sum"))
# (kind, dim, mode, id width of the batch): the recipe without a host wait
NOWAIT_CASES = (("e4m3", 16, "sum", "i64"), ("mxfp4", 32, "weighted+pad", "u32"), ("f16", 8, "mean+pad", "i64"))
GRAPH_SCALES = (F(1), F(1), F(1), F(-0.75))      # iteration j of the captured loop takes fl(G[j % 3] * GRAPH_SCALES[j])


def graph_grads(dim):
    """The four gradients of the captured loop: every iteration reads batch 0's ids, the gradient buffer changes."""
    Gs = [G for _b, G in train_batches("f32", dim)]
    return [(Gs[j % K] * s).astype(F) for j, s in enumerate(GRAPH_SCALES)]


def graph_events(dim, mode_name):
    b = train_batches("f32", dim, 1)[0][0]
    lb = lookup_batch().args(mode_name)
    ev = []
    for G in graph_grads(dim):
        ev += [("lookup",) + lb, ("master_step",) + b.args(mode_name)[:2] + (G,) + b.args(mode_name)[2:] + (LR,), ("lookup",) + lb]
    return ev


def psw_events(dim):
    """The gradient of per_sample_weights, a writer update of every row the batch names, the gradient again."""
    b, G = train_batches("f32", dim, 1)[0]
    ids, off, _mode, _w, pad = b.args("weighted+pad")
    named = b.named_rows("weighted+pad")
    rows = (np.random.default_rng(9900 + dim).standard_normal((len(named), dim)) * 0.5).astype(F)
    return [("weights_grad", ids, off, G, pad), ("write_rows", named, rows), ("weights_grad", ids, off, G, pad)]



def recipe_events(dim, mode_name, width="i64", k=K, grads=None):
    """Per iteration: the lookup, the master step, the lookup again.  grads: one G per iteration instead of the batches' own."""
    lb = lookup_batch().args(mode_name)
    ev = []
    for j, (b, G) in enumerate(train_batches("f32", dim, k)):
        ev += [("lookup",) + lb, ("master_step",) + b.args(mode_name, width)[:2] + (G if grads is None else grads[j],) + b.args(mode_name, width)[2:] + (LR,),
               ("lookup",) + lb]
    return ev


def interleaved_events(dim, mode_name, optimizer, segment=None, witness=False):
    """A step on batch 0, a writer update of 64 rows -- half of them rows that step changed --, a step on batch 1, the lookup."""
    (b0, G0), (b1, G1) = train_batches("f32", dim, 2)
    if witness:
        G0, G1 = b0.witness_grads(dim), b1.witness_grads(dim)
    step = lambda b, G: ("fused_step",) + b.args(mode_name)[:2] + (G,) + b.args(mode_name)[2:] + (optimizer, LR, EPS, segment)  # noqa: E731
    ids, rows = written_rows(b0.named_rows(mode_name), dim)
    return [step(b0, G0), ("write_rows", ids, rows), step(b1, G1), ("lookup",) + lookup_batch().args("sum")]
