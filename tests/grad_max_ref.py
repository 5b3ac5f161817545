"""THE MAX-MODE BACKWARD of include/pimemb_grad.h as plain loops: the winners of the forward's max, and the row gradients that select
by them, in the position order or (S given) the segmented one.  numpy float32 throughout: every addition rounded on its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402

F = np.float32
NO_WINNER = 0xFFFFFFFF


def winners(kind, table_bytes, indices, offsets, padding_idx=None):
    """(win uint32 [B, dim], bags, kinds): per bag and element the first good position, replaced by a later good one only where its
    decoded value is strictly greater; NO_WINNER for a bag without a good position."""
    W = gr.decode(kind, table_bytes)
    B, dim = len(offsets), W.shape[1]
    bags = gr.bags_of(len(indices), offsets)
    kinds = gr.classify(W.shape[0], indices, bags, padding_idx)
    win = np.full((B, dim), NO_WINNER, dtype=np.uint32)
    cur = np.zeros((B, dim), dtype=F)
    for p in range(len(indices)):                # position order
        if kinds[p] != "good":
            continue
        b, x = bags[p], W[int(indices[p])]
        take = (win[b] == NO_WINNER) | (x > cur[b])      # element by element: the first good position, then a strict fp32 compare
        cur[b], win[b] = np.where(take, x, cur[b]), np.where(take, np.uint32(p), win[b])
    return win, bags, kinds


def sparse_grad(kind, table_bytes, indices, offsets, grad, padding_idx=None, S=None):
    """(rows int64 ascending, grads float32 [|U|, dim], number of bad positions, win).  U: every row with a good position; c_p is
    G[bag(p)] where p won and +0 elsewhere, and the zeros are added.  S: the segment length of the segmented order."""
    G = np.asarray(grad, dtype=F)
    win, bags, kinds = winners(kind, table_bytes, indices, offsets, padding_idx)
    runs = {}
    for p in range(len(indices)):
        if kinds[p] == "good":
            runs.setdefault(int(indices[p]), []).append(p)
    rows = np.array(sorted(runs), dtype=np.int64)
    grads = np.zeros((len(rows), G.shape[1]), dtype=F)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for k, r in enumerate(rows):
            c = [np.where(win[bags[p]] == p, G[bags[p]], F(0.0)).astype(F) for p in runs[int(r)]]
            segments = [c] if S is None else [c[j:j + S] for j in range(0, len(c), S)]
            acc = None
            for seg in segments:
                t = np.zeros(G.shape[1], dtype=F)            # +0.0f
                for cp in seg:
                    t = t + cp
                acc = t if acc is None else acc + t          # the sum of the partials starts FROM t_0
            grads[k] = acc
    return rows, grads, sum(k == "bad" for k in kinds), win
