"""numpy restatement of what torch's CPU F.embedding_bag computes for the pooled modes -- the rules the bag_pool_* kernels
follow (include/pimemb.h, emb_pool_spec).  Per output element, entries taken in index order:

  sum                    acc = +0; acc = acc + x
  weighted, no padding   acc = fmaf(w, x, acc)             (one rounding)
  weighted + padding     padding entries skipped; acc = acc + round(w * x)
  mean                   (sum over non-padding entries) / count, an IEEE division; count 0 -> +0
  max                    first non-padding row, then acc = x if x > acc else acc (first of equal values stays); empty -> +0

fp16 tables: the same on the rows widened to fp32.  Output fp32."""
from __future__ import annotations

import numpy as np


def fma32(w, x, acc):
    """Correctly rounded float32 fma(w, x, acc), elementwise.  The product of two float32 values is exact in float64; the
    sum with acc is rounded to float64 *to odd* (TwoSum gives the exact error), and a round-to-odd result with 53 >= 24 + 2
    bits rounds to the same float32 as the exact value would."""
    p = np.float64(w) * np.asarray(x, dtype=np.float64)
    a = np.asarray(acc, dtype=np.float64)
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)
    even = (s.view(np.int64) & 1) == 0
    nudge = (e != 0) & even
    s = np.where(nudge, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def embedding_bag(table, indices, offsets, mode="sum", per_sample_weights=None, padding_idx=None):
    """table [N, D] (fp32 or fp16), indices [n] ints, offsets [B] bag starts (the last bag runs to the end).
    Returns float32 [B, D]."""
    rows = np.asarray(table).astype(np.float32)
    idx = np.asarray(indices).astype(np.int64)
    off = np.asarray(offsets).astype(np.int64)
    B, D = len(off), rows.shape[1]
    w = None if per_sample_weights is None else np.asarray(per_sample_weights, dtype=np.float32)
    out = np.zeros((B, D), dtype=np.float32)
    for b in range(B):
        p0, p1 = int(off[b]), int(off[b + 1]) if b + 1 < B else len(idx)
        acc = np.zeros(D, dtype=np.float32)
        cnt = 0
        for p in range(p0, p1):
            r = int(idx[p])
            if padding_idx is not None and r == padding_idx:
                continue
            x = rows[r]
            if mode == "max":
                acc = x.copy() if cnt == 0 else np.where(x > acc, x, acc)
            elif w is None:
                acc = acc + x
            elif padding_idx is None:
                acc = fma32(w[p], x, acc)
            else:
                acc = acc + w[p] * x
            cnt += 1
        if mode == "mean" and cnt:
            acc = acc / np.float32(cnt)
        out[b] = acc
    return out
