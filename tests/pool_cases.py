"""Inputs for the pooled-lookup edge tests (test_pooling_reference.py on the CPU, test_gpu_pooled_edges.py on the GPU), built
deterministically from a seed.  No GPU code and no test functions: every builder returns its inputs TOGETHER WITH the facts the
tests must assert about them, so that a case cannot silently stop exercising the path it was written for.

wave_batch_case   indices / offsets / per-sample weights / padding_idx for the pooled wave-batch kernel (kind 0): 64 bags per
                  wavefront step, most bags of one index, with steps of three classes --
                    "spec"     every bag of length 1 and offsets[b] == b: the speculative index / weight loads are taken
                    "shifted"  every bag of length <= 1, an empty bag among them, some offsets[b] != b: speculation rejected
                    "general"  a bag of length >= 2: the round loop over pool_walk
                  (steps of one-index bags behind an empty or a long bag are "drift": speculation rejected, no empty bag).
special_table     a table over a palette of special values of one dtype (signed zeros, denormals, largest finite, inf, NaN)
special_bags      ragged bags of 0 .. 12 entries over such a table, the first few of them crafted: one per arithmetic rule
                  of tests/pool_ref.py that ordinary random data cannot tell from its plausible wrong version.
SPECS / reference the five pooling specs every GPU test loops over, and torch's CPU F.embedding_bag for one of them."""
from __future__ import annotations

from importlib import import_module
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

formats = import_module("pim-embedding-lookup_amd.formats")

# name: (mode, per-sample weights?, padding_idx?) -- the kernels' four ops (add, fma, mul-then-add, max) and the mean division
SPECS = {"sum+pad": ("sum", False, True), "mean+pad": ("mean", False, True), "max+pad": ("max", False, True),
         "weighted": ("sum", True, False), "weighted+pad": ("sum", True, True)}
SPECS_NO_PAD = {"mean": ("mean", False, False), "max": ("max", False, False)}


def reference(wide, idx, off, spec, w, pad):
    """torch's CPU F.embedding_bag over the fp32-widened table for one of SPECS: float32 numpy [bags, dim]."""
    mode, weighted, padded = spec
    out = F.embedding_bag(torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)), torch.from_numpy(wide),
                          torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)), mode=mode,
                          per_sample_weights=torch.from_numpy(w) if weighted else None, padding_idx=pad if padded else None)
    return out.numpy()


def _same(g, w, gn, wn):
    bad = (gn != wn) | (~wn & (g != w))
    if not bad.any():
        return True, ""
    at = np.argwhere(bad)
    return False, "%d of %d elements differ; first (bag, col, got, want): %s" % (
        len(at), g.size, [(int(b), int(c), hex(int(g[b, c])), hex(int(w[b, c]))) for b, c in at[:6]])


def same_bits(got, want):
    """fp32 rows: NaN positions equal, every other element equal as raw bits (+0 and -0 differ).  Returns (ok, text about the
    first differences)."""
    g, w = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, (g.shape, w.shape)
    return _same(g, w, (g & 0x7FFFFFFF) > 0x7F800000, (w & 0x7FFFFFFF) > 0x7F800000)


def same_bits16(got, want, bf16):
    """same_bits for rows of fp16 (bf16=False) or bf16 bit patterns (uint16 / int16 arrays)."""
    g, w = np.ascontiguousarray(got).view(np.uint16), np.ascontiguousarray(want).view(np.uint16)
    assert g.shape == w.shape, (g.shape, w.shape)
    top = 0x7F80 if bf16 else 0x7C00
    return _same(g, w, (g & 0x7FFF) > top, (w & 0x7FFF) > top)


# ---- the wave-batch layout ----------------------------------------------------------------------------------------------------
TINY_W = np.float32(2.0 ** -126)         # times a table entry below 1 in magnitude: an fp32 denormal product
OVER_W = np.float32(1.003)             # times a 2-byte format's largest finite value: past the midpoint to its infinity
PAD_PATTERNS = ("first", "last", "all", "chunk", "boundary", "none")


def long_lengths(unroll):
    return [2, 3, unroll - 1, unroll, unroll + 1, 2 * unroll, 2 * unroll + 1, 20]


def step_classes(lens, off):
    """Class of every 64-bag step ("spec" / "shifted" / "drift" / "general"), as the kernel's wavefront sees it."""
    B = len(lens)
    out = []
    for s in range(0, B, 64):
        ln, of = lens[s:s + 64], off[s:s + 64]
        if (ln >= 2).any():
            out.append("general")
        elif (ln == 1).all() and np.array_equal(of, np.arange(s, s + len(ln))):
            out.append("spec")
        elif (ln == 0).any():
            out.append("shifted")
        else:
            out.append("drift")
    return out


def wave_batch_case(rows, B, unroll, seed, tail="general", fill=None):
    """B bags over a table of `rows` rows for the pooled wave-batch kernel whose pool_walk takes `unroll` entries at a time.
    tail: class of the last, partial step ("general" or "shifted"); B must not be a multiple of 64.
    fill: None (random rows), or a special_bags() result whose bags are tiled into the layout -- every long bag takes the entries
    (and weights) of one of its bags, repeated to the long bag's length; the one-index bags walk over every row of the table.
    Returns a namespace: idx, off (int64), w (float32), pad, lens, classes (per step), counts (per class), tail_class,
    emptied (bags of padding only: +0 under every padded spec), pad_patterns (how many long bags carry each pattern),
    long_lens (how many long bags have each length), weights (how many entries carry each special weight)."""
    assert B % 64 != 0 and B > 64 * 64 and tail in ("general", "shifted")
    rng = np.random.default_rng(seed)
    n_steps = (B + 63) // 64
    lens = np.ones(B, np.int64)
    pad = rows // 3 if fill is None else int(fill.pad)
    lengths = long_lengths(unroll)
    head = 12                                             # full steps before the first irregular bag
    kind = rng.random(n_steps)
    long_bags = []
    for s in range(head, n_steps - 1):
        base = 64 * s
        if s == head + 1:                                 # (laid out by hand below)
            continue
        if kind[s] < 0.03:                                # a general step: 1 .. 6 long bags, now and then an empty one beside them
            for b in rng.choice(64, size=int(rng.integers(1, 7)), replace=False):
                lens[base + b] = lengths[len(long_bags) % len(lengths)]
                long_bags.append(base + int(b))
            if rng.random() < 0.5:
                b = base + int(rng.integers(0, 64))
                if lens[b] == 1:
                    lens[b] = 0
        elif kind[s] < 0.06:                              # a shifted step: 1 .. 5 empty bags
            lens[base + rng.choice(64, size=int(rng.integers(1, 6)), replace=False)] = 0
    # lanes 0 and 63 of a step, and a long bag straddled by empties
    base = 64 * (head + 1)
    lens[base], lens[base + 63] = lengths[len(long_bags) % len(lengths)], 20
    long_bags += [base, base + 63]
    t0 = 64 * (n_steps - 1)
    n_tail = B - t0
    if tail == "general":                                 # the last bag of all is long: it runs to the end of the indices
        lens[t0:] = 1
        lens[B - 1] = 2 * unroll + 1
        long_bags.append(B - 1)
        if n_tail > 2:
            lens[t0 + 1] = 0
    else:                                                 # bags of <= 1, the last one empty: its offset is n_indices
        lens[t0:] = 1
        lens[t0 + (1 if n_tail > 2 else 0)] = 0
        lens[B - 1] = 0
    long_bags = sorted(set(long_bags))
    off = np.zeros(B, np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    n = int(lens.sum())

    if fill is None:
        idx = rng.integers(0, rows - 1, size=n)
        idx[idx >= pad] += 1                              # the padding row appears only where it is placed
        w = rng.standard_normal(n).astype(np.float32)
    else:
        idx = (np.arange(n, dtype=np.int64) * 7) % rows   # (7 and the row count coprime or not: every residue class is walked)
        idx = np.where(idx == pad, (pad + 1) % rows, idx)
        w = rng.standard_normal(n).astype(np.float32)
    weights = {"+0": 0, "-0": 0, "tiny": 0}
    for name, val, every in (("+0", np.float32(0.0), 61), ("-0", np.float32(-0.0), 67), ("tiny", TINY_W, 29)):
        at = np.arange(every // 2, n, every)
        w[at] = val
        weights[name] = len(at)

    pad_patterns = dict.fromkeys(PAD_PATTERNS, 0)
    long_lens = dict.fromkeys(lengths, 0)
    emptied = []
    if fill is None:
        for k, b in enumerate(long_bags):
            p, L = int(off[b]), int(lens[b])
            long_lens[L] += 1
            want = PAD_PATTERNS[(k // len(lengths) + k) % len(PAD_PATTERNS)]
            if want == "chunk" and L < unroll:
                want = "first"
            if want == "boundary" and L < unroll + 1:
                want = "last"
            if want == "first":
                idx[p] = pad
            elif want == "last":
                idx[p + L - 1] = pad
            elif want == "all":
                idx[p:p + L] = pad
                emptied.append(b)
            elif want == "chunk":                         # a whole unroll chunk: the second one where the bag has two
                c = unroll if L >= 2 * unroll else 0
                idx[p + c:p + c + unroll] = pad
                if L == unroll:
                    want = "all"
                    emptied.append(b)
            elif want == "boundary":                      # both sides of the boundary between the first two chunks
                idx[p + unroll - 1:p + unroll + 1] = pad
            pad_patterns[want] += 1
            # special weights inside long bags too
            if L >= 3:
                w[p + 1] = (np.float32(0.0), np.float32(-0.0), TINY_W)[k % 3]
        ones = np.flatnonzero(lens == 1)
        for b in ones[5::97]:                             # one-index bags of padding: in spec, drift, shifted and general steps
            idx[off[b]] = pad
            emptied.append(int(b))
    else:
        src = [(int(a), int(b)) for a, b in zip(fill.off, np.append(fill.off[1:], len(fill.idx))) if b - a >= 2]
        assert src, "the special bags hold no bag of two or more entries"
        for k, b in enumerate(long_bags):
            p, L = int(off[b]), int(lens[b])
            long_lens[L] += 1
            a, e = src[k % len(src)]
            idx[p:p + L] = np.resize(fill.idx[a:e], L)
            w[p:p + L] = np.resize(fill.w[a:e], L)
        for b in long_bags:
            if (idx[off[b]:off[b] + lens[b]] == pad).all():
                emptied.append(b)
        ones = np.flatnonzero(lens == 1)
        for b in ones[5::97]:
            idx[off[b]] = pad
            emptied.append(int(b))

    classes = step_classes(lens, off)
    counts = {c: classes.count(c) for c in ("spec", "shifted", "drift", "general")}
    return SimpleNamespace(idx=idx.astype(np.int64), off=off, w=w, pad=pad, lens=lens, classes=classes, counts=counts,
                           tail_class=classes[-1], emptied=np.array(sorted(set(emptied)), np.int64), pad_patterns=pad_patterns,
                           long_lens=long_lens, weights=weights, long_bags=np.array(long_bags, np.int64), unroll=unroll)


def cut_range(c, b0, n):
    """Bags b0 .. b0 + n - 1 of a wave-batch case as a descriptor of their own: (idx, off, w), offsets from 0."""
    p0 = int(c.off[b0])
    p1 = int(c.off[b0 + n]) if b0 + n < len(c.off) else len(c.idx)
    return c.idx[p0:p1].copy(), c.off[b0:b0 + n] - p0, c.w[p0:p1].copy()


def check_wave_batch_case(c, B):
    """The conditions a wave-batch case must meet to run what it is for; raises AssertionError naming the one that fails."""
    assert len(c.off) == B and B % 64 != 0
    assert (c.lens == 1).sum() > B // 2 and len(c.idx) <= 2 * B, "not one-hot-ish: choose_kernel would not pick the wave batch"
    assert all(c.counts[k] >= 8 for k in ("spec", "shifted", "general")), c.counts
    assert c.classes[:8] == ["spec"] * 8, "the first irregular bag must come after several full steps"
    assert c.tail_class in ("general", "shifted")
    assert all(v >= 1 for v in c.long_lens.values()), c.long_lens
    assert all(v >= 1 for v in c.weights.values()), c.weights
    assert len(c.emptied) >= 8
    # a padded one-index bag in a step of each class
    cls = {c.classes[b // 64] for b in c.emptied if c.lens[b] == 1}
    assert {"spec", "general"} <= cls and ({"shifted", "drift"} & cls), cls


# ---- special values -----------------------------------------------------------------------------------------------------------
DTYPES = ("fp32", "fp16", "bf16", "e4m3", "e5m2", "mxfp4")
TORCH_DTYPE = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn,
               "e5m2": torch.float8_e5m2}
# smallest denormal, another denormal, smallest normal, largest finite, the power of two at which x + 1 == x (fp32: 2^24 -- what
# 2^24 + 1, itself no fp32, rounds to)
_FMT = {"fp32": (2.0 ** -149, float(np.float32(1e-40)), 2.0 ** -126, float(np.finfo(np.float32).max), 2.0 ** 24),
        "fp16": (2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -14, 65504.0, 2.0 ** 11),
        "bf16": (2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -126, float(np.uint32(0x7F7F0000).view(np.float32)), 2.0 ** 8),
        "e5m2": (2.0 ** -16, 3 * 2.0 ** -16, 2.0 ** -14, 57344.0, 2.0 ** 3),
        "e4m3": (2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -6, 448.0, 2.0 ** 4)}
HAS_INF = {"fp32": True, "fp16": True, "bf16": True, "e5m2": True, "e4m3": False, "mxfp4": True}     # (MXFP4: products beyond fp32)
HAS_NAN = {"fp32": True, "fp16": True, "bf16": True, "e5m2": True, "e4m3": True, "mxfp4": False}      # (no scale byte 255)
# whether a mean over three entries of the format can be an fp32 denormal (the format's smallest normal / 3 below 2^-126)
HAS_DENORMAL_MEAN = {"fp32": True, "fp16": False, "bf16": True, "e5m2": False, "e4m3": False, "mxfp4": True}
MX_SCALES = (0, 1, 2, 126, 127, 128, 253, 254)            # both ends of the range, never 255
_MX_SCALE_P = (0.14, 0.14, 0.12, 0.17, 0.19, 0.17, 0.035, 0.035)


def palette(dtype):
    """[(name, value, weight)] for a float dtype: inf and NaN rare enough that the reference's NaN share stays under the cap."""
    d1, d2, mn, mx, big = _FMT[dtype]
    p = [("+0", 0.0, 11), ("-0", -0.0, 11), ("+den", d1, 6), ("-den", -d1, 6), ("+den2", d2, 5), ("-den2", -d2, 5),
         ("minnorm", mn, 7), ("+max", mx, 3), ("-max", -mx, 3), ("+1", 1.0, 12), ("-1", -1.0, 12), ("3", 3.0, 9), ("big", big, 6)]
    if HAS_INF[dtype]:
        p += [("+inf", float("inf"), 1.2), ("-inf", float("-inf"), 1.2)]
    p += [("nan", float("nan"), 1.2)]
    return p


def special_table(rows, dim, dtype, seed):
    """A table of `rows` x `dim` special values.  Returns a namespace: dtype, dim, rows, wide (float32 numpy, the exact widening),
    table (what load_table takes: a torch CPU tensor; for MXFP4 fused uint8 rows, to be loaded with dtype=EMB_MXFP4),
    named {name: row id} -- rows filled with one palette value each, which the crafted bags are made of."""
    rng = np.random.default_rng(seed)
    if dtype == "mxfp4":
        assert dim % 32 == 0
        blocks = dim // 32
        n_pure = 16 * len(MX_SCALES)
        assert rows > n_pure + 8
        nib = rng.integers(0, 16, size=(rows, dim), dtype=np.uint8)
        sc = rng.choice(np.array(MX_SCALES, np.uint8), size=(rows, blocks), p=np.array(_MX_SCALE_P) / sum(_MX_SCALE_P))
        for si, s in enumerate(MX_SCALES):
            for n in range(16):
                nib[si * 16 + n], sc[si * 16 + n] = n, s
        fused = formats.mxfp4_join(nib[:, 0::2] | (nib[:, 1::2] << 4), sc)
        wide = formats.from_mxfp4(fused, dim)
        row = lambda s, n: MX_SCALES.index(s) * 16 + n   # noqa: E731
        named = {"+0": row(127, 0), "-0": row(127, 8), "+1": row(127, 2), "-1": row(127, 10), "3": row(127, 5),
                 "minnorm": row(1, 2), "+inf": row(254, 7), "-inf": row(254, 15), "+den": row(0, 1)}
        assert np.isinf(wide[named["+inf"]]).all() and (wide[named["minnorm"]] == np.float32(2.0 ** -126)).all()
        assert not np.isnan(wide).any() and np.signbit(wide[named["-0"]]).all() and (wide[named["-0"]] == 0).all()
        return SimpleNamespace(dtype=dtype, dim=dim, rows=rows, wide=wide, table=fused, named=named, n_pure=n_pure)
    pal = palette(dtype)
    assert rows > len(pal) + 8
    vals = np.array([v for _n, v, _w in pal], np.float32)
    p = np.array([w for _n, _v, w in pal], np.float64)
    values = vals[rng.choice(len(pal), size=(rows, dim), p=p / p.sum())]
    named = {}
    for r, (name, v, _w) in enumerate(pal):
        values[r], named[name] = v, r
    table = torch.from_numpy(values).to(TORCH_DTYPE[dtype])
    wide = table.float().numpy()
    ok = np.isnan(values) | (wide.view(np.uint32) == values.view(np.uint32))
    assert ok.all() and np.array_equal(np.isnan(wide), np.isnan(values)), "a palette value is not exact in " + dtype
    return SimpleNamespace(dtype=dtype, dim=dim, rows=rows, wide=wide, table=table, named=named, n_pure=len(pal))


def special_bags(tab, n_bags, seed):
    """Ragged bags of 0 .. 12 entries over a special_table(), with padding.  The first bags are crafted from the table's pure
    rows; `edges` maps each edge to its bag, or to None where the format cannot express it (HAS_INF / HAS_NAN /
    HAS_DENORMAL_MEAN).  Returns a namespace: idx, off (int64), w (float32), pad, lens, edges."""
    rng = np.random.default_rng(seed)
    nm, dt = tab.named, tab.dtype
    pad = tab.n_pure + 3                                   # a row of random palette values: an ordinary row where padding is off
    crafted = [("max keeps -0", [nm["-0"], nm["+0"]]),
               ("max keeps +0", [nm["+0"], nm["-0"]]),
               ("max keeps -0 behind padding", [pad, nm["-0"], pad, nm["+0"], nm["-0"]]),
               ("nan first in max", [nm["nan"], nm["+1"], nm["3"]] if HAS_NAN[dt] else None),
               ("nan later in max", [nm["+1"], nm["nan"], nm["-1"]] if HAS_NAN[dt] else None),
               ("nan first behind padding", [pad, nm["nan"], nm["3"]] if HAS_NAN[dt] else None),
               ("denormal mean of 3", [nm["minnorm"], nm["+0"], nm["-0"]] if HAS_DENORMAL_MEAN[dt] else None),
               ("denormal mean of 3 behind padding", [pad, nm["minnorm"], pad, nm["+0"], nm["+0"], pad] if HAS_DENORMAL_MEAN[dt] else None),
               ("+inf mean", [nm["+inf"], nm["+1"], nm["+1"]] if HAS_INF[dt] else None),
               ("-inf mean", [nm["-1"], nm["-inf"], nm["3"]] if HAS_INF[dt] else None),
               ("mean of 3 below the format's normals", [nm["minnorm"], nm["-0"], nm["+0"]]),
               ("weighted beyond the format's largest", [nm["+max"]] if dt != "mxfp4" else None),
               ("empty", []),
               ("all padding", [pad, pad, pad])]
    edges, bags = {}, []
    for name, b in crafted:
        edges[name] = None if b is None else len(bags)
        if b is not None:
            bags.append(np.array(b, np.int64))
    n_rand = n_bags - len(bags)
    assert n_rand > 50
    rl = rng.integers(0, 13, size=n_rand)
    for k, L in enumerate(rl):
        b = rng.integers(0, tab.rows, size=int(L))
        b[rng.random(int(L)) < 0.15] = pad
        if L and k % 9 == 0:
            b[0] = pad                                     # the first entry is padding
        if L and k % 31 == 0:
            b[:] = pad
        bags.append(b.astype(np.int64))
    lens = np.array([len(b) for b in bags], np.int64)
    off = np.zeros(len(bags), np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    idx = np.concatenate(bags) if lens.sum() else np.zeros(0, np.int64)
    w = rng.standard_normal(len(idx)).astype(np.float32)
    w[3::23], w[5::29], w[7::19] = np.float32(0.0), np.float32(-0.0), TINY_W
    w[:int(off[edges["empty"]])] = rng.standard_normal(int(off[edges["empty"]])).astype(np.float32)    # (ordinary weights on the crafted bags)
    if edges["weighted beyond the format's largest"] is not None:          # finite in fp32 for the 2-byte formats, beyond their largest
        w[off[edges["weighted beyond the format's largest"]]] = OVER_W
    return SimpleNamespace(idx=idx, off=off, w=w, pad=pad, lens=lens, edges=edges, n_crafted=n_bags - n_rand)


NAN_CAP = 0.25


def check_special_case(tab, sb, refs):
    """What a special case must contain, asserted on the REFERENCE outputs `refs` {spec name: float32 [bags, dim]} (SPECS and
    SPECS_NO_PAD): the NaN cap and one of each edge.  Raises AssertionError naming what is missing."""
    u = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)   # noqa: E731
    for name, r in refs.items():
        assert np.isnan(r).mean() <= NAN_CAP, "%s: %.1f %% of the reference is NaN" % (name, 100 * np.isnan(r).mean())
    e = sb.edges
    NEG0 = 0x80000000
    for mx in (refs["max+pad"], refs["max"]):
        assert (u(mx[e["max keeps -0"]]) == NEG0).all() and (u(mx[e["max keeps +0"]]) == 0).all()
    assert (u(refs["max+pad"][e["max keeps -0 behind padding"]]) == NEG0).all()
    if HAS_NAN[tab.dtype]:
        for mx in (refs["max+pad"], refs["max"]):
            assert np.isnan(mx[e["nan first in max"]]).all() and (mx[e["nan later in max"]] == 1.0).all()
        assert np.isnan(refs["max+pad"][e["nan first behind padding"]]).all()
    else:
        assert e["nan first in max"] is None and e["nan later in max"] is None
    if HAS_DENORMAL_MEAN[tab.dtype]:
        for b in (e["denormal mean of 3"], e["denormal mean of 3 behind padding"]):
            q = refs["mean+pad"][b]
            assert ((q > 0) & (q < np.float32(2.0 ** -126))).all(), q[:4]
            assert (sb.idx[sb.off[b]:sb.off[b] + sb.lens[b]] != sb.pad).sum() == 3
    else:
        assert e["denormal mean of 3"] is None
    if HAS_INF[tab.dtype]:
        for m in (refs["mean+pad"], refs["mean"]):
            assert (m[e["+inf mean"]] == np.inf).all() and (m[e["-inf mean"]] == -np.inf).all()
    else:
        assert e["+inf mean"] is None and e["-inf mean"] is None
    q = refs["mean+pad"][e["mean of 3 below the format's normals"]]
    assert (q == np.float32(tab.wide[tab.named["minnorm"], 0]) / np.float32(3)).all() and (q > 0).all()
    if e["weighted beyond the format's largest"] is not None:
        for name in ("weighted", "weighted+pad"):
            r = refs[name][e["weighted beyond the format's largest"]]
            assert (r > tab.wide[tab.named["+max"], 0]).all(), name     # (fp32 tables: +inf; 2-byte tables: finite, inf once rounded)
    for name, r in refs.items():
        assert (u(r[e["empty"]]) == 0).all(), name
        if SPECS.get(name, (0, 0, False))[2]:
            assert (u(r[e["all padding"]]) == 0).all(), name
    # ... and among the random bags: -0 and denormal outputs, so that the edges are not the crafted bags' alone
    assert (u(refs["max+pad"][sb.n_crafted:]) == NEG0).any() and (u(refs["sum+pad"]) == 0).any()
    if tab.dtype in ("fp32", "bf16", "mxfp4"):
        for name in ("sum+pad", "mean+pad", "weighted", "weighted+pad"):
            r = refs[name]
            assert ((r != 0) & (np.abs(r) < np.float32(2.0 ** -126))).any(), name + ": no denormal output"
