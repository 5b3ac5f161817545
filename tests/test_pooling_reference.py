"""The pooling rules the bag_pool_* kernels follow (tests/pool_ref.py) against live torch CPU F.embedding_bag, bit for bit:
every mode, weighted sums with and without padding_idx, empty bags and bags of padding only, ragged bags, several row
widths, fp16 tables through .float(), int32 and int64 ids.  CPU only: this pins the arithmetic the GPU must reproduce.
The second half proves the inputs of tests/test_gpu_pooled_edges.py (tests/pool_cases.py): the wave-batch layouts hold every
class of 64-bag step, the special-value cases stay under the NaN cap and contain each edge, and on all of them torch and
pool_ref agree on every NaN position and every other bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def make_case(seed, dim, n_rows=50, n_bags=24, max_len=40, dtype=np.float32):
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((n_rows, dim)).astype(dtype)
    table[3] = 0.0                              # +0 / -0 rows: max keeps the first of equal values
    table[4] = -0.0
    lens = rng.integers(0, max_len + 1, n_bags)
    lens[0], lens[1] = 0, 3                     # an empty bag; a short one
    idx = rng.integers(0, n_rows, int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    w = rng.standard_normal(len(idx)).astype(np.float32)
    return table, idx, off, w


def torch_bag(table, idx, off, mode, w=None, padding_idx=None, id_dtype=torch.int64):
    t = torch.from_numpy(np.ascontiguousarray(table)).float()
    out = F.embedding_bag(torch.from_numpy(idx).to(id_dtype), t, torch.from_numpy(off).to(id_dtype), mode=mode,
                          per_sample_weights=None if w is None else torch.from_numpy(w), padding_idx=padding_idx)
    return out.numpy()


@pytest.mark.parametrize("dim", [2, 3, 16, 100, 128, 257])
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("padding", [None, 7])
def test_modes_match_torch_bit_for_bit(dim, mode, padding):
    table, idx, off, _ = make_case(dim * 7 + len(mode), dim)
    if padding is not None:
        idx[off[2]:off[2] + 5] = padding        # part of a bag
        lens = np.diff(np.concatenate([off, [len(idx)]]))
        b = int(np.argmax(lens > 0) if lens[3] == 0 else 3)
        idx[off[b]:off[b] + lens[b]] = padding  # a bag of padding only
    want = torch_bag(table, idx, off, mode, padding_idx=padding)
    got = pool_ref.embedding_bag(table, idx, off, mode, padding_idx=padding)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("dim", [2, 3, 16, 100, 128, 257])
@pytest.mark.parametrize("padding", [None, 5])
def test_weighted_sum_matches_torch_bit_for_bit(dim, padding):
    table, idx, off, w = make_case(dim * 11 + 1, dim)
    if padding is not None:
        idx[::4] = padding
    want = torch_bag(table, idx, off, "sum", w=w, padding_idx=padding)
    got = pool_ref.embedding_bag(table, idx, off, "sum", per_sample_weights=w, padding_idx=padding)
    assert np.array_equal(bits(got), bits(want))


def test_fma_and_mul_add_rules_are_different_arithmetic():
    """The two weighted rules are not the same function: a restatement that used one for both would not pass above."""
    table, idx, off, w = make_case(3, 128, n_bags=64)
    fused = pool_ref.embedding_bag(table, idx, off, "sum", per_sample_weights=w)
    rows = table[idx] * w[:, None]
    unfused = np.stack([rows[a:b].sum(0, dtype=np.float32) if b > a else np.zeros(128, np.float32)
                        for a, b in zip(off, np.concatenate([off[1:], [len(idx)]]))])
    assert not np.array_equal(bits(fused), bits(unfused))


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64])
def test_fp16_tables_and_index_widths(mode, id_dtype):
    table, idx, off, _ = make_case(17, 24, dtype=np.float16)
    want = torch_bag(table.astype(np.float32), idx, off, mode, padding_idx=9, id_dtype=id_dtype)
    got = pool_ref.embedding_bag(table, idx, off, mode, padding_idx=9)
    assert np.array_equal(bits(got), bits(want))


def test_signed_zeros_in_max_and_empty_bags():
    table = np.array([[0.0, -0.0], [-0.0, 0.0], [1.0, 2.0]], dtype=np.float32)
    idx, off = np.array([0, 1, 1, 0, 2, 2], dtype=np.int64), np.array([0, 2, 4, 4, 5], dtype=np.int64)
    got = pool_ref.embedding_bag(table, idx, off, "max", padding_idx=2)
    want = torch_bag(table, idx, off, "max", padding_idx=2)
    assert np.array_equal(bits(got), bits(want))
    assert bits(got[0]).tolist() == bits([0.0, -0.0]).tolist()       # first of equal values stays
    assert bits(got[2]).tolist() == [0, 0] and bits(got[3]).tolist() == [0, 0]   # empty, padding only: +0
    for mode in ("sum", "mean"):
        assert np.array_equal(bits(pool_ref.embedding_bag(table, idx, off, mode, padding_idx=2)),
                              bits(torch_bag(table, idx, off, mode, padding_idx=2)))


# ---- the case builder of the pooled edge tests (tests/pool_cases.py), proven here before any GPU time is spent -----------------
import pool_cases  # noqa: E402

WB_B = 131072 + 5


def quiet_ref(*args):
    """pool_ref over special values: numpy's overflow / invalid warnings are the point of the data, not news."""
    with np.errstate(all="ignore"):
        return pool_ref.embedding_bag(*args)


def nan_and_bits_equal(got, want):
    g, w = bits(got), bits(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(g[~np.isnan(want)], w[~np.isnan(want)])


def cut(c, bags):
    """The bags `bags` of a case as a case of their own: (idx, off, w)."""
    lens = c.lens[bags]
    take = np.concatenate([np.arange(c.off[b], c.off[b] + c.lens[b]) for b in bags]) if lens.sum() else np.zeros(0, np.int64)
    off = np.zeros(len(bags), np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    return c.idx[take], off, c.w[take]


@pytest.mark.parametrize("unroll,tail", [(4, "general"), (8, "shifted"), (8, "general"), (4, "shifted")])
def test_wave_batch_case_meets_its_conditions(unroll, tail):
    rows = 3000
    c = pool_cases.wave_batch_case(rows, WB_B, unroll, seed=unroll, tail=tail)
    pool_cases.check_wave_batch_case(c, WB_B)
    assert c.tail_class == tail and len(c.classes) == 2049
    assert (c.lens == 1).sum() > 0.9 * WB_B                                    # most bags have one index
    assert sorted(c.long_lens) == sorted(set(pool_cases.long_lengths(unroll))) and set(np.unique(c.lens)) == {0, 1} | set(c.long_lens)
    # padding where the issue wants it: the first / last entry, the whole, a full unroll chunk of a long bag, both sides of a
    # chunk boundary; a one-index bag
    assert all(c.pad_patterns[k] >= 2 for k in ("first", "last", "all", "chunk", "boundary", "none")), c.pad_patterns
    is_pad = c.idx == c.pad
    seen = dict.fromkeys(("first", "last", "all", "chunk", "boundary"), 0)
    for b in c.long_bags:
        m = is_pad[c.off[b]:c.off[b] + c.lens[b]]
        seen["first"] += bool(m[0] and not m.all())
        seen["last"] += bool(m[-1] and not m.all())
        seen["all"] += bool(m.all())
        seen["chunk"] += any(m[k:k + unroll].all() for k in range(0, len(m) - unroll + 1, unroll)) and not m.all()
        seen["boundary"] += bool(len(m) > unroll and m[unroll - 1] and m[unroll] and not m[:unroll].all())
    assert all(v >= 2 for v in seen.values()), seen
    assert all(is_pad[c.off[b]:c.off[b] + c.lens[b]].all() for b in c.emptied) and (c.lens[c.emptied] == 1).sum() >= 8
    assert (c.idx < rows).all() and (c.idx >= 0).all() and c.off[-1] + c.lens[-1] == len(c.idx)
    # weights: +0, -0, a denormal product with a table entry, normals
    table = np.random.default_rng(1).standard_normal((rows, 4)).astype(np.float32)
    prod = c.w[:, None] * table[c.idx]
    assert ((prod != 0) & (np.abs(prod) < np.float32(2.0 ** -126))).any()
    assert (bits(c.w) == 0).any() and (bits(c.w) == -2**31).any() and (np.abs(c.w) > 0.5).mean() > 0.4
    # the same builder call gives the same case
    d = pool_cases.wave_batch_case(rows, WB_B, unroll, seed=unroll, tail=tail)
    assert np.array_equal(c.idx, d.idx) and np.array_equal(c.off, d.off) and np.array_equal(bits(c.w), bits(d.w))
    # torch and the numpy restatement agree, bit for bit, on every bag of every step that is not plain one-hot, and on the
    # first two steps
    steps = [s for s, k in enumerate(c.classes) if k in ("general", "shifted")] + [0, 1]
    bags = np.concatenate([np.arange(64 * s, min(64 * s + 64, WB_B)) for s in sorted(steps)])
    idx, off, w = cut(c, bags)
    for name, spec in pool_cases.SPECS.items():
        want = pool_cases.reference(table, c.idx, c.off, spec, c.w, c.pad)
        got = quiet_ref(table, idx, off, spec[0], w if spec[1] else None, c.pad if spec[2] else None)
        assert np.array_equal(bits(got), bits(want[bags])), name
        if spec[2]:
            assert not bits(want[c.emptied]).any(), name                       # emptied by padding: +0


SPECIAL_DIMS = {"fp32": (16, 3), "fp16": (16, 10), "bf16": (16, 36), "e4m3": (16, 10), "e5m2": (128, 36), "mxfp4": (32, 128)}


def special_refs(tab, sb):
    specs = dict(pool_cases.SPECS, **pool_cases.SPECS_NO_PAD)
    return {n: pool_cases.reference(tab.wide, sb.idx, sb.off, s, sb.w, sb.pad) for n, s in specs.items()}, specs


@pytest.mark.parametrize("dtype", pool_cases.DTYPES)
def test_special_cases_meet_their_conditions(dtype):
    for dim in SPECIAL_DIMS[dtype]:
        tab = pool_cases.special_table(400, dim, dtype, seed=dim)
        sb = pool_cases.special_bags(tab, 600, seed=dim + 1)
        assert sb.lens.max() == 12 and sb.lens.min() == 0 and len(sb.off) == 600 and (sb.idx < 400).all()
        refs, specs = special_refs(tab, sb)
        pool_cases.check_special_case(tab, sb, refs)                           # the NaN cap, one of each edge
        for n, s in specs.items():                                             # all seven mode / weights / padding combinations
            got = quiet_ref(tab.wide, sb.idx, sb.off, s[0], sb.w if s[1] else None, sb.pad if s[2] else None)
            assert nan_and_bits_equal(got, refs[n]), (dim, n)
        # the palette is all there: every named value in the table, signed zeros and denormals in the outputs
        if dtype != "mxfp4":
            assert len(tab.named) == len(pool_cases.palette(dtype))
            assert np.isnan(tab.wide).mean() < 0.02 and (pool_cases.HAS_INF[dtype] == bool(np.isinf(tab.wide).any()))
        else:
            el, sc = pool_cases.formats.mxfp4_split(tab.table, dim)
            assert set(np.unique(sc)) == set(pool_cases.MX_SCALES) and len(np.unique(np.concatenate([el & 15, el >> 4]))) == 16


@pytest.mark.parametrize("dtype", ["fp32", "e5m2"])
def test_special_bags_tiled_into_the_wave_batch_layout(dtype):
    """The special bags as the long bags of a wave-batch layout: still one-hot-ish, still under the NaN cap, torch and the
    numpy restatement still agree."""
    tab = pool_cases.special_table(400, 16, dtype, seed=5)
    sb = pool_cases.special_bags(tab, 600, seed=6)
    c = pool_cases.wave_batch_case(400, WB_B, 4 if dtype == "fp32" else 8, seed=7, fill=sb)
    pool_cases.check_wave_batch_case(c, WB_B)
    assert c.pad == sb.pad and len(np.unique(c.idx)) == 400                   # every row of the table is looked up
    steps = [s for s, k in enumerate(c.classes) if k in ("general", "shifted")] + [0, 1]
    bags = np.concatenate([np.arange(64 * s, min(64 * s + 64, WB_B)) for s in sorted(steps)])
    idx, off, w = cut(c, bags)
    for name, spec in pool_cases.SPECS.items():
        want = pool_cases.reference(tab.wide, c.idx, c.off, spec, c.w, c.pad)
        assert np.isnan(want).mean() <= pool_cases.NAN_CAP, name
        got = quiet_ref(tab.wide, idx, off, spec[0], w if spec[1] else None, c.pad if spec[2] else None)
        assert nan_and_bits_equal(got, want[bags]), name
    mx = pool_cases.reference(tab.wide, c.idx, c.off, pool_cases.SPECS["max+pad"], c.w, c.pad)[c.long_bags]
    assert (bits(mx) == -2**31).any() and np.isnan(mx).any()                  # -0 and NaN results of max among the long bags
