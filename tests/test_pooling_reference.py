"""The pooling rules the bag_pool_* kernels follow (tests/pool_ref.py) against live torch CPU F.embedding_bag, bit for bit:
every mode, weighted sums with and without padding_idx, empty bags and bags of padding only, ragged bags, several row
widths, fp16 tables through .float(), int32 and int64 ids.  CPU only: this pins the arithmetic the GPU must reproduce."""
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
