"""CPU: the max-mode backward's definition.  tests/grad_max_ref.py against torch's CPU autograd on inputs whose sums are exact in any
order, and the one-element rule of csrc/pimemb_grad_max.h, compiled on the host, against the same loop.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_max_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
F = np.float32


def exact_batch(dim):
    """7 rows of small integers -- rows 1 and 2 equal at the even elements (ties between two rows), row 3 twice in bag 0, row 5 the
    padding id, one padding-only and one empty bag -- and an integer-valued G: every sum is exact."""
    rng = np.random.default_rng(7 + dim)
    table = rng.integers(-3, 4, size=(7, dim)).astype(F)
    table[2, 0::2] = table[1, 0::2]
    lens = [4, 0, 3, 2, 5, 1]
    ids = np.array([3, 1, 3, 2, 2, 1, 5, 5, 5, 0, 5, 4, 1, 6, 6], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    G = rng.integers(-8, 9, size=(len(lens), dim)).astype(F)
    return table, ids, offsets, G


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dim", [1, 4, 6])
def test_the_loop_equals_torch_cpu_autograd_on_exact_sums(dim, padded):
    import torch
    table, ids, offsets, G = exact_batch(dim)
    pad = 5 if padded else None
    w = torch.from_numpy(table.copy()).requires_grad_(True)
    torch.nn.functional.embedding_bag(torch.from_numpy(ids), w, torch.from_numpy(offsets), mode="max", padding_idx=pad).backward(torch.from_numpy(G))
    rows, grads, n_bad, win = mr.sparse_grad("f32", table.view(np.uint8), ids, offsets, G, pad)
    dense = np.zeros_like(table)
    dense[rows] = grads
    assert n_bad == 0 and np.array_equal(dense, w.grad.numpy()), (dense, w.grad.numpy())
    assert (win[1] == mr.NO_WINNER).all() and ((win[3] == mr.NO_WINNER).all() if padded else (win[3] != mr.NO_WINNER).all())
    assert set(win[0]) <= {0, 1, 2, 3} and 2 not in win[0], "row 3 twice in bag 0: its first position keeps every tie"
    assert sorted(rows) == sorted(set(ids.tolist()) - ({5} if padded else set()))      # U lists rows that win nowhere too


def test_the_rule_of_the_header_on_zeros_ties_and_subnormals(tmp_path):
    exe = tmp_path / "grad_max_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "grad_max_check.cpp"),
                           "-o", str(exe)])
    sub = np.array([1, 2], dtype=np.uint32).view(F)                      # the two smallest subnormals
    for values in ([F(-0.0), F(0.0), F(-0.0)], [F(0.0), F(-0.0)], [F(2.0), F(2.0), F(3.0), F(3.0)], [sub[0], sub[1], sub[0]],
                   [-sub[1], -sub[0], F(-0.0), F(0.0), sub[0]], [F(-5.0)], [F(1.0), F(-np.inf), F(np.inf), F(np.inf)]):
        table = np.array(values, dtype=F).reshape(-1, 1)
        ids = np.arange(len(values), dtype=np.int64)
        want = [int(mr.winners("f32", table.view(np.uint8), ids[:k + 1], np.zeros(1, np.int64))[0][0, 0]) for k in range(len(values))]
        out = subprocess.check_output([str(exe)] + ["%08x" % int(v.view(np.uint32)) for v in table[:, 0]], text=True).split("\n")
        assert [int(x) for x in out[0].split()] == want, (values, out[0], want)
        assert out[1] == "1 00000000"                                    # a lost element contributes +0, whatever the gradient's sign
    assert want == [0, 0, 2, 2]
