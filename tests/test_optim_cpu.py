"""CPU: the fused Adagrad steps of the backward pass (include/pimemb_grad.h, THE ADAGRAD STEPS).  tests/optim_ref.py, the definition
as a loop, is pinned against torch.optim.Adagrad on the exact batch; the one-element arithmetic the kernels compile
(csrc/pimemb_grad_optim.h), run on the host, agrees with optim_ref bit for bit; and the new ABI is what the header says.  No GPU
work is called."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as gc  # noqa: E402
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402

ROOT = gr.ROOT
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
F = np.float32


def hexbits(x):
    return "%08x" % int(F(x).view(np.uint32))


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- optim_ref against torch.optim.Adagrad, on the exact batch ---------------------------------------------------------------------
def correctly_rounded_sqrt(s):
    """RN(sqrt(s)) for float32 s: the double-precision root rounded once more (53 >= 2 * 24 + 2 bits: the double rounding is
    innocuous for square roots).  numpy's own float32 sqrt has to agree with it: optim_ref relies on that."""
    with np.errstate(invalid="ignore"):
        want = np.sqrt(np.asarray(s, F).astype(np.float64)).astype(F)
        assert np.array_equal(bits(np.sqrt(np.asarray(s, F))), bits(want))
    return want


@pytest.mark.parametrize("mode_name", ["sum", "mean", "sum+pad", "mean+pad"])
def test_optim_ref_equals_torchs_sparse_adagrad_on_the_exact_batch(mode_name):
    """Three rounds (G scaled by 1, 2, 3) of nn.EmbeddingBag(sparse=True) + torch.optim.Adagrad(lr = 2^-6, eps = 1e-10) on
    arbitrary fp32 weights, against optim_ref after every round.  lr is a power of two: lr * x is exact, so the comparison does
    not depend on whether torch fuses its add_(alpha=).
      state["sum"]   bit for bit, every element, every round: sums of squares of small integers, exact in any arithmetic.
      W              bit for bit on every element whose square roots torch itself computes as the definition does.  The
                     definition's sqrt is the IEEE correctly rounded one; torch's CPU sqrt is a vendor routine that need not be
                     (it may be off by an ulp on an inexact root).  So the test asks torch for sqrt(S') of the very states of each
                     round and compares them with the correctly rounded roots: where they agree -- everywhere, with a correctly
                     rounding torch, and always where the root is exact -- W must equal torch's W in every bit, that round and
                     after; an element whose root torch rounded differently in some round says nothing about optim_ref from then
                     on and is left out (the count is printed).  What torch's W is compared on is decided by torch's sqrt
                     alone, never by the values under test."""
    import torch
    mode, _weighted, padded = gc.MODES[mode_name]
    ids, offsets, G, _w = gc.exact_batch(padded)
    lr, eps = 2.0 ** -6, 1e-10
    w0 = (np.random.default_rng(11).standard_normal((gc.EXACT_ROWS, 8)) * 3).astype(F)
    bag = torch.nn.EmbeddingBag(gc.EXACT_ROWS, 8, mode=mode, sparse=True, padding_idx=gc.PAD if padded else None, _weight=torch.from_numpy(w0.copy()))
    opt = torch.optim.Adagrad(bag.parameters(), lr=lr, eps=eps)
    table, state = w0.view(np.uint8).reshape(gc.EXACT_ROWS, -1).copy(), np.zeros((gc.EXACT_ROWS, 8), F)
    comparable = np.ones((gc.EXACT_ROWS, 8), dtype=bool)
    for scale in (1, 2, 3):
        Gs = (G * F(scale)).astype(F)
        opt.zero_grad()
        (bag(torch.from_numpy(ids), torch.from_numpy(offsets)) * torch.from_numpy(Gs)).sum().backward()
        opt.step()
        rows, grads, n_bad = gr.sparse_grad(gc.EXACT_ROWS, ids, offsets, Gs, mode, None, gc.PAD if padded else None)
        assert n_bad == 0 and len(rows) > 20
        table, state = orf.adagrad_step("f32", table, state, rows, grads, lr, eps)
        assert np.array_equal(bits(state), bits(opt.state[bag.weight]["sum"].numpy())), (mode_name, scale)
        root = correctly_rounded_sqrt(state)
        torch_root = torch.from_numpy(state.copy()).sqrt_().numpy()            # (in place on a contiguous tensor, as the optimizer calls it)
        agrees = bits(torch_root) == bits(root)
        exact = root.astype(np.float64) ** 2 == state.astype(np.float64)
        assert agrees[exact].all(), (mode_name, scale)                           # an exact root is exact with any sqrt worth the name
        comparable &= agrees
        differ = table.view(np.uint32) != bits(bag.weight.detach().numpy())
        print(f"{mode_name} round {scale}: torch's sqrt differs from the correctly rounded root in {int((~agrees).sum())} of {agrees.size} elements; "
              f"W differs from torch's in {int(differ.sum())}, of them comparable {int((differ & comparable).sum())}")
        assert not (differ & comparable).any(), (mode_name, scale, np.argwhere(differ & comparable)[:4])
        assert (scale != 1 or exact.all()) and comparable.mean() > 0.5           # (round 1's roots |g| are all exact; a sqrt that is mostly wrong is no reference)
    assert not np.array_equal(table.view(np.uint32), bits(w0)) and state.any()


# ---- the one-element arithmetic on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def optim_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("optim") / "optim_step_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "optim_step_check.cpp"), "-o", str(exe)])
    return str(exe)


def grid():
    """(S, g) pairs: S in {0, a denormal, 1e-12, ordinary, 1e30} x g in {+-0, denormals, ordinary values over +-2^+-20}."""
    rng = np.random.default_rng(21)
    s_vals = np.concatenate([[0.0], np.array([1, 0x00400000], np.uint32).view(F), [1e-12, 1e30], np.abs(rng.standard_normal(8)) * 3]).astype(F)
    g_vals = np.concatenate([[0.0, -0.0], np.array([1, 0x80000001, 0x007FFFFF, 0x00400000], np.uint32).view(F),
                             rng.standard_normal(82) * np.exp2(rng.integers(-20, 21, size=82))]).astype(F)
    S, g = np.meshgrid(s_vals, g_vals, indexing="ij")
    return S.reshape(-1).copy(), g.reshape(-1).copy()


def stored_weights(kind, n):
    rng = np.random.default_rng(22)
    return gr.encode(kind, (rng.standard_normal((n, 1)) * 3).astype(F))      # uint8 [n, element size]


def files(tmp_path, **arrays):
    out = {}
    for name, a in arrays.items():
        out[name] = str(tmp_path / (name + ".bin"))
        np.ascontiguousarray(a).tofile(out[name])
    return out


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_adagrad_element_equals_optim_ref(optim_exe, tmp_path, kind):
    S, g = grid()
    n = len(S)
    assert n >= 13 * 88
    raw = stored_weights(kind, n)
    lr, eps = F(0.1), F(1e-10)
    f = files(tmp_path, w=raw, g=g, s=S)
    ow, os_ = str(tmp_path / "ow.bin"), str(tmp_path / "os.bin")
    subprocess.check_call([optim_exe, "adagrad", kind, hexbits(lr), hexbits(eps), f["w"], f["g"], f["s"], ow, os_])
    got_w, got_s = np.fromfile(ow, np.uint8).reshape(raw.shape), np.fromfile(os_, F)
    new, want_s = orf.adagrad_values(gr.decode(kind, raw)[:, 0], g, S, lr, eps)
    want_w = gr.encode(kind, new[:, None])
    bad = np.flatnonzero((got_w != want_w).any(axis=1) | (bits(got_s) != bits(want_s)))
    assert bad.size == 0, (kind, S[bad[:4]], g[bad[:4]], got_w[bad[0]], want_w[bad[0]], got_s[bad[0]], want_s[bad[0]])
    assert np.isfinite(want_s).all() and (want_s[np.abs(g) > 1e-10] > 0).all()


@pytest.mark.parametrize("dim", [4, 48, 320])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_rowwise_chain_equals_optim_ref(optim_exe, tmp_path, kind, dim):
    """m -> S' -> step and step * g: v is optim_ref's tree sum of a row of `dim` copies of the grid's g (and of random rows)."""
    S, g = grid()
    n = len(S)
    rng = np.random.default_rng(dim)
    rows = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-20, 21, size=(n, 1)))).astype(F)
    rows[::2] = g[::2, None]                                                      # every other row: the grid's g in every element
    rows[:, 0] = g
    v = np.array([orf.pair_tree(r) for r in rows], dtype=F)
    raw = stored_weights(kind, n)
    lr, eps = F(0.1), F(1e-10)
    f = files(tmp_path, w=raw, g=g, s=S, v=v)
    ow, os_, ostep = str(tmp_path / "ow.bin"), str(tmp_path / "os.bin"), str(tmp_path / "ostep.bin")
    subprocess.check_call([optim_exe, "rowwise", kind, hexbits(lr), hexbits(eps), str(dim), f["w"], f["g"], f["s"], f["v"], ow, os_, ostep])
    got_w, got_s, got_step = np.fromfile(ow, np.uint8).reshape(raw.shape), np.fromfile(os_, F), np.fromfile(ostep, F)
    w = gr.decode(kind, raw)[:, 0]
    for k in range(n):
        step, s1 = orf.rowwise_step_size(v[k], dim, S[k], lr, eps)
        with np.errstate(all="ignore"):
            prod = step * g[k]
            new = w[k] - prod
        want_w = gr.encode(kind, np.array([[new]], F))[0]
        assert bits(got_step[k]) == bits(step) and bits(got_s[k]) == bits(s1), (kind, dim, k, v[k], S[k], got_step[k], step, got_s[k], s1)
        assert np.array_equal(got_w[k], want_w), (kind, dim, k, g[k], step, got_w[k], want_w)


def test_pair_tree_is_the_tree_of_the_definition():
    """Against an independent spelling: the xor butterfly over L lanes, lane l holding pieces l and l + 64."""
    rng = np.random.default_rng(5)
    for dim in (4, 8, 48, 256, 320, 512):
        g = (rng.standard_normal(dim) * np.exp2(rng.integers(-8, 8, size=dim))).astype(F)
        sq = g * g
        t = [F(F(F(sq[4 * c] + sq[4 * c + 1]) + sq[4 * c + 2]) + sq[4 * c + 3]) for c in range(dim // 4)]
        L = min(64, 1 << (len(t) - 1).bit_length())
        lanes = [t[l] if l < len(t) else F(0) for l in range(L)]
        lanes = [F(lanes[l] + t[l + 64]) if l + 64 < len(t) else lanes[l] for l in range(L)]
        h = 1
        while h < L:
            lanes = [F(lanes[l] + lanes[l ^ h]) for l in range(L)]
            h *= 2
        assert len({int(x.view(np.uint32)) for x in lanes}) == 1                  # every lane ends with the same bits
        assert bits(lanes[0]) == bits(orf.pair_tree(g)), dim
        assert abs(float(lanes[0]) - float(np.sum(sq.astype(np.float64)))) <= 1e-5 * float(lanes[0])


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_state_floats(pel):
    G = pel.lib.load_grad()
    assert pel.lib.EMB_OPT_ADAGRAD == 1 and pel.lib.EMB_OPT_ROWWISE_ADAGRAD == 2
    assert G.emb_opt_state_floats(1, 3001, 48) == 3001 * 48
    assert G.emb_opt_state_floats(2, 3001, 48) == 3001
    assert G.emb_opt_state_floats(1, 1 << 22, 128) == (1 << 29) and G.emb_opt_state_floats(2, 1 << 22, 128) == 1 << 22
    assert G.emb_opt_state_floats(1, (1 << 32) - 2, 512) == ((1 << 32) - 2) * 512      # 64-bit arithmetic
    assert G.emb_opt_state_floats(0, 10, 10) == 0 and G.emb_opt_state_floats(3, 10, 10) == 0
    assert G.emb_opt_state_floats(1, 0, 8) == 0


def test_header_compiles_as_c_and_cxx_and_the_spec_matches(pel, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pimemb_grad.h"\nint main(void){emb_opt_spec s = {EMB_OPT_ROWWISE_ADAGRAD, 0.1f, 0.f, 0};\n'
                   'printf("%zu %zu %zu %zu %zu %u %d %d\\n", sizeof(emb_opt_spec), offsetof(emb_opt_spec, kind), offsetof(emb_opt_spec, lr), '
                   'offsetof(emb_opt_spec, eps), offsetof(emb_opt_spec, reserved), s.kind, (int)EMB_OPT_ADAGRAD, (int)EMB_OPT_ROWWISE_ADAGRAD);\n'
                   'return 0;}\n')
    S = pel.lib.EmbOptSpec
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"),
                               str(src), "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
        assert got == [C.sizeof(S), S.kind.offset, S.lr.offset, S.eps.offset, S.reserved.offset, 2, 1, 2]
    assert C.sizeof(S) == 16


def test_step_refuses_null_and_bad_arguments_without_a_gpu(pel):
    G = pel.lib.load_grad()
    INV = pel.lib.EMB_ERR_INVALID
    d = pel.lib.EmbGradDesc()
    states = (C.c_void_p * 1)()
    spec = lambda kind=1, lr=0.1, eps=1e-10, reserved=0: C.byref(pel.lib.EmbOptSpec(kind, lr, eps, reserved))  # noqa: E731
    assert G.emb_grad_step(None, C.byref(d), states, 1, 0, spec(), None) == INV and b"context is NULL" in G.emb_grad_last_error()
    assert G.emb_grad_step(None, C.byref(d), states, 1, 0, None, None) == INV and b"spec is NULL" in G.emb_grad_last_error()
    for kind in (0, 3, 0xFFFFFFFF):
        assert G.emb_grad_step(None, C.byref(d), states, 1, 0, spec(kind=kind), None) == INV and b"unknown optimizer kind" in G.emb_grad_last_error()
    assert G.emb_grad_step(None, C.byref(d), states, 1, 0, spec(reserved=1), None) == INV and b"reserved" in G.emb_grad_last_error()
    for eps in (-1e-10, -0.5, float("nan")):
        assert G.emb_grad_step(None, C.byref(d), states, 1, 0, spec(kind=2, eps=eps), None) == INV and b"eps" in G.emb_grad_last_error()
