"""CPU: the fused Adam steps of the backward pass (include/pimemb_grad.h, THE ADAM STEPS).  The arithmetic the kernels compile
(csrc/pimemb_grad_adam.h), run on the host by tests/cpp/adam_step_check.cpp, agrees with tests/adam_ref.py bit for bit; adam_ref agrees
with torch.optim.SparseAdam on the CPU; emb_adam_constants gives Python's own doubles; the new ABI is what the header says and refuses
what it says; the new code object holds the expected kernels and no scratch.  No GPU work is called."""
import ctypes as C
import math
import os
import subprocess
import sys
import threading
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as ar  # noqa: E402
import grad_ref as gr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
F = np.float32
HYPER = [(1e-3, (0.9, 0.999), 1e-8), (0.05, (0.5, 0.9), 1e-6), (0.3, (0.0, 0.99), 1e-3)]
# W against torch: max |dW| / (ss * |x|) measured between adam_ref and torch 2.10 on the CPU was 2.003e-07, in 5 of 4 284 words
# (profiles/adam/README.md; neither side is the code under test).  Twice that, rounded up to a power of two: 4.006e-07 -> 2^-21.
W_BOUND = 2.0 ** -21


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("adam") / "adam_step_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "adam_step_check.cpp"),
                           "-o", str(out)])
    return str(out)


def hexbits(x):
    return "%x" % int(np.array([x], F).view(np.uint32)[0])


def dec_words(kind, words):
    """The fp32 values of stored elements that travel one per uint32 word."""
    raw = words.astype(np.uint32) if kind == "f32" else words.astype(np.uint16)
    return gr.decode(kind, raw.view(np.uint8)[None, :])[0]


def values(n, seed):
    """(g, M, V): randoms over many magnitudes, then the special ones -- g = 0 and -0, denormal V and g, V = M = 0, huge values."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, size=n))).astype(F)
    m = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 20, size=n))).astype(F)
    v = (np.abs(rng.standard_normal(n)) * np.exp2(rng.integers(-60, 40, size=n))).astype(F)
    g[:8] = np.array([0.0, -0.0, 1e-39, 1e-30, 0.0, 3e38, 1.0, -1e-42], F)
    v[:8] = np.array([0.0, 0.0, 1e-44, 0x00400000 * 1.4e-45, 1e-40, 1e38, 0.0, 0.0], F)
    m[:8] = np.array([0.0, 0.0, 0.0, 1e-41, -1.0, -3e38, 0.0, 1e-45], F)
    return g, m, v


@pytest.mark.parametrize("eps", [1e-8, 0.0])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_header_arithmetic_equals_the_reference(exe, tmp_path, kind, eps):
    n = 4096
    g, m, v = values(n, 3)
    stored = gr.encode(kind, (np.random.default_rng(4).standard_normal((1, n)) * 3).astype(F))
    st32 = (stored.view(F).view(np.uint32) if kind == "f32" else stored.view(np.uint16).astype(np.uint32)).reshape(-1)
    om1, om2, ss = ar.constants(0.05, (0.9, 0.999), 3)
    consts = [hexbits(om1), hexbits(om2), hexbits(ss), hexbits(F(eps))]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    # EMB_ADAM
    np.stack([st32, g.view(np.uint32), m.view(np.uint32), v.view(np.uint32)], axis=1).tofile(src)
    subprocess.check_call([exe, "adam", kind] + consts + [str(src), str(dst)])
    got = np.fromfile(dst, np.uint32).reshape(n, 3)
    new, m1, v1, _ = ar.adam_values(gr.decode(kind, stored)[0], g, m, v, om1, om2, ss, eps)
    want_w = gr.encode(kind, new[None, :])
    want_w = (want_w.view(np.uint32) if kind == "f32" else want_w.view(np.uint16).astype(np.uint32)).reshape(-1)
    nan = np.isnan(new)                                       # (NaN payloads are unspecified)
    assert np.array_equal(got[~nan, 0], want_w[~nan]) and np.isnan(dec_words(kind, got[nan, 0])).all()
    assert np.array_equal(got[:, 1], m1.view(np.uint32)) and np.array_equal(got[:, 2], v1.view(np.uint32))
    if eps == 0.0:
        assert nan[0] and nan[1]                              # g = 0, V' = 0, eps = 0: 0 / 0 in both
    # EMB_ROWWISE_ADAM: one record per "row" of dim 8, the tree's sum given
    dim = 8
    sums = np.array([ar.orf.pair_tree(g[k:k + dim]) for k in range(0, n, dim)], F).repeat(dim)
    sums[:dim] = 0                                            # V' = 0: rate = ss / eps, inf with eps = 0
    vr = v[::dim].repeat(dim)
    np.stack([st32, g.view(np.uint32), m.view(np.uint32), vr.view(np.uint32), sums.view(np.uint32)], axis=1).tofile(src)
    subprocess.check_call([exe, "rowwise", kind] + consts + [str(dim), str(src), str(dst)])
    got = np.fromfile(dst, np.uint32).reshape(n, 4)
    with np.errstate(all="ignore"):
        v1 = ar.average(vr, sums / F(dim), om2)
        rate = ss / (np.sqrt(v1) + F(eps))
        m1 = ar.average(m, g, om1)
        new = gr.decode(kind, stored)[0] - rate * m1
    assert np.array_equal(got[:, 1], m1.view(np.uint32)) and np.array_equal(got[:, 2], v1.view(np.uint32)) and np.array_equal(got[:, 3], rate.view(np.uint32))
    want_w = gr.encode(kind, new[None, :])
    want_w = (want_w.view(np.uint32) if kind == "f32" else want_w.view(np.uint16).astype(np.uint32)).reshape(-1)
    ok = ~np.isnan(new)
    assert np.array_equal(got[ok, 0], want_w[ok])
    if eps == 0.0:
        assert np.isinf(rate[0])


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_constants_are_pythons_own_doubles(pel, exe, t):
    G = pel.lib.load_grad()
    for lr, (b1, b2), eps in HYPER:
        out = (C.c_float * 3)()
        assert G.emb_adam_constants(C.byref(pel.lib.EmbAdamSpec(1, eps, lr, b1, b2, t, None, 0)), out) == 0
        want = [F(1.0 - b1), F(1.0 - b2), F(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))]
        assert [F(x) for x in out] == want and list(ar.constants(lr, (b1, b2), t)) == want
        host = subprocess.check_output([exe, "constants", repr(lr), repr(b1), repr(b2), str(t)], text=True).split()
        assert host == [hexbits(x) for x in want]


def test_declared_exported_bound_and_linked(pel):
    build = import_module("pim-embedding-lookup_amd.build")
    header = open(os.path.join(ROOT, "include", "pimemb_grad.h")).read()
    assert "THE ADAM STEPS" in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    G = pel.lib.load_grad()
    for name in ("emb_adam_constants", "emb_adam_state_floats", "emb_grad_adam_step"):
        assert name + "(" in header and name in exported and getattr(G, name).argtypes == pel.lib.GRAD_SIGNATURES[name][1]
    dyn = subprocess.check_output(["readelf", "-d", build.GRAD_LIB_PATH], text=True)
    assert "libpimemb_grad_adam.so" in dyn and "$ORIGIN" in dyn
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_ADAM_LIB_PATH], text=True)
    assert "pimemb_grad_adam_launch" in {line.split()[-1] for line in syms.splitlines()}
    S = pel.lib.EmbAdamSpec
    assert C.sizeof(S) == 56 and (S.kind.offset, S.eps.offset, S.lr.offset, S.beta2.offset, S.step.offset, S.step_size_dev.offset, S.reserved.offset) == (0, 4, 8, 24, 32, 40, 48)
    f = G.emb_adam_state_floats
    assert (f(1, 10, 8, 0), f(1, 10, 8, 1), f(2, 10, 8, 0), f(2, 10, 8, 1), f(3, 10, 8, 0), f(1, 10, 8, 2)) == (80, 80, 80, 10, 0, 0)
    assert G.emb_opt_state_floats(3, 10, 8) == 0              # the Adagrad enum is what it was


def test_refusals_of_bad_specs_and_of_a_null_context(pel):
    """On a thread of its own: emb_grad_last_error is thread-local and never cleared, and tests/test_grad_cpu.py, which runs later in the
    same process, reads the main thread's as the empty text of a library that has refused nothing yet."""
    failed = []
    t = threading.Thread(target=lambda: refusals(pel) or failed.clear(), daemon=True)
    failed.append("the thread did not finish")
    t.start()
    t.join()
    assert not failed, failed


def refusals(pel):
    G = pel.lib.load_grad()
    INV = pel.lib.EMB_ERR_INVALID
    d, ptrs, err = pel.lib.EmbGradDesc(), (C.c_void_p * 1)(), G.emb_grad_last_error
    good = dict(kind=1, eps=1e-8, lr=0.1, beta1=0.9, beta2=0.999, step=1, step_size_dev=None, reserved=0)
    step = lambda g, **kw: G.emb_grad_adam_step(g, C.byref(d), ptrs, ptrs, 1, 0, C.byref(pel.lib.EmbAdamSpec(**{**good, **kw})), None)  # noqa: E731
    assert step(None) == INV and b"context is NULL" in err()
    out = (C.c_float * 3)()
    for kw, text in ((dict(kind=0), b"kind"), (dict(kind=3), b"kind"), (dict(reserved=1), b"reserved"), (dict(beta1=1.0), b"beta"), (dict(beta2=-0.1), b"beta"),
                     (dict(beta1=float("nan")), b"beta"), (dict(eps=-1.0), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(lr=float("inf")), b"lr"),
                     (dict(lr=float("nan")), b"lr"), (dict(step=0), b"step"), (dict(step_size_dev=6), b"4-byte aligned")):
        assert step(None, **kw) == INV and text in err(), kw      # refused before the context is looked at: the text names the spec
        assert G.emb_adam_constants(C.byref(pel.lib.EmbAdamSpec(**{**good, **kw})), out) == INV and text in err(), kw
    assert G.emb_grad_adam_step(None, C.byref(d), ptrs, ptrs, 1, 0, None, None) == INV and b"spec is NULL" in err()
    assert G.emb_adam_constants(C.byref(pel.lib.EmbAdamSpec(**good)), None) == INV
    fake = C.c_void_p(16)
    assert G.emb_grad_adam_step(fake, C.byref(d), None, ptrs, 1, 0, C.byref(pel.lib.EmbAdamSpec(**good)), None) == INV and b"is NULL" in err()
    assert G.emb_grad_adam_step(fake, C.byref(d), ptrs, ptrs, 1, 7, C.byref(pel.lib.EmbAdamSpec(**good)), None) == INV and b"index type" in err()
    assert G.emb_grad_step(None, C.byref(d), ptrs, 1, 0, C.byref(pel.lib.EmbOptSpec(3, 0.1, 1e-10, 0)), None) == INV and b"unknown optimizer kind 3" in err()


def test_the_adam_kernels_have_a_code_object_of_their_own_and_use_no_scratch():
    codeobj = import_module("pim-embedding-lookup_amd.codeobj")
    build = import_module("pim-embedding-lookup_amd.build")
    res = codeobj.kernel_resources(build.GRAD_ADAM_LIB_PATH)
    inst = lambda name, *args: "%d%sIL" % (len(name), name) + "EL".join(args) + "EEE"  # noqa: E731
    want = [inst("grad_adam_rows_group", "i%d" % k, "b%d" % s) for k in (1, 2) for s in (0, 1)] + [inst("grad_adam_rows_elem", "i1", "b%d" % s) for s in (0, 1)]
    assert len(res) == 6 and all(sum(w in k for k in res) == 1 for w in want), sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
    for path in (build.GRAD_LIB_PATH, build.GRAD_MASTER_LIB_PATH, build.GRAD_SR_LIB_PATH, build.GRAD_MAX_LIB_PATH, build.LIB_PATH, build.ROWS_LIB_PATH):
        assert not [k for k in codeobj.kernel_resources(path) if "adam" in k], path


def test_adam_ref_equals_torch_sparse_adam_on_the_cpu():
    """7 steps x 3 hyper-parameter sets on [50, 12], the reference re-synchronised with torch every step: exp_avg and exp_avg_sq bit for
    bit, W within W_BOUND * ss * |x| and bit-equal in at least 99 % of its words."""
    import torch
    words = equal = 0
    worst = 0.0
    for h, (lr, betas, eps) in enumerate(HYPER):
        rng = np.random.default_rng(70 + h)
        w = torch.nn.Parameter(torch.from_numpy(rng.standard_normal((50, 12)).astype(F)))
        opt = torch.optim.SparseAdam([w], lr=lr, betas=betas, eps=eps)
        for t in range(1, 8):
            rows = np.sort(rng.choice(50, size=17, replace=False)).astype(np.int64)
            g = (rng.standard_normal((17, 12)) * np.exp2(rng.integers(-6, 6, size=(17, 1)))).astype(F)
            w0 = w.detach().numpy().copy()
            st = opt.state.get(w, {})
            m0 = st["exp_avg"].numpy().copy() if st else np.zeros((50, 12), F)
            v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros((50, 12), F)
            w.grad = torch.sparse_coo_tensor(torch.from_numpy(rows)[None, :], torch.from_numpy(g), (50, 12)).coalesce()
            opt.step()
            table, m1, v1 = ar.adam_step("f32", w0.view(np.uint8).reshape(50, -1), m0, v0, rows, g, lr, betas, eps, t)
            got_w, want_w = table.view(F), w.detach().numpy()
            assert np.array_equal(m1.view(np.uint32), opt.state[w]["exp_avg"].numpy().view(np.uint32)), (h, t)
            assert np.array_equal(v1.view(np.uint32), opt.state[w]["exp_avg_sq"].numpy().view(np.uint32)), (h, t)
            ss = ar.constants(lr, betas, t)[2]
            x = ar.adam_values(w0[rows], g, m0[rows], v0[rows], *ar.constants(lr, betas, t)[:2], ss, eps)[3]
            rel = np.abs(got_w[rows].astype(np.float64) - want_w[rows]) / (float(ss) * np.abs(x).astype(np.float64))
            worst = max(worst, float(rel.max()))
            words += rows.size * 12
            equal += int((got_w[rows].view(np.uint32) == want_w[rows].view(np.uint32)).sum())
            assert np.array_equal(np.delete(got_w, rows, 0), np.delete(want_w, rows, 0))
    print("adam_ref against torch SparseAdam: max |dW| / (ss |x|) = %.4g, %d of %d words bit-equal" % (worst, equal, words))
    assert worst <= W_BOUND and equal >= 0.99 * words, (worst, equal, words)
