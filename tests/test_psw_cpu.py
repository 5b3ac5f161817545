"""CPU: the gradient of per_sample_weights (include/pimemb_grad.h, THE GRADIENT OF PER_SAMPLE_WEIGHTS; emb_grad_weights).  The ABI is what
the header says and refuses what needs no device to refuse; tests/psw_ref.py, the definition as a loop, has the row-wise step's
pair tree, agrees bit for bit with the arithmetic the kernels compile (csrc/pimemb_grad_dot.h, run on the host) and with torch's
CPU autograd on inputs whose sums are exact in any order; the new kernels use no scratch, spills or LDS, and every kernel the
library held before is still there, bit for bit.  No GPU work is called."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import optim_ref as orf  # noqa: E402
import psw_ref as pr  # noqa: E402

ROOT = gr.ROOT
HEADER = os.path.join(ROOT, "include", "pimemb_grad.h")
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
PARENT_HASHES = os.path.join(ROOT, "tests", "golden", "grad_kernel_hashes_parent.json")
build = import_module("pim-embedding-lookup_amd.build")
codeobj = import_module("pim-embedding-lookup_amd.codeobj")
F = np.float32
DIMS = (1, 3, 4, 48, 130, 260, 512, 516)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_bound(pel):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+emb_grad_weights\s*\(\s*emb_grad\s*\*\s*g\s*,\s*const\s+emb_grad_desc\s*\*\s*descs\s*,\s*float\s*\*\s*const\s*\*\s*dw_out\s*,"
                     r"\s*uint32_t\s+n_descs\s*,\s*emb_index_type\s+itype\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_LIB_PATH], text=True)
    assert "emb_grad_weights" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "emb_grad_weights" in pel.lib.GRAD_SIGNATURES
    assert pel.lib.load_grad().emb_grad_weights is not None


def test_header_no_longer_lists_the_gradient_as_missing():
    text = open(HEADER).read()
    assert "THE GRADIENT OF PER_SAMPLE_WEIGHTS" in text and "optim_ref.pair_tree" in text
    assert "Out of scope: the gradient with respect to per_sample_weights" not in text
    tm = open(os.path.join(ROOT, "pim-embedding-lookup_amd", "torch_module.py")).read()
    assert "Not there: the gradient with respect to" not in tm
    assert "are not trained" not in open(os.path.join(ROOT, "pim-embedding-lookup_amd", "dlrm_harness.py")).read()


def test_refuses_null_and_bad_arguments_without_a_gpu(pel):
    G = pel.lib.load_grad()
    INV = pel.lib.EMB_ERR_INVALID
    d = pel.lib.EmbGradDesc()
    outs = (C.c_void_p * 1)()
    assert G.emb_grad_weights(None, C.byref(d), outs, 1, 0, None) == INV and b"emb_grad_weights: context is NULL" in G.emb_grad_last_error()
    assert G.emb_grad_weights(None, None, outs, 1, 0, None) == INV and b"descs or dw_out is NULL" in G.emb_grad_last_error()
    assert G.emb_grad_weights(None, C.byref(d), None, 1, 0, None) == INV and b"descs or dw_out is NULL" in G.emb_grad_last_error()
    assert G.emb_grad_weights(None, None, None, 0, 0, None) == INV and b"descs or dw_out is NULL" in G.emb_grad_last_error()
    for itype in (2, 7, -1):
        assert G.emb_grad_weights(None, C.byref(d), outs, 1, itype, None) == INV and b"bad index type" in G.emb_grad_last_error()
    assert G.emb_grad_weights(None, C.byref(d), outs, 0, 1, None) == INV and b"context is NULL" in G.emb_grad_last_error()


# ---- psw_ref's tree is the row-wise step's pair tree ---------------------------------------------------------------------------------
def test_tree_over_squares_is_the_rowwise_pair_tree():
    rng = np.random.default_rng(7)
    for dim in range(4, 513, 4):
        g = (rng.standard_normal(dim) * np.exp2(rng.integers(-8, 8, size=dim))).astype(F)
        assert bits(pr.dot(g, g)) == bits(orf.pair_tree(g)), dim


def test_tree_against_an_independent_spelling():
    """The xor butterfly over L lanes, lane l holding pieces l, l + 64, l + 128, ...; and the signed zeros of the +0 padding."""
    rng = np.random.default_rng(8)
    for dim in DIMS + (6, 8, 64, 256, 1100):
        prod = (rng.standard_normal(dim) * np.exp2(rng.integers(-8, 8, size=dim))).astype(F)
        p = np.zeros(-(-dim // 4) * 4, F)
        p[:dim] = prod
        t = [F(F(F(p[4 * c] + p[4 * c + 1]) + p[4 * c + 2]) + p[4 * c + 3]) for c in range(len(p) // 4)]
        L = min(64, 1 << (len(t) - 1).bit_length())
        lanes = []
        for l in range(L):
            v = t[l] if l < len(t) else F(0)
            for c in range(l + 64, len(t), 64):
                v = F(v + t[c])
            lanes.append(v)
        h = 1
        while h < L:
            lanes = [F(lanes[l] + lanes[l ^ h]) for l in range(L)]
            h *= 2
        assert len({int(x.view(np.uint32)) for x in lanes}) == 1
        assert bits(lanes[0]) == bits(pr.tree(prod)), dim
    for dim, negative in ((4, True), (64, True), (48, False), (3, False)):
        dw = pr.dot(np.full(dim, -0.0, F), np.full(dim, 1.5, F))
        assert dw == 0 and bool(np.signbit(dw)) == negative, dim


# ---- the shared header on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dot_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("psw") / "psw_dot_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "psw_dot_check.cpp"), "-o", str(exe)])
    return str(exe)


def rows_for(kind, dim):
    """(stored rows uint8 [n, stride], G float32 [n, dim]): random rows over many binades, and special ones."""
    rng = np.random.default_rng(1000 + dim)
    n = 96
    w = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-12, 12, size=(n, 1)))).astype(F)
    g = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-12, 12, size=(n, 1)))).astype(F)
    g[0], w[1] = -0.0, 0.0                                   # signed zeros
    g[2], w[2] = -0.0, np.abs(w[2]) + F(1)
    g[3] = np.array([1, 0x007FFFFF, 0x80000001, 0x00400000], dtype=np.uint32).view(F)[np.arange(dim) % 4]      # denormals
    w[4] = F(2.0 ** -14) * F(0.37)                           # fp16 subnormals once stored
    g[5], w[5] = F(3e38), F(4.0)                             # overflow of a product
    w[6, 0] = np.inf
    g[7, -1] = np.inf
    w[8], g[8] = F(65504.0), F(1.0)
    raw = gr.encode(kind, w)
    return raw, g


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_shared_header_equals_psw_ref(dot_exe, tmp_path, kind, dim):
    raw, g = rows_for(kind, dim)
    fw, fg, fo = tmp_path / "w.bin", tmp_path / "g.bin", tmp_path / "o.bin"
    raw.tofile(fw)
    g.tofile(fg)
    subprocess.check_call([dot_exe, kind, str(dim), str(fw), str(fg), str(fo)])
    got = np.fromfile(fo, F)
    w = gr.decode(kind, raw)
    want = np.array([pr.dot(g[k], w[k]) for k in range(len(g))], F)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert bad.size == 0, (kind, dim, bad[:4], got[bad[:4]], want[bad[:4]])
    assert np.isfinite(want).sum() > 80


# ---- psw_ref against torch's CPU autograd, on inputs whose sums are exact in any order ----------------------------------------------------
def exact_inputs(dim, seed=0):
    """Table values k/8 and gradients k/4 with |k| <= 8: every product is a multiple of 1/32 below 4 and every partial sum of up
    to 516 of them is exact in fp32, whatever the order.  16 rows, 9 bags (two empty, one of padding only), padding row 5."""
    rng = np.random.default_rng(50 + dim + seed)
    table = (rng.integers(-8, 9, size=(16, dim)) / 8.0).astype(F)
    lens = [3, 0, 5, 1, 2, 0, 7, 4, 2]
    ids = rng.integers(0, 16, size=sum(lens)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ids[offsets[4]:offsets[4] + 2] = 5                       # a bag of padding only
    ids[1] = 5
    G = (rng.integers(-8, 9, size=(len(lens), dim)) / 4.0).astype(F)
    w = (rng.integers(-8, 9, size=len(ids)) / 4.0).astype(F)
    return table, ids, offsets, G, w


def torch_cpu_weights_grad(table, ids, offsets, G, w, padding_idx):
    import torch
    bag = torch.nn.EmbeddingBag(table.shape[0], table.shape[1], mode="sum", padding_idx=padding_idx, _weight=torch.from_numpy(table.copy()))
    wt = torch.from_numpy(w.copy()).requires_grad_(True)
    bag(torch.from_numpy(ids), torch.from_numpy(offsets), per_sample_weights=wt).backward(torch.from_numpy(G.copy()))
    return wt.grad.numpy()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dim", DIMS)
def test_psw_ref_equals_torch_cpu_autograd_on_exact_inputs(dim, padded):
    table, ids, offsets, G, w = exact_inputs(dim)
    pad = 5 if padded else None
    want = torch_cpu_weights_grad(table, ids, offsets, G, w, pad)
    dw, n_bad = pr.weights_grad("f32", table.view(np.uint8).reshape(16, -1), ids, offsets, G, pad)
    assert n_bad == 0 and dw.dtype == F
    assert np.array_equal(bits(dw), bits(want)), (dim, padded, dw, want)
    assert (want != 0).sum() >= (1 if dim == 1 else 8)
    if padded:
        assert (dw[ids == 5] == 0).all() and not np.signbit(dw[ids == 5]).any()


# ---- the code object --------------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_no_spills_and_no_lds():
    res = codeobj.kernel_resources(build.GRAD_LIB_PATH)
    group = {k: v for k, v in res.items() if "grad_psw_group" in k}
    assert len(group) == 2, sorted(group)                     # uint32 and int64 ids
    for name, r in group.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (name, r)
    assert len([k for k in res if "grad_psw_elem" in k]) == 2
    assert not [k for k in res if "psw" in k and ("grad_seg_" in k or "grad_" not in k)]


def test_every_kernel_of_the_parent_is_still_there_bit_for_bit():
    want = json.load(open(PARENT_HASHES))
    got = codeobj.kernel_hashes(build.GRAD_LIB_PATH)
    assert len(want) == 31 and not [k for k in want if "psw" in k]
    changed = sorted(k for k in want if got.get(k) != want[k])
    assert not changed, changed
    added = sorted(set(got) - set(want))
    assert added and all("grad_psw_" in k for k in added), added
