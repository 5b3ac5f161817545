"""CPU: the backward pass's companion library (libpimemb_grad.so, include/pimemb_grad.h) builds, loads next to the other two,
exports and binds what its header declares and keeps the three code objects closed against each other; its one-element step
(csrc/pimemb_grad_step.h, the very text the kernels compile), run on the host, agrees bit for bit with tests/grad_ref.py; and
grad_ref itself is pinned against torch's CPU autograd on the exact batch.  No GPU work is called."""
import ctypes as C
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as gc  # noqa: E402
import grad_ref as gr  # noqa: E402

ROOT = gr.ROOT
HEADER = os.path.join(ROOT, "include", "pimemb_grad.h")
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
build = import_module("pim-embedding-lookup_amd.build")
codeobj = import_module("pim-embedding-lookup_amd.codeobj")


def declared_functions(path):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"typedef\s+(struct|enum)\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b([a-z_][a-z0-9_]*)\s*\([^;{]*\)\s*;", text)))


def test_third_library_is_built_and_loads_next_to_the_other_two(pel):
    assert os.path.exists(build.GRAD_LIB_PATH), "libpimemb_grad.so must be built in-tree (__graft_entry__.build())"
    assert os.path.dirname(build.GRAD_LIB_PATH) == os.path.dirname(pel.LIB_PATH)
    G = pel.lib.load_grad()
    assert G.emb_grad_last_error() == b""
    pel.lib.load_rows()
    maps = [line.split()[-1] for line in open("/proc/self/maps") if "libpimemb" in line]
    assert {os.path.basename(m) for m in maps} >= {"libpimemb.so", "libpimemb_rows.so", "libpimemb_grad.so"}
    assert len({m for m in maps if os.path.basename(m) == "libpimemb.so"}) == 1      # ONE engine library in the process


def test_exports_and_binds_every_declared_function(pel):
    fns = declared_functions(HEADER)
    assert {"emb_grad_create", "emb_grad_destroy", "emb_grad_sparse", "emb_grad_sgd", "emb_grad_report", "emb_grad_scratch_bytes",
            "emb_grad_last_error"} <= set(fns)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in fns if f not in exported]
    assert sorted(pel.lib.GRAD_SIGNATURES) == fns
    assert not set(pel.lib.GRAD_SIGNATURES) & (set(pel.lib.SIGNATURES) | set(pel.lib.ROWS_SIGNATURES))
    G = pel.lib.load_grad()
    for name in fns:
        assert getattr(G, name) is not None


def test_header_compiles_as_c_and_cxx_and_the_record_matches(pel, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pimemb_grad.h"\nint main(void){emb_grad *g = 0; (void)g;\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(emb_grad_desc), offsetof(emb_grad_desc, grad), offsetof(emb_grad_desc, grad_ld), '
                   'offsetof(emb_grad_desc, pool));\nreturn 0;}\n')
    D = pel.lib.EmbGradDesc
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"),
                               str(src), "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
        assert got == [C.sizeof(D), D.grad.offset, D.grad_ld.offset, D.pool.offset]


def test_links_the_engine_and_one_hip_runtime_by_unversioned_name(pel):
    out = subprocess.check_output(["objdump", "-p", build.GRAD_LIB_PATH], text=True)
    needed = re.findall(r"NEEDED\s+(\S+)", out)
    assert "libamdhip64.so" in needed and "libpimemb.so" in needed
    assert not any(re.match(r"libamdhip64\.so\.\d", n) or n.startswith("libtorch") or n.startswith("libc10") or "rows" in n for n in needed)
    assert "$ORIGIN" in re.search(r"RUNPATH\s+(\S+)", out).group(1)


def test_scratch_bytes_is_monotone_in_both_arguments(pel):
    G = pel.lib.load_grad()
    sizes = (1, 2, 255, 256, 1023, 1024, 1025, 2037, 65536, 65537, 1 << 20, (1 << 24) + 1, 1 << 30)
    prev_row = None
    for n in sizes:
        row = [G.emb_grad_scratch_bytes(n, b) for b in sizes]
        assert all(x <= y for x, y in zip(row, row[1:])), n
        assert row[0] >= 24 * n + 4                                  # two (key, position) pairs, the bag and the unique number per index
        if prev_row is not None:
            assert all(x <= y for x, y in zip(prev_row, row)), n
        prev_row = row
    assert G.emb_grad_scratch_bytes(1 << 16, 1 << 20) - G.emb_grad_scratch_bytes(1 << 16, 1) >= 4 * ((1 << 20) - 64)      # 4 bytes per bag


def test_refuses_null_and_bad_arguments_without_a_gpu(pel):
    G = pel.lib.load_grad()
    INV = pel.lib.EMB_ERR_INVALID
    h = C.c_void_p()
    assert G.emb_grad_create(None, 16, 16, C.byref(h)) == INV
    assert b"NULL" in G.emb_grad_last_error()
    d = pel.lib.EmbGradDesc()
    assert G.emb_grad_sparse(None, C.byref(d), 0, None, None, 0, None, None) == INV
    assert G.emb_grad_sgd(None, C.byref(d), 1, 0, 0.1, None) == INV
    assert G.emb_grad_report(None, None) == INV
    assert G.emb_grad_destroy(None) == pel.lib.EMB_OK


def test_all_three_code_objects_stay_closed_against_each_other(pel):
    grad = codeobj.kernel_hashes(build.GRAD_LIB_PATH)
    rows = codeobj.kernel_hashes(build.ROWS_LIB_PATH)
    main = codeobj.kernel_hashes(pel.LIB_PATH)
    assert grad and all("grad_" in k for k in grad), sorted(grad)
    for want in ("grad_classify", "grad_sort_count", "grad_sort_scatter", "grad_scan_chunks", "grad_scan_sums", "grad_rows_group", "grad_rows_elem"):
        assert any(want in k for k in grad), want
    assert not set(grad) & set(main) and not set(grad) & set(rows) and not set(rows) & set(main)
    assert not [k for k in list(main) + list(rows) if "grad_" in k]
    # the other two hold what they held: the row writer its four kernel families, the main library the census's homes
    assert all(any(n in k for n in ("rows_write_group", "rows_write_mx", "rows_write_elem", "rows_claim")) for k in rows)
    kc = import_module("kernel_census")
    others = [k for k in main if "bag_" not in k]
    assert main and len(others) < len(main)
    assert {kc.helper_name(k) for k in others} == set(kc.HELPER_KERNELS)


# ---- the one-element step on the host -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("grad") / "grad_step_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "grad_step_check.cpp"), "-o", str(exe)])
    return str(exe)


def run_step(exe, kind, raw, g, lr, tmp_path):
    fw, fg, fo = tmp_path / "w.bin", tmp_path / "g.bin", tmp_path / "o.bin"
    np.ascontiguousarray(raw).tofile(fw)
    np.ascontiguousarray(g, dtype=np.float32).tofile(fg)
    subprocess.check_call([exe, kind, "%08x" % int(np.float32(lr).view(np.uint32)), str(fw), str(fg), str(fo)])
    return np.fromfile(fo, dtype=np.uint8).reshape(raw.shape)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_step_equals_grad_ref_element_by_element(step_exe, tmp_path, kind):
    """Over the case tables and gradients (the crafted ties, subnormal and overflow results among them), over EVERY stored value
    of the 2-byte dtypes with random gradients (dec on every bit pattern but the NaNs' payloads), and over edge gradients."""
    dim = 8
    table = gc.step_table(kind, dim)
    rows, grads, _ = gc.reference("i64", "sum", dim)
    raw = table[rows]
    got = run_step(step_exe, kind, raw, grads, gc.LR, tmp_path)
    want = gr.step_values(kind, raw, grads, gc.LR)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (kind, rows[bad[:4]], got[bad[0]], want[bad[0]])
    for (k, cls), row in gc.SPECIAL.items():             # the crafted results are what they were crafted to be
        if k != kind:
            continue
        at = int(np.flatnonzero(rows == row)[0])
        new = gr.decode(kind, want[at][None, :])[0]
        top = {"f16": 65504.0, "bf16": float(np.uint32(0x7F7F0000).view(np.float32))}[kind]
        exact = gr.decode(kind, raw[at][None, :])[0].astype(np.float64) - np.float64(np.float32(gc.LR) * grads[at].astype(np.float32))
        if cls == "over":
            assert np.isinf(new).all() and (np.abs(exact) > top).all()
        elif cls == "sub":
            assert (new != 0).all() and (np.abs(new) < {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}[kind]).all() and (new != exact).all()
        else:
            assert (new != exact).all() and (new == 1.0).all()          # the tie 1 + half an ulp goes to the even neighbour
    rng = np.random.default_rng(3)
    if kind != "f32":
        codes = np.arange(1 << 16, dtype=np.uint16)
        finite = np.isfinite(gr.decode(kind, codes.view(np.uint8).reshape(-1, 2)))[:, 0]
        codes = codes[finite]
        codes = np.concatenate([codes, codes[: -len(codes) % 8]]).reshape(-1, 8)
        raw = codes.view(np.uint8).reshape(codes.shape[0], -1)
    else:
        raw = rng.integers(0, 1 << 32, size=(1 << 14, 8), dtype=np.uint64).astype(np.uint32)
        raw = np.where((raw & 0x7F800000) == 0x7F800000, raw & np.uint32(0xBFFFFFFF), raw).astype(np.uint32).view(np.uint8).reshape(1 << 14, -1)
    n = raw.shape[0]
    g = (rng.standard_normal((n, 8)) * np.exp2(rng.integers(-30, 30, size=(n, 1)))).astype(np.float32)
    g[::7, 0] = 0.0
    g[1::7, 1] = -0.0
    g[2::7, 2] = np.float32(1e-41)
    g[3::7, 3] = np.float32(3e38)
    got = run_step(step_exe, kind, raw, g, gc.LR, tmp_path)
    want = gr.step_values(kind, raw, g, gc.LR)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (kind, raw[bad[0]], g[bad[0]], got[bad[0]], want[bad[0]])


# ---- grad_ref against torch's CPU autograd, on the exact batch ------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", ["sum", "weighted", "mean", "sum+pad", "weighted+pad", "mean+pad"])
def test_grad_ref_equals_torch_cpu_autograd_on_the_exact_batch(mode_name):
    """F.embedding_bag(..., sparse=True) backward on the CPU: weight.grad.coalesce() equals grad_ref's unique list and gradients
    bit for bit, and w - lr * grad (lr = 0.5) grad_ref's stepped fp32 table.  With padding torch lists the padding row -- and may
    list rows whose contributions are all zero -- with an all-zero gradient: rows torch lists with an all-zero gradient that
    grad_ref does not list are dropped before comparing."""
    import torch
    import torch.nn.functional as F
    mode, weighted, padded = gc.MODES[mode_name]
    ids, offsets, G, w = gc.exact_batch(padded)
    table = gc.exact_table()
    weight = torch.from_numpy(table.copy()).requires_grad_(True)
    out = F.embedding_bag(torch.from_numpy(ids), weight, torch.from_numpy(offsets), mode=mode, sparse=True,
                          per_sample_weights=torch.from_numpy(w) if weighted else None, padding_idx=gc.PAD if padded else None)
    out.backward(torch.from_numpy(G))
    sp = weight.grad.coalesce()
    t_rows, t_vals = sp.indices()[0].numpy(), sp.values().numpy()
    rows, grads, n_bad = gr.sparse_grad(gc.EXACT_ROWS, ids, offsets, G, mode, w if weighted else None, gc.PAD if padded else None)
    assert n_bad == 0 and len(rows) > 20
    keep = np.array([bool(r in set(rows.tolist()) or t_vals[k].any()) for k, r in enumerate(t_rows.tolist())], dtype=bool)
    assert padded or keep.all()
    t_rows, t_vals = t_rows[keep], t_vals[keep]
    assert np.array_equal(t_rows, rows)
    assert np.array_equal(t_vals.view(np.uint32), grads.view(np.uint32))
    raw = gr.sgd_step("f32", table.view(np.uint8).reshape(gc.EXACT_ROWS, -1), rows, grads, np.float32(0.5))
    with torch.no_grad():
        want = (weight - 0.5 * weight.grad.to_dense()).numpy()
    assert np.array_equal(raw.view(np.float32).reshape(want.shape).view(np.uint32), want.view(np.uint32))
