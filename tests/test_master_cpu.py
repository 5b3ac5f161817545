"""CPU: the fused master-weight steps of the backward pass (include/pimemb_grad.h, THE MASTER-WEIGHT STEPS).  tests/master_ref.py, the
definition as a loop, gives the bytes of the documented recipe (train_ref.master_step) and tells a contracted update apart; the
one-block MXFP4 arithmetic and the piece encoders the kernels compile (csrc/pimemb_grad_master.h), run on the host, agree with
formats.py bit for bit; and the new ABI is what the header says.  No GPU work is called."""
import ctypes as C
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import master_ref as mr  # noqa: E402
import rows_cases as rc  # noqa: E402
import train_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
F = np.float32
formats = rc.formats


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the reference against the recipe ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,mode_name", tr.RECIPE_CASES)
def test_master_ref_gives_the_bytes_of_the_recipe(kind, dim, mode_name):
    """SGD, three batches: master_ref.master_step and train_ref.master_step leave the same table and the same master; the wrong
    one-rounding recipe (contract=True) differs somewhere on these batches -- they can tell."""
    st = tr.initial_state(kind, dim)
    table, master = st.table, st.master
    c_table, c_master = st.table, st.master
    differs = False
    for b, G in tr.train_batches(kind, dim):
        ids, off, mode, w, pad = b.args(mode_name)
        want_t, want_m, want_rows, want_bad = tr.master_step(kind, table, master, ids, off, G, mode, w, pad)
        table, master, opt, rows, n_bad, unenc = mr.master_step(kind, table, master, None, ids, off, G, mode, w, pad, "sgd")
        assert opt is None and unenc == 0 and n_bad == want_bad == b.n_bad and np.array_equal(rows, want_rows)
        assert np.array_equal(table, want_t) and np.array_equal(bits(master), bits(want_m)), (kind, dim, mode_name, b.k)
        c_table, c_master, _o, _r, _b, _u = mr.master_step(kind, c_table, c_master, None, ids, off, G, mode, w, pad, "sgd", contract=True)
        differs = differs or not np.array_equal(c_table, table) or not np.array_equal(bits(c_master), bits(master))
    assert differs, (kind, dim, mode_name)
    assert np.array_equal(table, rc.host_encode(kind, master))      # W == enc_T(M) is kept


def test_master_ref_skips_and_counts_unencodable_mxfp4_rows():
    rows = np.array([3, 7, 9])
    new = np.ones((3, 32), F)
    new[1, 5] = np.inf
    table0 = rc.host_encode("mxfp4", np.zeros((12, 32), F))
    table, unenc = mr.encode_rows("mxfp4", table0, rows, new)
    assert unenc == 1 and np.array_equal(table[7], table0[7]) and not np.array_equal(table[3], table0[3])
    table, unenc = mr.encode_rows("e5m2", rc.host_encode("e5m2", np.zeros((12, 32), F)), rows, new)
    assert unenc == 0 and table[7, 5] == 0x7C


# ---- the block header on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("master") / "master_block_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "master_block_check.cpp"), "-o", str(exe)])
    return str(exe)


E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def finite_blocks():
    """float32 [n, 32]: random blocks over 40 binades; all zero; all -0; an amax below 2^-125 and a denormal amax; every midpoint
    tie of the seven E2M1 code pairs (at two scales, both signs, with the values one ulp below and above); rows_cases' edge blocks."""
    rng = np.random.default_rng(77)
    rnd = (rng.standard_normal((400, 32)) * np.exp2(rng.integers(-20, 20, size=(400, 1)).astype(np.float64))).astype(F)
    assert len(np.unique(np.floor(np.log2(np.abs(rnd).max(axis=1))))) >= 38
    zero = np.zeros(32, F)
    neg = np.full(32, -0.0, F)
    small = np.zeros(32, F)
    small[:4] = [2.0 ** -126, -(2.0 ** -127), 2.0 ** -130, 2.0 ** -149]
    den = np.zeros(32, F)
    den[:3] = np.array([0x00400000, 0x80000003, 0x00000001], np.uint32).view(F)
    ties = []
    mids = [(E2M1[c] + E2M1[c + 1]) / 2 for c in range(7)]
    assert len(mids) == 7
    for scale in (1.0, 2.0 ** -9):
        for amax in (4.0, 6.0, 7.5):
            b = np.zeros(32, np.float64)
            b[0] = amax
            vals = []
            for m in mids:
                m32 = F(m)
                vals += [m32, np.nextafter(m32, F(0)), np.nextafter(m32, F(9))]
            b[1:1 + len(vals)] = vals
            b[22:29] = [-m for m in mids]
            ties.append((b * scale).astype(F))
    out = np.concatenate([rnd, np.stack([zero, neg, small, den] + ties), rc.mx_edge_blocks()]).astype(F)
    assert np.isfinite(out).all()
    return out, 400


def test_block_header_equals_formats_to_mxfp4(block_exe, tmp_path):
    blocks, n_rnd = finite_blocks()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    blocks.tofile(src)
    subprocess.check_call([block_exe, "mx", str(src), str(dst)])
    got = np.fromfile(dst, np.uint8).reshape(len(blocks), 18)
    want = formats.to_mxfp4(blocks)                      # [n, stride 32]: 16 element bytes, the scale byte, zero padding
    assert want.shape[1] == 32 and not want[:, 17:].any()
    bad = np.flatnonzero((got[:, :17] != want[:, :17]).any(axis=1))
    assert bad.size == 0, (bad[:8], blocks[bad[0]], got[bad[0]], want[bad[0]])
    assert not got[:, 17].any()
    assert got[n_rnd, 16] == 127 and not got[n_rnd, :16].any()                     # all zero: scale 127
    assert got[n_rnd + 1, 16] == 127 and (got[n_rnd + 1, :16] == 0x88).all()       # all -0: scale 127, the signs kept
    assert got[n_rnd + 2, 16] == 0 and got[n_rnd + 3, 16] == 0                     # amax below 2^-125, denormal amax: the lower clamp
    assert len(np.unique(got[:n_rnd, 16])) >= 38


@pytest.mark.parametrize("special", [np.inf, -np.inf, np.nan])
def test_block_header_flags_a_non_finite_block(block_exe, tmp_path, special):
    blocks, _n = finite_blocks()
    blocks = blocks[:64].copy()
    at = np.arange(64) % 32
    blocks[np.arange(0, 64, 2), at[::2]] = special       # every other block, every element position once
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    blocks.tofile(src)
    subprocess.check_call([block_exe, "mx", str(src), str(dst)])
    got = np.fromfile(dst, np.uint8).reshape(64, 18)
    assert np.array_equal(got[:, 17], (np.arange(64) % 2 == 0).astype(np.uint8))   # only the flag is compared there
    assert np.array_equal(got[1::2, :17], formats.to_mxfp4(blocks[1::2])[:, :17])


@pytest.mark.parametrize("kind", ["f16", "bf16", "e4m3", "e5m2"])
def test_piece_encoders_equal_formats(block_exe, tmp_path, kind):
    """The packed pieces of the 2-byte and 1-byte tails: rows_cases' sources with the format's edge values, NaN payloads included."""
    src_rows = rc.source(kind, 64, 48, seed=5)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src_rows.tofile(src)
    subprocess.check_call([block_exe, "piece", kind, str(src), str(dst)])
    want = rc.host_encode(kind, src_rows)
    esz = rc.KINDS[kind][1]
    got = np.fromfile(dst, np.uint8)
    if esz == 1:
        got = got.reshape(64, 48)
    else:
        got = got.reshape(64, 48 * 2)
    assert np.array_equal(got, want), kind


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx_and_the_master_spec_matches(pel, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pimemb_grad.h"\nint main(void){emb_master_spec s = {EMB_MASTER_ROWWISE_ADAGRAD, 0.1f, 0.f, 0};\n'
                   'printf("%zu %zu %zu %zu %zu %u %d %d %d\\n", sizeof(emb_master_spec), offsetof(emb_master_spec, kind), offsetof(emb_master_spec, lr), '
                   'offsetof(emb_master_spec, eps), offsetof(emb_master_spec, reserved), s.kind, (int)EMB_MASTER_SGD, (int)EMB_MASTER_ADAGRAD, '
                   '(int)EMB_MASTER_ROWWISE_ADAGRAD);\nreturn (int)(sizeof(&emb_grad_master_step) + sizeof(&emb_grad_master_report)) == 0;}\n')
    S = pel.lib.EmbMasterSpec
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"),
                               str(src), "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
        assert got == [C.sizeof(S), S.kind.offset, S.lr.offset, S.eps.offset, S.reserved.offset, 2, 0, 1, 2]
    assert C.sizeof(S) == 16
    assert (pel.lib.EMB_MASTER_SGD, pel.lib.EMB_MASTER_ADAGRAD, pel.lib.EMB_MASTER_ROWWISE_ADAGRAD) == (0, 1, 2)


def test_master_step_refuses_null_and_bad_arguments_without_a_gpu(pel):
    G = pel.lib.load_grad()
    INV = pel.lib.EMB_ERR_INVALID
    d = pel.lib.EmbGradDesc()
    ptrs = (C.c_void_p * 1)()
    spec = lambda kind=0, lr=0.1, eps=1e-10, reserved=0: C.byref(pel.lib.EmbMasterSpec(kind, lr, eps, reserved))  # noqa: E731
    err = G.emb_grad_last_error
    assert G.emb_grad_master_step(None, C.byref(d), ptrs, ptrs, 1, 0, spec(), None) == INV and b"context is NULL" in err()
    assert G.emb_grad_master_step(None, C.byref(d), ptrs, ptrs, 1, 0, None, None) == INV and b"spec is NULL" in err()
    # the bad-spec cases refuse before the context is looked at (it is NULL here, and that is not what the text names)
    for kind in (3, 7, 0xFFFFFFFF):
        assert G.emb_grad_master_step(None, C.byref(d), ptrs, ptrs, 1, 0, spec(kind=kind), None) == INV and b"unknown master step kind" in err()
    assert G.emb_grad_master_step(None, C.byref(d), ptrs, ptrs, 1, 0, spec(reserved=1), None) == INV and b"reserved" in err()
    for eps in (-1e-10, -0.5, float("nan")):
        for kind in (0, 1, 2):
            assert G.emb_grad_master_step(None, C.byref(d), ptrs, ptrs, 1, 0, spec(kind=kind, eps=eps), None) == INV and b"eps" in err()
    # NULL descs / masters (/ states where the kind needs them) refuse before the context is touched: any non-NULL value stands in for it
    fake = C.c_void_p(16)
    assert G.emb_grad_master_step(fake, None, ptrs, ptrs, 1, 0, spec(), None) == INV and b"is NULL" in err()
    assert G.emb_grad_master_step(fake, C.byref(d), None, ptrs, 1, 0, spec(), None) == INV and b"is NULL" in err()
    assert G.emb_grad_master_step(fake, C.byref(d), ptrs, None, 1, 0, spec(kind=1), None) == INV and b"is NULL" in err()
    assert G.emb_grad_master_step(fake, C.byref(d), ptrs, ptrs, 1, 7, spec(), None) == INV and b"index type" in err()
    assert G.emb_grad_master_report(None, None) == INV and b"context is NULL" in err()


def test_python_surface(pel):
    import inspect
    eng = import_module("pim-embedding-lookup_amd.engine")
    sig = inspect.signature(eng.GradContext.master_step)
    assert list(sig.parameters)[1:] == ["table_ids", "indices", "offsets", "grads", "masters", "lr", "optimizer", "states", "eps", "modes",
                                        "per_sample_weights", "padding_idx", "fixed_pooling", "stream"]
    assert sig.parameters["optimizer"].default == "sgd" and sig.parameters["eps"].default == 1e-10 and sig.parameters["states"].default is None
    assert callable(eng.GradContext.master_report) and callable(eng.EmbeddingEngine.master_of)
    assert pel.lib.MASTER_KINDS == {"sgd": 0, "adagrad": 1, "rowwise": 2}


def test_the_grad_library_finds_its_master_kernels_next_to_itself(pel):
    build = import_module("pim-embedding-lookup_amd.build")
    dyn = subprocess.check_output(["readelf", "-d", build.GRAD_LIB_PATH], text=True)
    assert "libpimemb_grad_master.so" in dyn and "$ORIGIN" in dyn
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_MASTER_LIB_PATH], text=True)
    assert {"pimemb_grad_master_launch", "pimemb_grad_master_clear"} <= {line.split()[-1] for line in syms.splitlines()}
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_LIB_PATH], text=True)
    assert {"emb_grad_master_step", "emb_grad_master_report"} <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_every_kernel_of_the_grad_library_is_named_grad_and_the_master_kernels_are_there(pel):
    codeobj = import_module("pim-embedding-lookup_amd.codeobj")
    build = import_module("pim-embedding-lookup_amd.build")
    grad = codeobj.kernel_resources(build.GRAD_LIB_PATH)
    assert grad and all("grad_" in k for k in grad), sorted(grad)
    assert not [k for k in grad if "master" in k]        # the master kernels have a code object of their own, next to the library
    res = codeobj.kernel_resources(build.GRAD_MASTER_LIB_PATH)
    assert res and all("grad_" in k for k in res), sorted(res)
    assert sum("grad_master_clear" in k for k in res) == 1
    assert len(res) == 11 and all("grad_master_" in k for k in res), sorted(res)      # nothing but the master kernels: no second copy of a shared one
    group = {k: v for k, v in res.items() if "grad_master_rows_group" in k}
    elem = {k: v for k, v in res.items() if "grad_master_rows_elem" in k}
    assert len(group) == 6 and len(elem) == 4, (sorted(group), sorted(elem))      # three kinds (two element-wise) x two orders
    for k, v in {**group, **elem}.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["lds"] == 0, (k, v)


# ---- the harness ------------------------------------------------------------------------------------------------------------------
def test_harness_master_weights_flag_goes_with_a_fused_step_and_not_with_the_multi_table_step():
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    with pytest.raises(SystemExit) as ei:
        h.main(["--arch-embedding-size=10-10", "--master-weights"])
    assert "--master-weights goes with" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        h.main(["--arch-embedding-size=10-10", "--master-weights", "--fused-sgd", "0.1", "--multi-table-step"])
    assert "no multi-table master step" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        h.main(["--arch-embedding-size=10-10", "--master-weights", "--fused-sgd", "0.1"])
    assert "an f32 table is its own master" in str(ei.value)
    for dt in ("fp8_e4m3", "fp8_e5m2", "mxfp4"):                # the harness refuses to train them in place, before any GPU work
        with pytest.raises(SystemExit) as ei:
            h.main(["--arch-embedding-size=10-10", "--table-dtype", dt, "--fused-adagrad", "0.1"])
        assert "trains with --master-weights only" in str(ei.value)
    import inspect
    for name in ("enable_fused_sgd", "enable_fused_adagrad"):
        cls = [c for c in vars(h).values() if inspect.isclass(c) and hasattr(c, name) and c.__module__ == h.__name__]
        assert cls and inspect.signature(getattr(cls[0], name)).parameters["master_weights"].default is False


def test_modules_keep_master_weights_off_by_default():
    import inspect
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    for cls in (tm.PoolingEmbeddingBag, tm.FusedPoolingEmbeddingBags):
        for name in ("enable_fused_sgd", "enable_fused_adagrad"):
            assert inspect.signature(getattr(cls, name)).parameters["master_weights"].default is False


def test_master_probe_lists_its_measurements_and_refuses_unknown_ones():
    import importlib.util
    spec = importlib.util.spec_from_file_location("master_probe", os.path.join(ROOT, "tools", "master_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    assert set(probe.STEPS) == {f"{s}-{k}" for s in ("uniform", "zipf", "kaggle") for k in ("bf16", "e4m3", "mxfp4")} - {"kaggle-mxfp4"}
    assert probe.SHAPES["uniform"] == (4 << 20, 128, 32, 2048) and probe.SHAPES["kaggle"] == (10131227, 16, 1, 39292) and probe.SEGMENT == 64
    with pytest.raises(SystemExit) as ei:
        probe.main(["--steps", "uniform-f32"])
    assert "unknown step" in str(ei.value)
    assert probe.median_spread([3.0, 1.0, 2.0])["median_us"] == 2.0
