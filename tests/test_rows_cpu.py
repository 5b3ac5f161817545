"""CPU: the row writer's companion library (libpimemb_rows.so, include/pimemb_rows.h) builds, loads next to libpimemb.so,
exports and binds what its header declares, keeps its kernels out of the main library's code object -- and its encoders
(csrc/pimemb_rows_encode.h, the very text the kernels compile), run on the host, agree bit for bit with formats.py on random bit
patterns and on every edge class.  No GPU work is called."""
import ctypes as C
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_cases as rc  # noqa: E402

ROOT = rc.ROOT
HEADER = os.path.join(ROOT, "include", "pimemb_rows.h")
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
build = import_module("pim-embedding-lookup_amd.build")
codeobj = import_module("pim-embedding-lookup_amd.codeobj")


def declared_functions(path):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"typedef\s+(struct|enum)\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b([a-z_][a-z0-9_]*)\s*\([^;{]*\)\s*;", text)))


def test_companion_library_is_built_and_loads_next_to_the_main_one(pel):
    assert os.path.exists(build.ROWS_LIB_PATH), "libpimemb_rows.so must be built in-tree (__graft_entry__.build())"
    assert os.path.dirname(build.ROWS_LIB_PATH) == os.path.dirname(pel.LIB_PATH)
    R = pel.lib.load_rows()
    assert R.emb_rows_last_error() == b""
    maps = [line.split()[-1] for line in open("/proc/self/maps") if "libpimemb" in line]
    assert {os.path.basename(m) for m in maps} >= {"libpimemb.so", "libpimemb_rows.so"}
    assert len({m for m in maps if os.path.basename(m) == "libpimemb.so"}) == 1      # ONE engine library in the process


def test_exports_and_binds_every_declared_function(pel):
    fns = declared_functions(HEADER)
    assert {"emb_rows_create", "emb_rows_destroy", "emb_rows_update", "emb_rows_report", "emb_rows_scratch_bytes"} <= set(fns)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.ROWS_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in fns if f not in exported]
    assert sorted(pel.lib.ROWS_SIGNATURES) == fns
    assert not set(pel.lib.ROWS_SIGNATURES) & set(pel.lib.SIGNATURES)
    R = pel.lib.load_rows()
    for name in fns:
        assert getattr(R, name) is not None


def test_header_compiles_as_c_and_cxx_and_constants_match(pel, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "pimemb_rows.h"\nint main(void){emb_rows *w = 0; (void)w;\n'
                   'printf("%d %d %u %zu\\n", (int)EMB_ROWS_SRC_F32, (int)EMB_ROWS_SRC_TABLE_DTYPE, EMB_ROWS_UNIQUE_IDS, sizeof(emb_rows_src));\n'
                   'return 0;}\n')
    L = pel.lib
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"),
                               str(src), "-o", str(exe)])
        got = subprocess.check_output([str(exe)], text=True).split()
        assert [int(x) for x in got] == [L.EMB_ROWS_SRC_F32, L.EMB_ROWS_SRC_TABLE_DTYPE, L.EMB_ROWS_UNIQUE_IDS, C.sizeof(C.c_int)]


def test_scratch_bytes_is_monotone_and_holds_two_slots_per_row(pel):
    R = pel.lib.load_rows()
    prev_s = prev_p = 0
    for n in (1, 2, 31, 32, 33, 255, 256, 1037, 65536, 65537, 1 << 20, (1 << 24) + 1, (1 << 31) - 1):
        s, p = R.emb_rows_scratch_bytes(n), R.emb_rows_stage_bytes(n)
        assert s >= prev_s and p >= prev_p, n
        assert s >= 2 * n * 12, n                 # a 64-bit key and a 32-bit winner per slot, at least 2 n slots
        slots = (s - 256) // 12
        assert slots >= 2 * n and slots & (slots - 1) == 0, n
        prev_s, prev_p = s, p
    assert R.emb_rows_stage_bytes(1) >= 2 * (4 * 2048 + 8 + 32)          # either half holds the widest source row the kernels take


def test_hot_count_is_exported_and_bound(pel):
    assert "emb_table_hot_count" in declared_functions(os.path.join(ROOT, "include", "pimemb.h"))
    assert "emb_table_hot_count" in pel.lib.SIGNATURES
    L = pel.lib.load()
    n = C.c_uint32(7)
    assert L.emb_table_hot_count(None, 0, C.byref(n)) == pel.lib.EMB_ERR_INVALID


def test_refuses_bad_arguments_without_a_gpu(pel):
    R = pel.lib.load_rows()
    h = C.c_void_p()
    assert R.emb_rows_create(None, 16, C.byref(h)) == pel.lib.EMB_ERR_INVALID
    assert b"NULL" in R.emb_rows_last_error()
    assert R.emb_rows_update(None, 0, None, 0, 0, None, 0, 0, 0, None, None) == pel.lib.EMB_ERR_INVALID
    assert R.emb_rows_report(None, None) == pel.lib.EMB_ERR_INVALID
    assert R.emb_rows_destroy(None) == pel.lib.EMB_OK


def test_links_the_engine_and_one_hip_runtime_by_unversioned_name(pel):
    out = subprocess.check_output(["objdump", "-p", build.ROWS_LIB_PATH], text=True)
    needed = re.findall(r"NEEDED\s+(\S+)", out)
    assert "libamdhip64.so" in needed and "libpimemb.so" in needed
    assert not any(re.match(r"libamdhip64\.so\.\d", n) or n.startswith("libtorch") or n.startswith("libc10") for n in needed)
    assert "$ORIGIN" in re.search(r"RUNPATH\s+(\S+)", out).group(1)


def test_the_main_librarys_code_object_stays_closed(pel):
    """Every kernel of the write path lives in the companion's code object; the main library's holds none of them (its census,
    tests/test_kernel_census_cpu.py, and the profiles tied to its kernels' machine code depend on that)."""
    rows = codeobj.kernel_hashes(build.ROWS_LIB_PATH)
    main = codeobj.kernel_hashes(pel.LIB_PATH)
    names = ("rows_write_group", "rows_write_mx", "rows_write_elem", "rows_claim")
    assert rows and all(any(n in k for n in names) for k in rows), sorted(rows)
    for want in names:
        assert any(want in k for k in rows), want
    assert not [k for k in main if any(n in k for n in names)]
    assert not set(rows) & set(main)


# ---- the encoders on the host -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encode_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rows") / "rows_encode_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "rows_encode_check.cpp"), "-o", str(exe)])
    return str(exe)


def run_encoder(exe, kind, w, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(w, dtype=np.float32).tofile(src)
    subprocess.check_call([exe, kind, str(w.shape[1]), str(src), str(dst)])
    return np.fromfile(dst, dtype=np.uint8).reshape(w.shape[0], -1)


@pytest.mark.parametrize("kind", ["f16", "bf16", "e4m3", "e5m2"])
def test_encoders_equal_formats_py(encode_exe, tmp_path, kind):
    """Random BIT PATTERNS (every exponent, NaNs and denormals included), the edge block, and every value next to a rounding
    boundary of the target: all its own values widened, with the fp32 neighbours of each midpoint."""
    rng = np.random.default_rng(7)
    pats = rng.integers(0, 1 << 32, size=1 << 18, dtype=np.uint64).astype(np.uint32).view(np.float32)
    eb, mb, bias, _maxf = rc._FMT[kind]
    codes = np.arange(1 << (eb + mb), dtype=np.uint32)                           # every non-negative value of the format ...
    if kind == "bf16":
        own = (codes << np.uint32(16)).view(np.float32)
    elif kind == "f16":
        own = codes.astype(np.uint16).view(np.float16).astype(np.float32)
    else:
        own = rc.formats.from_f8_bits(codes.astype(np.uint8), kind)
    own = own[np.isfinite(own)]
    mids = ((own[:-1].astype(np.float64) + own[1:].astype(np.float64)) / 2).astype(np.float32)     # ... and the ties between neighbours
    near = np.concatenate([own, mids, np.nextafter(mids, np.float32(0)), np.nextafter(mids, np.float32(np.inf))])
    vals = np.concatenate([pats, rc.edge_values(kind), near, -near])
    vals = np.concatenate([vals, np.zeros(-len(vals) % 16, np.float32)]).reshape(-1, 16)
    got = run_encoder(encode_exe, kind, vals, tmp_path)
    want = rc.host_encode(kind, vals)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (kind, vals[bad[0]].view(np.uint32), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("dim", [32, 96])
def test_mxfp4_encoder_equals_formats_py(encode_exe, tmp_path, dim):
    w = rc.source("mxfp4", 4096, dim, seed=dim)
    rng = np.random.default_rng(dim + 1)
    # blocks of random finite bit patterns: every pairing of a large amax with tiny, denormal and zero elements
    pats = rng.integers(0, 1 << 32, size=(2048, dim), dtype=np.uint64).astype(np.uint32)
    pats = np.where((pats & 0x7F800000) == 0x7F800000, pats & np.uint32(0xBFFFFFFF), pats).astype(np.uint32)
    pats[::2] &= np.uint32(0x87FFFFFF)                                           # half of the rows: small exponents, scale bytes near the clamp
    w = np.concatenate([w, pats.view(np.float32)])
    got = run_encoder(encode_exe, "mxfp4", w, tmp_path)
    want = rc.host_encode("mxfp4", w)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (dim, bad[:5], got[bad[0]], want[bad[0]])
    # a non-finite value anywhere makes the row bad (formats.to_mxfp4 raises)
    w2 = w[:4].copy()
    w2[1, dim - 1], w2[3, 0] = np.inf, np.nan
    got = run_encoder(encode_exe, "mxfp4", w2, tmp_path)
    assert (got[[1, 3]] == 0xEE).all() and np.array_equal(got[[0, 2]], want[[0, 2]])
    with pytest.raises(ValueError):
        rc.formats.to_mxfp4(w2)
