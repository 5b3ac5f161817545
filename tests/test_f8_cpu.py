"""CPU: the FP8 table dtypes (EMB_F8_E4M3 = OCP e4m3fn, EMB_F8_E5M2 = OCP e5m2) as far as they can be checked without a GPU --
the two #defines in the header (outside the enum, whose body other tests pin) and the binding, the numpy bit helpers of
formats.py against torch over every pattern and a million roundings, the code object of the cross-compiled library (an fp8
instantiation next to every bf16 one, none spilling, every launch record resolving), the Python refusals that come before
any C call, and the engine's host side over the HIP runtime stub as a stand-alone program under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pimemb.h")
KINDS = [("e4m3", torch.float8_e4m3fn, 8), ("e5m2", torch.float8_e5m2, 9)]
IDS = [k[0] for k in KINDS]


@pytest.fixture(scope="module")
def formats():
    from importlib import import_module
    return import_module("pim-embedding-lookup_amd.formats")


def test_defines_in_header_and_binding(pel):
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)                         # strip comments
    assert re.search(r"^#define\s+EMB_F8_E4M3\s+\(\(emb_dtype\)8\)\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+EMB_F8_E5M2\s+\(\(emb_dtype\)9\)\s*$", text, flags=re.M)
    body = re.search(r"typedef\s+enum\s+emb_dtype\s*\{(.*?)\}\s*emb_dtype\s*;", text, flags=re.S).group(1)
    enum = {k: int(v) for k, v in re.findall(r"\b(EMB_\w+)\s*=\s*(\d+)", body)}
    assert enum == {"EMB_F32": 0, "EMB_F16": 1, "EMB_FIXED32": 2, "EMB_BF16": 3}       # the enum's body is what it was
    assert pel.lib.EMB_F8_E4M3 == 8 and pel.lib.EMB_F8_E5M2 == 9
    assert pel.EMB_F8_E4M3 == 8 and pel.EMB_F8_E5M2 == 9
    assert "EMB_F8_E4M3" in pel.__all__ and "EMB_F8_E5M2" in pel.__all__


@pytest.mark.parametrize("kind,tdt,dt", KINDS, ids=IDS)
def test_from_f8_bits_every_pattern(formats, kind, tdt, dt):
    bits = np.arange(256, dtype=np.uint8)
    want = torch.arange(256, dtype=torch.uint8).view(tdt).float().numpy()
    for k in (kind, dt):                                                     # by name and by dtype value
        got = formats.from_f8_bits(bits, k)
        assert got.dtype == np.float32 and got.shape == bits.shape
        nan = np.isnan(want)
        assert nan.sum() == (2 if kind == "e4m3" else 6)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))      # bit for bit: signed zeros, subnormals, infinities
    assert formats.from_f8_bits(bits.reshape(16, 16), kind).shape == (16, 16)
    with pytest.raises(ValueError):
        formats.from_f8_bits(bits, "e3m4")


def _rounding_inputs(formats, kind):
    """fp32 inputs as tests/test_bf16_cpu.py::_rounding_inputs builds them, for an fp8 grid: random bit patterns, every fp8
    value and the exact ties between neighbours (even and odd) with their own neighbours, the fp8 subnormal range, values around
    the largest finite value, +-0, +-inf, NaNs."""
    rng = np.random.default_rng(8)
    parts = [rng.integers(0, 1 << 32, size=1_000_000, dtype=np.uint64).astype(np.uint32)]       # random fp32 bit patterns
    grid = formats.from_f8_bits(np.arange(256, dtype=np.uint8), kind)
    pos = np.sort(grid[np.isfinite(grid) & (grid >= 0)].astype(np.float64))
    pos = np.unique(pos)
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)                                         # exact ties (representable in fp32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)
    for base in (pos.astype(np.float32), mid):
        u = base.view(np.uint32)
        for delta in (-2, -1, 0, 1, 2):
            v = (u.astype(np.int64) + delta).clip(0, 0x7F7FFFFF).astype(np.uint32)
            parts += [v, v | np.uint32(0x80000000)]
    # in-range magnitudes, dense: random mantissas over the exponents the format covers, plus the subnormal range and below
    lo, hi = float(pos[1]), float(pos[-1])
    mags = np.exp(rng.uniform(np.log(lo / 16), np.log(hi * 1.2), size=200_000)).astype(np.float32)
    sub = rng.uniform(0, float(pos[8]), size=100_000).astype(np.float32)                        # the fp8 subnormals and the first normals
    parts += [mags.view(np.uint32), (-mags).view(np.uint32), sub.view(np.uint32), (-sub).view(np.uint32)]
    top = np.float32(hi)
    step = np.float32(pos[-1] - pos[-2])
    around = np.float32([top - step, top - step / 2, top, top + step / 4, top + step / 2, top + step, top * 2, 3.0e38])
    around = np.concatenate([around, np.nextafter(around, np.float32(0)), np.nextafter(around, np.float32(np.inf))])
    parts += [around.view(np.uint32), (-around).view(np.uint32)]
    parts.append(np.array([0x7F800000, 0xFF800000, 0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x00800000], np.uint32))      # +-inf, +-0, fp32 denormals
    parts.append(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F80FFFF, 0x7FBF0000], np.uint32))  # NaNs
    return np.concatenate(parts)


@pytest.mark.parametrize("kind,tdt,dt", KINDS, ids=IDS)
def test_to_f8_bits_rounds_like_torch(formats, kind, tdt, dt):
    u = _rounding_inputs(formats, kind)
    x = u.view(np.float32)
    assert len(x) >= 1_000_000
    got = formats.to_f8_bits(x, kind)
    want_t = torch.from_numpy(x.copy()).to(tdt)
    want = want_t.view(torch.uint8).numpy()
    assert got.dtype == np.uint8 and got.shape == x.shape
    want_nan = np.isnan(want_t.float().numpy())                             # (e4m3fn: overflow is NaN, so more than the NaN inputs)
    assert np.isnan(x).sum() > 1000 and (~want_nan).sum() > 900_000
    assert np.array_equal(got[~want_nan], want[~want_nan])
    assert np.isnan(formats.from_f8_bits(got[want_nan], kind)).all()        # NaN stays NaN; whatever torch overflows to NaN does here
    assert np.array_equal(got[want_nan] & 0x80, want[want_nan] & 0x80)      # ... under the sign torch keeps
    f32 = lambda *v: np.float32(v)                                          # noqa: E731
    if kind == "e4m3":
        assert formats.to_f8_bits(f32(448, 464, 465, 480, -480, np.inf, -np.inf), kind).tolist() == [0x7E, 0x7E, 0x7F, 0x7F, 0xFF, 0x7F, 0xFF]
        assert formats.to_f8_bits(f32(1.0, 1.0625, 1.1875, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10), kind).tolist() == [0x38, 0x38, 0x3A, 0x01, 0x00, 0x02]
    else:
        assert formats.to_f8_bits(f32(57344, 61439, 61440, -61440, np.inf, -np.inf), kind).tolist() == [0x7B, 0x7B, 0x7C, 0xFC, 0x7C, 0xFC]
        assert formats.to_f8_bits(f32(1.0, 1.125, 1.375, 2.0 ** -16, 2.0 ** -17, 3 * 2.0 ** -17), kind).tolist() == [0x3C, 0x3C, 0x3E, 0x01, 0x00, 0x02]
    assert formats.to_f8_bits(np.float32([0.0, -0.0]), kind).tolist() == [0x00, 0x80]
    # a round trip of fp8 values is the identity
    b = np.arange(256, dtype=np.uint8)
    f = formats.from_f8_bits(b, kind)
    keep = ~np.isnan(f)
    assert np.array_equal(formats.to_f8_bits(f, kind)[keep], b[keep])
    assert formats.to_f8_bits(np.zeros((3, 5), np.float32), dt).shape == (3, 5)


def _dtype_kernels(names, dt, pool_name):
    """{(kernel, index type, the template arguments after DT): mangled name} of the fp32-out bag kernels instantiated for table
    dtype `dt` (template heads <IdxT, DT, ...>; j = uint32, l = int64).  The pooled kernels of bf16 / fp8 tables are the
    bag_pool_* kernels under a name of their own (`pool_name`): the same kernel here."""
    pat = re.compile(r"^_ZN6pimemb\d+(bag_(?:sum|%s)_\w+?_kernel)I([jl])Li%dE(.*)$" % (pool_name, dt))
    out = {}
    for n in names:
        m = pat.match(n)
        if m:
            out[(m.group(1).replace("bag_%s_" % pool_name, "bag_pool_"), m.group(2), m.group(3))] = n
    return out


def _f8_records(itype, dt):
    """Every launch record an fp8 plan can describe: kinds 0 / 1 / 2 / 3 / 4, 1 ... 64 lanes per row, ranged, pooled."""
    recs = []
    for lpr in (1, 2, 4, 8, 16, 32, 64):
        for kind in (0, 1, 2, 4):
            if kind == 2 and lpr > 4:
                continue
            for ranged in ((0, 1) if kind in (0, 2) else (0,)):
                recs.append(dict(kind=kind, dtype=dt, itype=itype, lanes_per_row=lpr, ranged=ranged))
        for kind in (0, 1):
            recs.append(dict(kind=kind, dtype=dt, itype=itype, lanes_per_row=lpr, pool=1))
    for vec in (0, 1):
        recs.append(dict(kind=3, dtype=dt, itype=itype, lanes_per_row=0, anydim_vec=vec, ranged=0))
        recs.append(dict(kind=3, dtype=dt, itype=itype, lanes_per_row=0, anydim_vec=vec, pool=1))
    return recs


@pytest.mark.parametrize("kind,tdt,dt", KINDS, ids=IDS)
def test_every_bf16_kernel_has_an_fp8_twin_without_spills(pel, kind, tdt, dt):
    from pim_embedding_lookup_amd import codeobj
    hashes = codeobj.kernel_hashes(pel.LIB_PATH)
    res = codeobj.kernel_resources(pel.LIB_PATH)
    bf16, f8 = _dtype_kernels(hashes, 3, "bf16pool"), _dtype_kernels(hashes, dt, "f8pool")
    assert len(bf16) >= 100, len(bf16)                                      # every family: wave-batch (+ ranged, two-batch), group, hot, any-dim, pooled
    # equal template arguments but for the configuration, which differs by dtype in NAME only when its values are the same
    # type: BagCfg<...> spells its values out, so the mangled arguments are equal text
    assert set(bf16) == set(f8), (sorted(set(bf16) - set(f8))[:4], sorted(set(f8) - set(bf16))[:4])
    assert len(set(f8.values())) == len(f8)
    for family in ("bag_sum_wavebatch_kernel", "bag_sum_group_kernel", "bag_sum_hot_kernel", "bag_sum_anydim_kernel",
                   "bag_sum_anydim_vec_kernel", "bag_pool_wavebatch_kernel", "bag_pool_group_kernel", "bag_pool_anydim_kernel"):
        assert any(k[0] == family for k in f8), family
    for n in sorted(f8.values()):
        r = res[n]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
    # every launch record an fp8 plan can describe names exactly one of them
    seen = set()
    for itype in (0, 1):
        for rec in _f8_records(itype, dt):
            sym, _sha = codeobj.kernel_of_launch(pel.LIB_PATH, rec)
            assert sym in f8.values(), (rec, sym)
            assert ("bag_f8pool_" in sym) == ("pool" in rec), (rec, sym)
            seen.add(sym)
    assert seen == set(f8.values())                                         # ... and nothing is instantiated that no record names


def test_the_kernel_sets_other_tests_pin_are_what_they_were(pel):
    from pim_embedding_lookup_amd import codeobj
    names = list(codeobj.kernel_hashes(pel.LIB_PATH))
    assert sum("bag_pool_" in n for n in names) == 64
    assert sum("bag_f8pool_" in n for n in names) == 2 * 2 * (7 + 7 + 2)      # index width x encoding x (wave-batch + lane-group + any-dim)
    # resolution of the existing dtypes' records has not moved
    for dt, pool in ((0, "bag_pool_"), (1, "bag_pool_"), (3, "bag_bf16pool_")):
        sym, _ = codeobj.kernel_of_launch(pel.LIB_PATH, dict(kind=1, dtype=dt, itype=0, lanes_per_row=8, pool=1))
        assert pool in sym and "Li%dELi8E" % dt in sym
        sym, _ = codeobj.kernel_of_launch(pel.LIB_PATH, dict(kind=0, dtype=dt, itype=1, lanes_per_row=8, ranged=0))
        assert "bag_sum_wavebatch_kernelIlLi%dELi8E" % dt in sym


def test_load_table_takes_uint8_only_as_declared_fp8(pel):
    """numpy has no fp8: a uint8 array is refused unless dtype= says which encoding its bits are (decided before the engine is
    touched, so no GPU is needed to see the refusal)."""
    eng = pel.EmbeddingEngine.__new__(pel.EmbeddingEngine)                  # (no emb_create: load_table must refuse before any C call)
    with pytest.raises(KeyError):
        eng.load_table(0, np.zeros((4, 16), np.uint8))

    # ... and with dtype= the array reaches the C call as what it was declared to be; float8 tensors without saying so
    class StubLib:
        calls = []

        def emb_load_table(self, h, table_id, nr_rows, dim, dtype, ptr, space):
            self.calls.append((table_id, nr_rows, dim, dtype, ptr, space))
            return 0
    eng._L, eng._h, eng._tables, eng._same_dim = StubLib(), None, {}, {}
    bits = np.arange(64, dtype=np.uint8).reshape(4, 16)
    eng.load_table(3, bits, dtype=pel.EMB_F8_E4M3)
    eng.load_table(4, bits, dtype=pel.EMB_F8_E5M2)
    t8 = torch.zeros((5, 32)).to(torch.float8_e4m3fn)
    t9 = torch.zeros((6, 48)).to(torch.float8_e5m2)
    eng.load_table(5, t8)
    eng.load_table(6, t9)
    calls = StubLib.calls
    assert [c[:4] for c in calls] == [(3, 4, 16, 8), (4, 4, 16, 9), (5, 5, 32, 8), (6, 6, 48, 9)]
    assert calls[0][4] == bits.ctypes.data and calls[2][4] == t8.data_ptr() and all(c[5] == pel.EMB_MEM_HOST for c in calls)
    assert eng._tables == {3: (4, 16, 8), 4: (4, 16, 9), 5: (5, 32, 8), 6: (6, 48, 9)}


@pytest.mark.parametrize("dt", [8, 9], ids=IDS)
def test_out_dtype_table_on_an_fp8_table_is_refused_before_any_c_call(pel, dt):
    eng = pel.EmbeddingEngine.__new__(pel.EmbeddingEngine)
    eng._tables = {0: (16, 16, dt)}
    idx, off = np.arange(4, dtype=np.int64), np.arange(4, dtype=np.int64)
    needs = "returns fp32 rows only"
    with pytest.raises(TypeError, match=needs):
        eng.lookup_batched([0], [idx], [off], out_dtype="table")
    with pytest.raises(TypeError, match=needs):
        eng.lookup(0, idx, off, out_dtype="table")
    with pytest.raises(TypeError, match=needs):
        eng.lookup_pooled([0], [idx], [off], "mean", out_dtype="table")
    with pytest.raises(TypeError, match=needs):
        eng.plan([0], [idx], [off], out_dtype="table")
    with pytest.raises(TypeError):                                          # (no 1-byte output buffer either)
        eng.lookup_batched([0], [idx], [off], outs=[np.zeros((4, 16), np.uint8)], out_dtype="table")
    from pim_embedding_lookup_amd import torch_module
    with pytest.raises(ValueError, match="float8"):
        torch_module._engine_out_dtype("weight", torch.float8_e4m3fn if dt == 8 else torch.float8_e5m2)


def test_host_side_under_sanitizers(tmp_path):
    """tests/cpp/f8_host_check.cpp: the engine's host side of the fp8 dtypes -- staging sizes of HOST calls out of exactly sized
    1-byte tables, hot-row staging, plan bytes / text / signature, the refusals, the request queue and a one-rank shard -- over
    the HIP runtime stub, under AddressSanitizer + UBSan.  The library's host objects are built as for
    tests/cpp/host_logic_check, the program linked as tests/test_half_out_cpu.py links its own."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    clang = os.path.join(os.path.dirname(hipcc), "..", "lib", "llvm", "bin", "clang++")
    out = tmp_path / "obj"
    build = subprocess.run(["bash", os.path.join(ROOT, "tests", "cpp", "build_host_logic_check.sh"), "address,undefined", str(out)],
                           capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and "libclang_rt" in build.stderr and "No such file" in build.stderr:
        pytest.skip("sanitizer runtime not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-3000:]
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.check_call([clang, "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "f8_host_check.cpp"), "-o", str(out / "f8_host_check.o")])
    objs = [str(out / (n + ".o")) for n in ("f8_host_check", "pimemb_kernels", "pimemb_engine", "pimemb_compat", "pimemb_shard",
                                            "pimemb_peer", "hip_runtime_stub")]
    undefined = subprocess.check_output(["nm", "-u", str(out / "pimemb_kernels.o")], text=True)
    defs = ["-Wl,--defsym=%s=pimemb_stub_fatbin" % sym for sym in sorted(set(re.findall(r"__hip_fatbin_[0-9a-f]+", undefined)))]
    exe = out / "f8_host_check"
    subprocess.check_call([clang, *san, *objs, "-o", str(exe), *defs, "-lpthread", "-ldl", "-lrt"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "f8 host logic ok" in run.stdout, run.stdout[-1500:] + run.stderr[-4000:]
    assert "pimemb:" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-4000:]
