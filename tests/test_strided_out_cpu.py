"""CPU: strided pooled output (emb_lookup_strided / emb_plan_create_strided, engine.lookup_concat) as far as it can be
checked without a GPU -- the two entry points in the header, the exports and the binding; the code object of the
cross-compiled library (a strided twin, under a name of its own and without spills, for every launch record a strided plan can
describe; the same records without `strided` resolve as before); the refusal of bad output views before the engine is
touched; and the engine's host side as a stand-alone program over the HIP runtime stub, under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pimemb.h")
ENTRY_POINTS = ("emb_lookup_strided", "emb_plan_create_strided")
PINNED = ("bag_sum_", "bag_pool_", "bag_bf16pool_", "bag_f8pool_", "bag_hpool_", "mx4")      # fragments other tests pin kernel sets by


def test_entry_points_in_header_exports_and_binding(pel):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pel.LIB_PATH], text=True)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(emb_engine \*e, const emb_lookup_desc \*descs, const emb_pool_spec \*pools\s*,\s*"
                         r"const uint64_t \*out_stride, uint32_t n_descs, emb_index_type itype," % name, text), name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert name in pel.lib.SIGNATURES and getattr(pel.lib.load(), name) is not None
    assert len(pel.lib.SIGNATURES["emb_lookup_strided"][1]) == 9 and len(pel.lib.SIGNATURES["emb_plan_create_strided"][1]) == 7


def sum_records(itype, dtype):
    """Every plain-sum launch record a strided plan can describe for (index type, dtype): 7 wave-batch + 3 two-batch + 7
    lane-group -- without `strided`."""
    recs = []
    for lpr in (1, 2, 4, 8, 16, 32, 64):
        for kind in (0, 1):
            recs.append(dict(kind=kind, dtype=dtype, itype=itype, lanes_per_row=lpr, anydim_vec=0, ranged=0))
        if lpr <= 4:
            recs.append(dict(kind=2, dtype=dtype, itype=itype, lanes_per_row=lpr, anydim_vec=0, ranged=0))
    return recs


def pool_records(itype, dtype):
    """... and every pooled one: 7 wave-batch + 7 lane-group."""
    return [dict(kind=kind, dtype=dtype, itype=itype, lanes_per_row=lpr, anydim_vec=0, ranged=0, pool=1)
            for lpr in (1, 2, 4, 8, 16, 32, 64) for kind in (0, 1)]


def mx4_records(itype):
    """MXFP4: the lane-group pair, seven row widths each."""
    return [dict(kind=1, dtype=10, itype=itype, lanes_per_row=lpr, anydim_vec=0, ranged=0, **extra)
            for lpr in (1, 2, 4, 8, 16, 32, 64) for extra in ({}, {"pool": 1})]


@pytest.fixture(scope="module")
def code(pel):
    from pim_embedding_lookup_amd import codeobj
    return codeobj, codeobj.kernel_hashes(pel.LIB_PATH), codeobj.kernel_resources(pel.LIB_PATH)


@pytest.mark.parametrize("itype", [0, 1], ids=["u32", "i64"])
def test_every_strided_record_names_one_kernel_of_its_own(pel, code, itype):
    codeobj, hashes, res = code
    recs = []
    for dtype in (0, 1, 3, 8, 9):                 # f32, f16, bf16, fp8 e4m3 / e5m2
        s, p = sum_records(itype, dtype), pool_records(itype, dtype)
        assert len(s) == 7 + 3 + 7 and len(p) == 7 + 7
        recs += s + p
    recs += mx4_records(itype)
    assert len(recs) == 5 * (17 + 14) + 14
    seen = set()

    def hits(r):
        frags = codeobj.symbol_fragments(r)
        return [k for k in hashes if all(f in k for f in frags)]
    for rec in recs:
        plain, twin = hits(rec), hits(dict(rec, strided=1))
        assert len(plain) == 1 and len(twin) == 1, (rec, plain, twin)
        assert plain[0] != twin[0] and hashes[plain[0]] != hashes[twin[0]], rec
        assert codeobj.kernel_of_launch(pel.LIB_PATH, dict(rec, strided=1))[0] == twin[0]
        assert "bag_strided_" in twin[0] and not any(f in twin[0] for f in PINNED), twin[0]
        assert "bag_strided_" not in plain[0], plain[0]
        r = res[twin[0]]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (twin[0], r)
        seen.add(twin[0])
    assert len(seen) == len(recs)                 # one kernel per record, no two records share one


def test_the_strided_set_is_exactly_the_twins_and_pinned_sets_are_what_they_were(pel, code):
    _codeobj, hashes, _res = code
    names = list(hashes)
    twins = [n for n in names if "bag_strided_" in n]
    assert len(twins) == 2 * (5 * (17 + 14) + 14)                    # both index widths; no ranged, hot-row, any-dim or half-output twin
    assert not any("anydim" in n or "hot" in n for n in twins)
    assert all("Lb0EEEvPK" in n for n in twins if "bag_strided_sum_wavebatch" in n)          # never RANGED
    assert sum("mx4" in n for n in names) == 28 and sum("bag_pool_" in n for n in names) == 64
    assert sum("bag_bf16pool_" in n for n in names) == 32 and sum("bag_f8pool_" in n for n in names) == 64
    assert sum("bag_hpool_" in n for n in names) == 64


def test_records_no_strided_twin_exists_for_are_refused(pel, code):
    codeobj, _hashes, _res = code
    base = dict(kind=1, dtype=0, itype=0, lanes_per_row=4, anydim_vec=0, ranged=0, strided=1)
    for bad in (dict(base, kind=3, lanes_per_row=0), dict(base, kind=4), dict(base, out=1, dtype=1), dict(base, kind=0, ranged=1),
                dict(base, kind=2, pool=1), dict(base, dtype=10, kind=0)):
        with pytest.raises(LookupError):
            codeobj.symbol_fragments(bad)


def bare_engine(pel):
    eng = pel.EmbeddingEngine.__new__(pel.EmbeddingEngine)          # (no emb_create: the refusal must come before any C call)
    eng._tables = {0: (100, 16, pel.EMB_F32), 1: (100, 32, pel.EMB_F32)}
    return eng


@pytest.mark.parametrize("method", ["lookup_concat", "plan_concat"])
def test_bad_output_views_are_refused_before_any_c_call(pel, method):
    eng = bare_engine(pel)
    call = getattr(eng, method)
    idx = torch.arange(8)
    args = ([0, 1], [idx, idx], [idx, idx])
    with pytest.raises(ValueError, match="inner stride"):
        call(*args, out=torch.zeros((8, 128))[:, ::2])
    with pytest.raises(ValueError, match="too narrow"):
        call(*args, out=torch.zeros((8, 44)))
    with pytest.raises(ValueError, match="too narrow"):
        call(*args, out=torch.zeros((8, 48)), col=4)
    with pytest.raises(ValueError, match="multiple of 4"):
        call(*args, out=torch.zeros((8, 50)))
    with pytest.raises(ValueError, match="multiple of 4"):
        call(*args, out=torch.zeros((8, 52)), col=2)
    with pytest.raises(ValueError, match="overlap"):               # an expanded view: row stride 0, which the C call would read as dense
        call(*args, out=torch.zeros((1, 48)).expand(8, 48))
    with pytest.raises(ValueError, match="2-D"):
        call(*args, out=torch.zeros((8 * 48,)))
    with pytest.raises(ValueError, match="rows"):
        call(*args, out=torch.zeros((7, 48)))
    for wrong in (torch.zeros((8, 48), dtype=torch.float64), torch.zeros((8, 48), dtype=torch.float16), np.zeros((8, 48), np.float32)):
        with pytest.raises(TypeError, match="float32 torch tensor"):
            call(*args, out=wrong)
    with pytest.raises(TypeError, match="CUDA"):                    # a fine view -- of host memory: strided output is device-only
        call(*args, out=torch.zeros((8, 48)))
    with pytest.raises(KeyError):
        call([0, 5], [idx, idx], [idx, idx])
    with pytest.raises(ValueError, match="same number of bags"):
        call([0, 1], [idx, idx], [idx, idx[:4]])


def test_fused_modules_refuse_concat_with_half_output(pel):
    from pim_embedding_lookup_amd import torch_module as tm

    class Bag:           # what the fused modules read off a bag before they touch an engine
        _engine_out, _table_dtype = "table", torch.float16
    with pytest.raises(ValueError, match="concat=True"):
        tm._concat_flag(True, [Bag()], None)
    assert tm._concat_flag(False, [Bag()], None) is False


def test_host_side_under_sanitizers(tmp_path):
    """tests/cpp/strided_out_host_check.cpp: every refusal, the grouping of mixed descriptors, plan text / signature / bytes,
    the stride in DevDesc.words[3] of strided launches and zero in dense, ranged and queue launches, a deferred finding
    reported once -- over the HIP runtime stub, under AddressSanitizer + UBSan, as a program of its own.  The library's host
    objects are built as for tests/cpp/host_logic_check; the linker's --wrap lets the program see every kernel launch."""
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
                           os.path.join(ROOT, "tests", "cpp", "strided_out_host_check.cpp"), "-o", str(out / "strided_out_host_check.o")])
    # the twins' translation unit, which the shared build script does not know: the host half, with the script's flags
    src = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "-fPIC", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", src,
                           "-x", "hip", "--cuda-host-only", *san, "-Wno-option-ignored", "-Wno-unused-command-line-argument", "-c",
                           os.path.join(src, "pimemb_strided_kernels.hip"), "-o", str(out / "pimemb_strided_kernels.o")])
    objs = [str(out / (n + ".o")) for n in ("strided_out_host_check", "pimemb_kernels", "pimemb_strided_kernels", "pimemb_engine", "pimemb_compat",
                                            "pimemb_shard", "pimemb_peer", "hip_runtime_stub")]
    undefined = subprocess.check_output(["nm", "-u", str(out / "pimemb_kernels.o"), str(out / "pimemb_strided_kernels.o")], text=True)
    defs = ["-Wl,--defsym=%s=pimemb_stub_fatbin" % sym for sym in sorted(set(re.findall(r"__hip_fatbin_[0-9a-f]+", undefined)))]
    wraps = ["-Wl,--wrap=hipLaunchKernel", "-Wl,--wrap=__hipRegisterFunction"]
    exe = out / "strided_out_host_check"
    subprocess.check_call([clang, *san, *objs, "-o", str(exe), *defs, *wraps, "-lpthread", "-ldl", "-lrt"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "strided-out host logic ok" in run.stdout, run.stdout[-1500:] + run.stderr[-4000:]
    assert "pimemb:" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-4000:]
