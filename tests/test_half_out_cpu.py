"""CPU: half-width pooled output (EMB_POOL_OUT_TABLE_DTYPE) as far as it can be checked without a GPU -- the flag in the
header and the binding, the code object of the cross-compiled library (a half-output twin, under a name of its own and
without spills, for every launch record a plan can describe with out=1; the fp32-out records resolve as before) and the
refusal of outputs of the wrong dtype before the engine is touched; and the engine's host side of the flag as a stand-alone
program over the HIP runtime stub, under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pimemb.h")
NEEDS = 'out_dtype="table" needs an output of'      # the refusal these tests are about (not a TypeError for an unknown keyword)


def test_flag_in_header_and_binding(pel):
    text = open(HEADER).read()
    L = pel.lib
    assert re.search(r"#define EMB_POOL_OUT_TABLE_DTYPE %du\b" % L.EMB_POOL_OUT_TABLE_DTYPE, text)
    assert L.EMB_POOL_OUT_TABLE_DTYPE == 2
    assert L.EMB_POOL_OUT_TABLE_DTYPE != L.EMB_POOL_PADDING and L.EMB_POOL_OUT_TABLE_DTYPE & L.EMB_POOL_PADDING == 0


def records(itype, dtype):
    """Every launch record of a (index type, 2-byte table dtype) the engine can describe, without `out`."""
    recs = []
    for pool in (None, 1):
        extra = {} if pool is None else {"pool": pool}
        for lpr in (1, 2, 4, 8, 16, 32, 64):
            for kind in (0, 1):
                recs.append(dict(kind=kind, dtype=dtype, itype=itype, lanes_per_row=lpr, anydim_vec=0, ranged=0, **extra))
            if lpr <= 4 and pool is None:        # (the pooled family has one wave-batch geometry)
                recs.append(dict(kind=2, dtype=dtype, itype=itype, lanes_per_row=lpr, anydim_vec=0, ranged=0))
        for vec in (0, 1):                        # kind 3: element / piece
            recs.append(dict(kind=3, dtype=dtype, itype=itype, lanes_per_row=0, anydim_vec=vec, ranged=0, **extra))
    return recs


@pytest.mark.parametrize("dtype", [1, 3], ids=["fp16", "bf16"])
@pytest.mark.parametrize("itype", [0, 1], ids=["u32", "i64"])
def test_every_half_out_record_names_one_kernel_of_its_own(pel, itype, dtype):
    from pim_embedding_lookup_amd import codeobj
    hashes = codeobj.kernel_hashes(pel.LIB_PATH)
    res = codeobj.kernel_resources(pel.LIB_PATH)
    seen = set()
    recs = records(itype, dtype)
    assert len(recs) == 2 * (7 * 2 + 2) + 3
    for rec in recs:
        def hits(r):
            frags = codeobj.symbol_fragments(r)
            return [k for k in hashes if all(f in k for f in frags)]
        plain, half = hits(rec), hits(dict(rec, out=1))
        assert len(plain) == 1 and len(half) == 1, (rec, plain, half)
        assert plain[0] != half[0], rec
        assert codeobj.kernel_of_launch(pel.LIB_PATH, dict(rec, out=1))[0] == half[0]
        r = res[half[0]]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (half[0], r)
        seen.add(half[0])
        # the fp32-out record resolves to the kernel it resolves to today: its family's name, the table's public dtype value
        family = ("bag_bf16pool_" if dtype == 3 else "bag_pool_") if "pool" in rec else "bag_sum_"
        assert family in plain[0] and ("Li%dE" % dtype) in plain[0], (rec, plain[0])
        assert "bag_pool_" not in half[0] and "bag_bf16pool_" not in half[0], half[0]
    assert len(seen) == len(recs)                # one kernel per record, no two records share one


def test_fp32_out_kernel_sets_are_what_they_were(pel):
    """The sets other tests pin by name: 64 bag_pool_* kernels, and none of the new kernels carries a public dtype value in
    a bag_sum_* / bag_pool_* / bag_bf16pool_* name."""
    from pim_embedding_lookup_amd import codeobj
    names = list(codeobj.kernel_hashes(pel.LIB_PATH))
    assert sum("bag_pool_" in n for n in names) == 64
    half = [n for n in names if "bag_hpool_" in n or re.search(r"bag_sum_\w+?_kernelI[jl]Li1[79]E", n)]
    # index width x {fp16, bf16} x (7 wave-batch + 3 two-batch + 7 lane-group + 2 any-dim) sum twins, and x (7 + 7 + 2) pooled twins
    assert len(half) == 2 * 2 * (7 + 3 + 7 + 2) + 2 * 2 * (7 + 7 + 2), len(half)


@pytest.mark.parametrize("out", [torch.zeros((4, 8), dtype=torch.float32), np.zeros((4, 8), np.float32),
                                 torch.zeros((4, 8), dtype=torch.float64)], ids=["torch-f32", "numpy-f32", "torch-f64"])
def test_outs_of_the_wrong_dtype_are_refused_before_any_c_call(pel, out):
    eng = pel.EmbeddingEngine.__new__(pel.EmbeddingEngine)          # (no emb_create: the refusal must come before any C call)
    idx, off = np.arange(4, dtype=np.int64), np.arange(4, dtype=np.int64)
    with pytest.raises(TypeError, match=NEEDS):
        eng.lookup_batched([0], [idx], [off], outs=[out], out_dtype="table")
    with pytest.raises(TypeError, match=NEEDS):
        eng.lookup(0, idx, off, out=out, out_dtype="table")
    with pytest.raises(TypeError, match=NEEDS):
        eng.lookup_pooled([0], [idx], [off], "mean", outs=[out], out_dtype="table")
    with pytest.raises(TypeError, match=NEEDS):
        eng.plan([0], [idx], [off], outs=[out], out_dtype="table")
    with pytest.raises(ValueError):
        eng.lookup_batched([0], [idx], [off], out_dtype="float16")  # only None / "table"


def test_a_half_buffer_of_the_other_dtype_is_refused_too(pel):
    """fp16 rows for a bf16 table (and the other way round): known only with the table's dtype, still before any C call."""
    eng = pel.EmbeddingEngine.__new__(pel.EmbeddingEngine)
    eng._tables = {0: (16, 8, pel.EMB_BF16), 1: (16, 8, pel.EMB_F16)}
    idx, off = np.arange(4, dtype=np.int64), np.arange(4, dtype=np.int64)
    with pytest.raises(TypeError, match=NEEDS):
        eng.lookup_batched([0], [idx], [off], outs=[np.zeros((4, 8), np.float16)], out_dtype="table")
    with pytest.raises(TypeError, match=NEEDS):
        eng.lookup_batched([1], [idx], [off], outs=[np.zeros((4, 8), np.uint16)], out_dtype="table")
    t_idx = torch.arange(4)
    with pytest.raises(TypeError, match=NEEDS):
        eng.lookup_batched([0], [t_idx], [t_idx], outs=[torch.zeros((4, 8), dtype=torch.float16)], out_dtype="table")


def test_host_side_under_sanitizers(tmp_path):
    """tests/cpp/half_out_host_check.cpp: the engine's host side of the flag -- staging and copy-out sizes of HOST calls into
    exactly sized 2-byte outputs, checked calls, mixed descriptors, plan text / signature / bytes, refusals -- over the HIP
    runtime stub, under AddressSanitizer + UBSan.  The library's host objects are built as for tests/cpp/host_logic_check."""
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
                           os.path.join(ROOT, "tests", "cpp", "half_out_host_check.cpp"), "-o", str(out / "half_out_host_check.o")])
    objs = [str(out / (n + ".o")) for n in ("half_out_host_check", "pimemb_kernels", "pimemb_engine", "pimemb_compat", "pimemb_shard",
                                            "pimemb_peer", "hip_runtime_stub")]
    undefined = subprocess.check_output(["nm", "-u", str(out / "pimemb_kernels.o")], text=True)
    defs = ["-Wl,--defsym=%s=pimemb_stub_fatbin" % sym for sym in sorted(set(re.findall(r"__hip_fatbin_[0-9a-f]+", undefined)))]
    exe = out / "half_out_host_check"
    subprocess.check_call([clang, *san, *objs, "-o", str(exe), *defs, "-lpthread", "-ldl", "-lrt"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "half-out host logic ok" in run.stdout, run.stdout[-1000:] + run.stderr[-4000:]
    assert "pimemb:" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-4000:]
