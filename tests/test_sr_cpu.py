"""CPU: the stochastically rounded steps of the backward pass (include/pimemb_grad.h, THE STOCHASTICALLY ROUNDED STEPS).  The generator
and the encoder the kernels compile (csrc/pimemb_grad_sr.h), run on the host by tests/cpp/grad_sr_check.cpp, agree with tests/sr_ref.py
bit for bit -- Philox on its known answers, enc_sr on every fp16 / bf16 value, on every fp32 exponent at the thresholds that prove
exactly F words round up, through the fp16 subnormal range and at the edges of both formats -- and sr_ref's recipe on the bits agrees
with its definition on values; the reference holds the drift that rounding to nearest loses; and the new ABI is what the header says.
No GPU work is called."""
import ctypes as C
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_ref as gr  # noqa: E402
import sr_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pim-embedding-lookup_amd", "csrc")
F = np.float32
KINDS = ("f16", "bf16")
TOP = (1 << 32) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("sr") / "grad_sr_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "grad_sr_check.cpp"),
                           "-o", str(out)])
    return str(out)


def header_enc(exe, tmp_path, kind, bits32, R):
    """enc_sr of the header on arrays of fp32 patterns and words: uint16."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.stack([np.asarray(bits32, np.uint32), np.asarray(R, np.uint32)], axis=1).tofile(src)
    subprocess.check_call([exe, "enc", kind, str(src), str(dst)])
    return np.fromfile(dst, np.uint16)


def ref_enc(kind, bits32, R):
    return sr.enc_sr(kind, np.asarray(bits32, np.uint32).view(F), np.asarray(R, np.uint32))


def fraction(kind, bits32):
    """F of one finite fp32 pattern, from the definition on values: the number of words that round away from zero, by bisection over R
    on sr_ref.enc_sr_value (lo for R < 2^32 - F, hi from there on)."""
    lo_out = sr.enc_sr_value(kind, bits32, 0)
    if sr.enc_sr_value(kind, bits32, TOP) == lo_out:
        return 0
    a, b = 0, TOP                                         # enc(a) == lo, enc(b) == hi
    while b - a > 1:
        mid = (a + b) // 2
        if sr.enc_sr_value(kind, bits32, mid) == lo_out:
            a = mid
        else:
            b = mid
    return (1 << 32) - b


# ---- Philox -----------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers_from_the_header_and_from_the_reference(exe):
    for ctr, key, want in sr.KNOWN_ANSWERS:
        got = subprocess.check_output([exe, "philox"] + ["%x" % v for v in ctr + key], text=True).split()
        assert [int(w, 16) for w in got] == list(want), (ctr, key, got)
        ref = sr.philox4x32_10(*ctr, *key)
        assert [int(w[0]) for w in ref] == list(want), (ctr, key)


def test_the_words_of_a_row_are_the_blocks_of_its_pieces(exe, tmp_path):
    for seed, t, row, dim in ((sr.DRIFT_SEED, 0, 5, 128), (0xFFFFFFFFFFFFFFFF, (1 << 64) - 1, 96, 512), (7, (3 << 32) + 9, 0, 3), (1 << 63, 1 << 40, 0xFFFFFFFE, 130)):
        dst = tmp_path / "w.bin"
        pieces = (dim + 3) // 4
        subprocess.check_call([exe, "words", "%x" % seed, "%x" % t, str(row), str(pieces), str(dst)])
        got = np.fromfile(dst, np.uint32)
        assert np.array_equal(got[:dim], sr.words(seed, t, row, dim)), (seed, t, row, dim)
        c = pieces - 1                                    # the counter is (row, piece, t_lo, t_hi), the key (seed_lo, seed_hi)
        want = sr.philox4x32_10(row, c, t & TOP, t >> 32, seed & TOP, seed >> 32)
        assert [int(w[0]) for w in want] == [int(v) for v in got[4 * c:4 * c + 4]]
    assert not np.array_equal(sr.words(1, 0, 0, 8), sr.words(1, 1, 0, 8)) and not np.array_equal(sr.words(1, 0, 0, 8), sr.words(2, 0, 0, 8))
    assert not np.array_equal(sr.words(1, 0, 0, 8), sr.words(1, 0, 1, 8))


# ---- enc_sr -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_representable_value_is_stored_as_itself_for_every_word(exe, tmp_path, kind):
    stored = np.arange(1 << 16, dtype=np.uint16)
    wide = gr.decode(kind, stored.view(np.uint8).reshape(-1, 2)).reshape(-1).view(np.uint32)      # every value of T, widened exactly
    finite = np.isfinite(wide.view(F))
    for R in (0, 1, 1 << 31, TOP):
        words = np.full(wide.shape, R, np.uint32)
        got = header_enc(exe, tmp_path, kind, wide, words)
        assert np.array_equal(got, ref_enc(kind, wide, words)), (kind, R)
        assert np.array_equal(got[finite], stored[finite]), (kind, R)             # unchanged, -0 and the subnormals included
        assert np.array_equal(got[~finite], gr.encode(kind, wide.view(F)[None, :]).view(np.uint16)[0][~finite])      # inf / NaN: enc_T


def exponent_sweep(kind):
    """(fp32 patterns, words): every biased exponent 0 .. 254, mantissas {0, 1, the grid's half-way pattern - 1 / itself / + 1, all
    ones}, both signs, each with the words {0, 2^32 - F - 1, 2^32 - F, 2^32 - 1}; F by the definition on values."""
    half = 0x8000 if kind == "bf16" else 0x1000
    pats, words, Fs = [], [], []
    for e in range(255):
        for m in (0, 1, half - 1, half, half + 1, 0x7FFFFF):
            for sign in (0, 1):
                u = (sign << 31) | (e << 23) | m
                Fr = fraction(kind, u)
                for R in (0, TOP + 1 - Fr - 1, (TOP + 1 - Fr) & TOP, TOP):
                    pats.append(u)
                    words.append(R)
                    Fs.append(Fr)
    return np.array(pats, np.uint32), np.array(words, np.uint32), np.array(Fs, np.uint64)


@pytest.mark.parametrize("kind", KINDS)
def test_exactly_F_words_round_away_from_zero_at_every_exponent(exe, tmp_path, kind):
    pats, words, Fs = exponent_sweep(kind)
    got = header_enc(exe, tmp_path, kind, pats, words)
    want = np.array([sr.enc_sr_value(kind, int(u), int(R)) for u, R in zip(pats, words)], np.uint16)      # the definition on values
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(ref_enc(kind, pats, words), want)                       # the reference's recipe on the bits
    g = got.reshape(-1, 4).astype(np.int64)
    Fq = Fs.reshape(-1, 4)[:, 0]
    assert (g[:, 0] == g[:, 1]).all()                                             # R = 0 and the last word below the threshold: lo
    moved = Fq > 0
    assert (g[moved, 2] == g[moved, 3]).all() and (g[moved, 2] == g[moved, 0] + 1).all()      # the threshold itself and 2^32 - 1: hi, one step away from zero
    assert (g[~moved, 3] == g[~moved, 0]).all()                                   # F = 0: itself for every word
    if kind == "bf16":                                                            # F is the dropped 16 bits
        assert np.array_equal(Fq, (pats.reshape(-1, 4)[:, 0].astype(np.uint64) & np.uint64(0xFFFF)) << np.uint64(16))
    assert not ((got & 0x7FFF) > (0x7F80 if kind == "bf16" else 0x7C00)).any()    # a carry gives inf, never a NaN


def test_the_fp16_subnormal_range_at_every_shift(exe, tmp_path):
    """s = 126 - max(e, 1) = 14 .. 57 and beyond: fp32 exponents 112 down to 69 (and 1, 0).  Below s = 32 the fraction is exact; from
    there F truncates it; from s = 56 it is 0 and nothing ever rounds up."""
    pats, words = [], []
    for s in list(range(14, 58)) + [100, 125]:
        e = 126 - s
        for m in (0, 1, 0x400000, 0x400001, 0x7FFFFF, 0x2AAAAA):
            for sign in (0, 1):
                u = (sign << 31) | (e << 23) | m
                Fr = fraction("f16", u)
                full = ((m | 0x800000) % (1 << s)) if s < 24 else (m | 0x800000)
                assert Fr == ((full << 32) >> s)
                if s >= 56:
                    assert Fr == 0
                for R in (0, TOP - Fr, (TOP + 1 - Fr) & TOP, TOP, 0x9E3779B9):
                    pats.append(u)
                    words.append(R)
    for m in (1, 0x400000, 0x7FFFFF):                     # fp32 denormals: e = 0 counts as e' = 1, no implicit one
        for R in (0, TOP):
            pats.append(m)
            words.append(R)
    pats, words = np.array(pats, np.uint32), np.array(words, np.uint32)
    got = header_enc(exe, tmp_path, "f16", pats, words)
    want = np.array([sr.enc_sr_value("f16", int(u), int(R)) for u, R in zip(pats, words)], np.uint16)
    assert np.array_equal(got, want) and np.array_equal(ref_enc("f16", pats, words), want)
    assert (got & 0x7FFF).max() <= 0x400                  # a subnormal, or 2^-14 by the carry of the largest one


def test_the_edges_of_both_formats(exe, tmp_path):
    f = lambda v: int(np.array([v], F).view(np.uint32)[0])  # noqa: E731
    big_bf16 = 0x7F7F0000
    cases = {"f16": [f(65504.0), f(65504.0) + 1, f(65520.0), f(65536.0) - 1, f(65536.0), f(65536.0) + 1, f(1e9), f(2.0 ** -14), f(2.0 ** -14) - 1, f(2.0 ** -24),
                     f(2.0 ** -25), f(1.0) + 0x1FFF, f(1.0) + 0x1000],
             "bf16": [big_bf16, big_bf16 + 1, big_bf16 + 0x8000, big_bf16 + 0xFFFF, f(1.0) + 0xFFFF, f(1.0) + 1, 0x00000001, 0x0000FFFF, 0x00010000, 0x007FFFFF]}
    special = [0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F801000, 0xFF802000, 0x7F80FFFF]
    for kind in KINDS:
        pats = [u | s for u in cases[kind] for s in (0, 0x80000000)]
        both = np.array([(u, R) for u in pats + special for R in (0, 1, 0x7FFFFFFF, 0x80000000, TOP - 1, TOP)], np.uint32)
        got = header_enc(exe, tmp_path, kind, both[:, 0], both[:, 1])
        want = np.array([sr.enc_sr_value(kind, int(u), int(R)) for u, R in both], np.uint16)
        assert np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:8])
        assert np.array_equal(ref_enc(kind, both[:, 0], both[:, 1]), want)
        n_special = len(special) * 6
        nearest = gr.encode(kind, both[-n_special:, 0].copy().view(F)[None, :]).view(np.uint16)[0]
        assert np.array_equal(got[-n_special:], nearest)                          # inf / NaN: the row writer's encoder, R unused
    inf16 = header_enc(exe, tmp_path, "f16", [f(65536.0), f(65520.0), f(65520.0), 0x80000000 | f(1e9)], [0, TOP, 0, 0])
    assert list(inf16) == [0x7C00, 0x7C00, 0x7BFF, 0xFC00]
    inf_bf = header_enc(exe, tmp_path, "bf16", [big_bf16 + 1, big_bf16 + 1, 0x80000000 | (big_bf16 + 0xFFFF)], [TOP, 0, 0x10000], )
    assert list(inf_bf) == [0x7F80, 0x7F7F, 0xFF80]


@pytest.mark.parametrize("kind", KINDS)
def test_the_header_step_is_the_plain_step_but_for_the_last_rounding(exe, tmp_path, kind):
    """step_sr on random elements: the fp32 value is grad_ref's (one multiply, one subtract), the encoding sr_ref's."""
    rng = np.random.default_rng(11)
    n = 4096
    stored = gr.encode(kind, (rng.standard_normal((1, n)) * np.exp2(rng.integers(-16, 8, size=(1, n)))).astype(F)).view(np.uint16)[0]
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 4, size=n))).astype(F)
    lr = F(0.1)
    R = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    rec = np.stack([stored.astype(np.uint32), g.view(np.uint32), np.full(n, lr).astype(F).view(np.uint32), R], axis=1)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    rec.tofile(src)
    subprocess.check_call([exe, "step", kind, str(src), str(dst)])
    got = np.fromfile(dst, np.uint16)
    prod = lr * g
    x = gr.decode(kind, stored.view(np.uint8).reshape(1, -1))[0] - prod
    want = sr.enc_sr(kind, x, R)
    assert np.array_equal(got, want)
    nearest = gr.encode(kind, x[None, :]).view(np.uint16)[0]
    # a word rounds the other way than nearest-even with probability min(f, 1 - f): 1/4 on average for a fraction spread evenly, less
    # where the update is far below an ulp -- the two steps differ, and never on more than about a quarter of the elements
    assert 0.02 < np.mean(got != nearest) < 0.3


# ---- the drift: what the step is for ------------------------------------------------------------------------------------------------
def test_the_reference_holds_the_drift_that_rounding_to_nearest_loses():
    plain = sr.drift_tables(stochastic=False)
    assert all(np.array_equal(t, sr.drift_table()) for t in plain)                # every update is below half an ulp: nothing ever moves
    tables = sr.drift_tables()
    total = sr.ulps_above_one(tables[-1])
    print("ulps above 1.0 after 64 steps:", total)
    assert total == sr.DRIFT_ULPS == 8266
    assert abs(total - 8192) <= 5 * 89                    # 4096 elements x 64 steps x 2^-5 ulp; sd = sqrt(4096 * 64 * (1/32)(31/32)) = 89
    assert all(sr.ulps_above_one(a) <= sr.ulps_above_one(b) for a, b in zip(tables, tables[1:]))


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx_and_the_sr_spec_matches(pel, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pimemb_grad.h"\nint main(void){emb_sr_spec s = {1, 2, NULL, 0};\n'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(emb_sr_spec), offsetof(emb_sr_spec, seed), offsetof(emb_sr_spec, step), '
                   'offsetof(emb_sr_spec, step_dev), offsetof(emb_sr_spec, reserved), (int)(s.seed + s.step));\n'
                   'return (int)(sizeof(&emb_grad_sgd_sr) + sizeof(&emb_grad_step_sr)) == 0;}\n')
    S = pel.lib.EmbSrSpec
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        out = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(out)])
        got = [int(x) for x in subprocess.check_output([str(out)], text=True).split()]
        assert got == [C.sizeof(S), S.seed.offset, S.step.offset, S.step_dev.offset, S.reserved.offset, 3]
    assert C.sizeof(S) == 32 and (S.seed.offset, S.step.offset, S.step_dev.offset, S.reserved.offset) == (0, 8, 16, 24)


def test_declared_exported_and_bound(pel):
    build = import_module("pim-embedding-lookup_amd.build")
    header = open(os.path.join(ROOT, "include", "pimemb_grad.h")).read()
    assert "THE STOCHASTICALLY ROUNDED STEPS" in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    G = pel.lib.load_grad()
    for name in ("emb_grad_sgd_sr", "emb_grad_step_sr"):
        assert name + "(" in header and name in exported and name in pel.lib.GRAD_SIGNATURES and getattr(G, name).argtypes
    dyn = subprocess.check_output(["readelf", "-d", build.GRAD_LIB_PATH], text=True)
    assert "libpimemb_grad_sr.so" in dyn and "$ORIGIN" in dyn
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.GRAD_SR_LIB_PATH], text=True)
    assert "pimemb_grad_sr_launch" in {line.split()[-1] for line in syms.splitlines()}
    assert os.path.dirname(build.GRAD_SR_LIB_PATH) == os.path.dirname(build.GRAD_MASTER_LIB_PATH)


def test_the_steps_refuse_null_and_bad_arguments_without_a_gpu(pel):
    G = pel.lib.load_grad()
    INV = pel.lib.EMB_ERR_INVALID
    d = pel.lib.EmbGradDesc()
    ptrs = (C.c_void_p * 1)()
    srs = lambda seed=1, step=0, dev=None, reserved=0: C.byref(pel.lib.EmbSrSpec(seed, step, dev, reserved))  # noqa: E731
    opt = lambda kind=1, lr=0.1, eps=1e-10, reserved=0: C.byref(pel.lib.EmbOptSpec(kind, lr, eps, reserved))  # noqa: E731
    err = G.emb_grad_last_error
    assert G.emb_grad_sgd_sr(None, C.byref(d), 1, 0, 0.1, srs(), None) == INV and b"context is NULL" in err()
    assert G.emb_grad_step_sr(None, C.byref(d), ptrs, 1, 0, opt(), srs(), None) == INV and b"context is NULL" in err()
    # the bad-spec cases refuse before the context is looked at (it is NULL here, and that is not what the text names)
    assert G.emb_grad_sgd_sr(None, C.byref(d), 1, 0, 0.1, None, None) == INV and b"spec is NULL" in err()
    assert G.emb_grad_step_sr(None, C.byref(d), ptrs, 1, 0, opt(), None, None) == INV and b"spec is NULL" in err()
    for reserved in (1, 1 << 40):
        assert G.emb_grad_sgd_sr(None, C.byref(d), 1, 0, 0.1, srs(reserved=reserved), None) == INV and b"reserved" in err()
        assert G.emb_grad_step_sr(None, C.byref(d), ptrs, 1, 0, opt(), srs(reserved=reserved), None) == INV and b"reserved" in err()
    for dev in (4, 0x1001, 0x7F0000000002):
        assert G.emb_grad_sgd_sr(None, C.byref(d), 1, 0, 0.1, srs(dev=dev), None) == INV and b"8-byte aligned" in err()
        assert G.emb_grad_step_sr(None, C.byref(d), ptrs, 1, 0, opt(), srs(dev=dev), None) == INV and b"8-byte aligned" in err()
    assert G.emb_grad_step_sr(None, C.byref(d), ptrs, 1, 0, None, srs(), None) == INV and b"optimizer spec is NULL" in err()
    assert G.emb_grad_step_sr(None, C.byref(d), ptrs, 1, 0, opt(kind=5), srs(), None) == INV and b"unknown optimizer kind" in err()
    assert G.emb_grad_step_sr(None, C.byref(d), ptrs, 1, 0, opt(eps=-1.0), srs(), None) == INV and b"eps" in err()
    fake = C.c_void_p(16)
    assert G.emb_grad_sgd_sr(fake, None, 1, 0, 0.1, srs(), None) == INV and b"is NULL" in err()
    assert G.emb_grad_step_sr(fake, C.byref(d), None, 1, 0, opt(), srs(), None) == INV and b"is NULL" in err()
    assert G.emb_grad_sgd_sr(fake, C.byref(d), 1, 7, 0.1, srs(), None) == INV and b"index type" in err()


def test_the_sr_kernels_have_a_code_object_of_their_own_and_use_no_scratch(pel):
    codeobj = import_module("pim-embedding-lookup_amd.codeobj")
    build = import_module("pim-embedding-lookup_amd.build")
    res = codeobj.kernel_resources(build.GRAD_SR_LIB_PATH)
    assert res and all("grad_sr_" in k for k in res), sorted(res)                 # nothing but the SR kernels: no second copy of a shared one
    group = {k: v for k, v in res.items() if "grad_sr_rows_group" in k}
    elem = {k: v for k, v in res.items() if "grad_sr_rows_elem" in k}
    assert len(group) == 6 and len(elem) == 4 and len(res) == 10, sorted(res)     # three kinds (two element-wise) x two orders
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (k, v)
        assert v["vgpr"] <= 72, (k, v)                    # Philox costs the Adagrad kernels one wave of occupancy at the most (7 of 8 per SIMD)
    for path in (build.GRAD_LIB_PATH, build.GRAD_MASTER_LIB_PATH, build.LIB_PATH, build.ROWS_LIB_PATH):
        assert not [k for k in codeobj.kernel_resources(path) if "grad_sr_" in k], path


# ---- the harness, the modules, the probe ------------------------------------------------------------------------------------------
def test_harness_stochastic_rounding_flag_goes_with_a_fused_step_on_half_precision_tables():
    h = import_module("pim-embedding-lookup_amd.dlrm_harness")
    for extra, text in (([], "--stochastic-rounding goes with one of"),
                        (["--fused-sgd", "0.1", "--table-dtype", "bf16", "--master-weights"], "alternatives"),
                        (["--fused-sgd", "0.1", "--table-dtype", "f16", "--multi-table-step"], "no stochastically rounded multi-table step"),
                        (["--fused-adagrad", "0.1"], "nothing to round"),
                        (["--fused-adagrad", "0.1", "--table-dtype", "mxfp4"], "trains with --master-weights only")):
        with pytest.raises(SystemExit) as ei:
            h.main(["--arch-embedding-size=10-10", "--stochastic-rounding"] + extra)
        assert text in str(ei.value), (extra, str(ei.value))
    import inspect
    for name in ("enable_fused_sgd", "enable_fused_adagrad"):
        p = inspect.signature(getattr(h.EmbeddingBagCollection, name)).parameters
        assert p["stochastic_rounding"].default is False and p["sr_seed"].default == 0


def test_modules_keep_stochastic_rounding_off_by_default():
    import inspect
    tm = import_module("pim-embedding-lookup_amd.torch_module")
    for cls in (tm.PoolingEmbeddingBag, tm.FusedPoolingEmbeddingBags):
        for name in ("enable_fused_sgd", "enable_fused_adagrad", "sgd_step_", "adagrad_step_"):
            p = inspect.signature(getattr(cls, name)).parameters
            assert p["stochastic_rounding"].default is False and p["sr_seed"].default == 0, (cls, name)
        assert isinstance(cls.sr_step, property)


def test_sr_probe_lists_its_measurements_and_refuses_unknown_ones():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sr_probe", os.path.join(ROOT, "tools", "sr_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    assert set(probe.STEPS) == {f"{s}-{k}" for s in ("uniform", "zipf", "kaggle") for k in ("bf16", "f16")}
    assert probe.SHAPES["uniform"] == (4 << 20, 128, 32, 2048) and probe.SHAPES["kaggle"] == (10131227, 16, 1, 39292) and probe.SEGMENT == 64
    with pytest.raises(SystemExit) as ei:
        probe.main(["--steps", "uniform-f32"])
    assert "unknown step" in str(ei.value)
    assert probe.median_spread([3.0, 1.0, 2.0])["median_us"] == 2.0


# ---- Python -----------------------------------------------------------------------------------------------------------------------
def test_python_surface():
    import inspect
    eng = import_module("pim-embedding-lookup_amd.engine")
    for name in ("sgd_step", "adagrad_step"):
        assert inspect.signature(getattr(eng.GradContext, name)).parameters["sr"].default is None
    with pytest.raises(ValueError, match="multi=True"):
        eng.GradContext._sr_spec((1, 2), True)
    with pytest.raises(ValueError, match="seed, step"):
        eng.GradContext._sr_spec((1,), False)
    spec = eng.GradContext._sr_spec((-1, (1 << 64) + 5), False)
    assert (spec.seed, spec.step, spec.step_dev, spec.reserved) == ((1 << 64) - 1, 5, None, 0)
    assert eng.GradContext._sr_spec(None, True) is None
