"""CPU: the bfloat16 table dtype (EMB_BF16) as far as it can be checked without a GPU -- the enum value in the header and
the binding, the two numpy bit helpers of formats.py against torch, and the code object of the cross-compiled library: a
bf16 instantiation next to every fp16 one, none of them spilling."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pimemb.h")


@pytest.fixture(scope="module")
def formats():
    from importlib import import_module
    return import_module("pim-embedding-lookup_amd.formats")


def test_enum_value_in_header_and_binding(pel):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)       # strip comments
    body = re.search(r"typedef\s+enum\s+emb_dtype\s*\{(.*?)\}\s*emb_dtype\s*;", text, flags=re.S).group(1)
    enum = {k: int(v) for k, v in re.findall(r"\b(EMB_\w+)\s*=\s*(\d+)", body)}
    assert enum == {"EMB_F32": 0, "EMB_F16": 1, "EMB_FIXED32": 2, "EMB_BF16": 3}
    assert pel.lib.EMB_BF16 == 3 and pel.EMB_BF16 == 3 and "EMB_BF16" in pel.__all__
    assert (pel.lib.EMB_F32, pel.lib.EMB_F16, pel.lib.EMB_FIXED32) == (0, 1, 2)


def test_from_bf16_bits_every_pattern(formats):
    bits = np.arange(65536, dtype=np.uint16)
    got = formats.from_bf16_bits(bits)
    want = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert got.dtype == np.float32 and got.shape == bits.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))       # bit for bit: NaN payloads, signed zeros, denormals
    assert np.array_equal(got.view(np.uint32), bits.astype(np.uint32) << 16)
    assert formats.from_bf16_bits(bits.reshape(256, 256)).shape == (256, 256)


def _rounding_inputs():
    rng = np.random.default_rng(16)
    parts = [rng.integers(0, 1 << 32, size=1_200_000, dtype=np.uint64).astype(np.uint32)]     # random fp32 bit patterns
    hi = rng.integers(0, 1 << 16, size=70_000, dtype=np.uint64).astype(np.uint32) << 16
    hi = np.concatenate([hi, np.arange(65536, dtype=np.uint32) << 16])
    for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):          # exact ties (0x8000) over even and odd upper halves, and their neighbours
        parts.append(hi | np.uint32(low))
    den = rng.integers(1, 1 << 23, size=100_000, dtype=np.uint64).astype(np.uint32)            # fp32 denormals, both signs
    parts += [den, den | np.uint32(0x80000000), np.array([1, 0x7FFF, 0x8000, 0x8001, 0x007FFFFF, 0x00800000], np.uint32)]
    top = np.array([0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0x7F7F0000], np.uint32)  # around the largest bf16: up to inf
    parts += [top, top | np.uint32(0x80000000)]
    parts.append(np.array([0x7F800000, 0xFF800000, 0, 0x80000000], np.uint32))                 # +-inf, +-0
    parts.append(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F80FFFF, 0x7FBF0000], np.uint32))  # NaNs
    return np.concatenate(parts)


def test_to_bf16_bits_rounds_like_torch(formats):
    u = _rounding_inputs()
    x = u.view(np.float32)
    assert len(x) >= 1_000_000
    got = formats.to_bf16_bits(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert got.dtype == np.uint16 and got.shape == x.shape
    nan = np.isnan(x)
    assert nan.sum() > 1000 and (~nan).sum() > 1_000_000
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(formats.from_bf16_bits(got[nan])).all()                 # NaN stays NaN (never rounds into inf)
    # what the cases above are there for
    assert formats.to_bf16_bits(np.array([0x3F808000, 0x3F818000], np.uint32).view(np.float32)).tolist() == [0x3F80, 0x3F82]   # ties to even
    assert formats.to_bf16_bits(np.array([0x7F7F8000], np.uint32).view(np.float32)).tolist() == [0x7F80]                      # up to +inf
    assert formats.to_bf16_bits(np.float32([np.inf, -np.inf, 0.0, -0.0])).tolist() == [0x7F80, 0xFF80, 0x0000, 0x8000]
    # a round trip of bf16 values is the identity
    b = np.arange(65536, dtype=np.uint16)
    f = formats.from_bf16_bits(b)
    keep = ~np.isnan(f)
    assert np.array_equal(formats.to_bf16_bits(f)[keep], b[keep])
    assert formats.to_bf16_bits(np.zeros((3, 5), np.float32)).shape == (3, 5)


def _dtype_kernels(names, dt):
    """{(kernel, index type, the template arguments after DT): mangled name} of the bag kernels instantiated for table dtype
    `dt`: their template heads are <IdxT, DT, ...> (j = uint32, l = int64).  The pooled kernels of bf16 tables are the
    bag_pool_* kernels under the name bag_bf16pool_* (pimemb_bag_kernels.h): the same kernel here."""
    pat = re.compile(r"^_ZN6pimemb\d+(bag_(?:sum|pool|bf16pool)_\w+?_kernel)I([jl])Li%dE(.*)$" % dt)
    out = {}
    for n in names:
        m = pat.match(n)
        if m:
            out[(m.group(1).replace("bag_bf16pool_", "bag_pool_"), m.group(2), m.group(3))] = n
    return out


def test_every_fp16_kernel_has_a_bf16_twin_without_spills(pel):
    from pim_embedding_lookup_amd import codeobj
    hashes = codeobj.kernel_hashes(pel.LIB_PATH)
    res = codeobj.kernel_resources(pel.LIB_PATH)
    f16, bf16 = _dtype_kernels(hashes, 1), _dtype_kernels(hashes, 3)
    assert len(f16) >= 100, len(f16)                                        # every family: wave-batch (+ ranged, two-batch), group, hot, any-dim, pooled
    assert set(f16) == set(bf16), (sorted(set(f16) - set(bf16))[:4], sorted(set(bf16) - set(f16))[:4])      # otherwise equal template arguments
    assert len(set(f16.values())) == len(f16) and len(set(bf16.values())) == len(bf16)
    for family in ("bag_sum_wavebatch_kernel", "bag_sum_group_kernel", "bag_sum_hot_kernel", "bag_sum_anydim_kernel",
                   "bag_sum_anydim_vec_kernel", "bag_pool_wavebatch_kernel", "bag_pool_group_kernel", "bag_pool_anydim_kernel"):
        assert any(k[0] == family for k in bf16), family
    for n in sorted(bf16.values()):
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch"] == 0, (n, res[n])
    sym, _sha = codeobj.kernel_of_launch(pel.LIB_PATH, dict(kind=0, dtype=3, itype=0, lanes_per_row=2, ranged=0))
    assert sym in bf16.values()
    # ... and every launch an fp16 plan can describe resolves for bf16 too
    for itype in (0, 1):
        for lpr in (1, 2, 4, 8, 16, 32, 64):
            for kind in (0, 1, 2, 4):
                if kind == 2 and lpr > 4:
                    continue
                for ranged in ((0, 1) if kind in (0, 2) else (0,)):
                    codeobj.kernel_of_launch(pel.LIB_PATH, dict(kind=kind, dtype=3, itype=itype, lanes_per_row=lpr, ranged=ranged))
            for kind in (0, 1):
                codeobj.kernel_of_launch(pel.LIB_PATH, dict(kind=kind, dtype=3, itype=itype, lanes_per_row=lpr, pool=1))
        for vec in (0, 1):
            codeobj.kernel_of_launch(pel.LIB_PATH, dict(kind=3, dtype=3, itype=itype, lanes_per_row=0, anydim_vec=vec, ranged=0))
            codeobj.kernel_of_launch(pel.LIB_PATH, dict(kind=3, dtype=3, itype=itype, lanes_per_row=0, anydim_vec=vec, pool=1))


def test_load_table_takes_uint16_only_as_declared_bf16(pel):
    """numpy has no bfloat16: a uint16 array is refused unless dtype=EMB_BF16 says what its bits are (decided before the
    engine is touched, so no GPU is needed to see the refusal)."""
    eng = pel.EmbeddingEngine.__new__(pel.EmbeddingEngine)                  # (no emb_create: load_table must refuse before any C call)
    with pytest.raises(KeyError):
        eng.load_table(0, np.zeros((4, 8), np.uint16))
