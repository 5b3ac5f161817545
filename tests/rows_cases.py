"""Sources and references of the row-writer tests (tests/test_rows_cpu.py, tests/test_gpu_rows.py): fp32 rows made of randoms
plus a fixed block of edge values per target dtype, the host encoders of formats.py as the reference for the stored bytes, and
an explicit sequential loop for what a table holds after an update.  Nothing here runs the code under test."""
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
formats = import_module("pim-embedding-lookup_amd.formats")

NR_ROWS = 3001          # as the kernel census: no multiple of any tile
N_UPDATE = 1037         # more than one workgroup, no multiple of a tile

# kind -> (EMB_* dtype value, bytes per element; MXFP4: 0)
KINDS = {"f32": (0, 4), "f16": (1, 2), "bf16": (3, 2), "e4m3": (8, 1), "e5m2": (9, 1), "mxfp4": (10, 0)}
# the issue's dims: the smallest and the awkward lane-group widths per dtype, then the any-dim ones
GROUP_DIMS = {"mxfp4": (32, 96, 128), "e4m3": (16, 48, 1024), "e5m2": (16, 48, 1024), "f16": (8, 24, 512), "bf16": (8, 24, 512),
              "f32": (4, 12, 256)}
ANYDIM = (("f32", 5), ("bf16", 17), ("e4m3", 7), ("e5m2", 1028))
# (exponent bits, mantissa bits, bias, largest finite) of the rounded formats
_FMT = {"f16": (5, 10, 15, 65504.0), "bf16": (8, 7, 127, float(np.uint32(0x7F7F0000).view(np.float32))), "e4m3": (4, 3, 7, 448.0),
        "e5m2": (5, 2, 15, 57344.0)}


def row_stride(kind, dim):
    return formats.mxfp4_row_stride(dim) if kind == "mxfp4" else dim * KINDS[kind][1]


def host_encode(kind, w):
    """float32 [n, dim] -> uint8 [n, row stride]: the bytes formats.py's host encoders give, the reference of every comparison."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    if kind == "f32":
        out = w
    elif kind == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            out = w.astype(np.float16)
    elif kind == "bf16":
        out = formats.to_bf16_bits(w)
    elif kind in ("e4m3", "e5m2"):
        out = formats.to_f8_bits(w, kind)
    else:
        return formats.to_mxfp4(w)
    return np.ascontiguousarray(out).view(np.uint8).reshape(w.shape[0], -1)


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def edge_values(kind):
    """The fixed block of edge values of a rounded format, fp32, both signs: zeros, fp32 denormals, exact rounding ties of the
    target (normal and subnormal range, and at the step into the normal range), values just below and above its largest finite
    value and the rounding threshold beyond it, infinities and NaNs with payloads (quiet, signalling, payload only in the bits the
    target drops, payload at the first bit it keeps)."""
    v = [_bits(0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00800000),
         _bits(0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFC12345, 0x7F801000,
               0x7F802000, 0x7F810000, 0xFF80FFFF, 0x7FBFFFFF, 0x7F7FFFFF, 0xFF7FFFFF)]
    if kind != "f32":
        eb, mb, bias, maxf = _FMT[kind]
        ties = []
        for e in (0, 1, -3, 5, 1 - bias, 2 - bias):                       # normal range, down to the smallest normal exponent
            for k in (0, 1, 2, 3, (1 << mb) - 1):                         # mantissa k, exactly half way to k + 1 (the last: a carry into the exponent)
                ties.append((1.0 + (2 * k + 1) * 2.0 ** -(mb + 1)) * 2.0 ** e)
        q = 2.0 ** (1 - bias - mb)                                        # the subnormal quantum
        for k in (0, 1, 2, 3, (1 << mb) - 1):
            ties += [(k + 0.5) * q, np.nextafter(np.float32((k + 0.5) * q), np.float32(0)), np.nextafter(np.float32((k + 0.5) * q), np.float32(1))]
        ties += [q, q / 2, q / 4, 2.0 ** (1 - bias)]
        half_ulp = 2.0 ** (int(np.floor(np.log2(maxf))) - mb - 1)
        thr = np.float32(maxf + half_ulp)                                 # the tie between the largest finite value and overflow
        top = [maxf, np.nextafter(np.float32(maxf), np.float32(0)), np.nextafter(np.float32(maxf), np.float32(np.inf)), thr,
               np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(np.inf)), min(2 * maxf, 3.0e38), maxf / 2]
        both = np.array(ties + top, dtype=np.float64).astype(np.float32)
        v += [both, -both]
    return np.concatenate(v).astype(np.float32)


def mx_edge_blocks():
    """Edge BLOCKS of 32 fp32 values for MXFP4 (finite only): all zero (with -0), all tiny (fp32 denormals: the block quantises to
    zeros and keeps its signs), amax an exact power of two and one ulp below it with the other elements on every rounding tie,
    saturation, fp32 denormal elements under small scales (scale bytes 5 and the lower clamp 0), the largest fp32."""
    def block(vals):
        b = np.zeros(32, dtype=np.float64)
        b[:len(vals)] = vals
        b[16:16 + len(vals)] = -np.asarray(vals, dtype=np.float64)
        return b.astype(np.float32)
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5]
    near = [float(np.nextafter(np.float32(t), np.float32(0))) for t in ties] + [float(np.nextafter(np.float32(t), np.float32(9))) for t in ties]
    zero = np.zeros(32, np.float32)
    zero[1::2] = -0.0
    tiny = _bits(*range(1, 33)).copy()
    tiny[::3] *= -1
    out = [zero, tiny,
           block([4.0] + ties), block([4.0] + near), block([float(np.nextafter(np.float32(4.0), np.float32(0)))] + ties),
           block([float(np.nextafter(np.float32(4.0), np.float32(0)))] + [t / 2 for t in ties] + [t / 2 for t in near[:6]]),
           block([6.0, 5.0, float(np.nextafter(np.float32(5.0), np.float32(0))), float(np.nextafter(np.float32(5.0), np.float32(9)))]),
           block([7.9, 7.0, 6.5, 6.0, 5.0]),
           block([2.0 ** -120] + [t * 2.0 ** -122 for t in ties] + [2.0 ** -127, 2.0 ** -130, 2.0 ** -149]),
           block([2.0 ** -126] + [t * 2.0 ** -127 for t in ties] + [2.0 ** -149, 3 * 2.0 ** -149]),
           block([2.0 ** -125] + [t * 2.0 ** -127 for t in ties]), block([2.0 ** -127, 2.0 ** -128, 2.0 ** -129, 3 * 2.0 ** -129]),
           block([float(_bits(0x7F7FFFFF)[0]), 2.0 ** 127, 2.0 ** 126 * 1.25, 1.0, 2.0 ** -149]),
           block([2.0 ** 10 * t for t in [4.0] + ties])]
    return np.stack(out)


def source(kind, n, dim, seed):
    """fp32 [n, dim]: randoms over many magnitudes, the edge values of the target format laid over the first rows."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-12, 12, size=(n, 1)))).astype(np.float32)
    if kind == "mxfp4":
        w[n // 2:] = (rng.standard_normal((n - n // 2, dim)) * np.exp2(rng.integers(-140, 120, size=(n - n // 2, 1)).astype(np.float64))).astype(np.float32)
        w = np.where(np.isfinite(w), w, np.float32(1.0)).astype(np.float32)
        eb = mx_edge_blocks()
        nblk = dim // 32
        for i, b in enumerate(eb):                 # edge block i in every block position once, the row's other blocks stay random
            w[i, (i % nblk) * 32:(i % nblk) * 32 + 32] = b
            w[len(eb) + i] = np.tile(b, nblk)      # and a row made of it alone
        return w
    ev = edge_values(kind)
    flat = w.reshape(-1)
    m = min(len(ev), flat.size // 2)
    flat[:m] = ev[:m]                              # (dims too small to hold them all in half the rows keep the head of the list)
    return w


def sequential_update(table_bytes, ids, enc_rows, bad_rows=()):
    """What the table holds after `for p: W[ids[p]] = rows[p]`, skipping ids outside the table and the positions in bad_rows:
    (new table bytes, number of rows skipped).  An explicit loop: the order of repeats is the point."""
    out = table_bytes.copy()
    n = out.shape[0]
    skipped = 0
    for p, i in enumerate(ids):
        i = int(i)
        if i < 0 or i >= n or p in bad_rows:
            skipped += 1
            continue
        out[i] = enc_rows[p]
    return out, skipped
