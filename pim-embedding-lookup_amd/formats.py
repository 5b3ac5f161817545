"""On-disk formats either side of the hot path.

The reference's CLI names them (`--processed-data-file=…kaggleAdDisplayChallenge_processed.npz`,
`--load-model=…`, README.md:6,10; upmem/run.sh:117-118; data/model dirs in .gitignore:149,152) but
ships neither files nor readers (they live in the empty `PIM-dlrm-new` submodule).  Formats below
follow upstream facebookresearch/dlrm [EXT, not verifiable from the checkout]:

  * processed Criteo-Kaggle `.npz`: arrays `X_int` [N,13], `X_cat` [N,26] (already re-indexed to
    0..count-1 per feature), `y` [N], `counts` [26] (cardinality per categorical feature);
  * DLRM checkpoint `.pt`: a dict with `state_dict` (or the state dict itself) holding
    `emb_l.<k>.weight` [N_k, D] per table.

Only what the embedding path needs is read: indices/offsets per table, table shapes, weights."""
from __future__ import annotations

import numpy as np


def to_bf16_bits(x) -> np.ndarray:
    """float32 array -> the uint16 bits of its bfloat16 rounding (nearest, ties to even -- what
    `tensor.to(torch.bfloat16)` gives); NaN stays NaN (quiet bit set, sign and upper payload kept).  numpy has no bfloat16:
    EmbeddingEngine.load_table takes such an array with dtype=EMB_BF16."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    rounded = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)   # (wraps only for NaNs)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), rounded).astype(np.uint16)


def from_bf16_bits(bits) -> np.ndarray:
    """uint16 bfloat16 bits -> float32, exact for every pattern (a bf16 is the upper half of an fp32)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


_F8_KINDS = {"e4m3": (4, 3, 7), "e4m3fn": (4, 3, 7), "e5m2": (5, 2, 15)}      # exponent bits, mantissa bits, bias


def _f8_kind(kind):
    """"e4m3" / "e4m3fn" / "e5m2", or the dtype value EMB_F8_E4M3 (8) / EMB_F8_E5M2 (9) -> (name, ebits, mbits, bias)."""
    name = {8: "e4m3", 9: "e5m2"}.get(kind, kind) if not isinstance(kind, str) else kind
    name = str(name).replace("torch.", "").replace("float8_", "").replace("fp8_", "")
    if name not in _F8_KINDS:
        raise ValueError(f"fp8 kind must be 'e4m3' or 'e5m2' (or EMB_F8_E4M3 / EMB_F8_E5M2), got {kind!r}")
    return ("e5m2" if name == "e5m2" else "e4m3",) + _F8_KINDS[name]


def from_f8_bits(bits, kind) -> np.ndarray:
    """uint8 OCP fp8 bits (kind "e4m3": e4m3fn, no infinities, 0x7f / 0xff NaN; "e5m2": IEEE-like) -> float32, exact for all
    256 patterns: integer work on the bits, as `tensor.view(torch.float8_*).float()` gives."""
    name, ebits, mbits, bias = _f8_kind(kind)
    b = np.ascontiguousarray(bits, dtype=np.uint8).astype(np.uint32)
    sign = (b & np.uint32(0x80)) << np.uint32(24)
    e = (b >> np.uint32(mbits)) & np.uint32((1 << ebits) - 1)
    m = b & np.uint32((1 << mbits) - 1)
    normal = sign | ((e + np.uint32(127 - bias)) << np.uint32(23)) | (m << np.uint32(23 - mbits))
    # subnormal: m * 2^(1 - bias - mbits), exact in fp32 arithmetic (m < 8)
    sub = (m.astype(np.float32) * np.float32(2.0 ** (1 - bias - mbits))).view(np.uint32) | sign
    out = np.where(e == 0, sub, normal)
    if name == "e5m2":
        top = e == np.uint32(31)
        out = np.where(top, sign | np.uint32(0x7F800000) | (m << np.uint32(21)), out)          # inf, NaN (payload kept)
    else:
        out = np.where((b & np.uint32(0x7F)) == np.uint32(0x7F), sign | np.uint32(0x7FC00000), out)
    return out.astype(np.uint32).view(np.float32)


def to_f8_bits(x, kind) -> np.ndarray:
    """float32 array -> the uint8 bits of its OCP fp8 rounding (nearest, ties to even), as `tensor.to(torch.float8_e4m3fn)` /
    `.to(torch.float8_e5m2)` give them, overflow included: e4m3fn has no infinity, so whatever rounds beyond its largest finite
    value (448) -- infinities too -- becomes NaN (0x7f | sign); e5m2 rounds beyond 57344 to +-inf (0x7c | sign).  NaN stays NaN.
    numpy has no fp8: EmbeddingEngine.load_table takes such an array with dtype=EMB_F8_E4M3 / EMB_F8_E5M2."""
    name, ebits, mbits, bias = _f8_kind(kind)
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    sign = ((u >> np.uint32(24)) & np.uint32(0x80)).astype(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    shift = 23 - mbits
    min_normal = np.uint32((127 - bias + 1) << 23)                                   # smallest normal fp8 as fp32 bits
    # normal range: re-bias, round the dropped `shift` bits to nearest even (a carry runs into the exponent, as it should)
    v = a.astype(np.int64) - ((127 - bias) << 23)
    v = (v + ((1 << (shift - 1)) - 1) + ((v >> shift) & 1)) >> shift
    # subnormal range: adding 2^(1 - bias - mbits + 23) in fp32 leaves the rounded multiple of the fp8 quantum in the low bits
    magic = np.float32(2.0 ** (1 - bias - mbits + 23))
    with np.errstate(invalid="ignore", over="ignore"):
        subn = ((a.view(np.float32) + magic).view(np.uint32) - magic.view(np.uint32)).astype(np.int64)
    r = np.where(a < min_normal, subn, v)
    if name == "e5m2":
        r = np.where(r >= 0x7C, 0x7C, r)                                             # beyond 57344 (or inf): inf
        r = np.where(a > np.uint32(0x7F800000), 0x7F, r)                             # NaN
    else:
        r = np.where(r >= 0x7F, 0x7F, r)                                             # beyond 448, inf, NaN: NaN
        r = np.where(a >= np.uint32(0x7F800000), 0x7F, r)
    return (r.astype(np.uint32) | sign).astype(np.uint8)


# ---- MXFP4 (OCP Microscaling v1.0): blocks of 32 E2M1 elements under one E8M0 scale; EMB_MXFP4 tables ------------------------
# A fused row, as pimemb.h lays it out: dim/2 element bytes (element 2j in the low nibble of byte j), dim/32 scale bytes, zero
# padding up to a multiple of 16.
_E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float64)
_E2M1_MIDS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=np.float64)      # between code k and code k + 1


def mxfp4_row_bytes(dim: int) -> int:
    return dim // 2 + dim // 32


def mxfp4_row_stride(dim: int) -> int:
    """Bytes from one fused row to the next (EMB_MXFP4_ROW_STRIDE): 32 / 48 / 80 / 144 / 272 / 1088 at dim 32 / 64 / 128 / 256 / 512 / 2048."""
    return (mxfp4_row_bytes(dim) + 15) & ~15


def mxfp4_dim_of_stride(stride: int) -> int:
    """The dim whose fused rows are `stride` bytes wide (17 bytes per block, rounded up to 16: no two dims share a stride)."""
    blocks = stride // 17
    if blocks < 1 or mxfp4_row_stride(32 * blocks) != stride:
        raise ValueError(f"{stride} bytes is not the row stride of any MXFP4 dim (EMB_MXFP4_ROW_STRIDE)")
    return 32 * blocks


def _mxfp4_check_dim(dim: int) -> None:
    if dim <= 0 or dim % 32:
        raise ValueError(f"MXFP4 rows are blocks of 32 elements: dim {dim} is no positive multiple of 32")


def mxfp4_split(rows, dim: int):
    """Fused rows uint8 [rows, stride] -> (elements uint8 [rows, dim/2], scales uint8 [rows, dim/32]), copies."""
    _mxfp4_check_dim(dim)
    r = np.asarray(rows, dtype=np.uint8)
    if r.ndim != 2 or r.shape[1] < mxfp4_row_bytes(dim):
        raise ValueError(f"fused MXFP4 rows of dim {dim} are [rows, >= {mxfp4_row_bytes(dim)}] uint8, got {r.shape}")
    return r[:, :dim // 2].copy(), r[:, dim // 2:mxfp4_row_bytes(dim)].copy()


def mxfp4_join(elements, scales) -> np.ndarray:
    """(elements uint8 [rows, dim/2], scales uint8 [rows, dim/32]) -> fused rows uint8 [rows, stride], zero padded."""
    el, sc = np.asarray(elements, dtype=np.uint8), np.asarray(scales, dtype=np.uint8)
    if el.ndim != 2 or sc.ndim != 2 or el.shape[0] != sc.shape[0] or el.shape[1] != 16 * sc.shape[1] or sc.shape[1] == 0:
        raise ValueError(f"MXFP4 pair: elements [rows, dim/2] and scales [rows, dim/32], got {el.shape} and {sc.shape}")
    dim = 2 * el.shape[1]
    out = np.zeros((el.shape[0], mxfp4_row_stride(dim)), dtype=np.uint8)
    out[:, :dim // 2] = el
    out[:, dim // 2:mxfp4_row_bytes(dim)] = sc
    return out


def from_mxfp4(rows_u8, dim: int) -> np.ndarray:
    """Fused MXFP4 rows -> float32 [rows, dim]: e2m1 * 2^(s - 127) as fp32 arithmetic gives it -- exact, fp32 denormals included,
    but for the few products beyond the largest fp32 (scale bytes 253 / 254 under the largest magnitudes), which are +-inf; a block
    whose scale byte is 0xFF is NaN."""
    el, sc = mxfp4_split(rows_u8, dim)
    nib = np.empty((el.shape[0], dim), dtype=np.uint8)
    nib[:, 0::2] = el & 0xF
    nib[:, 1::2] = el >> 4
    val = np.where(nib & 8, -1.0, 1.0) * _E2M1[nib & 7]                         # (-0.0 for nibble 0x8)
    s = np.repeat(sc.astype(np.int32), 32, axis=1)
    with np.errstate(over="ignore"):
        out = np.ldexp(val, s - 127).astype(np.float32)                         # float64 product of two exact values: exact
    out[s == 255] = np.nan
    return out


def to_mxfp4(x_f32) -> np.ndarray:
    """[rows, dim] real array (dim a multiple of 32) -> fused MXFP4 rows uint8 [rows, stride], by the OCP MX v1.0 rule: per block
    X = 2^(floor(log2(max|v|)) - 2), its scale byte clamped to [0, 254]; elements v / X rounded to nearest, ties to the even
    code, saturating at +-6.  A block that quantises to all zeros (an all-zero block; a block too small for scale byte 0) gets
    scale byte 127 and keeps its signs, so the function is idempotent on its own output.  Non-finite input raises ValueError.
    (Wider than fp32 on purpose: a float64 array can reach the upper clamp, which no finite fp32 does.)"""
    x = np.asarray(x_f32, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("to_mxfp4 takes a 2-D [rows, dim] array")
    _mxfp4_check_dim(x.shape[1])
    if not np.isfinite(x).all():
        raise ValueError("to_mxfp4: non-finite input (MXFP4 elements have no inf and no NaN)")
    rows, dim = x.shape
    blk = x.reshape(rows, dim // 32, 32)
    amax = np.abs(blk).max(axis=2)
    _, ex = np.frexp(amax)                                                      # amax = m * 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    s = np.clip(ex.astype(np.int64) - 1 - 2 + 127, 0, 254)
    a = np.abs(np.ldexp(blk, (127 - s)[:, :, None]))                            # |v / X|, exact in float64
    code = np.zeros(a.shape, dtype=np.uint8)
    for k, mid in enumerate(_E2M1_MIDS):                                        # a tie goes to the even one of codes k, k + 1
        code += (a >= mid) if k % 2 else (a > mid)
    s = np.where((code == 0).all(axis=2), 127, s)
    nib = (code | (np.signbit(blk).astype(np.uint8) << 3)).reshape(rows, dim)
    return mxfp4_join(nib[:, 0::2] | (nib[:, 1::2] << 4), s.astype(np.uint8))


class CriteoKaggleNpz:
    """Categorical side of a processed Criteo-Kaggle file as embedding-lookup batches."""

    def __init__(self, path: str, mmap: bool = True):
        z = np.load(path, mmap_mode="r" if mmap else None)
        if "X_cat" not in z or "counts" not in z:
            raise ValueError(f"{path}: expected arrays X_cat and counts (processed DLRM npz)")
        self.x_cat = z["X_cat"]
        self.counts = [int(c) for c in z["counts"]]
        if self.x_cat.ndim != 2 or self.x_cat.shape[1] != len(self.counts):
            raise ValueError("X_cat must be [N, len(counts)]")
        self.n_samples = int(self.x_cat.shape[0])

    @property
    def table_rows(self) -> list[int]:
        """`--arch-embedding-size` as DLRM derives it from `counts`."""
        return list(self.counts)

    def batch(self, start: int, size: int, index_dtype=np.int64):
        """(lS_o, lS_i) for samples [start, start+size): one index per bag (Criteo is one-hot), so
        lS_o[k] = arange(B) and lS_i[k] = X_cat[start:start+B, k] -- the layout
        `dlrm_s_pytorch.py::apply_emb` consumes [EXT]."""
        stop = min(start + size, self.n_samples)
        x = np.asarray(self.x_cat[start:stop])
        if x.size and (x.min() < 0 or (x.max(axis=0) >= np.asarray(self.counts)).any()):
            raise ValueError("X_cat holds an index outside [0, counts[k])")
        B = stop - start
        off = np.arange(B, dtype=index_dtype)
        return [off] * x.shape[1], [np.ascontiguousarray(x[:, k]).astype(index_dtype) for k in range(x.shape[1])]

    def batches(self, batch_size: int, index_dtype=np.int64):
        for s in range(0, self.n_samples, batch_size):
            yield self.batch(s, batch_size, index_dtype)


def load_dlrm_embedding_weights(path: str):
    """Embedding tables of a DLRM checkpoint: list of float32 [N_k, D] numpy arrays in table order."""
    import torch
    obj = torch.load(path, map_location="cpu", weights_only=True)
    sd = obj.get("state_dict", obj) if isinstance(obj, dict) else obj
    keys = sorted((k for k in sd if k.startswith("emb_l.") and k.endswith(".weight")),
                  key=lambda k: int(k.split(".")[1]))
    if not keys:
        raise ValueError(f"{path}: no emb_l.<k>.weight entries")
    if [int(k.split(".")[1]) for k in keys] != list(range(len(keys))):
        raise ValueError("emb_l indices are not 0..T-1")
    return [sd[k].detach().to(torch.float32).contiguous().numpy() for k in keys]


def load_dlrm_pooling_weights(path: str, n_tables: int):
    """The per-row pooling weights of a DLRM checkpoint trained with --weighted-pooling learned: `v_W_l.<k>` (DLRM's
    ParameterList v_W_l, one float32 [N_k] vector per table) as numpy arrays in table order."""
    import torch
    obj = torch.load(path, map_location="cpu", weights_only=True)
    sd = obj.get("state_dict", obj) if isinstance(obj, dict) else obj
    missing = [k for k in range(n_tables) if f"v_W_l.{k}" not in sd]
    if missing:
        raise ValueError(f"{path}: no v_W_l.<k> entry for table(s) {missing} (was the model trained with --weighted-pooling learned?)")
    return [sd[f"v_W_l.{k}"].detach().to(torch.float32).reshape(-1).contiguous().numpy() for k in range(n_tables)]


def save_dlrm_embedding_weights(path: str, tables, pooling_weights=None) -> None:
    """Write tables back in the same layout (tests, round trips)."""
    import torch
    sd = {f"emb_l.{k}.weight": torch.as_tensor(np.asarray(t)) for k, t in enumerate(tables)}
    for k, v in enumerate(pooling_weights or []):
        sd[f"v_W_l.{k}"] = torch.as_tensor(np.asarray(v, dtype=np.float32))
    torch.save({"state_dict": sd}, path)
