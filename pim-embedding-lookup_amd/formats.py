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
