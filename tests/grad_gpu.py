"""What the GPU tests of the backward pass share (tests/test_gpu_grad.py, test_gpu_optim.py, test_gpu_grad_multi.py,
test_gpu_grad_order.py): arrays to the device, tables in and out as bytes.  A plain module like tests/grad_cases.py; the engine
and context fixtures stay in the test files, their contexts differ in size.  Nothing here runs the code under test."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_cases as rc  # noqa: E402

DEV = "cuda:0"
F = np.float32
CODE = {"f32": 0, "f16": 1, "bf16": 3, "e4m3": 8, "e5m2": 9, "mxfp4": 10}      # kind -> emb_dtype


def to_dev(a):
    """numpy -> CUDA tensor (uint32 bits travel as int32)."""
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)      # (the shared case arrays are read-only: torch wants its own)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def load_bytes(eng, t, kind, raw):
    view = {"f32": np.float32, "f16": np.uint16, "bf16": np.uint16}.get(kind, np.uint8)
    eng.load_table(t, np.ascontiguousarray(raw).view(view), dtype=CODE[kind])


def table_bytes(eng, t):
    """The whole table as it lies in HBM, through emb_copy_to_host."""
    ptr, n, dim, dt = eng.table_info(t)
    kind = {v: k for k, v in CODE.items()}.get(dt, "fixed32")
    stride = rc.formats.mxfp4_row_stride(dim) if kind == "mxfp4" else dim * {"f32": 4, "fixed32": 4, "f16": 2, "bf16": 2}.get(kind, 1)
    out = np.empty((n, stride), dtype=np.uint8)
    torch.cuda.synchronize()
    assert eng._L.emb_copy_to_host(eng._h, out.ctypes.data, ptr, out.nbytes) == 0
    return out
