"""What the GPU tests of the backward pass share (tests/test_gpu_grad.py, test_gpu_optim.py, test_gpu_grad_multi.py,
test_gpu_grad_order.py, test_gpu_grad_segmented.py, test_gpu_grad_segmented_ragged.py, test_gpu_grad_graph.py, test_gpu_train_loop.py): arrays to the device,
tables in and out as bytes, the assertions on tables and states, the ragged batch on the device.  A plain module like tests/grad_cases.py; the engine
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


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def check_table(got, want, what):
    """The assertion of every table comparison: every byte of every row."""
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "table rows", bad[:8], got[bad[0]][:16], want[bad[0]][:16])


def check_state(d_state, want, what):
    """The assertion of every optimizer-state comparison: every bit of every row's state."""
    got = host(d_state).reshape(want.shape)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(want.shape[0], -1).any(axis=1))
    assert bad.size == 0, (what, "state rows", bad[:8], got[bad[0]], want[bad[0]])


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


def in_place(G, ld, col):
    """G as a view of a wider NaN buffer: columns col .. col + dim of ld."""
    wide = torch.full((G.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, col:col + G.shape[1]] = G
    return wide[:, col:col + G.shape[1]]


class SparseCall:
    """A raw emb_grad_sparse call over device tensors, its descriptor built once: the C ABI's pure enqueue, which leaves |U| on
    the device (GradContext.sparse_grad waits for it)."""

    def __init__(self, ctx, table, idx, off, G, mode="sum", w=None, pad=None):
        import ctypes
        from importlib import import_module
        lib = import_module("pim-embedding-lookup_amd.lib")
        self.ctx, self.desc, self.keep = ctx, lib.EmbGradDesc(), []
        self.itype, on_device = ctx._desc(self.desc, table, idx, off, G, mode, w, pad, 0, self.keep)
        assert on_device and self.desc.grad == G.data_ptr()
        self.n, self._check, self._ref = int(self.desc.n_indices), lib.check_grad, ctypes.byref(self.desc)

    def enqueue(self, rows_out, grads_out, n_unique, stream):
        """rows_out int64 [capacity], grads_out float32 [capacity, dim], n_unique int64 [1]: all on the device, capacity >= n."""
        assert rows_out.dtype == torch.int64 and grads_out.dtype == torch.float32 and n_unique.dtype == torch.int64
        assert rows_out.is_contiguous() and grads_out.is_contiguous() and grads_out.shape[0] == rows_out.shape[0] >= self.n
        self._check(self.ctx._G.emb_grad_sparse(self.ctx._h, self._ref, self.itype, rows_out.data_ptr(), grads_out.data_ptr(), rows_out.shape[0],
                                                n_unique.data_ptr(), stream))


class RaggedBatch:
    """One variant of grad_seg_ref.ragged_case on the device, with what the calls take."""

    def __init__(self, case, mode_name, width, dim, lead=False, narrow=False, bags=None, view=None):
        ids, off, mode, w, pad = case.args(mode_name, width, lead, bags)
        self.case, self.key, self.host_args = case, (mode_name, width, dim, lead, narrow, bags), (ids, off, mode, w, pad)
        self.idx, self.off = to_dev(case.ids_array(width, bags)), to_dev(case.offsets_array(width, lead, bags))
        self.G = to_dev(case.grads(dim, narrow)[:bags])
        if view is not None:
            self.G = in_place(self.G, *view)
        self.mode, self.pad = mode, pad
        self.w = None if w is None else to_dev(w)
        self.n, self.B, self.n_bad = len(ids), len(off), case.n_bad(lead, bags)

    def reference(self, S):
        mode_name, width, dim, lead, narrow, bags = self.key
        return self.case.reference(S, mode_name, width, dim, lead, narrow, bags)

    def sparse(self, ctx, t):
        return ctx.sparse_grad(t, self.idx, self.off, self.G, mode=self.mode, per_sample_weights=self.w, padding_idx=self.pad)
