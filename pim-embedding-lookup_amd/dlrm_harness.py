"""`apply_emb`-shaped harness over the engine.

Stands where `dlrm_s_pytorch.py::apply_emb` stands in the reference's stack [EXT: that file is an
empty submodule here; flags from README.md:6,10,14 and upmem/run.sh:72-82,111-121]: a list of
`nn.EmbeddingBag(n_k, m, mode="sum")` called per table with (indices_k, offsets_k), each returning
[B, m].  Here all tables are served by ONE fused HIP launch.  Inference by default (as the reference's
`--inference-only` runs); `--fused-sgd LR` trains the tables: apply_emb's result is attached to the autograd graph and
loss.backward() applies the fused SGD step of the backward pass (include/pimemb_grad.h) to the served tables;
`--fused-adagrad LR` / `--fused-rowwise-adagrad LR` do the same with the fused Adagrad / row-wise Adagrad step (the three are
mutually exclusive; `--multi-table-step` sends them through the multi-table entry points, `--segmented-sums [S]` makes them sum in the
segmented order of additions; `--master-weights` keeps fp32 master rows and runs the fused master-weight step, with which fp8 and
mxfp4 tables train; `--stochastic-rounding [SEED]` rounds the last operation of a step on f16 / bf16 tables stochastically instead,
with no master).  No MLPs -- the rest of the model is out of scope.

    python -m pim_embedding_lookup_amd.dlrm_harness --arch-sparse-feature-size=16 \
        --arch-embedding-size=1460-583-10131227-… --mini-batch-size=39292 --inference-only
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from . import workloads
from .engine import EmbeddingEngine


class EmbeddingBagCollection:
    """emb_l of a DLRM: T tables of dim m in HBM; forward(lS_o, lS_i) -> list of [B, m]."""

    def __init__(self, ln_emb, m_spa: int, device: int = 0, weights=None, seed: int = 0, dtype="f32",
                 trusted_inputs: bool = False, deferred_check: bool = False, weighted_pooling: str | None = None,
                 pooling_weights=None, out_dtype: str | None = None, quantize_on_device: bool = False):
        import torch
        self.torch = torch
        # quantize_on_device=True: fp32 weights are encoded into `dtype` ON THE GPU (engine.load_table_f32: the row writer,
        # bit for bit what the host encoders below give) instead of on the host -- no encoded copy of a table in host memory
        # out_dtype="weight": f16 / bf16 tables return rows of their own dtype (the fp32 sum rounded once), as nn.EmbeddingBag
        # does; None: fp32 rows whatever the tables hold
        if out_dtype not in (None, "weight"):
            raise ValueError('out_dtype must be None or "weight"')
        if out_dtype == "weight" and dtype == "mxfp4":
            raise ValueError('out_dtype="weight" needs f16 or bf16 tables: mxfp4 tables return fp32 rows only')
        if out_dtype == "weight" and str(dtype).startswith("fp8"):
            raise ValueError('out_dtype="weight" needs f16 or bf16 tables: fp8 tables return fp32 rows only')
        self._out = "table" if out_dtype == "weight" and dtype in ("f16", "bf16") else None
        self.trusted_inputs = bool(trusted_inputs)     # False: every apply_emb checks its indices first (IndexError)
        self.deferred_check = bool(deferred_check)     # ... without waiting for the verdict (a later call / close() raises it)
        self.device = torch.device("cuda", device)
        self.ln_emb, self.m = [int(n) for n in ln_emb], int(m_spa)
        self.engine = EmbeddingEngine(device=device, max_tables=len(self.ln_emb))
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        for k, n in enumerate(self.ln_emb):
            if weights is not None:
                w = torch.as_tensor(np.asarray(weights[k]), dtype=torch.float32)
                if tuple(w.shape) != (n, self.m):
                    raise ValueError(f"table {k}: weight shape {tuple(w.shape)} != ({n}, {self.m})")
            else:  # DLRM init: U(-sqrt(1/n), sqrt(1/n))
                a = float(np.sqrt(1.0 / n))
                w = torch.empty((n, self.m), dtype=torch.float32, device=self.device).uniform_(-a, a, generator=g)
            if quantize_on_device:
                from . import lib as _lib
                codes = {"f32": _lib.EMB_F32, "f16": _lib.EMB_F16, "bf16": _lib.EMB_BF16, "fp8_e4m3": _lib.EMB_F8_E4M3,
                         "fp8_e5m2": _lib.EMB_F8_E5M2, "mxfp4": _lib.EMB_MXFP4}
                if dtype not in codes:
                    raise ValueError("dtype must be 'f32', 'f16', 'bf16', 'fp8_e4m3', 'fp8_e5m2' or 'mxfp4'")
                self.engine.load_table_f32(k, w, codes[dtype])
                continue
            tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "fp8_e4m3": torch.float8_e4m3fn,
                   "fp8_e5m2": torch.float8_e5m2}.get(dtype)
            if dtype == "mxfp4":       # fp32 checkpoints are quantised by the OCP MX rule (formats.to_mxfp4); m a multiple of 32
                from .formats import to_mxfp4
                from .lib import EMB_MXFP4
                self.engine.load_table(k, to_mxfp4(w.float().cpu().numpy()), dtype=EMB_MXFP4)
                continue
            if tdt is None:
                raise ValueError("dtype must be 'f32', 'f16', 'bf16', 'fp8_e4m3', 'fp8_e5m2' or 'mxfp4'")
            if dtype != "f32":
                w = w.to(tdt)          # (fp32 checkpoints are rounded by torch: nearest even)
            self.engine.load_table(k, w)
        self._plans = {}
        self._ids = list(range(len(self.ln_emb)))
        self._fused_lr = None
        self.table_dtype, self.master_weight = dtype, None      # master_weight: the tables' fp32 masters while --master-weights is on (_set_masters)
        self.multi_table_step = False                           # the fused steps go through the multi-table entry points (--multi-table-step)
        self.segmented_sums = None                              # the fused steps' segment length in the segmented order of additions; None: position order (--segmented-sums)
        self._fused_adagrad, self.adagrad_sum = None, None      # (lr, eps, rowwise) and the per-table fp32 states of enable_fused_adagrad
        self.sr_seed, self.sr_step = None, 0                    # --stochastic-rounding: the seed while it is on, and the step number of the next table stepped
        # DLRM --weighted-pooling: v_W_l[k] is a weight per ROW of table k (ones for "fixed", the checkpoint's for "learned");
        # a bag entry is weighted by its row's weight, gathered with torch (dlrm_s_pytorch.py: v_W_l[k].gather(0, indices))
        if weighted_pooling not in (None, "fixed", "learned"):
            raise ValueError("weighted_pooling must be None, 'fixed' or 'learned'")
        self.weighted_pooling = weighted_pooling
        self.v_W_l = None
        if weighted_pooling is not None:
            if weighted_pooling == "learned" and pooling_weights is None:
                raise ValueError("weighted_pooling='learned' needs the per-row weights (pooling_weights / from_checkpoint)")
            self.v_W_l = [torch.ones(n, dtype=torch.float32, device=self.device) if weighted_pooling == "fixed" else
                          torch.as_tensor(np.asarray(pooling_weights[k]), dtype=torch.float32).to(self.device).contiguous()
                          for k, n in enumerate(self.ln_emb)]
            for k, v in enumerate(self.v_W_l):
                if v.numel() != self.ln_emb[k]:
                    raise ValueError(f"table {k}: {v.numel()} pooling weights for {self.ln_emb[k]} rows")

    @classmethod
    def from_checkpoint(cls, path: str, device: int = 0, weighted_pooling: str | None = None, dtype="f32",
                        quantize_on_device: bool = False):
        from .formats import load_dlrm_embedding_weights, load_dlrm_pooling_weights
        ws = load_dlrm_embedding_weights(path)
        vw = load_dlrm_pooling_weights(path, len(ws)) if weighted_pooling == "learned" else None
        return cls([w.shape[0] for w in ws], ws[0].shape[1], device=device, weights=ws, weighted_pooling=weighted_pooling,
                   pooling_weights=vw, dtype=dtype, quantize_on_device=quantize_on_device)

    def apply_emb(self, lS_o, lS_i, concat: bool = False, out=None, col: int = 0):
        """lS_o[k], lS_i[k]: offsets / indices of table k (torch CUDA tensors, int64 or int32, or
        numpy arrays -> host path).  Returns ly: list of [B_k, m] fp32, freshly allocated -- one fused
        launch on torch's current stream, no plan and no state kept (every batch brings new tensors).
        concat=True (torch CUDA tensors): ONE [B, T * m] fp32 tensor instead, equal to torch.cat(ly, dim=1) and written in place
        by the lookup -- the row the interaction layer reads; out= / col=: a 2-D float32 CUDA buffer whose columns col ..
        col + T * m receive it, e.g. behind the dense features (engine.lookup_concat)."""
        if len(lS_o) != len(self.ln_emb) or len(lS_i) != len(self.ln_emb):
            raise ValueError("need one (offsets, indices) pair per table")
        # validated and looked up in ONE engine call; nothing runs on bad input
        check = False if self.trusted_inputs else ("deferred" if self.deferred_check else True)
        if not concat and (out is not None or col):
            raise ValueError("out= / col= need concat=True")
        if concat and self._out is not None:
            raise ValueError('concat=True returns one fp32 tensor: it does not combine with out_dtype="weight"')
        if self._fused_lr is not None or self._fused_adagrad is not None:
            return self._apply_emb_fused_sgd(lS_o, lS_i, check, concat, out, col)
        if self.v_W_l is not None:
            return self._apply_emb_weighted(lS_o, lS_i, check, concat, out, col)
        if concat:
            return self.engine.lookup_concat(self._ids, list(lS_i), list(lS_o), out=out, col=col, check=check)
        if self._out is None and hasattr(lS_i, "dim") and hasattr(lS_o, "dim") and lS_i.dim() == 2 and lS_o.dim() == 2 and lS_i.is_cuda:
            # DLRM stacks fixed-size batches into [T, N] / [T, B] tensors: one [T, B, m] result, unbound
            return list(self.engine.lookup_stacked(self._ids, lS_i, lS_o, check=check).unbind(0))
        return self.engine.lookup_batched(self._ids, list(lS_i), list(lS_o), check=check, out_dtype=self._out)

    def _apply_emb_weighted(self, lS_o, lS_i, check, concat=False, out=None, col=0):
        """--weighted-pooling: per-sample weights v_W_l[k][indices] (gathered by torch on the GPU), then ONE pooled call."""
        lS_i, lS_o = list(lS_i), list(lS_o)
        if not all(getattr(i, "is_cuda", False) for i in lS_i):
            raise TypeError("weighted pooling takes torch CUDA index tensors")
        if check:      # (a wild index must not reach torch's gather either)
            self.validate(lS_o, lS_i)
        gathered = [v.gather(0, i.long()) for v, i in zip(self.v_W_l, lS_i)]
        ws = [w.detach() for w in gathered]

        def lookup():
            if concat:
                return self.engine.lookup_concat(self._ids, lS_i, lS_o, out=out, col=col, modes="sum", per_sample_weights=ws, check=check)
            return self.engine.lookup_pooled(self._ids, lS_i, lS_o, "sum", per_sample_weights=ws, check=check, out_dtype=self._out)
        if self._pooling_weights_trained():      # (enable_pooling_weight_grad: the result joins the graph on the gathered weights)
            from . import torch_module as tm
            return tm._WeightedLookup.apply(tm._anchor(self, self.device), lookup, lambda g: self._weights_grads(lS_o, lS_i, g, concat, col), None, *gathered)
        return lookup()

    def enable_pooling_weight_grad(self, on: bool = True):
        """--weighted-pooling: make the per-row pooling weights v_W_l[k] leaves that require grad.  apply_emb's result then joins
        the autograd graph on v_W_l[k].gather(0, indices): its backward computes the gradient of those per-sample weights on the
        GPU (GradContext.weights_grad: one value per index, a fixed tree, the same bits on every run), and torch's own backward
        of gather scatters it into v_W_l[k].grad -- that scatter is torch's, and so is its order of additions.  With a fused step
        enabled the weights' gradient is enqueued first, the step behind it.  Returns self."""
        if self.v_W_l is None:
            raise ValueError("enable_pooling_weight_grad needs weighted_pooling")
        self.v_W_l = [v.detach().requires_grad_(bool(on)) for v in self.v_W_l]
        return self

    def _pooling_weights_trained(self) -> bool:
        return self.v_W_l is not None and self.torch.is_grad_enabled() and any(v.requires_grad for v in self.v_W_l)

    def _table_grads(self, g, concat, col):
        """Per table the [B, m] gradient of its pooled rows (None where there is none), read in place where it is ONE tensor."""
        from . import torch_module as tm
        if concat:
            g = g if g.dtype == self.torch.float32 else g.float()
            g = g if g.stride(1) == 1 and (g.shape[0] < 2 or g.stride(0) >= g.shape[1]) else g.contiguous()
            return [g[:, col + k * self.m:col + (k + 1) * self.m] for k in range(len(self._ids))]
        return [None if x is None else tm._grad_view(x, self.m) for x in g]

    def _weights_grads(self, lS_o, lS_i, g, concat, col):
        """float32 [n_k] per table: the gradient of the per-sample weights of one batch (None where a table has no gradient)."""
        from . import torch_module as tm
        grads = self._table_grads(g, concat, col)
        live = [k for k, x in enumerate(grads) if x is not None]
        out = [None] * len(grads)
        if live:
            order = ("segmented", self.m, int(self.segmented_sums)) if self.segmented_sums else ("position",)
            size = sum if self.multi_table_step else max      # (the context the fused step behind this call uses: made once)
            ctx = tm._grad_context(self.engine, size(i.shape[0] for i in lS_i), size(o.shape[0] for o in lS_o), *order)
            dws = ctx.weights_grad([self._ids[k] for k in live], [lS_i[k] for k in live], [lS_o[k] for k in live], [grads[k] for k in live])
            for k, dw in zip(live, dws):
                out[k] = dw
        return out

    def _set_masters(self, on: bool) -> None:
        """--master-weights: one fp32 master per table (self.master_weight), made from the served tables by exact widening when it is
        switched on and dropped when it is switched off, so that a master is never older than its table."""
        if not on:
            self.master_weight = None
        elif self.master_weight is None:
            if self.table_dtype == "f32":
                raise ValueError("master weights go with f16, bf16, fp8 and mxfp4 tables: an f32 table is its own master")
            if self.multi_table_step:
                raise ValueError("multi_table_step does not go with master weights: there is no multi-table master step")
            self.master_weight = [self.engine.master_of(t, self.device) for t in self._ids]

    def _set_sr(self, on: bool, seed: int, master_weights: bool) -> None:
        """--stochastic-rounding: the fused steps round their last operation stochastically (GradContext's sr=; f16 and bf16 tables);
        sr_step counts the tables stepped and is kept over enable_* calls."""
        if on:
            if master_weights:
                raise ValueError("stochastic rounding does not go with master weights: they are alternatives")
            if self.multi_table_step:
                raise ValueError("stochastic rounding does not go with multi_table_step: there is no stochastically rounded multi-table step")
            if self.table_dtype not in ("f16", "bf16"):
                raise ValueError("stochastic rounding goes with f16 and bf16 tables: an f32 table stores its fp32 result, there is nothing to round")
        self.sr_seed = int(seed) % (1 << 64) if on else None

    def _sr_take(self, n: int):
        """sr= of one context call over n tables (None while stochastic rounding is off); advances sr_step by n."""
        if self.sr_seed is None:
            return None
        if self.multi_table_step:
            raise ValueError("stochastic rounding does not go with multi_table_step: there is no stochastically rounded multi-table step")
        step = self.sr_step
        self.sr_step = (step + n) % (1 << 64)
        return (self.sr_seed, step)

    def enable_fused_sgd(self, lr, master_weights: bool = False, stochastic_rounding: bool = False, sr_seed: int = 0):
        """From now on apply_emb (lists of torch CUDA tensors; f32 / f16 / bf16 tables) returns tensors attached to the autograd
        graph whose backward applies W -= lr * grad to the served tables (GradContext.sgd_step): loss.backward() is the tables'
        whole training step.  lr=None switches it off.  The per-row pooling weights of --weighted-pooling get their gradient in the
        same backward after enable_pooling_weight_grad(), computed before the step, at the table the forward read."""
        self._set_sr(stochastic_rounding and lr is not None, sr_seed, master_weights)
        self._fused_lr = None if lr is None else float(lr)
        self._fused_adagrad = None
        self._set_masters(master_weights and lr is not None)
        return self

    def enable_fused_adagrad(self, lr, eps: float = 1e-10, rowwise: bool = False, initial_accumulator_value: float = 0.0, master_weights: bool = False,
                             stochastic_rounding: bool = False, sr_seed: int = 0):
        """As enable_fused_sgd, with the fused Adagrad step (rowwise=True: row-wise Adagrad, one accumulator per row;
        GradContext.adagrad_step).  The fp32 states -- self.adagrad_sum, one tensor per table -- are allocated here, once per
        flavour, filled with initial_accumulator_value.  lr=None switches it off.  Switches a fused SGD off."""
        import torch
        self._set_sr(stochastic_rounding and lr is not None, sr_seed, master_weights)
        if lr is None:
            self._fused_adagrad = None
            self._set_masters(False)
            return self
        self._set_masters(master_weights)
        if self.adagrad_sum is None or (self.adagrad_sum[0].dim() == 1) != bool(rowwise):
            shape = lambda n: (n,) if rowwise else (n, self.m)  # noqa: E731
            self.adagrad_sum = [torch.full(shape(int(n)), float(initial_accumulator_value), dtype=torch.float32, device=self.device) for n in self.ln_emb]
        self._fused_adagrad, self._fused_lr = (float(lr), float(eps), bool(rowwise)), None
        return self

    def _apply_emb_fused_sgd(self, lS_o, lS_i, check, concat, out, col):
        from . import torch_module as tm
        lS_i, lS_o = [i.contiguous() for i in lS_i], [o.contiguous() for o in lS_o]
        if not all(getattr(i, "is_cuda", False) for i in lS_i):
            raise TypeError("the fused SGD step takes lists of torch CUDA index tensors")
        if self.v_W_l is not None and check:
            self.validate(lS_o, lS_i)
        gathered = None if self.v_W_l is None else [v.gather(0, i.long()) for v, i in zip(self.v_W_l, lS_i)]
        ws = None if gathered is None else [w.detach() for w in gathered]
        lr, ada = self._fused_lr, self._fused_adagrad

        def lookup():
            if concat:
                return self.engine.lookup_concat(self._ids, lS_i, lS_o, out=out, col=col, modes="sum", per_sample_weights=ws, check=check)
            return self.engine.lookup_pooled(self._ids, lS_i, lS_o, "sum", per_sample_weights=ws, check=check, out_dtype=self._out)

        def step(g):
            grads = self._table_grads(g, concat, col)
            live = [k for k, x in enumerate(grads) if x is not None]
            multi = bool(self.multi_table_step)      # (its context holds all tables' indices and bags at once)
            size = sum if multi else max
            order = ("segmented", self.m, int(self.segmented_sums)) if self.segmented_sums else ("position",)
            ctx = tm._grad_context(self.engine, size(i.shape[0] for i in lS_i), size(o.shape[0] for o in lS_o), *order)
            args = ([self._ids[k] for k in live], [lS_i[k] for k in live], [lS_o[k] for k in live], [grads[k] for k in live])
            w_live = [None if ws is None else ws[k] for k in live]
            masters = self.master_weight
            if masters is not None:      # the fused master-weight step (emb_grad_master_step): every table dtype but fp32, table after table
                if multi:
                    raise ValueError("multi_table_step does not go with master weights: there is no multi-table master step")
                if ada is None:
                    ctx.master_step(*args, [masters[k] for k in live], lr, optimizer="sgd", per_sample_weights=w_live)
                else:
                    ctx.master_step(*args, [masters[k] for k in live], ada[0], optimizer="rowwise" if ada[2] else "adagrad",
                                    states=[self.adagrad_sum[k] for k in live], eps=ada[1], per_sample_weights=w_live)
            elif ada is None:
                ctx.sgd_step(*args, lr, per_sample_weights=w_live, multi=multi, sr=self._sr_take(len(live)))
            else:
                ctx.adagrad_step(*args, [self.adagrad_sum[k] for k in live], ada[0], eps=ada[1], rowwise=ada[2], per_sample_weights=w_live,
                                 multi=multi, sr=self._sr_take(len(live)))
        if self._pooling_weights_trained():      # the weights' gradient first, the step behind it
            return tm._WeightedLookup.apply(tm._anchor(self, self.device), lookup, lambda g: self._weights_grads(lS_o, lS_i, g, concat, col), step, *gathered)
        return tm._FusedSGD.apply(tm._anchor(self, self.device), lookup, step)

    def validate(self, lS_o, lS_i) -> None:
        """emb_validate_inputs over one batch: IndexError on an index >= table rows or broken offsets, as
        nn.EmbeddingBag raises (the lookup kernels themselves are unchecked, like the reference's DPU program)."""
        stacked = hasattr(lS_i, "dim") and lS_i.dim() == 2
        bad = self.engine.validate(self._ids, list(lS_i.unbind(0)) if stacked else list(lS_i),
                                   list(lS_o.unbind(0)) if stacked else list(lS_o))
        if bad:
            raise IndexError(f"{bad} index / offset value(s) out of range (emb_validate_inputs)")

    def prepare(self, lS_o, lS_i):
        """For callers that reuse the SAME device tensors every step (static-shape serving, hipGraph
        capture): a prepared plan over these buffers.  plan.launch() enqueues the lookup (3-4 us of host
        time), plan.outputs are its fixed output tensors.  The caller keeps the inputs alive."""
        plan = self.engine.plan(self._ids, list(lS_i), list(lS_o), out_dtype=self._out)
        self._plans[id(plan)] = plan
        return plan

    forward = __call__ = apply_emb

    def close(self):
        for p in self._plans.values():
            p.destroy()
        self._plans.clear()
        self.engine.close()


class ShardedEmbeddingBagCollection:
    """The same `apply_emb(lS_o, lS_i) -> list of [B, m]` contract with the tables SHARDED over the ranks of one node
    (one process per GPU; every rank passes its own bags and gets its own pooled rows): `plan_shards` places each table --
    replicated, whole on an owner, or split by row range -- and every call is ONE library call (`emb_shard_lookup`).  The
    reference's lookup() likewise serves all its devices from one call (emb_host.h:258-270, 297, 312-321).

        comm = sharding.native_comm(engine, rank, world)   (RCCL; or peer=sharding.PeerGroup(...) for the peer-store exchange)
        ebc = ShardedEmbeddingBagCollection(ln_emb, m, rank, world, comm=comm)
        ly = ebc.apply_emb(lS_o, lS_i)                     # COLLECTIVE: every rank, every batch

    weights: per table [n, m] arrays (every rank passes the same; each keeps its shards), or None: W[k][r][c] from a hash
    of (k, r, c) in DLRM's U(-sqrt(1/n), sqrt(1/n)) range, so that ranks agree without exchanging anything."""

    def __init__(self, ln_emb, m_spa: int, rank: int, world: int, comm=None, peer=None, device: int = 0, weights=None, seed: int = 0,
                 replicate_bytes: int = 64 << 20, pooling: float = 1.0, trusted_inputs: bool = False, engine=None):
        import torch
        from . import sharding
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.ln_emb, self.m, self.rank, self.world = [int(n) for n in ln_emb], int(m_spa), int(rank), int(world)
        self.plan = sharding.plan_shards(self.ln_emb, self.m, 4, world, replicate_bytes=replicate_bytes, pooling=pooling)
        self.engine = engine if engine is not None else EmbeddingEngine(device=device, max_tables=len(self.plan.units) + 1)
        self._own_engine = engine is None
        self.sharded = sharding.ShardedEmbeddingBags(self.plan, self.engine, rank, comm, depth=0, check=not trusted_inputs, peer=peer)

        def rows_of(t, lo, hi):
            if weights is not None:
                return torch.as_tensor(np.asarray(weights[t][lo:hi]), dtype=torch.float32)
            a = float(np.float32(2.0 * np.sqrt(1.0 / self.ln_emb[t])))
            out = torch.empty((hi - lo, self.m), dtype=torch.float32, device=self.device)
            for r0 in range(lo, hi, 1 << 22):
                r1 = min(r0 + (1 << 22), hi)
                e = torch.arange(r0 * self.m, r1 * self.m, dtype=torch.int64, device=self.device)
                h = (e * 2654435761 + (t + 1) * 40503 + seed * 7919) % 2147483647
                out[r0 - lo:r1 - lo] = ((h.to(torch.float32) / 2147483647.0 - 0.5) * a).reshape(r1 - r0, self.m)
            return out

        self.sharded.load_tables(rows_of)

    def apply_emb(self, lS_o, lS_i):
        """lS_o[k], lS_i[k]: this rank's offsets / indices of table k (torch CUDA tensors, int64 or int32).  Returns this
        rank's ly: [B, m] fp32 per table.  With a PeerGroup the tensors of tables other ranks hold are copied into the
        group's arena first (peers gather from them in place)."""
        if len(lS_o) != len(self.ln_emb) or len(lS_i) != len(self.ln_emb):
            raise ValueError("need one (offsets, indices) pair per table")
        peer = self.sharded.peer
        if peer is not None:
            return self._apply_emb_peer(peer, list(lS_o), list(lS_i))
        return self.sharded.forward(list(lS_o), list(lS_i))

    def _apply_emb_peer(self, peer, lS_o, lS_i):
        """Peer stores: the owners gather this rank's indices IN PLACE and store pooled rows straight into its buffers, so all
        three must live in the group's ARENA -- a bump allocator that frees nothing before the group closes.  A training /
        serving loop therefore must not carve fresh blocks per call (round 4's harness did: the arena ran dry after a few
        hundred batches): three rotating slots per table, grown geometrically when a batch outgrows them, reused for ever.
        The rows a call returns stay valid for the next two calls."""
        t = self.torch
        T = len(self.ln_emb)
        if not hasattr(self, "_arena"):
            self._arena = {"slot": 0, "idx": [[None] * T for _ in range(3)], "off": [[None] * T for _ in range(3)], "out": [None] * 3}
        a = self._arena
        slot = a["slot"] = (a["slot"] + 1) % 3
        sh = self.sharded
        want = lS_i[0].dtype         # int64 (DLRM's) or int32: staged as they are -- the library takes both in place

        def staged(cache, k, x):
            x = sh._ids(x, want)
            n = int(x.numel())
            buf = cache[slot][k]
            if buf is None or buf.numel() < n or buf.dtype != want:
                buf = cache[slot][k] = peer.empty((max(2 * n, 64),), want)
            y = buf[:n]
            y.copy_(x)
            return y
        idx = [staged(a["idx"], k, lS_i[k]) for k in range(T)]
        off = [staged(a["off"], k, lS_o[k]) for k in range(T)]
        B = int(off[0].numel())
        one = a["out"][slot]
        if one is None or one.shape[1] < B:
            one = a["out"][slot] = peer.empty((T, max(2 * B, 16), self.m), t.float32)
        outs = [one[k][:B] for k in range(T)]
        return self.sharded.forward(off, idx, outs=outs)

    forward = __call__ = apply_emb

    def close(self):
        self.sharded.close()
        if self._own_engine:
            self.engine.close()


def random_batch(rng, ln_emb, batch: int, num_indices_per_lookup: int, fixed: bool, device=None):
    """DLRM's synthetic generator [EXT]: per sample and table, `num_indices_per_lookup` indices
    (fixed) or 1..num_indices_per_lookup (random), uniform over the table."""
    lS_o, lS_i = [], []
    for n in ln_emb:
        if fixed:
            lens = np.full(batch, num_indices_per_lookup, dtype=np.int64)
        else:
            lens = rng.integers(1, num_indices_per_lookup + 1, size=batch)
        off = np.zeros(batch, dtype=np.int64)
        off[1:] = np.cumsum(lens)[:-1]
        idx = rng.integers(0, n, size=int(lens.sum()), dtype=np.int64)
        lS_o.append(off)
        lS_i.append(idx)
    if device is not None:
        import torch
        lS_o = [torch.from_numpy(o).to(device) for o in lS_o]
        lS_i = [torch.from_numpy(i).to(device) for i in lS_i]
    return lS_o, lS_i


def main(argv=None):
    ap = argparse.ArgumentParser(description="embedding path of DLRM on the MI355X engine")
    ap.add_argument("--arch-sparse-feature-size", type=int, default=16)
    ap.add_argument("--arch-embedding-size", type=str, default="-".join(map(str, workloads.KAGGLE_ROWS)))
    ap.add_argument("--mini-batch-size", type=int, default=1)
    ap.add_argument("--num-indices-per-lookup", type=int, default=1)
    ap.add_argument("--num-indices-per-lookup-fixed", action="store_true")
    ap.add_argument("--num-batches", type=int, default=100)
    ap.add_argument("--inference-only", action="store_true")
    ap.add_argument("--data-set", type=str, default="random", choices=["random", "kaggle"])
    ap.add_argument("--data-generation", type=str, default="random", choices=["random", "dataset"])
    ap.add_argument("--processed-data-file", type=str, default="")
    ap.add_argument("--load-model", type=str, default="")
    ap.add_argument("--save-model", type=str, default="")
    ap.add_argument("--numpy-rand-seed", type=int, default=123)
    ap.add_argument("--weighted-pooling", type=str, default=None, choices=["fixed", "learned"])
    ap.add_argument("--concat-output", action="store_true",
                    help="apply_emb returns ONE [B, T * m] tensor, written in place by the lookup (the interaction layer's input)")
    ap.add_argument("--quantize-on-device", action="store_true",
                    help="fp32 weights (a checkpoint's, or the random init) reach the tables through the GPU row writer "
                         "(engine.load_table_f32) instead of the host encoders")
    ap.add_argument("--fused-sgd", type=float, default=None, metavar="LR",
                    help="train the tables: apply_emb's result joins the autograd graph, and the backward of a dummy loss (the sum of "
                         "the pooled rows) applies W -= LR * grad to the served tables on the GPU (include/pimemb_grad.h)")
    ap.add_argument("--fused-adagrad", type=float, default=None, metavar="LR",
                    help="as --fused-sgd, with the fused Adagrad step (eps 1e-10, fp32 state of the tables' shape)")
    ap.add_argument("--fused-rowwise-adagrad", type=float, default=None, metavar="LR",
                    help="as --fused-sgd, with the fused row-wise Adagrad step (one fp32 accumulator per row; feature size a multiple of 4)")
    ap.add_argument("--multi-table-step", action="store_true",
                    help="with one of the --fused-* flags: step the tables through the multi-table entry points (one pre-pass and one "
                         "launch per group of up to 16 tables instead of per table; the same bytes)")
    ap.add_argument("--table-dtype", type=str, default="f32", choices=["f32", "f16", "bf16", "fp8_e4m3", "fp8_e5m2", "mxfp4"],
                    help="the dtype the tables are served in (fp32 weights are encoded into it; mxfp4: feature size a multiple of 32); "
                         "fp8 and mxfp4 tables train with --master-weights only")
    ap.add_argument("--master-weights", action="store_true",
                    help="with one of the --fused-* flags: keep fp32 master rows and run the fused master-weight step "
                         "(emb_grad_master_step): the master is stepped in fp32 and the table row is its encoding -- the way to train "
                         "fp8 and mxfp4 tables, and f16 / bf16 ones without losing small updates; not for f32 tables, and not with "
                         "--multi-table-step")
    ap.add_argument("--stochastic-rounding", type=lambda v: int(v, 0), nargs="?", const=0, default=None, metavar="SEED",
                    help="with one of the --fused-* flags and --table-dtype f16 or bf16: the fused step rounds its last operation "
                         "stochastically (emb_grad_sgd_sr / emb_grad_step_sr; Philox words of SEED, default 0, and the step number), so the "
                         "stored table keeps on average the updates that rounding to nearest loses -- the alternative to --master-weights, "
                         "without a master; not with --multi-table-step")
    ap.add_argument("--segmented-sums", type=int, nargs="?", const=0, default=None, metavar="S",
                    help="with one of the --fused-* flags: sum a row's occurrences in segments of S (a power of two, 8 .. 1024; "
                         "default: GradContext's), the segmented order of include/pimemb_grad.h -- for skewed ids, where some rows "
                         "occur thousands of times in a batch; as fixed as the position order, other bits")
    ap.add_argument("--train-pooling-weights", type=float, default=None, metavar="LR",
                    help="with --weighted-pooling: train the per-row pooling weights too -- their gradient comes out of the same "
                         "backward (emb_grad_weights, then torch's scatter into the per-row weights) and torch.optim.SGD(lr=LR) steps them")
    args, ignored = ap.parse_known_args(argv)
    if ignored:   # MLP / training / logging flags of the reference command lines (README.md:6,10,14)
        print("ignored (outside the embedding path):", " ".join(ignored))
    fused = [(name, lr) for name, lr in (("SGD", args.fused_sgd), ("Adagrad", args.fused_adagrad), ("row-wise Adagrad", args.fused_rowwise_adagrad))
             if lr is not None]
    if len(fused) > 1:
        raise SystemExit("--fused-sgd, --fused-adagrad and --fused-rowwise-adagrad are mutually exclusive")
    if args.multi_table_step and not fused:
        raise SystemExit("--multi-table-step goes with one of --fused-sgd, --fused-adagrad and --fused-rowwise-adagrad")
    if args.master_weights and not fused:
        raise SystemExit("--master-weights goes with one of --fused-sgd, --fused-adagrad and --fused-rowwise-adagrad")
    if args.master_weights and args.multi_table_step:
        raise SystemExit("--master-weights does not go with --multi-table-step: there is no multi-table master step")
    if args.master_weights and args.table_dtype == "f32":
        raise SystemExit("--master-weights goes with --table-dtype f16, bf16, fp8_e4m3, fp8_e5m2 or mxfp4: an f32 table is its own master")
    if fused and args.table_dtype in ("fp8_e4m3", "fp8_e5m2", "mxfp4") and not args.master_weights:
        raise SystemExit(f"--table-dtype {args.table_dtype} trains with --master-weights only: a step in the stored precision mostly rounds away")
    if args.stochastic_rounding is not None:
        if not fused:
            raise SystemExit("--stochastic-rounding goes with one of --fused-sgd, --fused-adagrad and --fused-rowwise-adagrad")
        if args.master_weights:
            raise SystemExit("--stochastic-rounding does not go with --master-weights: they are alternatives")
        if args.multi_table_step:
            raise SystemExit("--stochastic-rounding does not go with --multi-table-step: there is no stochastically rounded multi-table step")
        if args.table_dtype not in ("f16", "bf16"):
            raise SystemExit("--stochastic-rounding goes with --table-dtype f16 or bf16: an f32 table stores its fp32 result, there is nothing to round")
    if args.segmented_sums is not None and not fused:
        raise SystemExit("--segmented-sums goes with one of --fused-sgd, --fused-adagrad and --fused-rowwise-adagrad")
    if args.train_pooling_weights is not None and args.weighted_pooling is None:
        raise SystemExit("--train-pooling-weights goes with --weighted-pooling")
    if not args.inference_only and not fused and args.train_pooling_weights is None:
        print("note: running the inference embedding path (--inference-only implied); --fused-sgd LR / --fused-adagrad LR / "
              "--fused-rowwise-adagrad LR train the tables")
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(args.numpy_rand_seed)
    data = None
    if args.data_set == "kaggle" and args.processed_data_file:
        from .formats import CriteoKaggleNpz
        data = CriteoKaggleNpz(args.processed_data_file)
        ln_emb = data.table_rows
    else:
        ln_emb = [int(x) for x in args.arch_embedding_size.split("-")]
    if args.load_model:
        ebc = EmbeddingBagCollection.from_checkpoint(args.load_model, weighted_pooling=args.weighted_pooling,
                                                     quantize_on_device=args.quantize_on_device, dtype=args.table_dtype)
    else:
        if args.weighted_pooling == "learned":
            raise SystemExit("--weighted-pooling learned needs --load-model (the per-row weights v_W_l come from it)")
        ebc = EmbeddingBagCollection(ln_emb, args.arch_sparse_feature_size, weighted_pooling=args.weighted_pooling,
                                     quantize_on_device=args.quantize_on_device, dtype=args.table_dtype)
    B = args.mini_batch_size
    batches = []
    for b in range(min(args.num_batches, 16)):
        if data is not None:
            o, i = data.batch((b * B) % max(data.n_samples - B, 1), B)
            batches.append(([torch.from_numpy(x).to(dev) for x in o], [torch.from_numpy(x).to(dev) for x in i]))
        else:
            batches.append(random_batch(rng, ebc.ln_emb, B, args.num_indices_per_lookup,
                                        args.num_indices_per_lookup_fixed, dev))
    cat = bool(args.concat_output)
    for o, i in batches:          # checked once here (IndexError on a bad index), unchecked in the timed loops
        ebc.apply_emb(o, i, concat=cat)
    ebc.trusted_inputs = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(args.num_batches):
        o, i = batches[b % len(batches)]
        ly = ebc.apply_emb(o, i, concat=cat)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.num_batches
    n_bags = int(ly.shape[0]) * len(ebc.ln_emb) if cat else sum(int(x.shape[0]) for x in ly)
    print(f"apply_emb{' (one [B, T * m] tensor)' if cat else ''}: {len(ebc.ln_emb)} tables, m={ebc.m}, batch {B}: {dt * 1e3:.4f} ms/batch, "
          f"{n_bags / dt:.3e} pooled lookups/s")
    if fused or args.train_pooling_weights is not None:      # forward + dummy loss + backward = lookup + the fused step on every table
        opt_name, opt_lr = fused[0] if fused else (None, None)
        ebc.multi_table_step = bool(args.multi_table_step)
        if args.segmented_sums is not None:
            from .engine import GradContext
            ebc.segmented_sums = args.segmented_sums or GradContext.DEFAULT_SEGMENT
        sr_kw = {} if args.stochastic_rounding is None else dict(stochastic_rounding=True, sr_seed=args.stochastic_rounding)
        if opt_name == "SGD":
            ebc.enable_fused_sgd(opt_lr, master_weights=args.master_weights, **sr_kw)
        elif opt_name is not None:
            ebc.enable_fused_adagrad(opt_lr, rowwise=opt_name != "Adagrad", master_weights=args.master_weights, **sr_kw)
        w_opt = None
        if args.train_pooling_weights is not None:      # the per-row pooling weights: plain torch.optim.SGD over v_W_l
            ebc.enable_pooling_weight_grad()
            w_opt = torch.optim.SGD(ebc.v_W_l, lr=args.train_pooling_weights)

        def train_step(o, i):
            if w_opt is not None:
                w_opt.zero_grad()
            ly = ebc.apply_emb(o, i, concat=cat)
            loss = ly.sum() if cat else sum(y.sum() for y in ly)
            loss.backward()
            if w_opt is not None:
                w_opt.step()
        train_step(*batches[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(args.num_batches):
            train_step(*batches[b % len(batches)])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.num_batches
        what = f"the fused {opt_name} step (lr {opt_lr})" if fused else "no table step"
        if w_opt is not None:
            what += f", the pooling weights trained by torch.optim.SGD (lr {args.train_pooling_weights})"
        print(f"apply_emb + loss.backward() with {what}{', multi-table' if args.multi_table_step else ''}"
              f"{', segmented sums of %d' % ebc.segmented_sums if ebc.segmented_sums else ''}: {dt * 1e3:.4f} ms/batch")
        ebc.close()
        return 0
    if ebc.v_W_l is not None:     # (prepared plans hold the sum path only)
        ebc.close()
        return 0
    plans = [ebc.prepare(o, i) for o, i in batches]        # same buffers every step: prepared plans
    for p in plans:
        p.launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(args.num_batches):
        plans[b % len(plans)].launch()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.num_batches
    print(f"prepared plans (static buffers): {dt * 1e3:.4f} ms/batch, {n_bags / dt:.3e} pooled lookups/s")
    if args.save_model:      # the embedding part of a DLRM checkpoint: emb_l.<k>.weight, straight out of HBM
        from .formats import save_dlrm_embedding_weights
        save_dlrm_embedding_weights(args.save_model, [ebc.engine.table_tensor(k).float().cpu().numpy()
                                                      for k in range(len(ebc.ln_emb))])
        print("saved", args.save_model)
    ebc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
