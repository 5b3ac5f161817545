"""`nn.EmbeddingBag(mode="sum")`-shaped modules over the engine -- the operator surface the reference
plugs into.  dlrm_s_pytorch.py::create_emb builds `emb_l = nn.ModuleList([nn.EmbeddingBag(n, m,
mode="sum", sparse=True) ...])` and apply_emb calls `emb_l[k](indices_k, offsets_k)` per table [EXT:
that file is an empty submodule here; call shape from README.md:6,10,14].  The reference's fork reroutes
exactly that call to populate_mram / lookup.  Here:

    emb_l[k] = EmbeddingBag.from_torch(emb_l[k])          # one table, same forward(input, offsets)
    ebc = FusedEmbeddingBags.from_torch(emb_l)            # all tables, ONE launch per apply_emb

Which class does what:
  EmbeddingBag / FusedEmbeddingBags                   the reference's path: mode="sum" only, no per-sample weights,
                                                      padding_idx or max_norm (the reference has none of them either,
                                                      SURVEY.md Appendix B.2); they refuse anything else.
  PoolingEmbeddingBag / FusedPoolingEmbeddingBags     the rest of nn.EmbeddingBag's inference side: mode "sum" / "mean" /
                                                      "max", per_sample_weights (sum only, as in torch) and padding_idx,
                                                      equal to torch's CPU result bit for bit (emb_lookup_pooled).
Training the tables: the Pooling modules have a backward pass on the GPU (libpimemb_grad.so, include/pimemb_grad.h), for mode
"sum" (with per_sample_weights and padding_idx) and "mean", every sum in position order -- the same bits on every run:
`sparse_grad(input, offsets, grad_output)` returns what nn.EmbeddingBag(sparse=True) leaves in weight.grad (coalesced),
`sgd_step_(input, offsets, grad_output, lr)` applies weight -= lr * grad in place (fp32 / fp16 / bf16 weights), and after
`enable_fused_sgd(lr)` forward() returns a tensor attached to the autograd graph whose backward runs that step, as fused-optimizer
embedding modules do: loss.backward() updates the served table, there is no weight.grad and nothing for an optimizer to do.  Off
by default: a module on which it was never called returns plain tensors, as before.  `enable_fused_adagrad(lr, eps, rowwise,
initial_accumulator_value)` / `adagrad_step_` are the same with the fused Adagrad or row-wise Adagrad step; the fp32 state is
`module.adagrad_sum` and, once it exists, `<prefix>adagrad_sum` in state_dict().  per_sample_weights that require grad are trained as well: forward()'s result joins
the autograd graph on them, and backward leaves their gradient -- one value per index, <grad_output[bag], weight[index]> over a
fixed tree (emb_grad_weights) -- in `.grad`, in their shape and dtype; with a fused step enabled it is computed first, at the
table forward() read, and the step runs behind it.  `per_sample_weights_grad(input, offsets, grad_output)` is the explicit call.
Not there: mode "max", momentum / Adam, weight decay, fp8 / MXFP4 weights, a second-order gradient.  max_norm is not supported
by any module.

Output dtype.  By default every module returns fp32 rows, whatever the table holds.  `out_dtype="weight"` makes a module
with an fp16 / bf16 weight return the weight's dtype, as nn.EmbeddingBag does: the fp32 pooled value rounded once (the
engine's out_dtype="table", EMB_POOL_OUT_TABLE_DTYPE).  The fused modules follow their bags unless told otherwise.
Weights may also be torch.float8_e4m3fn / torch.float8_e5m2 (dtype=, or a float8 `_weight`): 1-byte rows, `weight` and
`state_dict()` return them as float8; their output is always fp32 (out_dtype="weight" is refused).
dtype="mxfp4": an MXFP4 table (OCP Microscaling, 4.25 bits per element; embedding_dim a multiple of 32 up to 2048).  An fp32
`_weight` is quantised once (formats.to_mxfp4), prepacked fused rows -- uint8 [num_embeddings, EMB_MXFP4_ROW_STRIDE(dim)] -- are
taken as they are; `weight` and `state_dict()` hold the fused rows, which load back unchanged.  Output fp32 only.

Input checking.  The C ABI is as unchecked as the reference (an out-of-range index is a wild read there,
emb_dpu_lookup.c:113); these modules are what user tensors reach first, so by default every forward goes through
emb_lookup_batched_checked: indices / offsets are validated on the GPU first and IndexError is raised, like
nn.EmbeddingBag does, before anything is launched.  That costs one small kernel (7 us) and a wait for its one-word verdict per call (no
allocation, no device-wide synchronize); pass `trusted_inputs=True` (constructor or attribute) for the unchecked
fast path once the producer of the indices is known to be sound, or `deferred_check=True` to keep the check (a bad call's
lookup is still kept from running, on the GPU) without the wait: the IndexError then comes out of a LATER forward, of
`engine.check_report()` or of `engine.close()`, naming the call -- the wait inside the call is what a checked forward costs
on host-bound shapes (26 tables x 2048 bags: 14.4 us checked, 9.7 deferred, 6.6 unchecked; apply_emb with per-table lists: 31.5 / 20.7 /
17.5; 26 x 39 292 bags is GPU-bound: 28.8 either way, 20.9 unchecked -- profiles/r06/checked_calls/).

Checkpoints.  `state_dict()` carries `<prefix>weight` read out of HBM and `load_state_dict` uploads it, so a
DLRM whose `emb_l[k]` were swapped for these modules saves / loads the same keys and shapes as before."""
from __future__ import annotations

import threading

import torch

from . import lib as _l
from .engine import EmbeddingEngine

_engines: dict[int, EmbeddingEngine] = {}
_next_id: dict[int, int] = {}
_lock = threading.Lock()
_MAX_TABLES = 4096


def default_engine(device: int = 0) -> EmbeddingEngine:
    """One shared engine per GPU for the modules below (created on first use)."""
    with _lock:
        e = _engines.get(device)
        if e is None:
            e = _engines[device] = EmbeddingEngine(device=device, max_tables=_MAX_TABLES)
            _next_id[device] = 0
        return e


def _new_table_id(device: int) -> int:
    with _lock:
        t = _next_id[device]
        if t >= _MAX_TABLES:
            raise RuntimeError("default engine is full; pass engine= / table_id= explicitly")
        _next_id[device] = t + 1
        return t


def _engine_out_dtype(out_dtype, table_dtype):
    """A module's out_dtype (None: fp32 rows; "weight": the weight's dtype) -> the engine's (None | "table")."""
    if out_dtype not in (None, "weight"):
        raise ValueError(f'out_dtype has to be None or "weight", got {out_dtype!r}')
    if out_dtype == "weight" and table_dtype == "mxfp4":
        raise ValueError('out_dtype="weight" needs an fp16 or bf16 weight: an MXFP4 table returns fp32 rows only')
    if out_dtype == "weight" and table_dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        raise ValueError('out_dtype="weight" needs an fp16 or bf16 weight: a float8 weight returns fp32 rows only (an fp8 output would '
                         "round the pooled value lossily)")
    return "table" if out_dtype == "weight" and table_dtype in (torch.float16, torch.bfloat16) else None


def _mxfp4_rows(w, num_embeddings: int, embedding_dim: int, device):
    """A module's MXFP4 weight -> (fused rows as a uint8 tensor on `device`, None) or (None, the shape error): prepacked fused
    rows as they are, an fp32 [num_embeddings, embedding_dim] weight quantised once."""
    from .formats import mxfp4_row_stride, to_mxfp4
    if w.dtype == torch.uint8 and tuple(w.shape) == (num_embeddings, mxfp4_row_stride(embedding_dim)):
        return w.detach().to(device).contiguous(), None
    if w.dtype == torch.uint8 or tuple(w.shape) != (num_embeddings, embedding_dim):
        return None, (f"an MXFP4 weight is fp32 ({num_embeddings}, {embedding_dim}) or fused uint8 rows ({num_embeddings}, "
                      f"{mxfp4_row_stride(embedding_dim)}), got {w.dtype} {tuple(w.shape)}")
    return torch.from_numpy(to_mxfp4(w.detach().float().cpu().numpy())).to(device), None


def _bags_from(input, offsets, include_last_offset: bool):
    """torch's calling conventions -> (1-D indices, 1-D bag starts)."""
    if input.dim() == 2:
        if offsets is not None:
            raise ValueError("if input is 2D, then offsets has to be None")     # torch's own message
        B, L = input.shape
        return input.reshape(-1), torch.arange(0, B * L, L, dtype=input.dtype, device=input.device)
    if input.dim() != 1 or offsets is None or offsets.dim() != 1:
        raise ValueError("input has to be 1D with 1D offsets, or 2D without offsets")
    if offsets.dtype != input.dtype:
        offsets = offsets.to(input.dtype)
    if include_last_offset:
        offsets = offsets[:-1]      # the extra entry must be len(input): the last bag runs to the end either way
    return input, offsets


class EmbeddingBag(torch.nn.Module):
    """One table.  forward(input, offsets) -> [B, embedding_dim] fp32, like nn.EmbeddingBag(mode="sum"); with
    out_dtype="weight" in the weight's dtype."""

    def __init__(self, num_embeddings: int, embedding_dim: int, mode: str = "sum", sparse: bool = False,
                 _weight=None, include_last_offset: bool = False, device: int = 0, engine: EmbeddingEngine | None = None,
                 table_id: int | None = None, dtype=torch.float32, trusted_inputs: bool = False, deferred_check: bool = False,
                 out_dtype: str | None = None):
        super().__init__()
        self.trusted_inputs = bool(trusted_inputs)
        self.deferred_check = bool(deferred_check)
        self._table_dtype = dtype
        self.out_dtype = out_dtype
        self._engine_out = _engine_out_dtype(out_dtype, dtype)
        if mode != "sum":
            raise NotImplementedError("only mode='sum' (the reference pools by summation, emb_dpu_lookup.c:114)")
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        self.mode, self.sparse, self.include_last_offset = mode, sparse, include_last_offset
        self.engine = engine if engine is not None else default_engine(device)
        self.device_index = self.engine.device
        self.table_id = table_id if table_id is not None else _new_table_id(self.device_index)
        self._id_list = [self.table_id]
        dev = torch.device("cuda", self.device_index)
        if _weight is None:      # nn.EmbeddingBag's default init is N(0, 1)
            _weight = torch.randn((self.num_embeddings, self.embedding_dim), device=dev)
        w = torch.as_tensor(_weight)
        if dtype == "mxfp4":
            rows, err = _mxfp4_rows(w, self.num_embeddings, self.embedding_dim, dev)
            if err:
                raise ValueError(err)
            self.engine.load_table(self.table_id, rows, dtype=_l.EMB_MXFP4)
            return
        if tuple(w.shape) != (self.num_embeddings, self.embedding_dim):
            raise ValueError(f"weight shape {tuple(w.shape)} != ({self.num_embeddings}, {self.embedding_dim})")
        self.engine.load_table(self.table_id, w.detach().to(dtype).contiguous())

    @classmethod
    def from_pretrained(cls, embeddings, mode: str = "sum", include_last_offset: bool = False, **kw):
        return cls(embeddings.shape[0], embeddings.shape[1], mode=mode, _weight=embeddings,
                   include_last_offset=include_last_offset, **kw)

    @classmethod
    def from_torch(cls, module: torch.nn.EmbeddingBag, **kw):
        if module.padding_idx is not None or module.max_norm is not None:
            raise NotImplementedError("padding_idx / max_norm are not part of the reference path")
        return cls(module.num_embeddings, module.embedding_dim, mode=module.mode, sparse=module.sparse,
                   _weight=module.weight.detach(), include_last_offset=module.include_last_offset, **kw)

    @property
    def weight(self):
        """The table's rows in HBM as a torch tensor (zero-copy view; not a Parameter -- inference only)."""
        return self.engine.table_tensor(self.table_id)

    def forward(self, input, offsets=None, per_sample_weights=None):
        if per_sample_weights is not None:
            raise NotImplementedError("per_sample_weights are not part of the reference path")
        idx, off = _bags_from(input, offsets, self.include_last_offset)
        idx, off = idx.contiguous(), off.contiguous()
        check = False if self.trusted_inputs else ("deferred" if self.deferred_check else True)
        return self.engine.lookup_batched(self._id_list, [idx], [off], check=check, out_dtype=self._engine_out)[0]

    # ---- checkpoints: the same key and shape as nn.EmbeddingBag ("<prefix>weight", [num_embeddings, dim]) ----
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        destination[prefix + "weight"] = self.weight.detach().clone()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        key = prefix + "weight"
        if key not in state_dict:
            if strict:
                missing_keys.append(key)
            return
        w = state_dict[key]
        if self._table_dtype == "mxfp4":        # the fused rows a state_dict() of this module holds, or an fp32 weight to quantise
            rows, err = _mxfp4_rows(w, self.num_embeddings, self.embedding_dim, torch.device("cuda", self.device_index))
            if err:
                error_msgs.append(f"size mismatch for {key}: {err}")
            else:
                self.engine.load_table(self.table_id, rows, dtype=_l.EMB_MXFP4)
            return
        if tuple(w.shape) != (self.num_embeddings, self.embedding_dim):
            error_msgs.append(f"size mismatch for {key}: copying a param with shape {tuple(w.shape)} from checkpoint, "
                              f"the shape in current model is ({self.num_embeddings}, {self.embedding_dim}).")
            return
        self.engine.load_table(self.table_id, w.detach().to(self._table_dtype).contiguous())

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.embedding_dim}, mode='sum', table_id={self.table_id}, engine=MI355X"


class FusedEmbeddingBags(torch.nn.Module):
    """All tables of a model: forward(lS_o, lS_i) -> list of [B, m] with ONE fused launch (apply_emb).
    concat=True: forward returns ONE [B, sum(m)] fp32 tensor instead, equal to torch.cat(<the list>, dim=1) -- what the
    interaction layer reads -- written in place by the lookup (engine.lookup_concat), and takes out= / col=: a 2-D float32 CUDA
    buffer (or view, inner stride 1) whose columns col .. col + sum(m) receive the rows, e.g. behind the dense features."""

    def __init__(self, bags, trusted_inputs: bool | None = None, deferred_check: bool | None = None, out_dtype: str | None = None,
                 concat: bool = False):
        super().__init__()
        self.bags = torch.nn.ModuleList(bags)
        self.concat = _concat_flag(concat, bags, out_dtype)
        # unchecked only if every table says so (or the caller does); the same for the deferred verdict
        self.trusted_inputs = all(b.trusted_inputs for b in bags) if trusted_inputs is None else bool(trusted_inputs)
        self.deferred_check = all(b.deferred_check for b in bags) if deferred_check is None else bool(deferred_check)
        self._outs = _fused_out_dtypes(bags, out_dtype)
        engines = {id(b.engine) for b in self.bags}
        if len(engines) != 1:
            raise ValueError("all tables of a FusedEmbeddingBags must live in one engine")
        self.engine = self.bags[0].engine
        self._ids = [b.table_id for b in self.bags]

    @classmethod
    def from_torch(cls, emb_l, concat: bool = False, **kw):
        return cls([EmbeddingBag.from_torch(m, **kw) for m in emb_l], concat=concat)

    def forward(self, lS_o, lS_i, out=None, col: int = 0):
        check = False if self.trusted_inputs else ("deferred" if self.deferred_check else True)
        if not self.concat and (out is not None or col):
            raise ValueError("out= / col= need a module made with concat=True")
        if not self.concat and self._outs is None and hasattr(lS_i, "dim") and lS_i.dim() == 2 and hasattr(lS_o, "dim") and lS_o.dim() == 2 and lS_i.is_cuda:
            return list(self.engine.lookup_stacked(self._ids, lS_i, lS_o, check=check).unbind(0))      # (one fp32 [T, B, dim] tensor)
        idx, off = [], []
        for b, i, o in zip(self.bags, lS_i, lS_o):
            i1, o1 = _bags_from(i, o, b.include_last_offset)
            idx.append(i1.contiguous())
            off.append(o1.contiguous())
        if self.concat:
            return self.engine.lookup_concat(self._ids, idx, off, out=out, col=col, check=check)
        return self.engine.lookup_batched(self._ids, idx, off, check=check, out_dtype=self._outs)

    apply_emb = forward


def _concat_flag(concat, bags, out_dtype) -> bool:
    """concat=True of a fused module: one fp32 [B, sum(dim)] tensor -- which half-width rows cannot share."""
    if concat and _fused_out_dtypes(bags, out_dtype) is not None:
        raise ValueError('concat=True returns one fp32 tensor: it does not combine with out_dtype="weight"')
    return bool(concat)


def _fused_out_dtypes(bags, out_dtype):
    """The engine's out_dtype list of a fused module: each bag's own, or out_dtype="weight" for every bag; None when all
    rows leave as fp32."""
    outs = [b._engine_out if out_dtype is None else _engine_out_dtype(out_dtype, b._table_dtype) for b in bags]
    return outs if any(o is not None for o in outs) else None


class PoolingEmbeddingBag(torch.nn.Module):
    """One table with nn.EmbeddingBag's pooling options: forward(input, offsets=None, per_sample_weights=None) ->
    [B, embedding_dim] fp32 (out_dtype="weight": the weight's dtype) for mode "sum" / "mean" / "max", per_sample_weights (mode "sum" only, else NotImplementedError
    as torch raises), padding_idx (negative values count from the end, as torch normalises them), include_last_offset, 1-D
    input with offsets or 2-D input.  Same state_dict keys as EmbeddingBag; checking on by default (trusted_inputs,
    deferred_check as there)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, mode: str = "mean", sparse: bool = False, _weight=None,
                 include_last_offset: bool = False, padding_idx: int | None = None, device: int = 0,
                 engine: EmbeddingEngine | None = None, table_id: int | None = None, dtype=torch.float32,
                 trusted_inputs: bool = False, deferred_check: bool = False, out_dtype: str | None = None):
        super().__init__()
        self.out_dtype, self._table_dtype = out_dtype, dtype
        self._engine_out = _engine_out_dtype(out_dtype, dtype)
        if mode not in ("sum", "mean", "max"):
            raise ValueError(f"mode has to be one of sum, mean or max, got {mode!r}")
        self.num_embeddings, self.embedding_dim = int(num_embeddings), int(embedding_dim)
        if padding_idx is not None:
            padding_idx = int(padding_idx)
            if padding_idx < 0:
                padding_idx += self.num_embeddings
            if not 0 <= padding_idx < self.num_embeddings:
                raise ValueError("padding_idx must be within num_embeddings")     # torch's own check
        self.mode, self.sparse, self.include_last_offset, self.padding_idx = mode, sparse, include_last_offset, padding_idx
        self.trusted_inputs, self.deferred_check = bool(trusted_inputs), bool(deferred_check)
        # the table itself (upload, checkpoint I/O) is an EmbeddingBag held as a plain attribute, not a submodule: the
        # state_dict key stays "<prefix>weight", as nn.EmbeddingBag's
        object.__setattr__(self, "_table", EmbeddingBag(num_embeddings, embedding_dim, _weight=_weight,
                                                        include_last_offset=include_last_offset, device=device, engine=engine,
                                                        table_id=table_id, dtype=dtype))
        self.engine, self.table_id, self.device_index = self._table.engine, self._table.table_id, self._table.device_index
        self._id_list = [self.table_id]

    @classmethod
    def from_pretrained(cls, embeddings, mode: str = "mean", include_last_offset: bool = False, padding_idx=None, **kw):
        return cls(embeddings.shape[0], embeddings.shape[1], mode=mode, _weight=embeddings,
                   include_last_offset=include_last_offset, padding_idx=padding_idx, **kw)

    @classmethod
    def from_torch(cls, module: torch.nn.EmbeddingBag, **kw):
        if module.max_norm is not None:
            raise NotImplementedError("max_norm is not supported")
        return cls(module.num_embeddings, module.embedding_dim, mode=module.mode, sparse=module.sparse,
                   _weight=module.weight.detach(), include_last_offset=module.include_last_offset,
                   padding_idx=module.padding_idx, **kw)

    @property
    def weight(self):
        return self.engine.table_tensor(self.table_id)

    def _check(self):
        return False if self.trusted_inputs else ("deferred" if self.deferred_check else True)

    def forward(self, input, offsets=None, per_sample_weights=None):
        idx, off = _bags_from(input, offsets, self.include_last_offset)
        w = _weights_for(per_sample_weights, self.mode, input)
        idx, off = idx.contiguous(), off.contiguous()

        def lookup():
            return self.engine.lookup_pooled(self._id_list, [idx], [off], self.mode, per_sample_weights=None if w is None else [w],
                                             padding_idx=self.padding_idx, check=self._check(), out_dtype=self._engine_out)[0]
        lr, ada = getattr(self, "_fused_lr", None), getattr(self, "_fused_adagrad", None)
        if w is not None and per_sample_weights.requires_grad and torch.is_grad_enabled():
            # the weights are trained: the result joins the graph on them, and backward enqueues their gradient FIRST -- at the
            # table this forward read -- and the fused step, if one is enabled, behind it
            w = w.detach()
            step = None
            if ada is not None:
                step = lambda g: self._adagrad(idx, off, g, ada[0], ada[1], w)  # noqa: E731
            elif lr is not None:
                step = lambda g: self._step(idx, off, g, lr, w)  # noqa: E731
            return _WeightedLookup.apply(_anchor(self, idx.device), lookup, lambda g: [self._weights_grad(idx, off, g)], step, per_sample_weights)
        if ada is not None:
            return _FusedSGD.apply(_anchor(self, idx.device), lookup, lambda g: self._adagrad(idx, off, g, ada[0], ada[1], w))
        if lr is None:
            return lookup()
        return _FusedSGD.apply(_anchor(self, idx.device), lookup, lambda g: self._step(idx, off, g, lr, w))

    def enable_fused_sgd(self, lr: float, order: str = "position", master_weights: bool = False, stochastic_rounding: bool = False, sr_seed: int = 0):
        """stochastic_rounding=True (fp16 and bf16 tables): the step is the stochastically rounded one of include/pimemb_grad.h -- the last
        rounding goes up or down by a Philox word of (sr_seed, sr_step, row, element), so the stored table keeps, on average, the updates
        that rounding to nearest loses below half an ulp, without a master.  The module counts its steps in sr_step (a host integer, one
        per table stepped), and state_dict() carries `<prefix>sr_seed` / `<prefix>sr_step` while it is on: a resumed run continues the
        stream.  It is the alternative to master_weights=True (both: ValueError).  Off by default.
        master_weights=True: the module keeps fp32 master rows (master_weight, made from the table by exact widening on first
        use and saved as `<prefix>master_weight`) and the step is the fused master-weight step of include/pimemb_grad.h: the master
        is stepped in fp32 and the table row is its encoding -- the way to train fp8 and MXFP4 tables, and fp16 / bf16 ones without
        losing small updates.  Off by default.
        From now on forward() returns a tensor attached to the autograd graph, and its backward applies weight -= lr * grad
        to the served table (sgd_step_ with the inputs forward saw): loss.backward() is the whole training step of this table.
        lr=None switches it off again.  Switches a fused Adagrad off (its state stays).  order="segmented": a row's occurrences
        are summed in the segmented order of include/pimemb_grad.h (GradContext) -- for batches that name some rows thousands of
        times; as fixed as the position order, other bits.  Returns self."""
        _set_sr(self, stochastic_rounding, sr_seed, [self._table_dtype], master_weights)
        object.__setattr__(self, "_fused_order", _order(order))
        object.__setattr__(self, "_fused_lr", None if lr is None else float(lr))
        object.__setattr__(self, "_fused_adagrad", None)
        _set_master(self, master_weights)
        return self

    @property
    def sr_step(self) -> int:
        """The step number the next stochastically rounded step of this module uses (advanced by one per table stepped)."""
        return getattr(self, "_sr_step", 0)

    @property
    def sr_seed(self):
        """The seed of the module's stochastically rounded steps, or None while stochastic rounding is off."""
        return getattr(self, "_sr_seed", None)

    @property
    def master_weight(self):
        """The fp32 master rows (float32 CUDA tensor [num_embeddings, embedding_dim]), or None while master weights are off."""
        return getattr(self, "_master_weight", None) if getattr(self, "_fused_master", False) else None

    def enable_fused_adagrad(self, lr: float, eps: float = 1e-10, rowwise: bool = False, initial_accumulator_value: float = 0.0,
                             order: str = "position", master_weights: bool = False, stochastic_rounding: bool = False, sr_seed: int = 0):
        """As enable_fused_sgd (order=, stochastic_rounding= and sr_seed= included), with the fused Adagrad step (rowwise=True: row-wise Adagrad, one accumulator per row) of
        include/pimemb_grad.h: torch.optim.Adagrad(lr, eps=eps, initial_accumulator_value=...) without lr_decay and weight_decay.
        The fp32 state -- module.adagrad_sum, [num_embeddings, embedding_dim] or [num_embeddings] -- is allocated once, filled with
        initial_accumulator_value, kept over later calls (a change of `rowwise` allocates it anew), and saved by state_dict() as
        `<prefix>adagrad_sum`.  lr=None switches the step off (the state stays).  Switches a fused SGD off.  Returns self."""
        _set_sr(self, stochastic_rounding and lr is not None, sr_seed, [self._table_dtype], master_weights)
        object.__setattr__(self, "_fused_order", _order(order))
        if lr is None:
            object.__setattr__(self, "_fused_adagrad", None)
            return self
        _adagrad_state(self, bool(rowwise), float(initial_accumulator_value))
        object.__setattr__(self, "_fused_adagrad", (float(lr), float(eps)))
        object.__setattr__(self, "_fused_lr", None)
        _set_master(self, master_weights)
        return self

    @property
    def adagrad_sum(self):
        """The Adagrad state (float32 CUDA tensor), or None before enable_fused_adagrad / adagrad_step_ made one."""
        return getattr(self, "_adagrad_sum", None)

    def _context(self, idx, off, order=None):
        """The engine's backward context of `order` (None: the one enable_fused_* chose; the position order if none did)."""
        order = getattr(self, "_fused_order", "position") if order is None else _order(order)
        return _grad_context(self.engine, idx.shape[0], off.shape[0], order, self.embedding_dim)

    def _step(self, idx, off, grad_output, lr, w, order=None, sr_seed=None):
        """sr_seed None: as enable_fused_* set it; False: a plain step; an integer: a stochastically rounded step with that seed."""
        if grad_output is None:
            return
        g = _grad_view(grad_output, self.embedding_dim)
        if sr_seed not in (None, False):
            _check_sr([self._table_dtype], self.master_weight is not None)
        if self.master_weight is not None:
            self._context(idx, off, order).master_step(self._id_list, [idx], [off], [g], [self.master_weight], lr, optimizer="sgd", modes=self.mode,
                                                       per_sample_weights=w, padding_idx=self.padding_idx)
            return
        self._context(idx, off, order).sgd_step(self._id_list, [idx], [off], [g], lr, modes=self.mode, per_sample_weights=w,
                                                padding_idx=self.padding_idx, sr=_sr_take(self, 1, sr_seed))

    def _adagrad(self, idx, off, grad_output, lr, eps, w, order=None, sr_seed=None):
        if grad_output is None:
            return
        g = _grad_view(grad_output, self.embedding_dim)
        state = _adagrad_state(self)
        if sr_seed not in (None, False):
            _check_sr([self._table_dtype], self.master_weight is not None)
        if self.master_weight is not None:
            self._context(idx, off, order).master_step(self._id_list, [idx], [off], [g], [self.master_weight], lr,
                                                       optimizer="rowwise" if state.dim() == 1 else "adagrad", states=[state], eps=eps, modes=self.mode,
                                                       per_sample_weights=w, padding_idx=self.padding_idx)
            return
        self._context(idx, off, order).adagrad_step(self._id_list, [idx], [off], [g], [state], lr, eps=eps, rowwise=state.dim() == 1,
                                                    modes=self.mode, per_sample_weights=w, padding_idx=self.padding_idx, sr=_sr_take(self, 1, sr_seed))

    def _weights_grad(self, idx, off, grad_output):
        """float32 [len(idx)]: the gradient of per_sample_weights for one batch (None for a None gradient)."""
        if grad_output is None:
            return None
        if self.mode != "sum":
            raise NotImplementedError(f"per_sample_weights (and their gradient) are only supported for mode='sum' (got mode='{self.mode}')")
        g = _grad_view(grad_output, self.embedding_dim)
        return self._context(idx, off).weights_grad(self.table_id, idx, off, g, padding_idx=self.padding_idx)

    def per_sample_weights_grad(self, input, offsets, grad_output):
        """The gradient of per_sample_weights for one batch, a float32 tensor of input's shape: for every index
        <grad_output[its bag], weight[index]>, summed over a fixed tree (include/pimemb_grad.h, emb_grad_weights: the same bits on
        every run); +0 for padding_idx entries and for indices outside the table, which are counted
        (engine._module_grad.report()).  It does not depend on the weights' values.  The table is only read."""
        idx, off, _w = self._bags_on_device(input, offsets, None)
        dw = self._weights_grad(idx, off, torch.as_tensor(grad_output).to(idx.device))
        return dw.reshape(tuple(torch.as_tensor(input).shape))

    def adagrad_step_(self, input, offsets, grad_output, lr: float, eps: float = 1e-10, per_sample_weights=None, order: str = "position",
                      stochastic_rounding: bool = False, sr_seed: int = 0):
        """One fused Adagrad step on the rows the batch names, in place and in stream order with forward(), on the module's state
        (adagrad_sum; of the flavour enable_fused_adagrad chose, or element-wise zeros if there is none yet).  order: as
        enable_fused_sgd.  stochastic_rounding / sr_seed: this one step rounds stochastically, at the module's sr_step, which it
        advances.  Returns self."""
        idx, off, w = self._bags_on_device(input, offsets, per_sample_weights)
        self._adagrad(idx, off, torch.as_tensor(grad_output).to(idx.device), float(lr), float(eps), w, order, int(sr_seed) if stochastic_rounding else False)
        return self

    def _bags_on_device(self, input, offsets, per_sample_weights):
        dev = torch.device("cuda", self.device_index)
        idx, off = _bags_from(torch.as_tensor(input).to(dev), None if offsets is None else torch.as_tensor(offsets).to(dev), self.include_last_offset)
        w = _weights_for(None if per_sample_weights is None else torch.as_tensor(per_sample_weights).to(dev), self.mode, input)
        return idx.contiguous(), off.contiguous(), w

    def sparse_grad(self, input, offsets, grad_output, per_sample_weights=None, order: str = "position"):
        """The gradient of the weight for one batch: a coalesced torch.sparse_coo_tensor [num_embeddings, embedding_dim] (fp32, on the
        GPU) -- rows ascending, each the sum of its contributions in position order (order="segmented": in the segmented order) --
        as nn.EmbeddingBag(sparse=True) leaves it in weight.grad after .coalesce(), without the all-zero rows torch lists for
        padding entries.  The weight is not changed."""
        idx, off, w = self._bags_on_device(input, offsets, per_sample_weights)
        g = _grad_view(torch.as_tensor(grad_output).to(idx.device), self.embedding_dim)
        rows, grads = self._context(idx, off, order).sparse_grad(
            self.table_id, idx, off, g, mode=self.mode, per_sample_weights=w, padding_idx=self.padding_idx)
        return torch.sparse_coo_tensor(rows.unsqueeze(0), grads, size=(self.num_embeddings, self.embedding_dim), is_coalesced=True)

    def sgd_step_(self, input, offsets, grad_output, lr: float, per_sample_weights=None, order: str = "position", stochastic_rounding: bool = False,
                  sr_seed: int = 0):
        """weight[r] -= lr * grad[r] for every row the batch names, in place and in stream order with forward(): one fp32
        multiply and one fp32 subtract per element, rounded once into the weight's dtype (fp32 / fp16 / bf16).  Entries whose
        index lies outside the table are skipped and counted (engine._module_grad.report()).  order: as enable_fused_sgd.
        stochastic_rounding / sr_seed: this one step rounds stochastically (fp16 / bf16), at the module's sr_step, which it advances.
        Returns self."""
        idx, off, w = self._bags_on_device(input, offsets, per_sample_weights)
        self._step(idx, off, torch.as_tensor(grad_output).to(idx.device), float(lr), w, order, int(sr_seed) if stochastic_rounding else False)
        return self

    def update_rows_(self, ids, rows):
        """weight[ids[p]] = rows[p] (float32 [n, embedding_dim], encoded into the weight's dtype on the GPU), in place and in
        stream order with forward(): lookups issued afterwards -- and state_dict() -- see the new rows.  The last occurrence of
        a repeated id wins.  With master weights on, the master rows are written too (the fp32 rows themselves).  Returns self."""
        try:
            _update_rows(self.engine, self.table_id, ids, rows)      # validates, then writes the table (IndexError: after the valid rows were written)
        except IndexError:
            if self.master_weight is not None:
                _update_master(self.master_weight, ids, rows)
            raise
        if self.master_weight is not None:                           # (behind the table: a refused update leaves both as they were)
            _update_master(self.master_weight, ids, rows)
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self._table._save_to_state_dict(destination, prefix, keep_vars)
        if self.adagrad_sum is not None:      # (only a module that has an Adagrad state gains the key)
            destination[prefix + "adagrad_sum"] = self.adagrad_sum.detach().clone()
        if self.master_weight is not None:    # (only with master weights on)
            destination[prefix + "master_weight"] = self.master_weight.detach().clone()
        _save_sr(self, destination, prefix)   # (only with stochastic rounding on)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        self._table._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        _load_sr(self, state_dict, prefix, strict, missing_keys)
        mkey = prefix + "master_weight"
        if mkey in state_dict:
            m = state_dict[mkey]
            if tuple(m.shape) != (self.num_embeddings, self.embedding_dim):
                error_msgs.append(f"size mismatch for {mkey}: {(self.num_embeddings, self.embedding_dim)} expected, got {tuple(m.shape)}")
                return
            object.__setattr__(self, "_master_weight", m.detach().to(device=torch.device("cuda", self.device_index), dtype=torch.float32).contiguous().clone())
            object.__setattr__(self, "_fused_master", True)
        elif self.master_weight is not None and strict:
            missing_keys.append(mkey)
        key = prefix + "adagrad_sum"
        if key in state_dict:
            s = state_dict[key]
            shapes = ((self.num_embeddings, self.embedding_dim), (self.num_embeddings,))
            if tuple(s.shape) not in shapes:
                error_msgs.append(f"size mismatch for {key}: an Adagrad state is {shapes[0]} or, row-wise, {shapes[1]}, got {tuple(s.shape)}")
                return
            have = self.adagrad_sum
            if have is not None and have.dim() != s.dim():      # (the state's shape IS the flavour: a silent switch of optimizer otherwise)
                flavour = lambda t: "row-wise" if t.dim() == 1 else "element-wise"  # noqa: E731
                error_msgs.append(f"{key}: the checkpoint holds a {flavour(s)} Adagrad state {tuple(s.shape)}, this module has a {flavour(have)} one "
                                  f"{tuple(have.shape)}; call enable_fused_adagrad(..., rowwise={s.dim() == 1}) before loading")
                return
            dev = torch.device("cuda", self.device_index)
            object.__setattr__(self, "_adagrad_sum", s.detach().to(device=dev, dtype=torch.float32).contiguous().clone())
        elif self.adagrad_sum is not None and strict:
            missing_keys.append(key)

    def extra_repr(self) -> str:
        return (f"{self.num_embeddings}, {self.embedding_dim}, mode={self.mode!r}, padding_idx={self.padding_idx}, "
                f"table_id={self.table_id}, engine=MI355X")



_GRAD_INDICES = 65536     # indices per call of the modules' shared backward context (it grows when a batch is larger)


def _order(order: str) -> str:
    if order not in ("position", "segmented"):
        raise ValueError(f"order has to be 'position' or 'segmented', got {order!r}")
    return order


def _grad_context(engine: EmbeddingEngine, n_indices: int, n_bags: int, order: str = "position", dim: int = 0, segment: int | None = None):
    """The backward context of `order` the modules of one engine share -- one per order: engine._module_grad (the position order)
    and engine._module_grad_segmented -- replaced by a larger one when a batch, or for the segmented order a table of `dim`, does
    not fit.  segment: the segment length to use (None: the one in use, or GradContext's default)."""
    attr = "_module_grad" if order == "position" else "_module_grad_segmented"
    g = getattr(engine, attr, None)
    seg = order == "segmented"
    if g is None or not g._h or g.max_indices < n_indices or g.max_bags < n_bags or (seg and (g.max_dim < dim or segment not in (None, g.segment))):
        wide = max(int(dim), g.max_dim if g is not None and g.max_dim else 0)
        segment = g.segment if segment is None and g is not None else segment
        if g is not None and g._h:
            g.close()
        kw = dict(order="segmented", max_dim=max(wide, 1), segment=segment) if seg else {}
        g = engine.grad_context(max(_GRAD_INDICES, int(n_indices)), max(_GRAD_INDICES, int(n_bags)), **kw)
        setattr(engine, attr, g)
    return g


def _set_master(bag, on: bool) -> None:
    """Master weights on or off for one PoolingEmbeddingBag.  Switched on, the fp32 master is made from the served table by exact
    widening (EmbeddingEngine.master_of); a bag on which they ARE on keeps its master (over enable_* calls, or as a checkpoint
    loaded it).  Switched off, the master is dropped: whatever changes the table while they are off -- in-place steps,
    update_rows_, a loaded weight -- is in the master that the next switching-on derives, never overwritten by a stale one."""
    was_on = getattr(bag, "_fused_master", False) and getattr(bag, "_master_weight", None) is not None
    object.__setattr__(bag, "_fused_master", bool(on))
    if not on:
        object.__setattr__(bag, "_master_weight", None)
    elif not was_on:
        if bag._table_dtype == torch.float32:
            raise ValueError("master_weights=True goes with fp16, bf16, fp8 and MXFP4 tables: an fp32 table is its own master")
        object.__setattr__(bag, "_master_weight", bag.engine.master_of(bag.table_id, torch.device("cuda", bag.device_index)))


_U64 = 1 << 64


def _check_sr(table_dtypes, master: bool, multi_table: bool = False) -> None:
    """What stochastic rounding does not go with: master weights (the alternative), the multi-table step, any table but fp16 / bf16."""
    if master:
        raise ValueError("stochastic_rounding=True does not go with master_weights=True: they are alternatives (a master keeps every update exactly, "
                         "stochastic rounding keeps them on average without one)")
    if multi_table:
        raise ValueError("stochastic_rounding=True does not go with multi_table=True: there is no stochastically rounded multi-table step")
    if any(dt not in (torch.float16, torch.bfloat16) for dt in table_dtypes):
        raise ValueError("stochastic_rounding=True goes with fp16 and bf16 tables: an fp32 table stores its fp32 result, there is nothing to round "
                         "(fp8 and MXFP4 tables train with master_weights=True)")


def _set_sr(mod, on: bool, seed: int, table_dtypes, master: bool, multi_table: bool = False) -> None:
    """Stochastic rounding on or off for a module: _sr_seed is the seed while it is on, else None; _sr_step is kept over enable_* calls."""
    if on:
        _check_sr(table_dtypes, master, multi_table)
    object.__setattr__(mod, "_sr_seed", int(seed) % _U64 if on else None)


def _sr_take(mod, n: int, seed=None):
    """(seed, step) for a stochastically rounded call over n descriptors -- seed None: the module's, False: none -- or None for a plain
    call; advances the module's sr_step by n."""
    seed = getattr(mod, "_sr_seed", None) if seed is None else seed
    if seed is None or seed is False:
        return None
    step = getattr(mod, "_sr_step", 0)
    object.__setattr__(mod, "_sr_step", (step + int(n)) % _U64)
    return (int(seed) % _U64, step)


def _save_sr(mod, destination, prefix) -> None:
    if getattr(mod, "_sr_seed", None) is not None:
        signed = lambda v: v - _U64 if v >= 1 << 63 else v  # noqa: E731 -- (int64 tensors: the 64 bits as they are)
        destination[prefix + "sr_seed"] = torch.tensor(signed(mod._sr_seed), dtype=torch.int64)
        destination[prefix + "sr_step"] = torch.tensor(signed(getattr(mod, "_sr_step", 0)), dtype=torch.int64)


def _load_sr(mod, state_dict, prefix, strict, missing_keys) -> None:
    """A checkpoint that carries sr_seed / sr_step switches stochastic rounding on with them: the resumed run continues the stream."""
    skey, tkey = prefix + "sr_seed", prefix + "sr_step"
    if skey in state_dict and tkey in state_dict:
        object.__setattr__(mod, "_sr_seed", int(state_dict[skey]) % _U64)
        object.__setattr__(mod, "_sr_step", int(state_dict[tkey]) % _U64)
    elif getattr(mod, "_sr_seed", None) is not None and strict:
        missing_keys += [k for k in (skey, tkey) if k not in state_dict]


def _update_master(master, ids, rows) -> None:
    """master[ids[p]] = rows[p], the last occurrence of a repeated id winning, ids outside the table skipped: what the row writer
    does to the table, on torch's current stream."""
    ids = torch.as_tensor(ids).to(master.device).reshape(-1).to(torch.int64)
    rows = torch.as_tensor(rows).to(device=master.device, dtype=torch.float32)
    n = master.shape[0]
    at = torch.arange(ids.shape[0], device=master.device)
    ok = (ids >= 0) & (ids < n)
    last = torch.full((n + 1,), -1, dtype=torch.int64, device=master.device)
    last.scatter_reduce_(0, torch.where(ok, ids, torch.full_like(ids, n)), at, "amax")
    keep = ok & (last[torch.where(ok, ids, torch.full_like(ids, n))] == at)
    master.index_copy_(0, ids[keep], rows[keep])


def _adagrad_state(bag, rowwise=None, init: float = 0.0):
    """A PoolingEmbeddingBag's Adagrad state, made on first use: float32 [num_embeddings, embedding_dim], or [num_embeddings]
    row-wise, filled with `init`.  rowwise None: whatever is there (element-wise if nothing is).  A plain attribute, not a
    buffer: state_dict() lists it through the module's own _save_to_state_dict, and only once it exists."""
    s = getattr(bag, "_adagrad_sum", None)
    if s is not None and (rowwise is None or (s.dim() == 1) == rowwise):
        return s
    ctx = _grad_context(bag.engine, 1, 1)
    shape = ctx.state_shape(bag.table_id, bool(rowwise))
    s = torch.full(shape, float(init), dtype=torch.float32, device=torch.device("cuda", bag.device_index))
    object.__setattr__(bag, "_adagrad_sum", s)
    return s


def _grad_view(grad_output, dim: int):
    """A gradient the kernels can read in place: float32, [B, dim], inner stride 1, rows that do not overlap (the gradient of
    out.sum() is an expanded scalar: stride 0 -- that one is materialised)."""
    g = grad_output if grad_output.dtype == torch.float32 else grad_output.float()
    if g.dim() != 2 or g.shape[1] != dim:
        raise ValueError(f"grad_output must be [n_bags, {dim}], got {tuple(g.shape)}")
    if g.stride(1) != 1 or (g.shape[0] > 1 and g.stride(0) < dim):
        g = g.contiguous()
    return g


class _FusedSGD(torch.autograd.Function):
    """forward runs the lookup, backward the fused SGD step on the inputs forward saw.  The graph is anchored on a zero-sized
    dummy leaf (its gradient stays None): the served table itself is not an autograd leaf."""

    @staticmethod
    def forward(ctx, anchor, lookup, step):
        out = lookup()
        ctx.step, ctx.many = step, isinstance(out, (list, tuple))
        return tuple(out) if ctx.many else out

    @staticmethod
    def backward(ctx, *grads):
        ctx.step(list(grads) if ctx.many else grads[0])
        return None, None, None


class _WeightedLookup(torch.autograd.Function):
    """_FusedSGD with per_sample_weights that require grad as real tensor inputs: backward enqueues their gradients first
    (weights_grad(g): one float32 [n] tensor, or None, per weight tensor -- at the table the forward read), then the fused step
    (None: there is none, the table is left alone), on the same stream.  Each gradient is cast once into its weights' dtype and
    shape.  The zero-sized anchor stays for the table side."""

    @staticmethod
    def forward(ctx, anchor, lookup, weights_grad, step, *weights):
        out = lookup()
        ctx.weights_grad, ctx.step, ctx.many = weights_grad, step, isinstance(out, (list, tuple))
        ctx.like = [(tuple(w.shape), w.dtype) for w in weights]
        return tuple(out) if ctx.many else out

    @staticmethod
    def backward(ctx, *grads):
        g = list(grads) if ctx.many else grads[0]
        dws = ctx.weights_grad(g)
        if ctx.step is not None:
            ctx.step(g)
        outs = [None if dw is None or not need else dw.reshape(shape).to(dtype)
                for dw, (shape, dtype), need in zip(dws, ctx.like, ctx.needs_input_grad[4:])]
        return (None, None, None, None, *outs)


def _anchor(module, device):
    a = getattr(module, "_sgd_anchor", None)
    if a is None:      # (a plain attribute, not a Parameter: state_dict() keeps its keys)
        a = torch.zeros(0, device=device, requires_grad=True)
        object.__setattr__(module, "_sgd_anchor", a)
    return a


_UPDATE_ROWS = 65536      # rows per device-pointer call of the modules' shared row writer


def _update_rows(engine: EmbeddingEngine, table_id: int, ids, rows) -> None:
    """weight[ids[p]] = rows[p] in place on the GPU (engine.row_writer; the last occurrence of an id wins), enqueued on torch's
    current stream, rows encoded into the table's dtype there.  IndexError -- after the other rows were written -- for ids
    outside the table (and MXFP4 rows holding an inf or a NaN): the module asks the writer for its count of skipped rows, a
    host wait as the modules' checked lookups have one."""
    dev = torch.device("cuda", engine.device)
    ids = torch.as_tensor(ids).to(dev).reshape(-1).contiguous()
    if ids.dtype not in (torch.int64, torch.int32):
        ids = ids.to(torch.int64)
    rows = torch.as_tensor(rows).to(device=dev, dtype=torch.float32).contiguous()
    if rows.dim() != 2 or rows.shape[0] != ids.shape[0]:
        raise ValueError(f"update_rows_: rows must be [len(ids), dim], got {tuple(rows.shape)} for {ids.shape[0]} ids")
    w = getattr(engine, "_module_writer", None)
    if w is None or not w._h:
        w = engine._module_writer = engine.row_writer(_UPDATE_ROWS)
    for at in range(0, ids.shape[0], _UPDATE_ROWS):
        w.update(table_id, ids[at:at + _UPDATE_ROWS], rows[at:at + _UPDATE_ROWS])
    bad = w.report()
    if bad:
        raise IndexError(f"update_rows_: {bad} rows were skipped (an id outside the table, or a non-finite value for an MXFP4 table); the others were written")


def _weights_for(per_sample_weights, mode, input):
    if per_sample_weights is None:
        return None
    if mode != "sum":
        raise NotImplementedError("embedding_bag: per_sample_weights was not None. per_sample_weights is only supported "
                                  f"for mode='sum' (got mode='{mode}'). Please open a feature request on GitHub.")
    if tuple(per_sample_weights.shape) != tuple(input.shape):
        raise ValueError("embedding_bag: If per_sample_weights ({}) is not None, then it must have the same shape as the "
                         "input ({})".format(tuple(per_sample_weights.shape), tuple(input.shape)))
    return per_sample_weights.reshape(-1).float().contiguous()


class FusedPoolingEmbeddingBags(torch.nn.Module):
    """All tables of a model, each with its own mode and padding_idx: forward(lS_o, lS_i, lS_w=None) -> list of [B, m] with
    ONE engine call (lS_w: per-table per-sample weights or None, sum tables only).  concat=True, out= / col=: as
    FusedEmbeddingBags -- ONE [B, sum(m)] fp32 tensor, every mode, weights and padding included."""

    def __init__(self, bags, trusted_inputs: bool | None = None, deferred_check: bool | None = None, out_dtype: str | None = None,
                 concat: bool = False):
        super().__init__()
        self.bags = torch.nn.ModuleList(bags)
        self.concat = _concat_flag(concat, bags, out_dtype)
        self.trusted_inputs = all(b.trusted_inputs for b in bags) if trusted_inputs is None else bool(trusted_inputs)
        self.deferred_check = all(b.deferred_check for b in bags) if deferred_check is None else bool(deferred_check)
        self._outs = _fused_out_dtypes(bags, out_dtype)
        if len({id(b.engine) for b in self.bags}) != 1:
            raise ValueError("all tables of a FusedPoolingEmbeddingBags must live in one engine")
        self.engine = self.bags[0].engine
        self._ids = [b.table_id for b in self.bags]
        self._modes = [b.mode for b in self.bags]
        self._pads = [b.padding_idx for b in self.bags]

    @classmethod
    def from_torch(cls, emb_l, concat: bool = False, **kw):
        return cls([PoolingEmbeddingBag.from_torch(m, **kw) for m in emb_l], concat=concat)

    def forward(self, lS_o, lS_i, lS_w=None, out=None, col: int = 0):
        check = False if self.trusted_inputs else ("deferred" if self.deferred_check else True)
        if not self.concat and (out is not None or col):
            raise ValueError("out= / col= need a module made with concat=True")
        idx, off, ws = [], [], []
        for k, (b, i, o) in enumerate(zip(self.bags, lS_i, lS_o)):
            i1, o1 = _bags_from(i, o, b.include_last_offset)
            idx.append(i1.contiguous())
            off.append(o1.contiguous())
            ws.append(_weights_for(None if lS_w is None else lS_w[k], b.mode, i))
        wl = None if lS_w is None else ws

        def lookup():
            if self.concat:
                return self.engine.lookup_concat(self._ids, idx, off, out=out, col=col, modes=self._modes, per_sample_weights=wl,
                                                 padding_idx=self._pads, check=check)
            return self.engine.lookup_pooled(self._ids, idx, off, self._modes, per_sample_weights=wl, padding_idx=self._pads, check=check,
                                             out_dtype=self._outs)
        lr, ada = getattr(self, "_fused_lr", None), getattr(self, "_fused_adagrad", None)
        trained = [] if lS_w is None or not torch.is_grad_enabled() else [k for k, w in enumerate(lS_w) if w is not None and w.requires_grad]
        if trained:      # as PoolingEmbeddingBag.forward: the weights' gradients first, then the fused step if there is one
            wl = [None if w is None else w.detach() for w in ws]
            step = None
            if ada is not None:
                step = lambda g: self._adagrad(idx, off, g, ada[0], ada[1], wl, col)  # noqa: E731
            elif lr is not None:
                step = lambda g: self._step(idx, off, g, lr, wl, col)  # noqa: E731
            return _WeightedLookup.apply(_anchor(self, idx[0].device), lookup, lambda g: self._weights_grads(idx, off, g, col, trained), step,
                                         *[lS_w[k] for k in trained])
        if ada is not None:
            return _FusedSGD.apply(_anchor(self, idx[0].device), lookup, lambda g: self._adagrad(idx, off, g, ada[0], ada[1], wl, col))
        if lr is None:
            return lookup()
        return _FusedSGD.apply(_anchor(self, idx[0].device), lookup, lambda g: self._step(idx, off, g, lr, wl, col))

    apply_emb = forward

    def enable_fused_sgd(self, lr: float, multi_table: bool = False, order: str = "position", master_weights: bool = False,
                         stochastic_rounding: bool = False, sr_seed: int = 0):
        """stochastic_rounding=True: as PoolingEmbeddingBag.enable_fused_sgd, for all tables (all fp16 / bf16), table after table: table k
        of a step uses step number sr_step + k, and the MODEL's sr_step advances by the number of tables stepped; saved as `sr_seed` /
        `sr_step` under the model's prefix.  ValueError with master_weights=True and with multi_table=True.
        master_weights=True: every bag keeps its fp32 master (bags[k].master_weight) and the step is the fused master-weight step,
        table after table; there is no multi-table master step, so multi_table=True with it raises ValueError.
        As PoolingEmbeddingBag.enable_fused_sgd, for every table of the model: the backward of forward()'s result -- the list,
        or the one [B, sum(m)] tensor of concat=True -- steps all of them.  multi_table=True: by the multi-table step (one
        pre-pass and one launch per group of up to 16 tables instead of per table; the same bytes).  order: as there.
        Returns self."""
        _set_sr(self, stochastic_rounding, sr_seed, [b._table_dtype for b in self.bags], master_weights, multi_table)
        self._set_masters(master_weights, multi_table)
        object.__setattr__(self, "_fused_order", _order(order))
        object.__setattr__(self, "_fused_multi", bool(multi_table))
        object.__setattr__(self, "_fused_lr", None if lr is None else float(lr))
        object.__setattr__(self, "_fused_adagrad", None)
        return self

    def _set_masters(self, on: bool, multi_table: bool) -> None:
        if on and multi_table:
            raise ValueError("multi_table=True does not go with master_weights=True: there is no multi-table master step (the group record of the "
                             "multi-table kernels has no room for the master pointer); the master step runs table after table")
        for b in self.bags:
            _set_master(b, on)

    def _masters_on(self) -> bool:
        """Whether the step is the master step: read from the bags, which own the masters (a checkpoint may have loaded them)."""
        on = [b.master_weight is not None for b in self.bags]
        if any(on) and not all(on):
            raise ValueError("some tables of this model have master weights and some have not: call enable_fused_sgd / enable_fused_adagrad with "
                             "master_weights=True (or False) to put them all in one state")
        return all(on) and bool(on)

    @property
    def master_weight(self):
        """The bags' fp32 masters, in table order (None where master weights are off)."""
        return [b.master_weight for b in self.bags]

    def enable_fused_adagrad(self, lr: float, eps: float = 1e-10, rowwise: bool = False, initial_accumulator_value: float = 0.0,
                             multi_table: bool = False, order: str = "position", master_weights: bool = False, stochastic_rounding: bool = False,
                             sr_seed: int = 0):
        """As PoolingEmbeddingBag.enable_fused_adagrad, for every table of the model: each bag holds its own state
        (bags[k].adagrad_sum, saved as `bags.<k>.adagrad_sum`), one call steps them all.  multi_table, order, master_weights,
        stochastic_rounding and sr_seed: as enable_fused_sgd.  Returns self."""
        _set_sr(self, stochastic_rounding and lr is not None, sr_seed, [b._table_dtype for b in self.bags], master_weights, multi_table)
        self._set_masters(master_weights, multi_table)
        object.__setattr__(self, "_fused_order", _order(order))
        object.__setattr__(self, "_fused_multi", bool(multi_table))
        if lr is None:
            object.__setattr__(self, "_fused_adagrad", None)
            return self
        for b in self.bags:
            _adagrad_state(b, bool(rowwise), float(initial_accumulator_value))
        object.__setattr__(self, "_fused_adagrad", (float(lr), float(eps)))
        object.__setattr__(self, "_fused_lr", None)
        return self

    @property
    def adagrad_sum(self):
        """The bags' Adagrad states, in table order (None where a bag has none)."""
        return [b.adagrad_sum for b in self.bags]

    @property
    def sr_step(self) -> int:
        """The step number the first table of the model's next stochastically rounded step uses."""
        return getattr(self, "_sr_step", 0)

    @property
    def sr_seed(self):
        """The seed of the model's stochastically rounded steps, or None while stochastic rounding is off."""
        return getattr(self, "_sr_seed", None)

    def _sr_call(self, n: int, multi: bool, sr_seed):
        """The sr= of one context call over n tables (None: a plain call), with what it does not go with refused."""
        if sr_seed is False or (sr_seed is None and getattr(self, "_sr_seed", None) is None):
            return None
        _check_sr([b._table_dtype for b in self.bags], self._masters_on(), multi)
        return _sr_take(self, n, sr_seed)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        _save_sr(self, destination, prefix)   # (only with stochastic rounding on)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        for key in (prefix + "sr_seed", prefix + "sr_step"):      # (the model's own keys, not a parameter's or a buffer's)
            if key in unexpected_keys:
                unexpected_keys.remove(key)
        _load_sr(self, state_dict, prefix, strict, missing_keys)

    def _table_grads(self, grad_output, col):
        """Per table the gradient of its pooled rows as the kernels read it ([B, m_k] float32, inner stride 1), None where
        there is none: the entries of a list, or the column views of ONE [B, sum(m)] gradient."""
        dims = [b.embedding_dim for b in self.bags]
        if isinstance(grad_output, (list, tuple)):
            if len(grad_output) != len(dims):
                raise ValueError(f"{len(grad_output)} gradients for {len(dims)} tables")
            return [None if g is None else _grad_view(g, d) for g, d in zip(grad_output, dims)]
        # ONE [B, sum(m)] gradient (of a concat=True forward; of a wider buffer from column `col`): read in place, table by table
        g = grad_output if grad_output.dtype == torch.float32 else grad_output.float()
        if g.dim() != 2 or g.shape[1] < col + sum(dims):
            raise ValueError(f"grad_output must be [n_bags, >= {col + sum(dims)}], got {tuple(g.shape)}")
        if g.stride(1) != 1 or (g.shape[0] > 1 and g.stride(0) < g.shape[1]):
            g = g.contiguous()
        at = [col + sum(dims[:k]) for k in range(len(dims))]
        return [g[:, a:a + d] for a, d in zip(at, dims)]

    def _weights_grads(self, idx, off, grad_output, col, tables):
        """The gradients of the per_sample_weights of `tables` (numbers in the module list), in that order: float32 [n_k]
        tensors, None where a table has no output gradient.  One launch per table, on the modules' shared context."""
        if grad_output is None:
            return [None] * len(tables)
        grads = self._table_grads(grad_output, col)
        live = [k for k in tables if grads[k] is not None]
        out = dict.fromkeys(tables)
        if live:
            order = getattr(self, "_fused_order", "position")
            ctx = _grad_context(self.engine, max(idx[k].shape[0] for k in live), max(off[k].shape[0] for k in live), order,
                                max(b.embedding_dim for b in self.bags))
            dws = ctx.weights_grad([self._ids[k] for k in live], [idx[k] for k in live], [off[k] for k in live], [grads[k] for k in live],
                                   padding_idx=[self._pads[k] for k in live])
            out.update(zip(live, dws))
        return [out[k] for k in tables]

    def per_sample_weights_grad(self, lS_o, lS_i, grad_output, col: int = 0):
        """PoolingEmbeddingBag.per_sample_weights_grad for all tables: a list of float32 tensors of the inputs' shapes.
        grad_output: a list of [B, m_k] gradients, or the ONE [B, sum(m)] gradient of a concat=True forward (from column col)."""
        idx, off, _ws, g = self._inputs_on_device(lS_o, lS_i, grad_output, None)
        dws = self._weights_grads(idx, off, g, col, list(range(len(self.bags))))
        return [None if dw is None else dw.reshape(tuple(torch.as_tensor(i).shape)) for dw, i in zip(dws, lS_i)]

    def _live_grads(self, idx, off, grad_output, ws, col, multi=False, order=None):
        """What a step of either optimizer is called with: (the backward context, positional arguments, keyword arguments, the
        tables' numbers in the module list) over the tables that have a gradient, or None when none has.  multi: the context
        holds the live tables' indices and bags all at once (their sums), so that the multi-table step can fuse them."""
        dims = [b.embedding_dim for b in self.bags]
        grads = self._table_grads(grad_output, col)
        live = [k for k, g in enumerate(grads) if g is not None]
        if not live:
            return None
        size = sum if multi else max
        order = getattr(self, "_fused_order", "position") if order is None else _order(order)
        ctx = _grad_context(self.engine, size(idx[k].shape[0] for k in live), size(off[k].shape[0] for k in live), order, max(dims))
        args = ([self._ids[k] for k in live], [idx[k] for k in live], [off[k] for k in live], [grads[k] for k in live])
        kw = dict(modes=[self._modes[k] for k in live], per_sample_weights=[None if ws is None else ws[k] for k in live],
                  padding_idx=[self._pads[k] for k in live])
        return ctx, args, kw, live

    def _step(self, idx, off, grad_output, lr, ws, col=0, multi=None, order=None, sr_seed=None):
        multi = getattr(self, "_fused_multi", False) if multi is None else bool(multi)
        call = self._live_grads(idx, off, grad_output, ws, col, multi, order)
        if call is not None:
            ctx, args, kw, live = call
            sr = self._sr_call(len(live), multi, sr_seed)
            if sr is not None:
                ctx.sgd_step(*args, lr, sr=sr, **kw)
                return
            if self._masters_on():
                self._no_multi_master(multi)
                ctx.master_step(*args, [self.bags[k].master_weight for k in live], lr, optimizer="sgd", **kw)
                return
            ctx.sgd_step(*args, lr, multi=multi, **kw)

    @staticmethod
    def _no_multi_master(multi) -> None:
        if multi:
            raise ValueError("multi_table=True does not go with master weights: there is no multi-table master step")

    def _adagrad(self, idx, off, grad_output, lr, eps, ws, col=0, multi=None, order=None, sr_seed=None):
        multi = getattr(self, "_fused_multi", False) if multi is None else bool(multi)
        call = self._live_grads(idx, off, grad_output, ws, col, multi, order)
        if call is None:
            return
        ctx, args, kw, live = call
        states = [_adagrad_state(self.bags[k]) for k in live]
        for rowwise in (False, True):      # (one call per flavour: the bags of a model usually share one)
            sel = [j for j, s in enumerate(states) if (s.dim() == 1) == rowwise]
            if sel:
                pick = lambda v: [v[j] for j in sel]  # noqa: E731
                sr = self._sr_call(len(sel), multi, sr_seed)
                if sr is not None:
                    ctx.adagrad_step(*[pick(a) for a in args], pick(states), lr, eps=eps, rowwise=rowwise, sr=sr, **{k: pick(v) for k, v in kw.items()})
                    continue
                if self._masters_on():
                    self._no_multi_master(multi)
                    ctx.master_step(*[pick(a) for a in args], [self.bags[live[j]].master_weight for j in sel], lr,
                                    optimizer="rowwise" if rowwise else "adagrad", states=pick(states), eps=eps, **{k: pick(v) for k, v in kw.items()})
                    continue
                ctx.adagrad_step(*[pick(a) for a in args], pick(states), lr, eps=eps, rowwise=rowwise, multi=multi,
                                 **{k: pick(v) for k, v in kw.items()})

    def _inputs_on_device(self, lS_o, lS_i, grad_output, lS_w):
        """The explicit steps' inputs as forward() would hold them: (indices, offsets, weights or None, gradient), on the GPU."""
        dev = torch.device("cuda", self.engine.device)
        idx, off, ws = [], [], []
        for k, (b, i, o) in enumerate(zip(self.bags, lS_i, lS_o)):
            i1, o1 = _bags_from(torch.as_tensor(i).to(dev), None if o is None else torch.as_tensor(o).to(dev), b.include_last_offset)
            idx.append(i1.contiguous())
            off.append(o1.contiguous())
            ws.append(_weights_for(None if lS_w is None else torch.as_tensor(lS_w[k]).to(dev), b.mode, i))
        if not isinstance(grad_output, (list, tuple)):
            grad_output = torch.as_tensor(grad_output).to(dev)
        return idx, off, None if lS_w is None else ws, grad_output

    def sgd_step_(self, lS_o, lS_i, grad_output, lr: float, lS_w=None, multi_table: bool = False, order: str = "position",
                  stochastic_rounding: bool = False, sr_seed: int = 0):
        """PoolingEmbeddingBag.sgd_step_ for all tables in one call.  grad_output: a list of [B, m_k] gradients, or the ONE
        [B, sum(m)] gradient of a concat=True forward, which is read in place (each table's columns through the row stride).
        multi_table and order: as enable_fused_sgd.  stochastic_rounding / sr_seed: this one step rounds stochastically, at the model's
        sr_step, which it advances by the number of tables stepped."""
        idx, off, ws, g = self._inputs_on_device(lS_o, lS_i, grad_output, lS_w)
        self._step(idx, off, g, float(lr), ws, multi=multi_table, order=order, sr_seed=int(sr_seed) if stochastic_rounding else False)
        return self

    def adagrad_step_(self, lS_o, lS_i, grad_output, lr: float, eps: float = 1e-10, lS_w=None, multi_table: bool = False,
                      order: str = "position", stochastic_rounding: bool = False, sr_seed: int = 0):
        """PoolingEmbeddingBag.adagrad_step_ for all tables in one call, on the bags' states; grad_output as sgd_step_ takes it: the
        ONE [B, sum(m)] gradient of a concat=True forward is read in place.  multi_table and order: as enable_fused_sgd;
        stochastic_rounding / sr_seed: as sgd_step_."""
        idx, off, ws, g = self._inputs_on_device(lS_o, lS_i, grad_output, lS_w)
        self._adagrad(idx, off, g, float(lr), float(eps), ws, multi=multi_table, order=order, sr_seed=int(sr_seed) if stochastic_rounding else False)
        return self

    def update_rows_(self, table: int, ids, rows):
        """PoolingEmbeddingBag.update_rows_ on table number `table` of the model (its position in the module list)."""
        self.bags[table].update_rows_(ids, rows)
        return self


__all__ = ["EmbeddingBag", "FusedEmbeddingBags", "PoolingEmbeddingBag", "FusedPoolingEmbeddingBags", "default_engine"]
_ = _l  # (lib is imported for its side effect: torch first, then libpimemb.so)
