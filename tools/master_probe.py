"""Master-weight step probe (profiles/master/README.md): what one fused master-weight step (emb_grad_master_step,
include/pimemb_grad.h; GradContext.master_step, SGD) costs on the GPU next to what it replaces.

Shapes (one table each, device pointers only; tools/grad_probe.py's):
  uniform   dim 128, 32 indices per bag, 2048 bags, ids uniform over 4 194 304 rows     bf16, e4m3, mxfp4
  zipf      the same with Zipf-skewed ids, on a position-order and on an S = 64 context  bf16, e4m3, mxfp4
  kaggle    dim 16, one index per bag, 39 292 bags, ids uniform over 10 131 227 rows    bf16, e4m3 (MXFP4 needs dim % 32 == 0)
Per shape and dtype ONE process times, in turn and --repeats times over (alternating rounds; every figure of every round is kept,
so that the spread is on the record), device events around --iters back-to-back calls after --warmup untimed ones:
  master      GradContext.master_step(optimizer="sgd"): the pre-pass, and the master tail
  recipe      (a) the no-wait recipe of the README, which the fused step replaces: rows_out.fill_(-1), emb_grad_sparse, torch.where,
              the product, the gather and subtraction, index_copy_ into the master, RowWriter.update of all n slots -- on a table
              and a master of its own
  inplace     (b) bf16 only: GradContext.sgd_step on a bf16 table of its own -- the price of the master's extra 8 bytes per element
The recipe and the in-place step run through code this probe's commit does not change (their kernels keep the machine code of the
commit before the master step: tests/test_psw_cpu.py and the hash comparison of the commit message), so one build gives both sides.
The table and the master of the 4 M x 128 shapes are 0.25 - 1 GB and 2 GB; the recipe's own pair doubles that.

Without --step every measurement runs as a child process of its own under its own time limit, and the probe stops at the first
one that fails or runs out of time.

    python tools/master_probe.py --out master_probe.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"bf16": "EMB_BF16", "e4m3": "EMB_F8_E4M3", "mxfp4": "EMB_MXFP4"}
SHAPES = {"uniform": (4 << 20, 128, 32, 2048), "zipf": (4 << 20, 128, 32, 2048), "kaggle": (10131227, 16, 1, 39292)}      # rows, dim, L, B
STEPS = [f"{s}-{k}" for s in SHAPES for k in KINDS if not (s == "kaggle" and k == "mxfp4")]
STEP_LIMIT_S = 240
LR = 1e-3
SEGMENT = 64


def median_spread(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1], "rounds": xs}


def run_step(name, args):
    import ctypes as C
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("master_probe needs the GPU: nothing here is a CPU measurement")
    shape, kind = name.split("-")
    rows, dim, L, B = SHAPES[shape]
    rng = np.random.default_rng(0)
    n = B * L
    ids = pel.workloads.zipf_indices(rng, rows, n) if shape == "zipf" else pel.workloads.uniform_indices(rng, rows, n)
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    off = torch.arange(0, n, L, dtype=torch.int64, device="cuda")
    G = torch.randn((B, dim), dtype=torch.float32, device="cuda")
    code = getattr(pel.lib, KINDS[kind])
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    w = torch.randn((rows, dim), dtype=torch.float32, device="cuda") * 0.5
    T_FUSED, T_RECIPE, T_INPLACE = 0, 1, 2
    eng.load_table_f32(T_FUSED, w, code)
    eng.load_table_f32(T_RECIPE, w, code)
    master = w.clone()                                   # enc(master) is the table: it was encoded from these very rows
    spare = torch.zeros((rows + 1, dim), dtype=torch.float32, device="cuda")      # the recipe's master, with the spare row N
    spare[:rows] = w
    if kind == "bf16":
        eng.load_table_f32(T_INPLACE, w, code)
    del w
    contexts = {"position": eng.grad_context(n, B)}
    if shape == "zipf":
        contexts[f"S{SEGMENT}"] = eng.grad_context(n, B, order="segmented", segment=SEGMENT, max_dim=dim)
    writer = eng.row_writer(n)
    stream = torch.cuda.current_stream().cuda_stream
    rows_out = torch.zeros((n,), dtype=torch.int64, device="cuda")
    grads_out = torch.zeros((n, dim), dtype=torch.float32, device="cuda")
    n_unique = torch.zeros((1,), dtype=torch.int64, device="cuda")
    spare_ids = torch.full((n,), rows, dtype=torch.int64, device="cuda")

    def fused(ctx):
        ctx.master_step([T_FUSED], [idx], [off], [G], [master], LR, optimizer="sgd", stream=stream)

    def recipe(ctx):
        desc, keep = pel.lib.EmbGradDesc(), []
        itype, _dev = ctx._desc(desc, T_RECIPE, idx, off, G, "sum", None, None, 0, keep)

        def call():
            rows_out.fill_(-1)
            pel.lib.check_grad(ctx._G.emb_grad_sparse(ctx._h, C.byref(desc), itype, rows_out.data_ptr(), grads_out.data_ptr(), n, n_unique.data_ptr(), stream))
            r = torch.where(rows_out >= 0, rows_out, spare_ids)
            new = spare[r] - grads_out * LR
            spare.index_copy_(0, r, new)
            writer.update(T_RECIPE, rows_out, new, stream=stream)
        return call

    def inplace(ctx):
        ctx.sgd_step([T_INPLACE], [idx], [off], [G], LR, stream=stream)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    what = {}
    for cname, ctx in contexts.items():
        what[f"master@{cname}"] = lambda ctx=ctx: fused(ctx)
        what[f"recipe@{cname}"] = recipe(ctx)
        if kind == "bf16":
            what[f"inplace@{cname}"] = lambda ctx=ctx: inplace(ctx)
    figures = {k: [] for k in what}
    for _round in range(args.repeats):                   # alternating: one figure of everything per round
        for k, fn in what.items():
            figures[k].append(timed(fn))
    out = {"step": name, "rows": rows, "dim": dim, "bags": B, "per_bag": L, "iters": args.iters, "warmup": args.warmup,
           "longest_run": int(np.bincount(ids.astype(np.int64)).max()), "unencodable": [c.master_report() for c in contexts.values()],
           "figures": {k: median_spread(v) for k, v in figures.items()}}
    for cname in contexts:
        m, r = out["figures"][f"master@{cname}"]["median_us"], out["figures"][f"recipe@{cname}"]["median_us"]
        out[f"recipe_over_master@{cname}"] = r / m
        if kind == "bf16":
            out[f"master_over_inplace@{cname}"] = m / out["figures"][f"inplace@{cname}"]["median_us"]
    eng.close()
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one measurement in this process")
    ap.add_argument("--steps", type=str, default=",".join(STEPS), help="the measurements to run, each in a child process")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if args.step:
        run_step(args.step, args)
        return 0
    results = []
    for name in args.steps.split(","):
        if name not in STEPS:
            raise SystemExit(f"unknown step {name!r}: one of {STEPS}")
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(args.iters), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {STEP_LIMIT_S} s; stopping here", file=sys.stderr)
            break
        if res.returncode != 0:
            print(f"{name}: exit status {res.returncode}; stopping here\n{res.stderr[-2000:]}", file=sys.stderr)
            break
        results.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0 if len(results) == len(args.steps.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
