"""Stochastic-rounding step probe (profiles/sr/README.md): what one stochastically rounded step (emb_grad_sgd_sr / emb_grad_step_sr,
include/pimemb_grad.h; GradContext.sgd_step / adagrad_step with sr=) costs on the GPU next to its two neighbours.

Shapes (one table each, device pointers only; tools/master_probe.py's):
  uniform   dim 128, 32 indices per bag, 2048 bags, ids uniform over 4 194 304 rows     bf16, f16
  zipf      the same with Zipf-skewed ids, on a position-order and on an S = 64 context  bf16, f16
  kaggle    dim 16, one index per bag, 39 292 bags, ids uniform over 10 131 227 rows    bf16, f16
Per shape and dtype ONE process times, in turn and --repeats times over (alternating rounds; every figure of every round is kept,
so that the spread is on the record), device events around --iters back-to-back calls after --warmup untimed ones:
  sr-sgd      GradContext.sgd_step(sr=(seed, step)): the pre-pass, and the tail with one Philox block per piece
  sr-rowwise  GradContext.adagrad_step(rowwise=True, sr=...)
  inplace     GradContext.sgd_step on a table of its own: the same step rounded to nearest  (2 + 2 bytes per stepped element, as sr)
  inplace-rowwise   GradContext.adagrad_step(rowwise=True) likewise
  master      bf16 only: GradContext.master_step(optimizer="sgd") on a table and an fp32 master of its own  (4 + 4 + 2 bytes)
The in-place and the master step run through kernels this probe's commit does not change, so one build gives all sides.

Without --step every measurement runs as a child process of its own under its own time limit, and the probe stops at the first
one that fails or runs out of time.

    python tools/sr_probe.py --out sr_probe.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"bf16": "EMB_BF16", "f16": "EMB_F16"}
SHAPES = {"uniform": (4 << 20, 128, 32, 2048), "zipf": (4 << 20, 128, 32, 2048), "kaggle": (10131227, 16, 1, 39292)}      # rows, dim, L, B
STEPS = [f"{s}-{k}" for s in SHAPES for k in KINDS]
STEP_LIMIT_S = 240
LR = 1e-3
SEGMENT = 64
SEED = 0x5EED0123456789AB


def median_spread(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1], "rounds": xs}


def run_step(name, args):
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("sr_probe needs the GPU: nothing here is a CPU measurement")
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
    T_SR, T_INPLACE, T_MASTER = 0, 1, 2
    eng.load_table_f32(T_SR, w, code)
    eng.load_table_f32(T_INPLACE, w, code)
    master = None
    if kind == "bf16":
        eng.load_table_f32(T_MASTER, w, code)
        master = w.clone()
    del w
    state_sr = torch.zeros((rows,), dtype=torch.float32, device="cuda")
    state_plain = torch.zeros((rows,), dtype=torch.float32, device="cuda")
    contexts = {"position": eng.grad_context(n, B)}
    if shape == "zipf":
        contexts[f"S{SEGMENT}"] = eng.grad_context(n, B, order="segmented", segment=SEGMENT, max_dim=dim)
    stream = torch.cuda.current_stream().cuda_stream
    step = [0]

    def sr():
        step[0] += 1
        return (SEED, step[0])

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
        what[f"sr-sgd@{cname}"] = lambda ctx=ctx: ctx.sgd_step([T_SR], [idx], [off], [G], LR, stream=stream, sr=sr())
        what[f"inplace@{cname}"] = lambda ctx=ctx: ctx.sgd_step([T_INPLACE], [idx], [off], [G], LR, stream=stream)
        what[f"sr-rowwise@{cname}"] = lambda ctx=ctx: ctx.adagrad_step([T_SR], [idx], [off], [G], [state_sr], LR, rowwise=True, stream=stream, sr=sr())
        what[f"inplace-rowwise@{cname}"] = lambda ctx=ctx: ctx.adagrad_step([T_INPLACE], [idx], [off], [G], [state_plain], LR, rowwise=True, stream=stream)
        if master is not None:
            what[f"master@{cname}"] = lambda ctx=ctx: ctx.master_step([T_MASTER], [idx], [off], [G], [master], LR, optimizer="sgd", stream=stream)
    figures = {k: [] for k in what}
    for _round in range(args.repeats):                   # alternating: one figure of everything per round
        for k, fn in what.items():
            figures[k].append(timed(fn))
    out = {"step": name, "rows": rows, "dim": dim, "bags": B, "per_bag": L, "iters": args.iters, "warmup": args.warmup,
           "longest_run": int(np.bincount(ids.astype(np.int64)).max()), "figures": {k: median_spread(v) for k, v in figures.items()}}
    med = lambda k: out["figures"][k]["median_us"]  # noqa: E731
    for cname in contexts:
        out[f"sr_over_inplace@{cname}"] = med(f"sr-sgd@{cname}") / med(f"inplace@{cname}")
        out[f"sr_rowwise_over_inplace_rowwise@{cname}"] = med(f"sr-rowwise@{cname}") / med(f"inplace-rowwise@{cname}")
        if master is not None:
            out[f"sr_over_master@{cname}"] = med(f"sr-sgd@{cname}") / med(f"master@{cname}")
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
