"""Adam step probe (profiles/adam/README.md): what one fused SparseAdam / row-wise Adam step (emb_grad_adam_step, include/pimemb_grad.h;
GradContext.adam_step) costs on the GPU next to the Adagrad steps of the same batch and next to torch.

Shapes (one table each, device pointers only; tools/sr_probe.py's):
  uniform   dim 128, 32 indices per bag, 2048 bags, ids uniform over 4 194 304 rows     f32, bf16
  zipf      the same with Zipf-skewed ids, on an S = 64 context                          f32, bf16
  kaggle    dim 16, one index per bag, 39 292 bags, ids uniform over 10 131 227 rows    f32, bf16
Per shape and dtype ONE process times, in turn and --repeats times over (alternating rounds; every figure of every round is kept, so
that the spread is on the record), device events around --iters back-to-back calls after --warmup untimed ones:
  adam             GradContext.adam_step: the pre-pass, and the tail over the table piece, exp_avg and exp_avg_sq
  rowwise-adam     GradContext.adam_step(rowwise=True)
  adagrad          GradContext.adagrad_step on a table and a state of its own
  rowwise-adagrad  GradContext.adagrad_step(rowwise=True) likewise
  torch            f32 only: the backward of torch.nn.EmbeddingBag(sparse=True) on the GPU plus torch.optim.SparseAdam.step()
The Adagrad steps run through kernels this probe's commit does not change, so one build gives all sides.

Without --step every measurement runs as a child process of its own under its own time limit, and the probe stops at the first one
that fails or runs out of time.

    python tools/adam_probe.py --out adam_probe.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"f32": "EMB_F32", "bf16": "EMB_BF16"}
SHAPES = {"uniform": (4 << 20, 128, 32, 2048), "zipf": (4 << 20, 128, 32, 2048), "kaggle": (10131227, 16, 1, 39292)}      # rows, dim, L, B
STEPS = [f"{s}-{k}" for s in SHAPES for k in KINDS]
STEP_LIMIT_S = 240
LR = 1e-3
SEGMENT = 64


def median_spread(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1], "rounds": xs}


def run_step(name, args):
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("adam_probe needs the GPU: nothing here is a CPU measurement")
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
    T_ADAM, T_ROWWISE_ADAM, T_ADAGRAD, T_ROWWISE_ADAGRAD = 0, 1, 2, 3
    for t in range(4):
        eng.load_table_f32(t, w, code)
    zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    m, v, m_row, v_row, s_full, s_row = zeros(rows, dim), zeros(rows, dim), zeros(rows, dim), zeros(rows), zeros(rows, dim), zeros(rows)
    ctx = eng.grad_context(n, B, order="segmented", segment=SEGMENT, max_dim=dim) if shape == "zipf" else eng.grad_context(n, B)
    stream = torch.cuda.current_stream().cuda_stream
    step = [0]

    def t_next():
        step[0] += 1
        return step[0]

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

    what = {
        "adam": lambda: ctx.adam_step([T_ADAM], [idx], [off], [G], [m], [v], LR, step=t_next(), stream=stream),
        "rowwise-adam": lambda: ctx.adam_step([T_ROWWISE_ADAM], [idx], [off], [G], [m_row], [v_row], LR, step=t_next(), rowwise=True, stream=stream),
        "adagrad": lambda: ctx.adagrad_step([T_ADAGRAD], [idx], [off], [G], [s_full], LR, stream=stream),
        "rowwise-adagrad": lambda: ctx.adagrad_step([T_ROWWISE_ADAGRAD], [idx], [off], [G], [s_row], LR, rowwise=True, stream=stream),
    }
    if kind == "f32":
        bag = torch.nn.EmbeddingBag(rows, dim, mode="sum", sparse=True, _weight=w).cuda()
        opt = torch.optim.SparseAdam(bag.parameters(), lr=LR)
        pooled = bag(idx, off)

        def torch_step():
            opt.zero_grad()
            pooled.backward(G, retain_graph=True)
            opt.step()
        what["torch"] = torch_step
    figures = {k: [] for k in what}
    for _round in range(args.repeats):                   # alternating: one figure of everything per round
        for k, fn in what.items():
            figures[k].append(timed(fn))
    out = {"step": name, "rows": rows, "dim": dim, "bags": B, "per_bag": L, "iters": args.iters, "warmup": args.warmup, "context": ctx.order,
           "longest_run": int(np.bincount(ids.astype(np.int64)).max()), "figures": {k: median_spread(x) for k, x in figures.items()}}
    med = lambda k: out["figures"][k]["median_us"]  # noqa: E731
    out["adam_over_adagrad"] = med("adam") / med("adagrad")
    out["rowwise_adam_over_rowwise_adagrad"] = med("rowwise-adam") / med("rowwise-adagrad")
    if "torch" in what:
        out["torch_over_adam"] = med("torch") / med("adam")
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
