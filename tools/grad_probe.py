"""Backward-pass probe (profiles/grad/README.md): what one fused SGD step (emb_grad_sgd, include/pimemb_grad.h) costs on the GPU,
next to torch's own sparse backward + SGD and to the forward lookup over the same batch.

Shapes (one table each):
  uniform   dim 128, 32 indices per bag, 2048 bags, ids uniform over 4 194 304 rows     fp32 and bf16 tables
  zipf      the same with Zipf-skewed ids (workloads.zipf_indices)                      fp32 and bf16 tables
  kaggle    dim 16, one index per bag, 39 292 bags, ids uniform over 10 131 227 rows    fp32 table
Per shape and dtype, device events around --iters back-to-back calls after --warmup untimed ones:
  step        GradContext.sgd_step: pre-pass (bags, sort) + the fused row kernel
  torch       nn.EmbeddingBag(sparse=True) forward + backward + torch.optim.SGD.step(), and its forward alone: the difference is
              torch's backward + optimizer
  forward     emb_plan_time of the lookup over the same batch (the parent commit's kernels): the backward moves about the same
              gradient bytes, plus the sort
The pre-pass's share of a step is a kernel-trace matter (the step is one enqueue of many kernels): run one shape under
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/grad_probe.py --step uniform-f32 --only-step
and add up the grad_classify / grad_sort_* / grad_scan_* rows against grad_rows_*.

Without --step every measurement runs as a child process of its own under its own time limit, and the probe stops at the
first one that fails or runs out of time.

    python tools/grad_probe.py --out grad_probe.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["uniform-f32", "uniform-bf16", "zipf-f32", "zipf-bf16", "kaggle-f32"]
STEP_LIMIT_S = 240
SHAPES = {"uniform": (4 << 20, 128, 32, 2048), "zipf": (4 << 20, 128, 32, 2048), "kaggle": (10131227, 16, 1, 39292)}      # rows, dim, L, B


def run_step(name, args):
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("grad_probe needs the GPU: nothing here is a CPU measurement")
    shape, kind = name.split("-")
    rows, dim, L, B = SHAPES[shape]
    rng = np.random.default_rng(0)
    n = B * L
    ids = pel.workloads.zipf_indices(rng, rows, n) if shape == "zipf" else pel.workloads.uniform_indices(rng, rows, n)
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    off = torch.arange(0, n, L, dtype=torch.int64, device="cuda")
    G = torch.randn((B, dim), device="cuda") * 1e-3
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[kind]
    w = (torch.randn((rows, dim), device="cuda") * 0.05).to(tdt)
    eng = pel.EmbeddingEngine(device=0, max_tables=2)
    eng.load_table(0, w)
    ctx = eng.grad_context(n, B)
    counts = np.unique(ids, return_counts=True)[1]
    rec = {"step": name, "rows": rows, "dim": dim, "indices_per_bag": L, "bags": B, "unique_rows": int(counts.size), "longest_run": int(counts.max())}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters      # us per call

    rec["step_us"] = timed(lambda: ctx.sgd_step([0], [idx], [off], [G], 0.01))
    assert ctx.report() == 0
    if args.only_step:
        print(json.dumps(rec))
        return rec
    plan = eng.plan([0], [idx], [off])
    rec["forward_us"] = plan.time_us(args.warmup, args.iters)
    plan.destroy()
    bag = torch.nn.EmbeddingBag(rows, dim, mode="sum", sparse=True, _weight=w.clone()).cuda()
    opt = torch.optim.SGD(bag.parameters(), lr=0.01)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        bag(idx, off).backward(G.to(tdt))
        opt.step()
    rec["torch_fwd_bwd_sgd_us"] = timed(torch_step)
    with torch.no_grad():
        rec["torch_fwd_us"] = timed(lambda: bag(idx, off))
    rec["torch_bwd_sgd_us"] = rec["torch_fwd_bwd_sgd_us"] - rec["torch_fwd_us"]
    rec["step_over_torch"] = rec["step_us"] / rec["torch_bwd_sgd_us"]
    rec["step_over_forward"] = rec["step_us"] / rec["forward_us"]
    rec["verdict_vs_torch"] = "SLOWER" if rec["step_over_torch"] > 1 else "faster"
    print(json.dumps(rec))
    ctx.close()
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run this one measurement in this process: " + ", ".join(STEPS))
    ap.add_argument("--only-step", action="store_true", help="time the fused step alone (for a kernel trace)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.step:
        run_step(args.step, args)
        return 0
    results = []
    for name in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(args.iters), "--warmup", str(args.warmup)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {STEP_LIMIT_S} s -- stopping here", flush=True)
            return 1
        if res.returncode != 0:
            print(f"{name}: exit status {res.returncode} -- stopping here\n{res.stdout[-2000:]}", flush=True)
            return 1
        rec = json.loads(res.stdout.strip().splitlines()[-1])
        results.append(rec)
        print(f"{name:13s} step {rec['step_us']:8.1f} us   torch bwd+sgd {rec['torch_bwd_sgd_us']:8.1f} us ({rec['step_over_torch']:.2f}x, "
              f"{rec['verdict_vs_torch']})   forward lookup {rec['forward_us']:7.1f} us ({rec['step_over_forward']:.1f}x the forward)   "
              f"{rec['unique_rows']} unique rows, longest run {rec['longest_run']}", flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
