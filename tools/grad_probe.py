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

--order both (profiles/grad_segmented/README.md): the segmented order of additions next to the position order.  Per shape ONE
process times, in turn and --repeats times over, the step on a position-order context, on a segmented context per --segment
length, and torch's forward + backward + SGD and forward alone; every figure of every round is kept, so that the spread is on
the record.  The shapes are the five above and two of tools/grad_multi_probe.py -- kaggle8-f32 and kaggle26-f32: 8 / 26 tables
with the Criteo-Kaggle row counts, dim 16, 39 292 one-index bags each -- which are stepped table by table ("single") and by the
multi-table step ("multi").  --order segmented leaves the position-order context out.

    python tools/grad_probe.py --order both --segment 16,32,64,128,256 --repeats 5 --out grad_segmented_probe.json
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
MULTI_STEPS = ["kaggle8-f32", "kaggle26-f32"]          # --order both / segmented only
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


def run_orders(name, args):
    """--order both / segmented: one shape, every context and torch timed in turn, --repeats rounds: {"us": {what: [us per call, ...]}}."""
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("grad_probe needs the GPU: nothing here is a CPU measurement")
    shape, kind = name.split("-")
    if shape in ("kaggle8", "kaggle26"):
        rows_all = [r for r in pel.workloads.KAGGLE_ROWS if shape == "kaggle26" or r > pel.workloads.KAGGLE_BATCH]
        dim, L, B = pel.workloads.KAGGLE_DIM, 1, pel.workloads.KAGGLE_BATCH
    else:
        rows, dim, L, B = SHAPES[shape]
        rows_all = [rows]
    T, n = len(rows_all), B * L
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[kind]
    rng = np.random.default_rng(0)
    eng = pel.EmbeddingEngine(device=0, max_tables=T)
    tabs, idx, off, G, ws, longest, unique = list(range(T)), [], [], [], [], 0, 0
    for t, nr in enumerate(rows_all):
        ids = pel.workloads.zipf_indices(rng, nr, n) if shape == "zipf" else pel.workloads.uniform_indices(rng, nr, n)
        counts = np.unique(ids, return_counts=True)[1]
        longest, unique = max(longest, int(counts.max())), unique + int(counts.size)
        idx.append(torch.from_numpy(ids.astype(np.int64)).cuda())
        off.append(torch.arange(0, n, L, dtype=torch.int64, device="cuda"))
        G.append(torch.randn((B, dim), device="cuda") * 1e-3)
        ws.append((torch.randn((nr, dim), device="cuda") * 0.05).to(tdt))
        eng.load_table(t, ws[t])
    segments = [int(x) for x in args.segment.split(",")]
    ctxs = {} if args.order == "segmented" else {"position": eng.grad_context(T * n, T * B)}
    for S in segments:
        ctxs[f"segmented_{S}"] = eng.grad_context(T * n, T * B, order="segmented", segment=S, max_dim=dim)
    rec = {"step": name, "tables": T, "rows_total": int(sum(rows_all)), "dim": dim, "indices_per_bag": L, "bags_per_table": B, "unique_rows": unique,
           "longest_run": longest, "segments": segments, "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats}

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

    def step(ctx, multi):
        return lambda: ctx.sgd_step(tabs, idx, off, G, 0.01, multi=multi)
    runs = {}
    for what, ctx in ctxs.items():
        runs[what + ("_single" if T > 1 else "")] = step(ctx, False)
        if T > 1:
            runs[what + "_multi"] = step(ctx, True)
    if not args.only_step:
        bags = [torch.nn.EmbeddingBag(nr, dim, mode="sum", sparse=True, _weight=ws[t].clone()).cuda() for t, nr in enumerate(rows_all)]
        opt = torch.optim.SGD([p for b in bags for p in b.parameters()], lr=0.01)
        Gt = [g.to(tdt) for g in G]

        def torch_fwd():
            return [b(idx[t], off[t]) for t, b in enumerate(bags)]

        def torch_step():
            opt.zero_grad(set_to_none=True)
            torch.autograd.backward(torch_fwd(), Gt)
            opt.step()

        def torch_fwd_only():
            with torch.no_grad():
                torch_fwd()
        runs["torch_fwd_bwd_sgd"], runs["torch_fwd"] = torch_step, torch_fwd_only
    us = {k: [] for k in runs}
    for _ in range(args.repeats):                        # in turn: a drift of the machine lands on every figure alike
        for k, run in runs.items():
            us[k].append(timed(run))
    for ctx in ctxs.values():
        assert ctx.report() == 0
        ctx.close()
    if not args.only_step:
        us["torch_bwd_sgd"] = [a - b for a, b in zip(us["torch_fwd_bwd_sgd"], us["torch_fwd"])]
    rec["us"] = us
    print(json.dumps(rec))
    eng.close()
    return rec


def median(v):
    return float(np.median(v))


def print_orders(rec):
    us = rec["us"]
    print(f"{rec['step']:13s} {rec['tables']} table(s), {rec['unique_rows']} unique rows, longest run {rec['longest_run']}; us per step, median of "
          f"{rec['repeats']} (min .. max):", flush=True)
    torch_us = median(us["torch_bwd_sgd"]) if "torch_bwd_sgd" in us else None
    for k, v in us.items():
        if k in ("torch_fwd_bwd_sgd", "torch_fwd"):
            continue
        flavour = k.split("_")[-1] if k.endswith(("_single", "_multi")) else ""
        base = us.get("position" + ("_" + flavour if flavour else ""))
        line = f"    {k:24s} {median(v):9.1f}  ({min(v):9.1f} .. {max(v):9.1f})"
        if base and not k.startswith(("position", "torch")):
            r = median(v) / median(base)
            line += f"   {r:6.3f}x the position order ({'SLOWER' if r > 1 else 'faster'})"
        if torch_us and not k.startswith("torch"):
            r = median(v) / torch_us
            line += f"   {r:6.2f}x torch ({'SLOWER' if r > 1 else 'faster'})"
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run this one measurement in this process: " + ", ".join(STEPS))
    ap.add_argument("--only-step", action="store_true", help="time the fused step alone (for a kernel trace)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--out", default="")
    ap.add_argument("--order", default="position", choices=["position", "segmented", "both"],
                    help="segmented / both: time contexts of the segmented order of additions (both: next to a position-order one), in turn, --repeats times")
    ap.add_argument("--segment", default="64", help="--order segmented / both: the segment lengths to time, e.g. 16,32,64")
    ap.add_argument("--repeats", type=int, default=5, help="--order segmented / both: rounds over all contexts and torch")
    args = ap.parse_args()
    orders = args.order != "position"
    if args.step:
        (run_orders if orders else run_step)(args.step, args)
        return 0
    results = []
    steps = args.steps if args.steps != ",".join(STEPS) or not orders else ",".join(STEPS + MULTI_STEPS)
    for name in steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(args.iters), "--warmup", str(args.warmup)]
        if orders:
            cmd += ["--order", args.order, "--segment", args.segment, "--repeats", str(args.repeats)]
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
        if orders:
            print_orders(rec)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)
            continue
        print(f"{name:13s} step {rec['step_us']:8.1f} us   torch bwd+sgd {rec['torch_bwd_sgd_us']:8.1f} us ({rec['step_over_torch']:.2f}x, "
              f"{rec['verdict_vs_torch']})   forward lookup {rec['forward_us']:7.1f} us ({rec['step_over_forward']:.1f}x the forward)   "
              f"{rec['unique_rows']} unique rows, longest run {rec['longest_run']}", flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
