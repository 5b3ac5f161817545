"""Probe of the max-mode backward (profiles/grad_max/README.md): what one emb_grad_max_sgd (include/pimemb_grad.h) costs on the GPU, called
with device pointers, next to
  (a) sum_sgd     emb_grad_sgd in SUM mode on the same batch and context: existing code, the natural floor -- the max step adds one
                  launch (the winners) and doubles the bytes of the run walk
  (b) torch       torch's GPU F.embedding_bag(mode="max") backward (forward + backward minus the forward alone) plus a dense SGD step
                  over the whole weight: what training that table costs without this library
  (c) winners     emb_grad_max_winners alone, against `forward`, the prepared max-mode lookup of the same batch, which gathers the same rows

Shapes (one table each):
  uniform   dim 128, 32 indices per bag, 2048 bags, ids uniform over 4 194 304 rows     fp32 and bf16 tables, position-order context
  zipf      the same with Zipf-skewed ids (workloads.zipf_indices)                      fp32 and bf16 tables, segmented context (S = 64)
  kaggle    dim 16, one index per bag, 39 292 bags, ids uniform over 10 131 227 rows    fp32 table, position-order context
Per shape ONE process warms every measurement up and then times them in turn, --repeats rounds over, device events around --iters
back-to-back calls; every figure of every round is kept, the medians and the spread are printed.  Every shape runs as a child process
under its own time limit; the probe stops at the first one that fails or runs out of time.

    python tools/max_grad_probe.py --out max_grad_probe.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["uniform-f32", "uniform-bf16", "zipf-f32", "zipf-bf16", "kaggle-f32"]
STEP_LIMIT_S = 240
SEGMENT = 64
LR = 1e-4
SHAPES = {"uniform": (4 << 20, 128, 32, 2048), "zipf": (4 << 20, 128, 32, 2048), "kaggle": (10131227, 16, 1, 39292)}      # rows, dim, L, B


def run_step(name, args):
    import torch
    import torch.nn.functional as Fn
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("max_grad_probe needs the GPU: nothing here is a CPU measurement")
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
    ctx = eng.grad_context(n, B, **(dict(order="segmented", segment=SEGMENT, max_dim=dim) if shape == "zipf" else {}))
    counts = np.unique(ids, return_counts=True)[1]
    rec = {"step": name, "rows": rows, "dim": dim, "indices_per_bag": L, "bags": B, "unique_rows": int(counts.size), "longest_run": int(counts.max()),
           "order": ctx.order, "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters      # us per call

    keep, d_max, d_sum = [], pel.lib.EmbGradDesc(), pel.lib.EmbGradDesc()
    itype, _dev = ctx._desc(d_max, 0, idx, off, G, "max", None, None, 0, keep)
    ctx._desc(d_sum, 0, idx, off, G, "sum", None, None, 0, keep)
    win = torch.empty((B, dim), dtype=torch.int32, device="cuda")
    wins = (C.c_void_p * 1)(win.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    Gm = ctx._G

    def max_sgd():
        pel.lib.check_grad(Gm.emb_grad_max_sgd(ctx._h, C.byref(d_max), wins, 1, itype, LR, stream))

    def sum_sgd():
        pel.lib.check_grad(Gm.emb_grad_sgd(ctx._h, C.byref(d_sum), 1, itype, LR, stream))

    def winners():
        pel.lib.check_grad(Gm.emb_grad_max_winners(ctx._h, C.byref(d_max), wins, 1, itype, stream))
    plan = eng.plan_pooled([0], [idx], [off], "max")
    wt = w.clone().requires_grad_(True)
    Gt = G.to(tdt)

    def torch_fwd_bwd_step():
        wt.grad = None
        Fn.embedding_bag(idx, wt, off, mode="max").backward(Gt)
        with torch.no_grad():
            wt.add_(wt.grad, alpha=-LR)

    def torch_fwd():
        with torch.no_grad():
            Fn.embedding_bag(idx, wt, off, mode="max")
    runs = {"max_sgd": lambda: timed(max_sgd), "sum_sgd": lambda: timed(sum_sgd), "winners": lambda: timed(winners),
            "forward": lambda: plan.time_us(0, args.iters)}
    try:                                                 # (a torch without this backward for the dtype: said, not timed)
        torch_fwd_bwd_step()
        runs.update(torch_fwd_bwd_step=lambda: timed(torch_fwd_bwd_step), torch_fwd=lambda: timed(torch_fwd))
    except (NotImplementedError, RuntimeError) as ex:
        rec["torch"] = "not timed: " + str(ex).splitlines()[0]
    for _ in range(args.warmup):                         # every shape is warmed up: code objects loaded, torch's caches filled
        max_sgd()
        sum_sgd()
        winners()
        if "torch_fwd" in runs:
            torch_fwd_bwd_step()
            torch_fwd()
    plan.time_us(args.warmup, 1)
    us = {k: [] for k in runs}
    for _ in range(args.repeats):                        # in turn: a drift of the machine lands on every figure alike
        for k, run in runs.items():
            us[k].append(float(run()))
    if "torch_fwd" in us:
        us["torch_bwd_step"] = [a - b for a, b in zip(us["torch_fwd_bwd_step"], us["torch_fwd"])]
    assert ctx.report() == 0
    rec["us"] = us
    print(json.dumps(rec))
    plan.destroy()
    ctx.close()
    eng.close()
    return rec


def median_spread(v):
    return {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))}


def ratio_text(a, b):
    """a against b: how many times, and which way, with SLOWER written out."""
    r = a / b
    return f"{r:.2f}x SLOWER" if r > 1 else f"{1 / r:.2f}x faster"


def print_rec(rec):
    us = rec["us"]
    m = {k: median_spread(v) for k, v in us.items()}
    spread = lambda k: f"{m[k]['median_us']:8.1f} ({m[k]['min_us']:.1f} .. {m[k]['max_us']:.1f})"  # noqa: E731
    med = lambda k: m[k]["median_us"]  # noqa: E731
    torch_text = f"{spread('torch_bwd_step')}: max_sgd is {ratio_text(med('max_sgd'), med('torch_bwd_step'))}" if "torch_bwd_step" in m else rec.get("torch", "")
    print(f"{rec['step']:13s} ({rec['order']}) us per call, median of {rec['repeats']} (min .. max):  emb_grad_max_sgd {spread('max_sgd')}   "
          f"(a) emb_grad_sgd, sum mode {spread('sum_sgd')}: max_sgd is {ratio_text(med('max_sgd'), med('sum_sgd'))}   "
          f"(b) torch's backward + dense SGD {torch_text}   "
          f"(c) winners {spread('winners')} against the forward max lookup {spread('forward')}: {ratio_text(med('winners'), med('forward'))}   "
          f"longest run {rec['longest_run']}", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run this one shape in this process: " + ", ".join(STEPS))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    unknown = [s for s in ([args.step] if args.step else args.steps.split(",")) if s not in STEPS]
    if unknown:
        raise SystemExit(f"unknown step {unknown[0]!r}: one of {', '.join(STEPS)}")
    if args.step:
        run_step(args.step, args)
        return 0
    results = []
    for name in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(args.iters), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
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
        print_rec(rec)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
