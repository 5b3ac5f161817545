"""Probe of the gradient of per_sample_weights (profiles/psw/README.md): what one emb_grad_weights (include/pimemb_grad.h) costs on the
GPU, called with device pointers, next to torch's own GPU backward of per_sample_weights on the same batch and to the forward
pooled lookup of the same batch, which gathers the same rows -- the floor.

Shapes (one table each):
  uniform   dim 128, 32 indices per bag, 2048 bags, ids uniform over 4 194 304 rows     fp32 and bf16 tables
  zipf      the same with Zipf-skewed ids (workloads.zipf_indices)                      fp32 and bf16 tables
  kaggle    dim 16, one index per bag, 39 292 bags, ids uniform over 10 131 227 rows    fp32 table
Per shape ONE process warms every measurement up and then times them in turn, --repeats rounds over, device events around --iters
back-to-back calls; every figure of every round is kept, the medians and the spread are printed:
  psw         emb_grad_weights through ctypes, its descriptor built once
  forward     the prepared lookup over the same batch (Plan.time_us)
  torch       F.embedding_bag(mode="sum", per_sample_weights=w) forward + backward with only w requiring grad, and the forward
              alone: the difference is torch's backward of the weights
Every shape runs as a child process under its own time limit; the probe stops at the first one that fails or runs out of time.

    python tools/psw_probe.py --out psw_probe.json
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
SHAPES = {"uniform": (4 << 20, 128, 32, 2048), "zipf": (4 << 20, 128, 32, 2048), "kaggle": (10131227, 16, 1, 39292)}      # rows, dim, L, B


def run_step(name, args):
    import torch
    import torch.nn.functional as Fn
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("psw_probe needs the GPU: nothing here is a CPU measurement")
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
    psw = torch.rand((n,), device="cuda") + 0.5
    eng = pel.EmbeddingEngine(device=0, max_tables=2)
    eng.load_table(0, w)
    ctx = eng.grad_context(n, B)
    counts = np.unique(ids, return_counts=True)[1]
    rec = {"step": name, "rows": rows, "dim": dim, "indices_per_bag": L, "bags": B, "unique_rows": int(counts.size), "longest_run": int(counts.max()),
           "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters      # us per call

    desc, keep = pel.lib.EmbGradDesc(), []
    itype, _dev = ctx._desc(desc, 0, idx, off, G, "sum", None, None, 0, keep)
    dw = torch.empty((n,), dtype=torch.float32, device="cuda")
    outs = (C.c_void_p * 1)(dw.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream

    def psw_call():
        pel.lib.check_grad(ctx._G.emb_grad_weights(ctx._h, C.byref(desc), outs, 1, itype, stream))
    plan = eng.plan([0], [idx], [off])
    wt = psw.clone().requires_grad_(True)
    Gt = G.to(tdt)
    pt = psw.to(tdt)

    def torch_fwd_bwd():
        wt.grad = None
        Fn.embedding_bag(idx, w, off, mode="sum", per_sample_weights=wt.to(tdt)).backward(Gt)

    def torch_fwd():
        with torch.no_grad():
            Fn.embedding_bag(idx, w, off, mode="sum", per_sample_weights=pt)
    runs = {"psw": lambda: timed(psw_call), "forward": lambda: plan.time_us(0, args.iters)}
    try:                                                 # (this torch has no bfloat16 backward of per_sample_weights on the GPU: said, not timed)
        torch_fwd_bwd()
        runs.update(torch_fwd_bwd=lambda: timed(torch_fwd_bwd), torch_fwd=lambda: timed(torch_fwd))
    except NotImplementedError as ex:
        rec["torch"] = "not implemented: " + str(ex)
    for _ in range(args.warmup):                         # every shape is warmed up: code objects loaded, torch's caches filled
        psw_call()
        if "torch_fwd" in runs:
            torch_fwd_bwd()
            torch_fwd()
    plan.time_us(args.warmup, 1)
    us = {k: [] for k in runs}
    for _ in range(args.repeats):                        # in turn: a drift of the machine lands on every figure alike
        for k, run in runs.items():
            us[k].append(float(run()))
    if "torch_fwd" in us:
        us["torch_bwd"] = [a - b for a, b in zip(us["torch_fwd_bwd"], us["torch_fwd"])]
    assert ctx.report() == 0
    rec["us"] = us
    print(json.dumps(rec))
    plan.destroy()
    ctx.close()
    eng.close()
    return rec


def median(v):
    return float(np.median(v))


def print_rec(rec):
    us = rec["us"]
    m = {k: median(v) for k, v in us.items()}
    spread = lambda k: f"{m[k]:8.1f} ({min(us[k]):.1f} .. {max(us[k]):.1f})"  # noqa: E731
    vf = m["psw"] / m["forward"]
    if "torch_bwd" in m:
        vt = m["psw"] / m["torch_bwd"]
        torch_text = f"{spread('torch_bwd')}: {vt:.2f}x ({'SLOWER' if vt > 1 else 'faster'})"
    else:
        torch_text = rec.get("torch", "not timed")
    print(f"{rec['step']:13s} us per call, median of {rec['repeats']} (min .. max):  emb_grad_weights {spread('psw')}   torch's backward of the weights "
          f"{torch_text}   forward lookup {spread('forward')}: {vf:.2f}x the floor"
          f"{' (SLOWER)' if vf > 1 else ''}   longest run {rec['longest_run']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run this one shape in this process: " + ", ".join(STEPS))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
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
