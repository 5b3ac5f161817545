"""Fused-optimizer probe (profiles/optim/README.md): what one fused Adagrad / row-wise Adagrad step (emb_grad_step,
include/pimemb_grad.h) costs on the GPU, at the three points of tools/grad_probe.py (2048 bags x 32 indices of dim 128 over 4 M
rows, uniform and Zipf ids; the Kaggle shape), on fp32 and bf16 tables, next to:
  sgd        emb_grad_sgd on the same batch: the floor -- the same pre-pass and run walk without the state traffic
  torch      nn.EmbeddingBag(sparse=True) forward + backward + torch.optim.Adagrad.step() minus its forward alone, on the GPU
             (the element-wise kind's counterpart)
  unfused    the route the row-wise step replaces: emb_grad_sparse (with its wait for the number of rows), torch ops over the
             returned rows, the state and an fp32 master copy of the table, and emb_rows_update of the new rows
Device events around --iters back-to-back calls after --warmup untimed ones; the three steps of this library alternate for
--repeats rounds in one process (median, minimum and maximum are reported: the spread); every measurement a child process under its own
time limit, and the probe stops at the first one that fails or runs out of time.

    python tools/optim_probe.py --out optim_probe.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["uniform-f32", "uniform-bf16", "zipf-f32", "zipf-bf16", "kaggle-f32", "kaggle-bf16"]
STEP_LIMIT_S = 240
SHAPES = {"uniform": (4 << 20, 128, 32, 2048), "zipf": (4 << 20, 128, 32, 2048), "kaggle": (10131227, 16, 1, 39292)}      # rows, dim, L, B
LR, EPS = 0.01, 1e-10


def run_step(name, args):
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("optim_probe needs the GPU: nothing here is a CPU measurement")
    shape, kind = name.split("-")
    rows, dim, L, B = SHAPES[shape]
    rng = np.random.default_rng(0)
    n = B * L
    ids = pel.workloads.zipf_indices(rng, rows, n) if shape == "zipf" else pel.workloads.uniform_indices(rng, rows, n)
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    off = torch.arange(0, n, L, dtype=torch.int64, device="cuda")
    G = torch.randn((B, dim), device="cuda") * 1e-3
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[kind]
    master = torch.randn((rows, dim), device="cuda") * 0.05
    eng = pel.EmbeddingEngine(device=0, max_tables=2)
    eng.load_table(0, master.to(tdt))
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

    # the three steps of this library ALTERNATE, --repeats rounds in this one process: the median of a step's rounds is its
    # figure, their minimum and maximum the spread a difference has to exceed to mean anything
    S = torch.zeros(ctx.state_shape(0, False), device="cuda")
    Sr = torch.zeros(ctx.state_shape(0, True), device="cuda")
    ours = {"sgd": lambda: ctx.sgd_step([0], [idx], [off], [G], LR),
            "adagrad": lambda: ctx.adagrad_step([0], [idx], [off], [G], [S], LR, eps=EPS),
            "rowwise": lambda: ctx.adagrad_step([0], [idx], [off], [G], [Sr], LR, eps=EPS, rowwise=True)}
    rounds = {k: [] for k in ours}
    for _ in range(args.repeats):
        for k, fn in ours.items():
            rounds[k].append(timed(fn))
    for k, v in rounds.items():
        rec[k + "_us"], rec[k + "_us_min"], rec[k + "_us_max"], rec[k + "_us_rounds"] = float(np.median(v)), min(v), max(v), v
    del S
    assert ctx.report() == 0
    # (c) the unfused row-wise route: sparse gradient, torch ops on the rows, row writer
    writer = eng.row_writer(n)

    def unfused():
        r, g = ctx.sparse_grad(0, idx, off, G)                        # (waits for the number of rows)
        s = Sr[r] + (g * g).mean(dim=1)
        Sr[r] = s
        new = master[r] - (LR / (s.sqrt() + EPS)).unsqueeze(1) * g
        master[r] = new
        writer.update(0, r, new)
    rec["rowwise_unfused_us"] = timed(unfused)
    writer.close()
    del Sr
    # (b) torch's own sparse backward + Adagrad
    bag = torch.nn.EmbeddingBag(rows, dim, mode="sum", sparse=True, _weight=master.to(tdt)).cuda()
    del master
    opt = torch.optim.Adagrad(bag.parameters(), lr=LR, eps=EPS)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        bag(idx, off).backward(G.to(tdt))
        opt.step()
    rec["torch_fwd_bwd_adagrad_us"] = timed(torch_step)
    with torch.no_grad():
        rec["torch_fwd_us"] = timed(lambda: bag(idx, off))
    rec["torch_bwd_adagrad_us"] = rec["torch_fwd_bwd_adagrad_us"] - rec["torch_fwd_us"]
    rec["adagrad_over_sgd"] = rec["adagrad_us"] / rec["sgd_us"]
    rec["rowwise_over_sgd"] = rec["rowwise_us"] / rec["sgd_us"]
    rec["adagrad_over_torch"] = rec["adagrad_us"] / rec["torch_bwd_adagrad_us"]
    rec["rowwise_over_unfused"] = rec["rowwise_us"] / rec["rowwise_unfused_us"]
    # against the floor a step counts as SLOWER only where its fastest round is slower than the floor's slowest
    for k in ("adagrad", "rowwise"):
        rec[k + "_vs_sgd"] = "SLOWER" if rec[k + "_us_min"] > rec["sgd_us_max"] else "faster" if rec[k + "_us_max"] < rec["sgd_us_min"] else "within the spread"
    rec["adagrad_vs_torch"] = "SLOWER" if rec["adagrad_over_torch"] > 1 else "faster"
    rec["rowwise_vs_unfused"] = "SLOWER" if rec["rowwise_over_unfused"] > 1 else "faster"
    print(json.dumps(rec))
    ctx.close()
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run this one measurement in this process: " + ", ".join(STEPS))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds of the three steps of this library")
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
        sp = lambda k: f"{rec[k + '_us']:8.1f} [{rec[k + '_us_min']:.1f} .. {rec[k + '_us_max']:.1f}]"  # noqa: E731
        print(f"{name:13s} sgd {sp('sgd')} us   adagrad {sp('adagrad')} us ({rec['adagrad_over_sgd']:.2f}x sgd, {rec['adagrad_vs_sgd']}; torch bwd+adagrad "
              f"{rec['torch_bwd_adagrad_us']:8.1f} us: {rec['adagrad_over_torch']:.2f}x, {rec['adagrad_vs_torch']})   rowwise {sp('rowwise')} us "
              f"({rec['rowwise_over_sgd']:.2f}x sgd, {rec['rowwise_vs_sgd']}; unfused {rec['rowwise_unfused_us']:8.1f} us: {rec['rowwise_over_unfused']:.2f}x, {rec['rowwise_vs_unfused']})   "
              f"{rec['unique_rows']} unique rows, longest run {rec['longest_run']}", flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
