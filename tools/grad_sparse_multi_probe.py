"""Multi-table sparse gradient probe (profiles/grad_sparse_multi/README.md): what one emb_grad_sparse_multi call (one pre-pass and one launch
chain per group of up to 16 tables) costs next to a loop of emb_grad_sparse calls over the same descriptors, which this probe's commit does
not change and which is measured again in the same run as the yardstick.  Both are the C ABI's pure enqueues: device pointers only, the
counts stay on the device, nothing waits on the host inside a timed window.

Shapes (those of tools/adam_multi_probe.py and profiles/adam_multi/README.md):
  kaggle8-position     the 8 Criteo-Kaggle tables with more rows than bags, dim 16, 39 292 one-index bags each: no long runs
  uniform8-position    8 tables of 4 194 304 rows, dim 128, 2048 bags x 32 uniform ids each: no long runs
  kaggle26-segmented   all 26 Kaggle tables, dim 16, 39 292 one-index bags each, on an S = 64 context: seven tables of 3 .. 27 rows
Per shape ONE process times, in turn and --repeats times over (alternating rounds; every figure of every round is kept, so that the spread is
on the record), device events around --iters back-to-back calls after --warmup untimed ones:  multi, single.  Before the first round the two
are compared once, byte for byte.

Without --step every measurement runs as a child process of its own under its own time limit, and the probe stops at the first one that
fails or runs out of time.

    python tools/grad_sparse_multi_probe.py --out grad_sparse_multi_probe.json
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

STEPS = ("kaggle8-position", "uniform8-position", "kaggle26-segmented")
STEP_LIMIT_S = 300
SEGMENT = 64


def shape_of(name, pel):
    w = pel.workloads
    if name == "kaggle26":
        return list(w.KAGGLE_ROWS), w.KAGGLE_DIM, 1, w.KAGGLE_BATCH
    if name == "kaggle8":
        return [r for r in w.KAGGLE_ROWS if r > w.KAGGLE_BATCH], w.KAGGLE_DIM, 1, w.KAGGLE_BATCH
    return [4 << 20] * 8, 128, 32, 2048


def median_spread(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1], "rounds": xs}


def run_step(name, args):
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("grad_sparse_multi_probe needs the GPU: nothing here is a CPU measurement")
    shape, order = name.split("-")
    rows, dim, L, B = shape_of(shape, pel)
    T, n = len(rows), B * L
    rng = np.random.default_rng(0)
    eng = pel.EmbeddingEngine(device=0, max_tables=T)
    tabs = list(range(T))
    idx, off, G, longest = [], [], [], 0
    for t, nr in enumerate(rows):
        ids = pel.workloads.uniform_indices(rng, nr, n)
        longest = max(longest, int(np.unique(ids, return_counts=True)[1].max()))
        idx.append(torch.from_numpy(ids.astype(np.int64)).cuda())
        off.append(torch.arange(0, n, L, dtype=torch.int64, device="cuda"))
        G.append(torch.randn((B, dim), device="cuda") * 1e-3)
        eng.alloc_table(t, nr, dim, pel.lib.EMB_F32)      # (the call reads no table bytes)
    kw = dict(order="segmented", segment=SEGMENT, max_dim=dim) if order == "segmented" else {}
    ctx = eng.grad_context(T * n, T * B, **kw)
    groups = ctx.multi_groups(tabs, [n] * T, [B] * T)
    stream = torch.cuda.current_stream().cuda_stream
    keep = []
    descs, _, itype, _, _ = ctx._step_descs(tabs, idx, off, G, "sum", None, None, 0, stream, keep)

    def outputs():
        rows_o = [torch.full((n,), -1, dtype=torch.int64, device="cuda") for _ in tabs]
        grads_o = [torch.full((n, dim), -1.0, device="cuda") for _ in tabs]
        return rows_o, grads_o, torch.full((T,), -1, dtype=torch.int64, device="cuda")

    outs = {"multi": outputs(), "single": outputs()}
    ptrs = {k: ((C.c_void_p * T)(*[r.data_ptr() for r in o[0]]), (C.c_void_p * T)(*[g.data_ptr() for g in o[1]])) for k, o in outs.items()}
    caps = (C.c_uint64 * T)(*([n] * T))

    def multi():
        pel.lib.check_grad(ctx._G.emb_grad_sparse_multi(ctx._h, descs, T, itype, ptrs["multi"][0], ptrs["multi"][1], caps, outs["multi"][2].data_ptr(), stream))

    def single():
        rows_o, grads_o, counts = outs["single"]
        for t in tabs:
            pel.lib.check_grad(ctx._G.emb_grad_sparse(ctx._h, C.byref(descs[t]), itype, rows_o[t].data_ptr(), grads_o[t].data_ptr(), n,
                                                      counts.data_ptr() + 8 * t, stream))

    multi(), single()
    torch.cuda.synchronize()
    for a, b in zip(outs["multi"][0] + outs["multi"][1] + [outs["multi"][2]], outs["single"][0] + outs["single"][1] + [outs["single"][2]]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the multi call and the loop of single calls disagree"

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
        return a.elapsed_time(b) * 1e3 / args.iters      # us per call

    what = {"multi": multi, "single": single}
    figures = {k: [] for k in what}
    for _round in range(args.repeats):                   # alternating: one figure of everything per round
        for k, fn in what.items():
            figures[k].append(timed(fn))
    assert ctx.report() == 0
    out = {"step": name, "tables": T, "rows_total": int(sum(rows)), "dim": dim, "indices_per_bag": L, "bags_per_table": B, "longest_run": longest,
           "unique_rows": int(outs["multi"][2].sum()), "groups": [groups.count(g) for g in sorted(set(groups))], "context": ctx.order,
           "iters": args.iters, "warmup": args.warmup, "figures": {k: median_spread(x) for k, x in figures.items()}}
    out["multi_over_single"] = out["figures"]["multi"]["median_us"] / out["figures"]["single"]["median_us"]
    eng.close()
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one measurement in this process")
    ap.add_argument("--steps", type=str, default=",".join(STEPS), help="the measurements to run, each in a child process")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
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
