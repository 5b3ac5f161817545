"""Master-weight Adam step probe (profiles/master_adam/README.md): what one fused master-weight Adam step (emb_grad_master_adam_step,
include/pimemb_grad.h; GradContext.master_adam_step) costs on the GPU next to its neighbours and to what it replaces.

Shapes (one table each, device pointers only; tools/master_probe.py's):
  uniform   dim 128, 32 indices per bag, 2048 bags, ids uniform over 4 194 304 rows     bf16, e4m3, mxfp4
  zipf      the same with Zipf-skewed ids, on an S = 64 context                          bf16, e4m3, mxfp4
  kaggle    dim 16, one index per bag, 39 292 bags, ids uniform over 10 131 227 rows    bf16, e4m3 (MXFP4 needs dim % 32 == 0)
Per shape and dtype ONE process times, in turn and --repeats times over (alternating rounds; every figure of every round is kept, so
that the spread is on the record), device events around --iters back-to-back calls after --warmup untimed ones:
  madam       GradContext.master_adam_step, SparseAdam
  madam_rw    the same, row-wise Adam
  madagrad    GradContext.master_step(optimizer="adagrad") on a table, master and state of its own: the master tail with two streams less
  inplace     bf16 only: GradContext.adam_step on a bf16 table of its own: 20 bytes per stepped element against 24 + 2
  recipe      the unfused route the step replaces: rows_out.fill_(-1), emb_grad_sparse, torch ops on master, exp_avg and exp_avg_sq
              (gather, the moments, the subtract, three index_copy_), RowWriter.update of all n slots -- on a set of its own
The neighbours run through code this probe's commit does not change (their kernels keep their machine code), so one build gives all
sides.  The 4 M x 128 shapes hold 2 GB per fp32 array: about 25 GB in all.

Without --step every measurement runs as a child process of its own under its own time limit, and the probe stops at the first one
that fails or runs out of time.

    python tools/master_adam_probe.py --out master_adam_probe.json
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
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
SEGMENT = 64


def median_spread(xs):
    xs = sorted(xs)
    return {"median_us": xs[len(xs) // 2], "min_us": xs[0], "max_us": xs[-1], "rounds": xs}


def run_step(name, args):
    import ctypes as C
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("master_adam_probe needs the GPU: nothing here is a CPU measurement")
    shape, kind = name.split("-")
    rows, dim, L, B = SHAPES[shape]
    rng = np.random.default_rng(0)
    n = B * L
    ids = pel.workloads.zipf_indices(rng, rows, n) if shape == "zipf" else pel.workloads.uniform_indices(rng, rows, n)
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    off = torch.arange(0, n, L, dtype=torch.int64, device="cuda")
    G = torch.randn((B, dim), dtype=torch.float32, device="cuda")
    code = getattr(pel.lib, KINDS[kind])
    eng = pel.EmbeddingEngine(device=0, max_tables=8)
    w = torch.randn((rows, dim), dtype=torch.float32, device="cuda") * 0.5
    T_ADAM, T_RW, T_ADAGRAD, T_RECIPE, T_INPLACE = 0, 1, 2, 3, 4
    for t in (T_ADAM, T_RW, T_ADAGRAD, T_RECIPE):
        eng.load_table_f32(t, w, code)
    zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    sets = {"madam": (w.clone(), zeros(rows, dim), zeros(rows, dim)), "madam_rw": (w.clone(), zeros(rows, dim), zeros(rows)),
            "madagrad": (w.clone(), zeros(rows, dim)), "recipe": (w.clone(), zeros(rows, dim), zeros(rows, dim))}
    if kind == "bf16":
        eng.load_table_f32(T_INPLACE, w, code)
        sets["inplace"] = (zeros(rows, dim), zeros(rows, dim))
    del w
    ctx = eng.grad_context(n, B, order="segmented", segment=SEGMENT, max_dim=dim) if shape == "zipf" else eng.grad_context(n, B)
    writer = eng.row_writer(n)
    stream = torch.cuda.current_stream().cuda_stream
    rows_out = torch.zeros((n,), dtype=torch.int64, device="cuda")
    grads_out = torch.zeros((n, dim), dtype=torch.float32, device="cuda")
    n_unique = torch.zeros((1,), dtype=torch.int64, device="cuda")
    om1, om2, ss = ctx.adam_constants(LR, BETAS, EPS, 1)

    def madam(which, t, rowwise):
        p, m, v = sets[which]
        return lambda: ctx.master_adam_step([t], [idx], [off], [G], [p], [m], [v], LR, betas=BETAS, eps=EPS, step=1, rowwise=rowwise, stream=stream)

    def madagrad():
        p, s = sets["madagrad"]
        ctx.master_step([T_ADAGRAD], [idx], [off], [G], [p], LR, optimizer="adagrad", states=[s], eps=1e-10, stream=stream)

    def inplace():
        m, v = sets["inplace"]
        ctx.adam_step([T_INPLACE], [idx], [off], [G], [m], [v], LR, betas=BETAS, eps=EPS, step=1, stream=stream)

    def recipe():
        p, m, v = sets["recipe"]
        desc, keep = pel.lib.EmbGradDesc(), []
        itype, _dev = ctx._desc(desc, T_RECIPE, idx, off, G, "sum", None, None, 0, keep)

        def call():                                      # (the -1 slots write row 0 again and again with the value it has: a probe of time, not of bytes)
            rows_out.fill_(-1)
            pel.lib.check_grad(ctx._G.emb_grad_sparse(ctx._h, C.byref(desc), itype, rows_out.data_ptr(), grads_out.data_ptr(), n, n_unique.data_ptr(), stream))
            live = rows_out >= 0
            r = torch.where(live, rows_out, torch.zeros_like(rows_out))
            g = grads_out * live.unsqueeze(1)
            m1 = m[r] + (g - m[r]) * om1
            v1 = v[r] + (g * g - v[r]) * om2
            new = p[r] - ss * (m1 / (v1.sqrt() + EPS))
            m.index_copy_(0, r, torch.where(live.unsqueeze(1), m1, m[r]))
            v.index_copy_(0, r, torch.where(live.unsqueeze(1), v1, v[r]))
            p.index_copy_(0, r, torch.where(live.unsqueeze(1), new, p[r]))
            writer.update(T_RECIPE, rows_out, new, stream=stream)
        return call

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

    what = {"madam": madam("madam", T_ADAM, False), "madam_rw": madam("madam_rw", T_RW, True), "madagrad": madagrad, "recipe": recipe()}
    if kind == "bf16":
        what["inplace"] = inplace
    figures = {k: [] for k in what}
    for _round in range(args.repeats):                   # alternating: one figure of everything per round
        for k, fn in what.items():
            figures[k].append(timed(fn))
    out = {"step": name, "rows": rows, "dim": dim, "bags": B, "per_bag": L, "iters": args.iters, "warmup": args.warmup,
           "context": "S%d" % SEGMENT if shape == "zipf" else "position", "longest_run": int(np.bincount(ids.astype(np.int64)).max()),
           "unencodable": ctx.master_report(), "figures": {k: median_spread(v) for k, v in figures.items()}}
    med = lambda k: out["figures"][k]["median_us"]  # noqa: E731
    out["recipe_over_madam"] = med("recipe") / med("madam")
    out["madam_over_madagrad"] = med("madam") / med("madagrad")
    out["madam_rw_over_madam"] = med("madam_rw") / med("madam")
    if kind == "bf16":
        out["madam_over_inplace"] = med("madam") / med("inplace")
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
