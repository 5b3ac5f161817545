"""Multi-table backward probe (profiles/grad_multi/README.md): what one fused SGD step over MANY tables costs on the GPU -- by the
multi-table step (emb_grad_sgd_multi: one pre-pass and one hot launch per group of up to 16 tables), by emb_grad_sgd over the same
descriptors (one pre-pass per table), by the PARENT commit's build of emb_grad_sgd (the baseline: --parent-grad-lib, a
libpimemb_grad.so built from the commit before the multi-table step), by torch's sparse backward + SGD over as many
nn.EmbeddingBags, and next to the forward lookup of the same batch.

Shapes (fp32 tables, uniform ids):
  kaggle26   26 tables with the Criteo-Kaggle row counts (workloads.KAGGLE_ROWS), dim 16, 39 292 one-index bags each
  kaggle8    the same batch over the 8 Kaggle tables that have more rows than the batch has bags: no long runs (in kaggle26 the
             tables of 3 .. 27 rows name each row thousands of times, and a row's run is ONE chain of ordered additions)
  uniform8   8 tables of 4 194 304 rows, dim 128, 32 indices per bag, 2048 bags each
Device events around --iters back-to-back calls after --warmup untimed ones, as tools/grad_probe.py.  No Zipf shape: the
multi-table step does not change the chain of one long run (profiles/grad/README.md), so it has nothing to say there.

The per-kernel split and the launches per step are a kernel-trace matter, in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/grad_multi_probe.py --step kaggle26 --what multi
(and --what single): calls per kernel / (warmup + iters) = launches per step.

Without --step every shape runs as a child process of its own under its own time limit, and the probe stops at the first one
that fails or runs out of time.

    python tools/grad_multi_probe.py --out grad_multi_probe.json [--parent-grad-lib PATH [--repeats R]]

--repeats R (with a parent build) adds, per shape, R rounds of both builds' emb_grad_sgd and emb_grad_sgd_multi through the C ABI:
the check of a change to the host side, whose effect must lie within the spread of the parent's own repeats.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["kaggle26", "kaggle8", "uniform8"]
STEP_LIMIT_S = 400


def shape_of(name, pel):
    if name == "kaggle26":
        return list(pel.workloads.KAGGLE_ROWS), pel.workloads.KAGGLE_DIM, 1, pel.workloads.KAGGLE_BATCH
    if name == "kaggle8":
        return [r for r in pel.workloads.KAGGLE_ROWS if r > pel.workloads.KAGGLE_BATCH], pel.workloads.KAGGLE_DIM, 1, pel.workloads.KAGGLE_BATCH
    if name == "uniform8":
        return [4 << 20] * 8, 128, 32, 2048
    raise SystemExit(f"unknown shape {name}")


def repeats_against_parent(pel, eng, ctx, args, timed, tabs, idx, off, G, max_indices, max_bags):
    """--repeats R: emb_grad_sgd and emb_grad_sgd_multi of this build and of the parent's, straight through the C ABI over ONE
    descriptor array (no Python marshalling in the figure), and of a second load of each build as the control, all timed in turn,
    R rounds: {name: [us per call, ...]}.  The spread between the parent's own figures -- over the rounds and over its two loads --
    is the yardstick for a change that leaves the kernels alone."""
    import torch
    T = len(tabs)
    arr, keep = (pel.lib.EmbGradDesc * T)(), []
    itype = {ctx._desc(arr[t], t, idx[t], off[t], G[t], "sum", None, None, 0, keep)[0] for t in range(T)}.pop()
    stream = torch.cuda.current_stream().cuda_stream
    # each build twice: the second from a copy of the file, so it is a library of its own with its own code object and context --
    # what differs between the two is what differs between ANY two loads of the same code (the control)
    tmp, parent = tempfile.mkdtemp(), os.path.abspath(args.parent_grad_lib)
    libs = {"": (ctx._G, ctx._h)}
    for name, path in (("again_", shutil.copy(ctx._G._name, os.path.join(tmp, "this_again.so"))), ("parent_", parent),
                       ("parent_again_", shutil.copy(parent, os.path.join(tmp, "parent_again.so")))):
        P = C.CDLL(path)
        for fn in ("emb_grad_create", "emb_grad_destroy", "emb_grad_sgd", "emb_grad_sgd_multi"):
            getattr(P, fn).restype, getattr(P, fn).argtypes = pel.lib.GRAD_SIGNATURES[fn]
        h = C.c_void_p()
        assert P.emb_grad_create(eng._h, max_indices, max_bags, C.byref(h)) == 0
        libs[name] = (P, h)

    def call(lib, handle, fn):
        def run():
            assert getattr(lib, fn)(handle, arr, T, itype, 0.01, stream) == 0
        return run
    runs = {name + what: call(lib, h, fn) for what, fn in (("multi", "emb_grad_sgd_multi"), ("single", "emb_grad_sgd")) for name, (lib, h) in libs.items()}
    out = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            out[k].append(timed(run))
    torch.cuda.synchronize()
    for name, (P, h) in libs.items():
        if name:
            P.emb_grad_destroy(h)
    shutil.rmtree(tmp)
    return out


def run_step(name, args):
    import torch
    import pim_embedding_lookup_amd as pel
    if not torch.cuda.is_available():
        raise SystemExit("grad_multi_probe needs the GPU: nothing here is a CPU measurement")
    rows, dim, L, B = shape_of(name, pel)
    T, n = len(rows), B * L
    rng = np.random.default_rng(0)
    eng = pel.EmbeddingEngine(device=0, max_tables=T)
    tabs = list(range(T))
    idx, off, G, ws, longest = [], [], [], [], 0
    for t, nr in enumerate(rows):
        ids = pel.workloads.uniform_indices(rng, nr, n)
        longest = max(longest, int(np.unique(ids, return_counts=True)[1].max()))
        idx.append(torch.from_numpy(ids.astype(np.int64)).cuda())
        off.append(torch.arange(0, n, L, dtype=torch.int64, device="cuda"))
        G.append(torch.randn((B, dim), device="cuda") * 1e-3)
        ws.append(torch.randn((nr, dim), device="cuda") * 0.05)
        eng.load_table(t, ws[t])
    ctx = eng.grad_context(T * n, T * B)
    groups = ctx.multi_groups(tabs, [n] * T, [B] * T)
    rec = {"step": name, "tables": T, "rows_total": int(sum(rows)), "dim": dim, "indices_per_bag": L, "bags_per_table": B, "longest_run": longest,
           "groups": [groups.count(g) for g in sorted(set(groups))], "iters": args.iters, "warmup": args.warmup}

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

    if args.what in ("all", "multi"):
        rec["multi_us"] = timed(lambda: ctx.sgd_step(tabs, idx, off, G, 0.01, multi=True))
    if args.what in ("all", "single"):
        rec["single_us"] = timed(lambda: ctx.sgd_step(tabs, idx, off, G, 0.01))
    assert ctx.report() == 0
    if args.what == "all" and args.parent_grad_lib and args.repeats > 1:
        rec["repeats"] = repeats_against_parent(pel, eng, ctx, args, timed, tabs, idx, off, G, T * n, T * B)
    if args.what == "all" and args.parent_grad_lib:
        # the parent commit's libpimemb_grad.so, over the same engine (libpimemb.so is already mapped under its soname) and the very
        # descriptors GradContext fills: its own context, its own kernels
        P = C.CDLL(os.path.abspath(args.parent_grad_lib))
        for fn in ("emb_grad_create", "emb_grad_destroy", "emb_grad_sgd", "emb_grad_last_error"):
            getattr(P, fn).restype, getattr(P, fn).argtypes = pel.lib.GRAD_SIGNATURES[fn]
        rec["parent_has_multi"] = hasattr(P, "emb_grad_sgd_multi")
        h = C.c_void_p()
        assert P.emb_grad_create(eng._h, n, B, C.byref(h)) == 0, P.emb_grad_last_error()
        arr, keep = (pel.lib.EmbGradDesc * T)(), []
        itype = {ctx._desc(arr[t], t, idx[t], off[t], G[t], "sum", None, None, 0, keep)[0] for t in range(T)}.pop()
        stream = torch.cuda.current_stream().cuda_stream

        def parent_step():
            rc = P.emb_grad_sgd(h, arr, T, itype, 0.01, stream)
            assert rc == 0, P.emb_grad_last_error()
        rec["parent_single_us"] = timed(parent_step)
        torch.cuda.synchronize()
        P.emb_grad_destroy(h)
    if args.what == "all":
        plan = eng.plan(tabs, idx, off)
        rec["forward_us"] = plan.time_us(args.warmup, args.iters)
        plan.destroy()
    ctx.close()
    eng.close()
    if args.what == "all":
        bags = [torch.nn.EmbeddingBag(nr, dim, mode="sum", sparse=True, _weight=ws[t]).cuda() for t, nr in enumerate(rows)]
        opt = torch.optim.SGD([p for b in bags for p in b.parameters()], lr=0.01)

        def torch_fwd():
            return [b(idx[t], off[t]) for t, b in enumerate(bags)]

        def torch_step():
            opt.zero_grad(set_to_none=True)
            torch.autograd.backward(torch_fwd(), G)
            opt.step()
        rec["torch_fwd_bwd_sgd_us"] = timed(torch_step)
        with torch.no_grad():
            rec["torch_fwd_us"] = timed(torch_fwd)
        rec["torch_bwd_sgd_us"] = rec["torch_fwd_bwd_sgd_us"] - rec["torch_fwd_us"]
        base = rec.get("parent_single_us", rec["single_us"])
        rec["baseline"] = "parent_single_us" if "parent_single_us" in rec else "single_us (no parent build given)"
        rec["multi_over_baseline"] = rec["multi_us"] / base
        rec["multi_over_torch"] = rec["multi_us"] / rec["torch_bwd_sgd_us"]
        rec["multi_over_forward"] = rec["multi_us"] / rec["forward_us"]
        rec["verdict_vs_baseline"] = "SLOWER" if rec["multi_over_baseline"] > 1 else "faster"
        rec["verdict_vs_torch"] = "SLOWER" if rec["multi_over_torch"] > 1 else "faster"
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run this one shape in this process: " + ", ".join(STEPS))
    ap.add_argument("--what", default="all", choices=["all", "multi", "single"], help="multi / single: time that step alone (for a kernel trace)")
    ap.add_argument("--parent-grad-lib", default="", help="a libpimemb_grad.so built from the parent commit: the baseline")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=1, help="with --parent-grad-lib: time both builds' two calls through the C ABI this often, in turn")
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.step:
        run_step(args.step, args)
        return 0
    results = []
    for name in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(args.iters), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        if args.parent_grad_lib:
            cmd += ["--parent-grad-lib", args.parent_grad_lib]
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
        print(f"{name:9s} groups {rec['groups']} longest run {rec['longest_run']}  multi {rec['multi_us']:8.1f} us   {rec['baseline']} {rec.get('parent_single_us', rec['single_us']):8.1f} us "
              f"({rec['multi_over_baseline']:.2f}x, {rec['verdict_vs_baseline']})   this build single {rec['single_us']:8.1f} us   torch bwd+sgd "
              f"{rec['torch_bwd_sgd_us']:8.1f} us ({rec['multi_over_torch']:.2f}x, {rec['verdict_vs_torch']})   forward {rec['forward_us']:7.1f} us", flush=True)
        for k, v in rec.get("repeats", {}).items():
            print(f"    C ABI, {len(v)} rounds: {k:13s} min {min(v):9.1f}  max {max(v):9.1f} us   " + " ".join(f"{x:.1f}" for x in v), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
