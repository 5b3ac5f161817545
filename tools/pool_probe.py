"""Device time of the pooled lookups (bag_pool_* kernels) against the plain sum over the SAME seeded inputs: per shape, a sum
plan and one pooled plan per variant are built over one set of buffers and timed alternately (Plan.time_us: HIP events around
back-to-back launches), three repeats.  Prints one JSON line per (shape, variant, repeat) and a summary line per shape with
the median ratio pooled / sum.

Shapes: c2 -- 26 Kaggle-sized fp32 tables, dim 16, B = 39 292, one index per bag (DLRM --weighted-pooling on Criteo Kaggle);
c3 -- 16 tables of 1M rows, dim 128, B = 4096, 32 indices per bag; anydim -- 26 Kaggle-sized tables, dim 30 (120-byte rows), B = 8192,
8 indices per bag.  Usage: python tools/pool_probe.py [--out FILE] [--iters N]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pim_embedding_lookup_amd as pel  # noqa: E402

SHAPES = {
    "c2": dict(rows=pel.workloads.KAGGLE_ROWS, dim=16, B=39292, L=1, variants=["weighted"]),
    "c3": dict(rows=[1000000] * 16, dim=128, B=4096, L=32, variants=["weighted", "mean", "max"]),
    "anydim": dict(rows=pel.workloads.KAGGLE_ROWS, dim=30, B=8192, L=8, variants=["weighted", "mean", "max"]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in args.shapes.split(","):
        s = SHAPES[name]
        rows, dim, B, L = s["rows"], s["dim"], s["B"], s["L"]
        T = len(rows)
        eng = pel.EmbeddingEngine(device=0, max_tables=T)
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        for t, n in enumerate(rows):
            eng.load_table(t, torch.randn((n, dim), device=dev, generator=gen))
        rng = np.random.default_rng(11)
        idx = [torch.from_numpy(rng.integers(0, n, size=B * L).astype(np.int32)).to(dev) for n in rows]
        off = [torch.arange(B, dtype=torch.int32, device=dev) * L for _ in rows]
        w = [torch.from_numpy(rng.standard_normal(B * L).astype(np.float32)).to(dev) for _ in rows]
        ids = list(range(T))
        outs = [torch.empty((B, dim), device=dev) for _ in rows]
        plans = {"sum": eng.plan(ids, idx, off, outs=outs)}
        for v in s["variants"]:
            if v == "weighted":
                plans[v] = eng.plan_pooled(ids, idx, off, "sum", per_sample_weights=w, outs=outs)
            else:
                plans[v] = eng.plan_pooled(ids, idx, off, v, outs=outs)
        times = {k: [] for k in plans}
        for rep in range(3):
            for k, p in plans.items():          # alternated: sum, pooled variants, sum, ...
                us = p.time_us(5, args.iters)
                times[k].append(us)
                emit(dict(shape=name, variant=k, repeat=rep, us=round(us, 2), bytes=p.bytes()[0],
                          tbps=round(p.bytes()[0] / us / 1e6, 3), kind=[r["kind"] for r in p.describe()]))
        base = statistics.median(times["sum"])
        emit(dict(shape=name, summary=True, sum_us=round(base, 2),
                  ratio={k: round(statistics.median(v) / base, 3) for k, v in times.items() if k != "sum"}))
        for p in plans.values():
            p.destroy()
        eng.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
