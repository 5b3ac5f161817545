"""bf16 against fp16 tables, the same bytes per row: device time per prepared launch (emb_plan_time) of both dtypes over
IDENTICAL indices, in one process, warm, REPEATS timings per point.  The fp16 kernels are the yardstick (their machine code
is what the library shipped before bf16 existed); a point passes when

    median(bf16) <= median(fp16) + (max(fp16) - min(fp16))

i.e. bf16 costs what fp16 costs, give or take fp16's own run-to-run spread.  Points: the one-hot shapes of
f16_onehot_probe.py (26 Kaggle-sized tables, B = 39292, dims 16 / 32 / 64 / 128) and one pooled shape (dim 128, 32
entries per bag, Zipf 1.2).

    python bf16_probe.py [lib_path|-] [out.json|-] [control]        exit status 1 when a point misses

control: a SECOND set of fp16 tables (same values, same indices, its own allocations) is timed next to the two -- what two
sets of tables differ by when the kernel is the very same one, i.e. how much of a difference is placement, not code."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402
import pim_embedding_lookup_amd as pel  # noqa: E402

REPEATS = 7
lib_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
DTYPES = (("fp16", torch.float16), ("bf16", torch.bfloat16)) + ((("fp16_again", torch.float16),) if "control" in sys.argv[3:] else ())


def measure(label, rows, dim, make_batch, n_batches):
    """One engine per dtype over the same fp32 values and the same index tensors; the repeats of the two dtypes interleaved,
    so that a drift of the machine (clocks, neighbours) hits both alike."""
    ids = list(range(len(rows)))
    src = [torch.rand((n, dim), device=dev) - 0.5 for n in rows]
    batches = [make_batch() for _ in range(n_batches)]
    engines, plans = {}, {}
    for name, dt in DTYPES:
        eng = engines[name] = pel.EmbeddingEngine(device=0, max_tables=len(rows), lib_path=lib_path)
        for t, w in enumerate(src):
            eng.load_table(t, w.to(dt))
        plans[name] = [eng.plan(ids, idx, off) for idx, off in batches]
    del src
    for name, _ in DTYPES:                      # warm: code objects loaded, tables touched
        for p in plans[name]:
            p.time_us(3, 10)
    us = {name: [] for name, _ in DTYPES}
    for _ in range(REPEATS):
        for name, _dt in DTYPES:
            us[name].append(float(np.mean([p.time_us(5, 40) for p in plans[name]])))
    rec = {"point": label, "kinds": engines["bf16"].stats()["n_launches_by_kind"], "algorithmic_bytes": plans["bf16"][0].bytes()[0]}
    for name, _ in DTYPES:
        v = us[name]
        rec[name] = {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "repeats_us": [round(x, 2) for x in v]}
    spread = rec["fp16"]["max_us"] - rec["fp16"]["min_us"]
    rec["fp16_spread_us"] = spread
    rec["ok"] = rec["bf16"]["median_us"] <= rec["fp16"]["median_us"] + spread
    print("%-28s fp16 %8.2f us (min %.2f max %.2f)   bf16 %8.2f us (min %.2f max %.2f)   %+6.2f us vs margin %.2f  %s  %.0f GB/s" % (
        label, rec["fp16"]["median_us"], rec["fp16"]["min_us"], rec["fp16"]["max_us"], rec["bf16"]["median_us"], rec["bf16"]["min_us"],
        rec["bf16"]["max_us"], rec["bf16"]["median_us"] - rec["fp16"]["median_us"], spread, "ok" if rec["ok"] else "MISS",
        rec["algorithmic_bytes"] / rec["bf16"]["median_us"] / 1e3), flush=True)
    if "fp16_again" in rec:
        print("%-28s fp16 again %8.2f us (min %.2f max %.2f): %+.2f us from the first set" % (
            "", rec["fp16_again"]["median_us"], rec["fp16_again"]["min_us"], rec["fp16_again"]["max_us"],
            rec["fp16_again"]["median_us"] - rec["fp16"]["median_us"]), flush=True)
    for name, _ in DTYPES:
        for p in plans[name]:
            p.destroy()
        engines[name].close()
    torch.cuda.empty_cache()
    return rec


def main():
    rows = pel.workloads.KAGGLE_ROWS
    B = pel.workloads.KAGGLE_BATCH
    off = torch.arange(B, dtype=torch.int32, device=dev)
    records = []
    for dim in (16, 32, 64, 128):
        def one_hot():
            return [torch.from_numpy(pel.workloads.uniform_indices(rng, n, B).view(np.int32)).to(dev) for n in rows], [off] * len(rows)
        records.append(measure("one-hot dim %d" % dim, rows, dim, one_hot, 4))
    prow, pB, L = [1_000_000] * 8, 4096, 32
    poff = torch.from_numpy(pel.workloads.fixed_offsets(pB, L).view(np.int32)).to(dev)

    def pooled():
        return [torch.from_numpy(pel.workloads.zipf_indices(rng, n, pB * L, 1.2).view(np.int32)).to(dev) for n in prow], [poff] * len(prow)
    records.append(measure("pooled dim 128 L 32 zipf 1.2", prow, 128, pooled, 4))
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"repeats": REPEATS, "points": records}, f, indent=1)
    return 0 if all(r["ok"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
