"""Half-width pooled output against fp32 output over the same fp16 / bf16 tables: device time per prepared launch
(emb_plan_time) of an fp32-out plan and a half-out plan (out_dtype="table", EMB_POOL_OUT_TABLE_DTYPE) over IDENTICAL tables and
indices, in one process, warm, REPEATS timings per plan, the two interleaved.  The fp32-out plans run the kernels the library
shipped before the flag existed (their machine code is unchanged), so they are the yardstick; a point passes when

    median(half out) <= median(fp32 out) + (max(fp32 out) - min(fp32 out))

i.e. half-width output costs no more than fp32 output, give or take the fp32-out plan's own run-to-run spread.  Next to the
time ratio the probe prints the ALGORITHMIC-byte ratio of the two plans (emb_plan_bytes: 0.68 for one-hot uint32 lookups at
every dim): how much of it a launch realises is what the table is for.  Points: those of bf16_probe.py -- 26 Kaggle-sized
tables, B = 39292, dims 16 / 32 / 64 / 128, and one pooled shape (8 x 1M rows, dim 128, 32 per bag, Zipf 1.2) -- for fp16 and
for bf16 tables.

    python halfout_probe.py [lib_path|-] [out.json|-]        exit status 1 when a point misses"""
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
DTYPES = (("fp16", torch.float16), ("bf16", torch.bfloat16))
OUTS = (("f32out", None), ("halfout", "table"))


def measure(label, tname, tdt, rows, dim, make_batch, n_batches):
    """One engine, one set of tables; per batch an fp32-out plan and a half-out plan over the same index tensors; the repeats of
    the two interleaved, so that a drift of the machine (clocks, neighbours) hits both alike."""
    ids = list(range(len(rows)))
    eng = pel.EmbeddingEngine(device=0, max_tables=len(rows), lib_path=lib_path)
    for t, n in enumerate(rows):
        eng.load_table(t, (torch.rand((n, dim), device=dev) - 0.5).to(tdt))
    batches = [make_batch() for _ in range(n_batches)]
    plans = {name: [eng.plan(ids, idx, off, out_dtype=od) for idx, off in batches] for name, od in OUTS}
    for name, _ in OUTS:                        # warm: code objects loaded, tables touched
        for p in plans[name]:
            p.time_us(3, 10)
    us = {name: [] for name, _ in OUTS}
    for _ in range(REPEATS):
        for name, _od in OUTS:
            us[name].append(float(np.mean([p.time_us(5, 40) for p in plans[name]])))
    rec = {"point": label, "table_dtype": tname, "launches": {name: plans[name][0].describe() for name, _ in OUTS}}
    for name, _ in OUTS:
        v = us[name]
        rec[name] = {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "repeats_us": [round(x, 2) for x in v],
                     "algorithmic_bytes": plans[name][0].bytes()[0]}
    f, h = rec["f32out"], rec["halfout"]
    spread = f["max_us"] - f["min_us"]
    rec["f32out_spread_us"] = spread
    rec["time_ratio"] = h["median_us"] / f["median_us"]
    rec["byte_ratio"] = h["algorithmic_bytes"] / f["algorithmic_bytes"]
    rec["ok"] = h["median_us"] <= f["median_us"] + spread
    print("%-28s %-4s fp32 out %8.2f us (min %.2f max %.2f)   half out %8.2f us (min %.2f max %.2f)   %+7.2f us vs margin %.2f  %s   "
          "time x%.3f  bytes x%.3f  %.0f GB/s" % (label, tname, f["median_us"], f["min_us"], f["max_us"], h["median_us"], h["min_us"],
                                                   h["max_us"], h["median_us"] - f["median_us"], spread, "ok" if rec["ok"] else "MISS",
                                                   rec["time_ratio"], rec["byte_ratio"], h["algorithmic_bytes"] / h["median_us"] / 1e3), flush=True)
    for name, _ in OUTS:
        for p in plans[name]:
            p.destroy()
    eng.close()
    torch.cuda.empty_cache()
    return rec


def main():
    rows = pel.workloads.KAGGLE_ROWS
    B = pel.workloads.KAGGLE_BATCH
    off = torch.arange(B, dtype=torch.int32, device=dev)
    prow, pB, L = [1_000_000] * 8, 4096, 32
    poff = torch.from_numpy(pel.workloads.fixed_offsets(pB, L).view(np.int32)).to(dev)

    def one_hot():
        return [torch.from_numpy(pel.workloads.uniform_indices(rng, n, B).view(np.int32)).to(dev) for n in rows], [off] * len(rows)

    def pooled():
        return [torch.from_numpy(pel.workloads.zipf_indices(rng, n, pB * L, 1.2).view(np.int32)).to(dev) for n in prow], [poff] * len(prow)

    records = []
    for tname, tdt in DTYPES:
        for dim in (16, 32, 64, 128):
            records.append(measure("one-hot dim %d" % dim, tname, tdt, rows, dim, one_hot, 4))
        records.append(measure("pooled dim 128 L 32 zipf 1.2", tname, tdt, prow, 128, pooled, 4))
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"repeats": REPEATS, "points": records}, f, indent=1)
    return 0 if all(r["ok"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
