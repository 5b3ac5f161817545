"""fp8 against bf16 tables in ONE build: device time per prepared launch (emb_plan_time) of bf16, e4m3 and e5m2 tables made from
the same fp32 values over IDENTICAL indices, in one process, warm, REPEATS timings per point, the dtypes interleaved.  The bf16
kernels are the yardstick: their machine code is what the library shipped before fp8 existed, so this is a comparison with
the parent.  Per point the time ratio fp8 / bf16 is printed beside the algorithmic byte ratio (emb_plan_bytes); an fp8 launch
whose median exceeds bf16's median by more than bf16's own spread (max - min over its repeats) is marked SLOWER -- a finding
to explain, not a gate: nobody had measured an fp8 gather here, so there is no threshold and the exit status is always 0.

Points: the one-hot shapes of bf16_probe.py (26 Kaggle-sized tables, B = 39292, dims 16 / 32 / 64 / 128) and its pooled shape
(8 x 1M rows, dim 128, 32 entries per bag, Zipf 1.2).  `wide` adds one-hot dim 256 (16 lanes per fp8 row): with
dim 128 (8 lanes) these are the rows whose stores the library either re-deals inside the lane group or leaves to the L2
(-DPIMEMB_F8_WIDE_REDEAL, 1 by default; pimemb_bag_kernels.h) -- run the probe once per build for that A/B, or for the
narrow rows' non-temporal stores (-DPIMEMB_F8_NARROW_NT=1).  `resident` allocates the C5 share (64 tables x 30M rows x dim 64)
as fp16 and as e4m3 and reports emb_stats.table_bytes of each (allocation only).  `label=TEXT` says in the JSON what build the
library is (default: its path, or "in-tree").

    python f8_probe.py [lib_path|-] [out.json|-] [wide] [resident] [label=TEXT]"""
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
flags = sys.argv[3:]
label = next((f[len("label="):] for f in flags if f.startswith("label=")), lib_path or "in-tree")
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
DTYPES = (("bf16", torch.bfloat16), ("e4m3", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2))


def measure(label, rows, dim, make_batch, n_batches):
    """One engine per dtype over the same fp32 values and the same index tensors; the repeats of the dtypes interleaved, so
    that a drift of the machine (clocks, neighbours) hits all alike."""
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
    rec = {"point": label}
    for name, _ in DTYPES:
        v = us[name]
        rec[name] = {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "repeats_us": [round(x, 2) for x in v],
                     "algorithmic_bytes": plans[name][0].bytes()[0], "launches": plans[name][0].describe(),
                     "signature": "%016x" % plans[name][0].signature()}
    spread = rec["bf16"]["max_us"] - rec["bf16"]["min_us"]
    rec["bf16_spread_us"] = spread
    line = "%-30s bf16 %8.2f us (min %.2f max %.2f, kind %d)" % (label, rec["bf16"]["median_us"], rec["bf16"]["min_us"], rec["bf16"]["max_us"],
                                                                rec["bf16"]["launches"][0]["kind"])
    for name in ("e4m3", "e5m2"):
        r = rec[name]
        r["time_ratio"] = r["median_us"] / rec["bf16"]["median_us"]
        r["byte_ratio"] = r["algorithmic_bytes"] / rec["bf16"]["algorithmic_bytes"]
        r["slower_than_bf16_beyond_spread"] = r["median_us"] > rec["bf16"]["median_us"] + spread
        line += "   %s %8.2f us (min %.2f max %.2f, kind %d) time x%.3f bytes x%.3f %s %.0f GB/s" % (
            name, r["median_us"], r["min_us"], r["max_us"], r["launches"][0]["kind"], r["time_ratio"], r["byte_ratio"],
            "SLOWER" if r["slower_than_bf16_beyond_spread"] else "ok", r["algorithmic_bytes"] / r["median_us"] / 1e3)
    print(line + "   margin %.2f us" % spread, flush=True)
    for name, _ in DTYPES:
        for p in plans[name]:
            p.destroy()
        engines[name].close()
    torch.cuda.empty_cache()
    return rec


def resident():
    """emb_stats.table_bytes of the C5 share (64 tables x 30M rows x dim 64) as fp16 and as e4m3: allocation alone."""
    out = {}
    for name, dt in (("fp16", pel.EMB_F16), ("e4m3", pel.EMB_F8_E4M3)):
        eng = pel.EmbeddingEngine(device=0, max_tables=64, lib_path=lib_path)
        for t in range(64):
            eng.alloc_table(t, 30_000_000, 64, dt)
        out[name] = int(eng.stats()["table_bytes"])
        eng.close()
        print("C5 share resident as %-5s %.1f GB" % (name, out[name] / 1e9), flush=True)
    return out


def main():
    rows = pel.workloads.KAGGLE_ROWS
    B = pel.workloads.KAGGLE_BATCH
    off = torch.arange(B, dtype=torch.int32, device=dev)
    records = []
    for dim in (16, 32, 64, 128) + ((256,) if "wide" in flags else ()):
        def one_hot():
            return [torch.from_numpy(pel.workloads.uniform_indices(rng, n, B).view(np.int32)).to(dev) for n in rows], [off] * len(rows)
        records.append(measure("one-hot dim %d" % dim, rows, dim, one_hot, 4))
    prow, pB, L = [1_000_000] * 8, 4096, 32
    poff = torch.from_numpy(pel.workloads.fixed_offsets(pB, L).view(np.int32)).to(dev)

    def pooled():
        return [torch.from_numpy(pel.workloads.zipf_indices(rng, n, pB * L, 1.2).view(np.int32)).to(dev) for n in prow], [poff] * len(prow)
    records.append(measure("pooled dim 128 L 32 zipf 1.2", prow, 128, pooled, 4))
    result = {"repeats": REPEATS, "lib": label, "points": records}
    if "resident" in flags:
        result["c5_share_table_bytes"] = resident()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
