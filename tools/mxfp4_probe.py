"""MXFP4 against fp8 and bf16 tables in ONE build: device time per prepared launch (emb_plan_time) of bf16, e4m3 and MXFP4
tables over IDENTICAL indices, in one process, warm, REPEATS timings per point, the dtypes interleaved so that a drift of the
machine hits all alike.  Per point the time ratios mxfp4 / fp8 and mxfp4 / bf16 are printed beside the algorithmic byte ratios
(emb_plan_bytes).  There is no threshold -- nobody had measured an MXFP4 gather here, the format's standing value is capacity --
and the exit status is always 0; a launch whose median exceeds fp8's by more than fp8's own spread (max - min over its repeats)
is marked SLOWER, a finding to explain.

Points: the pooled shape of f8_probe.py (8 x 1M rows, dim 128, 32 entries per bag, Zipf 1.2) and one-hot launches (26
Kaggle-sized tables, B = 39292) at dims 32 / 64 / 128 / 256 -- MXFP4 always on the lane-group kernel, the others on whatever
choose_kernel gives them (the wave-batch kernel for these one-hot shapes).  Table VALUES do not matter to a timing: the bf16 and
e4m3 tables hold rounded uniform values, the MXFP4 tables random element bytes under scale bytes 120 ... 134.  `resident`
allocates the C5 share (64 tables x 30M rows x dim 64) as fp16, e4m3 and MXFP4 and reports emb_stats.table_bytes of each
(allocation only).  Run once per build for an A/B of a compile-time switch (-DPIMEMB_MX4_NT_STORE=1, -DPIMEMB_MX4_UNROLL=4);
`label=TEXT` says in the JSON what build the library is.

    python mxfp4_probe.py [lib_path|-] [out.json|-] [resident] [label=TEXT]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402
import pim_embedding_lookup_amd as pel  # noqa: E402
from pim_embedding_lookup_amd.formats import mxfp4_row_stride  # noqa: E402

REPEATS = 7
lib_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
flags = sys.argv[3:]
label = next((f[len("label="):] for f in flags if f.startswith("label=")), lib_path or "in-tree")
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
DTYPES = ("bf16", "e4m3", "mxfp4")


def load(eng, t, n, dim, name, gen):
    if name == "mxfp4":         # fused rows: random elements, scale bytes 120 ... 134, zero padding
        stride = mxfp4_row_stride(dim)
        rows = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        rows[:, :dim // 2] = torch.randint(0, 256, (n, dim // 2), dtype=torch.uint8, device=dev, generator=gen)
        rows[:, dim // 2:dim // 2 + dim // 32] = torch.randint(120, 135, (n, dim // 32), dtype=torch.uint8, device=dev, generator=gen)
        eng.load_table(t, rows, dtype=pel.EMB_MXFP4)
    else:
        w = torch.rand((n, dim), device=dev, generator=gen) - 0.5
        eng.load_table(t, w.to(torch.bfloat16 if name == "bf16" else torch.float8_e4m3fn))


def measure(point, rows, dim, make_batch, n_batches):
    ids = list(range(len(rows)))
    batches = [make_batch() for _ in range(n_batches)]
    engines, plans = {}, {}
    for name in DTYPES:
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        eng = engines[name] = pel.EmbeddingEngine(device=0, max_tables=len(rows), lib_path=lib_path)
        for t, n in enumerate(rows):
            load(eng, t, n, dim, name, gen)
        plans[name] = [eng.plan(ids, idx, off) for idx, off in batches]
    for name in DTYPES:                         # warm: code objects loaded, tables touched
        for p in plans[name]:
            p.time_us(3, 10)
    us = {name: [] for name in DTYPES}
    for _ in range(REPEATS):
        for name in DTYPES:
            us[name].append(float(np.mean([p.time_us(5, 40) for p in plans[name]])))
    rec = {"point": point}
    for name in DTYPES:
        v = us[name]
        rec[name] = {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "repeats_us": [round(x, 2) for x in v],
                     "algorithmic_bytes": plans[name][0].bytes()[0], "launches": plans[name][0].describe(),
                     "signature": "%016x" % plans[name][0].signature()}
    m, f8, bf = rec["mxfp4"], rec["e4m3"], rec["bf16"]
    spread = f8["max_us"] - f8["min_us"]
    m["time_ratio_to_fp8"], m["time_ratio_to_bf16"] = m["median_us"] / f8["median_us"], m["median_us"] / bf["median_us"]
    m["byte_ratio_to_fp8"], m["byte_ratio_to_bf16"] = m["algorithmic_bytes"] / f8["algorithmic_bytes"], m["algorithmic_bytes"] / bf["algorithmic_bytes"]
    m["slower_than_fp8_beyond_spread"] = m["median_us"] > f8["median_us"] + spread
    print("%-30s bf16 %8.2f us (kind %d)   e4m3 %8.2f us (min %.2f max %.2f, kind %d)   mxfp4 %8.2f us (min %.2f max %.2f, kind %d) "
          "time x%.3f of fp8, x%.3f of bf16; bytes x%.3f of fp8, x%.3f of bf16 %s %.0f GB/s" % (
              point, bf["median_us"], bf["launches"][0]["kind"], f8["median_us"], f8["min_us"], f8["max_us"], f8["launches"][0]["kind"],
              m["median_us"], m["min_us"], m["max_us"], m["launches"][0]["kind"], m["time_ratio_to_fp8"], m["time_ratio_to_bf16"],
              m["byte_ratio_to_fp8"], m["byte_ratio_to_bf16"], "SLOWER" if m["slower_than_fp8_beyond_spread"] else "ok",
              m["algorithmic_bytes"] / m["median_us"] / 1e3), flush=True)
    for name in DTYPES:
        for p in plans[name]:
            p.destroy()
        engines[name].close()
    torch.cuda.empty_cache()
    return rec


def resident():
    """emb_stats.table_bytes of the C5 share (64 tables x 30M rows x dim 64) as fp16, e4m3 and MXFP4: allocation alone."""
    out = {}
    for name, dt in (("fp16", pel.EMB_F16), ("e4m3", pel.EMB_F8_E4M3), ("mxfp4", pel.EMB_MXFP4)):
        eng = pel.EmbeddingEngine(device=0, max_tables=64, lib_path=lib_path)
        for t in range(64):
            eng.alloc_table(t, 30_000_000, 64, dt)
        out[name] = int(eng.stats()["table_bytes"])
        eng.close()
        print("C5 share resident as %-5s %.1f GB" % (name, out[name] / 1e9), flush=True)
    return out


def main():
    records = []
    prow, pB, L = [1_000_000] * 8, 4096, 32
    poff = torch.from_numpy(pel.workloads.fixed_offsets(pB, L).view(np.int32)).to(dev)

    def pooled():
        return [torch.from_numpy(pel.workloads.zipf_indices(rng, n, pB * L, 1.2).view(np.int32)).to(dev) for n in prow], [poff] * len(prow)
    records.append(measure("pooled dim 128 L 32 zipf 1.2", prow, 128, pooled, 4))
    rows = pel.workloads.KAGGLE_ROWS
    B = pel.workloads.KAGGLE_BATCH
    off = torch.arange(B, dtype=torch.int32, device=dev)
    for dim in (32, 64, 128, 256):
        def one_hot():
            return [torch.from_numpy(pel.workloads.uniform_indices(rng, n, B).view(np.int32)).to(dev) for n in rows], [off] * len(rows)
        records.append(measure("one-hot dim %d" % dim, rows, dim, one_hot, 4))
    result = {"repeats": REPEATS, "lib": label, "points": records}
    if "resident" in flags:
        result["c5_share_table_bytes"] = resident()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
