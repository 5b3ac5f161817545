"""Strided pooled output against the dense lookup plus torch.cat: what writing straight into [B, T * dim] saves or costs.

Per shape and table dtype, three figures, device time per step, in one process, warm, REPEATS timings each, interleaved:

    (a) the dense plan                          emb_plan_time: T blocks [B, dim]
    (b) the dense plan + torch.cat(outs, 1)     HIP events around launch + cat into a preallocated [B, T * dim]
    (c) the strided plan                        emb_plan_time: the same [B, T * dim] buffer, written in place (plan_concat)

(c) against (b) is what a caller that needs the concatenated layout gains; (c) against (a) is what the layout costs the lookup
itself (rows of neighbouring tables share cache lines).  Shapes: C2 -- 26 Kaggle-sized tables, dim 16, B = 39 292, one index
per bag, uint32 -- and the pooled point -- 8 tables of 1M rows, dim 128, B = 4096, 32 Zipf-1.2 indices per bag; fp32 and bf16
tables each.  (a) is also timed with the events (b) is timed with ("dense_events"), and the cat alone, so that the two
clocks can be compared.

    python strided_out_probe.py [lib_path|-] [out.json|-]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402
import pim_embedding_lookup_amd as pel  # noqa: E402

REPEATS = 7
ITERS = 200
lib_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)


def events_us(step, warmup=5, iters=ITERS):
    """Mean device time of step() between two HIP events on torch's current stream."""
    for _ in range(warmup):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def stats(v):
    return {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v)), "repeats_us": [round(float(x), 2) for x in v]}


def measure(label, rows, dim, tdt, idx, off):
    T, B = len(rows), off[0].numel()
    ids = list(range(T))
    eng = pel.EmbeddingEngine(device=0, max_tables=T, lib_path=lib_path)
    for t, n in enumerate(rows):
        eng.load_table(t, (torch.rand((n, dim), device=dev) - 0.5).to(tdt))
    blocks = list(torch.empty((T * B, dim), dtype=torch.float32, device=dev).split(B))       # what lookup_batched allocates
    dense = eng.plan(ids, idx, off, outs=blocks)
    cat = torch.empty((B, T * dim), dtype=torch.float32, device=dev)
    strided = eng.plan_concat(ids, idx, off, out=torch.empty((B, T * dim), dtype=torch.float32, device=dev))
    recs = strided.describe()
    assert all(r["strided"] == 1 for r in recs) and [r["kind"] for r in recs] == [r["kind"] for r in dense.describe()], recs
    stream = torch.cuda.current_stream().cuda_stream

    def dense_then_cat():
        dense.launch(stream)
        torch.cat(blocks, dim=1, out=cat)
    dense.launch(stream)
    strided.launch(stream)
    dense_then_cat()
    torch.cuda.synchronize()
    assert torch.equal(cat.view(torch.int32), strided.outputs.view(torch.int32)), "the strided plan and dense + cat differ"
    us = {k: [] for k in ("dense", "dense_events", "cat_only", "dense_plus_cat", "strided")}
    for _ in range(REPEATS):
        us["dense"].append(dense.time_us(5, ITERS, stream))
        us["strided"].append(strided.time_us(5, ITERS, stream))
        us["dense_events"].append(events_us(lambda: dense.launch(stream)))
        us["cat_only"].append(events_us(lambda: torch.cat(blocks, dim=1, out=cat)))
        us["dense_plus_cat"].append(events_us(dense_then_cat))
    rec = {"point": label, "tables": T, "dim": dim, "bags": B, "dtype": str(tdt).replace("torch.", ""), "kinds": [r["kind"] for r in recs],
           "algorithmic_bytes": dense.bytes()[0], "concat_bytes": 2 * T * B * dim * 4}
    rec.update({k: stats(v) for k, v in us.items()})
    a, b, c = rec["dense"]["median_us"], rec["dense_plus_cat"]["median_us"], rec["strided"]["median_us"]
    rec["strided_vs_dense_plus_cat"] = c / b
    rec["strided_vs_dense"] = c / a
    print("%-34s (a) dense %8.2f us  (b) dense + cat %8.2f us (cat alone %.2f)  (c) strided %8.2f us   c/b %.2f  c/a %.2f" % (
        label, a, b, rec["cat_only"]["median_us"], c, c / b, c / a), flush=True)
    for p in (dense, strided):
        p.destroy()
    eng.close()
    torch.cuda.empty_cache()
    return rec


def main():
    records = []
    rows, B = pel.workloads.KAGGLE_ROWS, pel.workloads.KAGGLE_BATCH
    off = [torch.arange(B, dtype=torch.int32, device=dev)] * len(rows)
    idx = [torch.from_numpy(pel.workloads.uniform_indices(rng, n, B).view(np.int32)).to(dev) for n in rows]
    prow, pB, L = [1_000_000] * 8, 4096, 32
    poff = [torch.from_numpy(pel.workloads.fixed_offsets(pB, L).view(np.int32)).to(dev)] * len(prow)
    pidx = [torch.from_numpy(pel.workloads.zipf_indices(rng, n, pB * L, 1.2).view(np.int32)).to(dev) for n in prow]
    for name, tdt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        records.append(measure("C2 one-hot dim 16 %s" % name, rows, 16, tdt, idx, off))
        records.append(measure("pooled dim 128 L 32 zipf 1.2 %s" % name, prow, 128, tdt, pidx, poff))
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"repeats": REPEATS, "iters": ITERS, "device": torch.cuda.get_device_name(0), "points": records}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
