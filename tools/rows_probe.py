"""Row-writer probe (profiles/rows/README.md): what it costs to bring an fp32 table into each table dtype, and what one
in-place update of 65 536 random rows costs.

  load    a [--rows, --dim] fp32 table per dtype, three ways: (a) the host encoder of formats.py + emb_load_table -- the only
          way before the row writer --, (b) EmbeddingEngine.load_table_f32 from the same host array (GPU encoders, fp32 chunks
          through the writer's pinned buffer), (c) load_table_f32 from a CUDA tensor.  Host clock around work that ends in a
          device synchronise; (b)'s table bytes are compared with (a)'s.
  update  RowWriter.update of --update-rows random rows through device pointers, with the duplicate pre-pass and with
          EMB_ROWS_UNIQUE_IDS, next to a device-to-device copy of the bytes the update stores (the floor): device events around
          --iters back-to-back calls after --warmup untimed ones.

    python tools/rows_probe.py --out rows_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4 << 20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--update-rows", type=int, default=65536)
    ap.add_argument("--chunk-rows", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtypes", default="f32,f16,bf16,e4m3,e5m2,mxfp4")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import pim_embedding_lookup_amd as pel
    from importlib import import_module
    formats = import_module("pim-embedding-lookup_amd.formats")
    if not torch.cuda.is_available():
        raise SystemExit("rows_probe needs the GPU: nothing here is a CPU measurement")
    L = pel.lib
    codes = {"f32": L.EMB_F32, "f16": L.EMB_F16, "bf16": L.EMB_BF16, "e4m3": L.EMB_F8_E4M3, "e5m2": L.EMB_F8_E5M2, "mxfp4": L.EMB_MXFP4}
    host_enc = {"f32": lambda w: w, "f16": lambda w: w.astype(np.float16), "bf16": formats.to_bf16_bits,
                "e4m3": lambda w: formats.to_f8_bits(w, "e4m3"), "e5m2": lambda w: formats.to_f8_bits(w, "e5m2"), "mxfp4": formats.to_mxfp4}
    rng = np.random.default_rng(0)
    n, dim = args.rows, args.dim
    w = rng.standard_normal((n, dim), dtype=np.float32)
    w_dev = torch.from_numpy(w).cuda()
    ids = torch.from_numpy(rng.integers(0, n, size=args.update_rows)).cuda()
    ids_unique = torch.from_numpy(rng.permutation(n)[:args.update_rows]).cuda()
    src = torch.from_numpy(rng.standard_normal((args.update_rows, dim), dtype=np.float32)).cuda()
    eng = pel.EmbeddingEngine(device=0, max_tables=4)
    writer = eng.row_writer(args.update_rows)
    results = []

    def same_bytes(t0, t1):      # compared where the tables are: on the GPU
        return bool(torch.equal(eng.table_tensor(t0).view(torch.uint8), eng.table_tensor(t1).view(torch.uint8)))

    def timed_events(fn):
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

    for kind in args.dtypes.split(","):
        code = codes[kind]
        rec = {"dtype": kind, "rows": n, "dim": dim}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc = host_enc[kind](w)
        t1 = time.perf_counter()
        eng.load_table(0, enc, dtype=code)
        eng.synchronize()
        t2 = time.perf_counter()
        rec["host_encode_s"], rec["load_table_s"], rec["parent_way_s"] = t1 - t0, t2 - t1, t2 - t0
        del enc
        t0 = time.perf_counter()
        eng.load_table_f32(1, w, code, chunk_rows=args.chunk_rows)
        eng.synchronize()
        rec["load_table_f32_host_s"] = time.perf_counter() - t0
        rec["bytes_equal"] = same_bytes(0, 1)
        t0 = time.perf_counter()
        eng.load_table_f32(1, w_dev, code, chunk_rows=args.chunk_rows)
        eng.synchronize()
        rec["load_table_f32_cuda_s"] = time.perf_counter() - t0
        rec["bytes_equal_cuda"] = same_bytes(0, 1)
        # one update of --update-rows random rows, device pointers
        out_bytes = args.update_rows * (eng.table_tensor(1).shape[1] * eng.table_tensor(1).element_size())
        a, b = torch.empty(out_bytes, dtype=torch.uint8, device="cuda"), torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
        rec["update_rows"], rec["update_out_bytes"] = args.update_rows, out_bytes
        rec["update_us"] = timed_events(lambda: writer.update(1, ids, src))
        rec["update_unique_us"] = timed_events(lambda: writer.update(1, ids_unique, src, unique=True))
        rec["d2d_copy_us"] = timed_events(lambda: b.copy_(a))
        assert writer.report() == 0
        print(json.dumps(rec), flush=True)
        results.append(rec)
    writer.close()
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
