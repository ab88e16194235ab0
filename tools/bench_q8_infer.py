"""The inference forward on int8 row-quantized tables against the fp32 / bf16 forward, on one MI355X (DESIGN.md
section 25).

    python tools/bench_q8_infer.py [--workload kaggle-d128-b2048] [--reps 200] [--quantizer] [--only NAMES]

Tables of the workload's rows at its feature size and batch, N(0,1) x, the workload's index distribution (uniform,
or Zipf over a fixed affine placement); 8 batches cycled, 8 batches per hipGraph replay, the median of five timed
windows of `reps` replays, in us per batch:

    infer_f32_us        HotPath.infer on fp32 tables
    infer_bf16_us       HotPath.infer on bf16 tables
    q8_f32_us           Q8Inference.infer, fp32 x / out (one launch)
    q8_bf16_us          Q8Inference.infer, bf16 x / out (one launch)
    q8_two_launch_us    dlrm_q8_maplookup + dlrm_interact_fwd, bf16 x / out
    q8_two_launch_f32_us  the same with fp32 x / out

Every set is built, timed and freed in turn, and the quantized set is made table by table, so the Terabyte rows
never need more than their bf16 tables.  --quantizer: dlrm_q8_quantize's rate over the workload's whole set in one
launch (bytes read + written per second, best of five) beside bench.py's measured copy rate.  Prints one JSON line.  No
threshold: the comparison base is the existing `infer` in the same run.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dlrm_pkg  # noqa: E402

NB = 8
NAMES = ("infer_f32_us", "infer_bf16_us", "q8_f32_us", "q8_bf16_us", "q8_two_launch_us", "q8_two_launch_f32_us")


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for k in range(NB):
                fn(k)
    torch.cuda.current_stream().wait_stream(s)
    return g


def median_us(g, reps):
    g.replay()
    torch.cuda.synchronize()
    windows = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(reps):
            g.replay()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) * 1e6 / (reps * NB))
    return statistics.median(windows), windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="kaggle-d128-b2048")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--quantizer", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated measurement names (default: all)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_q8_infer: needs the GPU (no CPU fallback, no CPU timing)")
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    w = pkg.WORKLOADS[a.workload]
    if w["lookups"] != 1:
        raise SystemExit("bench_q8_infer: one-hot workloads only")
    rows, D, B = w["rows"], w["dim"], w["batch"]
    T = len(rows)
    only = [n for n in a.only.split(",") if n] or list(NAMES)
    gen = torch.Generator(device=dev).manual_seed(51234)
    rng = np.random.default_rng(51234)
    if w.get("zipf"):
        perms = [pkg.zipf_perm(rng, n) for n in rows]
        idx = [np.stack([pkg.zipf_rows(rng, n, B, w["zipf"], perm=perms[t]) for t, n in enumerate(rows)])
               for _ in range(NB)]
    else:
        idx = [np.stack([rng.integers(0, n, size=B).astype(np.int32) for n in rows]) for _ in range(NB)]
    packs = [pkg.PackedIndices(torch.from_numpy(i).to(dev).reshape(T, B, 1).contiguous()) for i in idx]
    xs = {dt: [torch.randn((B, D), device=dev, generator=gen).to(dt) for _ in range(NB)]
          for dt in (torch.float32, torch.bfloat16)}

    def tables(dt):
        return pkg.EmbeddingTableSet([torch.empty((n, D), dtype=dt, device=dev).uniform_(-n ** -0.5, n ** -0.5, generator=gen)
                                      for n in rows])

    out = {}

    def measure(name, fn, check):
        for k in range(NB):  # eager warm-up of every batch
            fn(k)
        torch.cuda.synchronize()
        check()
        med, windows = median_us(graph_of(fn), a.reps)
        out[name] = round(med, 2)
        out[name.replace("_us", "_windows_us")] = [round(v, 2) for v in windows]

    for name, dt in (("infer_f32_us", torch.float32), ("infer_bf16_us", torch.bfloat16)):
        if name in only:
            hp = pkg.HotPath(tables(dt), B, 1, index_base=0)
            measure(name, lambda k: hp.infer(xs[dt][k], packs[k]), hp.check_bounds)
            assert hp._infer_ys is None  # the one-launch forward
            del hp
            torch.cuda.empty_cache()
    sdt = torch.bfloat16 if w["dtype"] == "bf16" else torch.float32
    out["source_bytes"] = sum(rows) * D * (2 if w["dtype"] == "bf16" else 4)
    if a.quantizer:  # the whole set in one launch, timed
        src = tables(sdt)
        q8 = pkg.QuantizedTableSet.from_tables(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = []
        for _ in range(5):
            e0.record()
            q8.quantize_from(src)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e-3)
        out["quantize_ms"] = round(min(t) * 1e3, 3)
        out["quantize_GBps"] = round((out["source_bytes"] + q8.nbytes) / min(t) / 1e9, 1)
        del src, q8
        torch.cuda.empty_cache()
    if any(n.startswith("q8") for n in only):
        # table by table, so that the source never stands whole beside the quantized set
        qs, sbs = [], []
        for n in rows:
            one = pkg.QuantizedTableSet.from_tables(
                [torch.empty((n, D), dtype=sdt, device=dev).uniform_(-n ** -0.5, n ** -0.5, generator=gen)])
            torch.cuda.synchronize()
            qs.append(one.qs[0])
            sbs.append(one.sbs[0])
            del one
            torch.cuda.empty_cache()
        q8 = pkg.QuantizedTableSet.from_arrays(qs, sbs)
        out["q8_bytes"] = q8.nbytes
        for name, dt, two in (("q8_f32_us", torch.float32, False), ("q8_bf16_us", torch.bfloat16, False),
                              ("q8_two_launch_us", torch.bfloat16, True), ("q8_two_launch_f32_us", torch.float32, True)):
            if name not in only:
                continue
            eng = pkg.Q8Inference(q8, B, 1, dtype=dt)
            fn = (lambda k: eng.two_launch(xs[dt][k], packs[k])) if two else (lambda k: eng.infer(xs[dt][k], packs[k]))
            measure(name, fn, eng.check_bounds)
            assert eng.route == ("two-launch" if two else "fused")
            del eng
        del q8
        torch.cuda.empty_cache()
    if a.quantizer:
        import bench
        out["ceiling"] = bench.measured_ceiling(dev, 128)
    print(json.dumps({
        "metric": "inference forward (lookup + interaction), int8 rows against fp32 / bf16 rows, 1 MI355X",
        "unit": "us per batch", **out,
        "config": {"workload": a.workload, "tables": T, "dim": D, "batch": B, "indices": "zipf" if w.get("zipf") else "uniform",
                   "launch": f"hipGraph replay ({NB} batches per graph)", "windows": 5, "replays_per_window": a.reps},
    }))


if __name__ == "__main__":
    main()
