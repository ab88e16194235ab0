"""The inference forward on int4 row-quantized tables against the fp32, bf16 and int8 forwards, on one MI355X
(DESIGN.md section 29).

    python tools/bench_q4_infer.py [--workload kaggle-d128-b2048] [--reps 200] [--quantizer] [--only NAMES]

Tables of the workload's rows at its feature size and batch, N(0,1) x, the workload's index distribution; 8 batches
cycled, 8 batches per hipGraph replay.  Every variant's tables stay resident and the variants alternate: each of the
five windows times `reps` replays of every variant in turn, so a drift of the machine falls on all of them.  The
median (min - max) of the five windows, in us per batch:

    infer_f32_us        HotPath.infer on fp32 tables
    infer_bf16_us       HotPath.infer on bf16 tables
    q8_bf16_us          Q8Inference.infer, bf16 x / out (one launch)
    q4_f32_us           Q4Inference.infer, fp32 x / out (one launch)
    q4_bf16_us          Q4Inference.infer, bf16 x / out (one launch)
    q4_two_launch_us    dlrm_q4_maplookup + dlrm_interact_fwd, bf16 x / out
    q4_two_launch_f32_us   the same, fp32 x / out
    q4_bags_f32_us      dlrm_q4_bags_interact_fwd, fp32 x / out (one launch)
    q4_bags_bf16_us     dlrm_q4_bags_interact_fwd, bf16 x / out (one launch)
    infer_bags_f32_us   HotPath(bags=True).infer on the fp32 tables of infer_f32_us (dlrm_bags_interact_fwd, one launch)
    infer_bags_bf16_us  the same on the bf16 tables of infer_bf16_us
    fwd_f32_us          HotPath.forward, the operator route's training forward with ys kept, on the fp32 tables
    fwd_bags_f32_us     the same with bags=True, bags_forward=True (dlrm_bags_interact_fwd with ys, one launch)
    fwd_bf16_us, fwd_bags_bf16_us   the two on the bf16 tables

A pooled workload (lookups > 1, e.g. pooled-64x256-l10) or one of more than 31 tables has no one-hot fused kernel:
q4_f32_us, q4_bf16_us and q8_bf16_us are left out there, and the comparison that matters is q4_bags_* against
q4_two_launch_* of the same run.

--quantizer: dlrm_q4_quantize's rate over the workload's whole set in one launch (bytes read + written per second,
best of five) beside bench.py's measured copy rate.  Prints one JSON line.  No threshold: the yardsticks are the
bf16 and the int8 forward of the same run.
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
NAMES = ("infer_f32_us", "infer_bf16_us", "q8_bf16_us", "q4_f32_us", "q4_bf16_us", "q4_two_launch_us",
         "q4_two_launch_f32_us", "q4_bags_f32_us", "q4_bags_bf16_us", "infer_bags_f32_us", "infer_bags_bf16_us",
         "fwd_f32_us", "fwd_bags_f32_us", "fwd_bf16_us", "fwd_bags_bf16_us")
HOT = {  # HotPath variants: name -> (table dtype, bags=, the training forward with ys kept instead of infer)
    "infer_f32_us": (torch.float32, False, False), "infer_bf16_us": (torch.bfloat16, False, False),
    "infer_bags_f32_us": (torch.float32, True, False), "infer_bags_bf16_us": (torch.bfloat16, True, False),
    "fwd_f32_us": (torch.float32, False, True), "fwd_bags_f32_us": (torch.float32, True, True),
    "fwd_bf16_us": (torch.bfloat16, False, True), "fwd_bags_bf16_us": (torch.bfloat16, True, True)}
ONEHOT = ("q8_bf16_us", "q4_f32_us", "q4_bf16_us")  # the one-hot fused kernels: lookups == 1, at most 31 tables


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="kaggle-d128-b2048")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--quantizer", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated measurement names (default: all)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_q4_infer: needs the GPU (no CPU fallback, no CPU timing)")
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    w = pkg.WORKLOADS[a.workload]
    rows, D, B, L = w["rows"], w["dim"], w["batch"], w["lookups"]
    T = len(rows)
    only = [n for n in a.only.split(",") if n] or list(NAMES)
    if L != 1 or T > 31:
        only = [n for n in only if n not in ONEHOT]
    else:  # the bags forward and the kept ys are for pooled bags and more than 31 tables
        only = [n for n in only if "bags" not in n and not n.startswith("fwd")]
    gen = torch.Generator(device=dev).manual_seed(51234)
    rng = np.random.default_rng(51234)
    if w.get("zipf"):
        perms = [pkg.zipf_perm(rng, n) for n in rows]
        idx = [np.stack([pkg.zipf_rows(rng, n, B * L, w["zipf"], perm=perms[t]) for t, n in enumerate(rows)])
               for _ in range(NB)]
    else:
        idx = [np.stack([rng.integers(0, n, size=B * L).astype(np.int32) for n in rows]) for _ in range(NB)]
    packs = [pkg.PackedIndices(torch.from_numpy(i).to(dev).reshape(T, B, L).contiguous()) for i in idx]
    xs = {dt: [torch.randn((B, D), device=dev, generator=gen).to(dt) for _ in range(NB)]
          for dt in (torch.float32, torch.bfloat16)}
    sdt = torch.bfloat16 if w["dtype"] == "bf16" else torch.float32

    def tables(dt):
        return pkg.EmbeddingTableSet([torch.empty((n, D), dtype=dt, device=dev).uniform_(-n ** -0.5, n ** -0.5, generator=gen)
                                      for n in rows])

    out = {"source_bytes": sum(rows) * D * (2 if w["dtype"] == "bf16" else 4)}
    if a.quantizer:  # the whole set in one launch, timed
        src = tables(sdt)
        q4 = pkg.Quantized4TableSet.from_tables(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = []
        for _ in range(5):
            e0.record()
            q4.quantize_from(src)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e-3)
        out["quantize_ms"] = round(min(t) * 1e3, 3)
        out["quantize_GBps"] = round((out["source_bytes"] + q4.nbytes) / min(t) / 1e9, 1)
        del src, q4
        torch.cuda.empty_cache()

    def quantized(cls):  # table by table, so that the source never stands whole beside the quantized set
        parts = []
        for n in rows:
            one = cls.from_tables([torch.empty((n, D), dtype=sdt, device=dev).uniform_(-n ** -0.5, n ** -0.5, generator=gen)])
            torch.cuda.synchronize()
            parts.append(one)
            torch.cuda.empty_cache()
        if cls is pkg.QuantizedTableSet:
            return cls.from_arrays([p.qs[0] for p in parts], [p.sbs[0] for p in parts])
        return cls.from_arrays([p.rows[0] for p in parts], D)

    variants = {}  # name -> (graph, what keeps its memory alive)
    sets = {}      # one table set per dtype, shared by the HotPath variants on it
    for name, (dt, bags, fwd) in HOT.items():
        if name in only:
            if dt not in sets:
                sets[dt] = tables(dt)
            # (the training forward: ys kept, no side-stream indexer build inside the timed graph)
            hp = pkg.HotPath(sets[dt], B, L, index_base=0, bags=bags, **({"materialize_ys": True, "overlap_indexer": False,
                                                                         "deterministic": False, "bags_forward": bags} if fwd else {}))
            variants[name] = (lambda k, call=hp.forward if fwd else hp.infer, dt=dt: call(xs[dt][k], packs[k]), hp)
    if "q8_bf16_us" in only:
        q8 = quantized(pkg.QuantizedTableSet)
        out["q8_bytes"] = q8.nbytes
        eng = pkg.Q8Inference(q8, B, 1, dtype=torch.bfloat16)
        variants["q8_bf16_us"] = (lambda k, eng=eng: eng.infer(xs[torch.bfloat16][k], packs[k]), eng)
    if any(n.startswith("q4") for n in only):
        q4 = quantized(pkg.Quantized4TableSet)
        out["q4_bytes"] = q4.nbytes
        for name, dt, how in (("q4_f32_us", torch.float32, "infer"), ("q4_bf16_us", torch.bfloat16, "infer"),
                              ("q4_two_launch_us", torch.bfloat16, "two_launch"),
                              ("q4_two_launch_f32_us", torch.float32, "two_launch"),
                              ("q4_bags_f32_us", torch.float32, "bags_fused"),
                              ("q4_bags_bf16_us", torch.bfloat16, "bags_fused")):
            if name in only:
                eng = pkg.Q4Inference(q4, B, L, dtype=dt)
                variants[name] = (lambda k, call=getattr(eng, how), dt=dt: call(xs[dt][k], packs[k]), eng)
    graphs = {}
    for name, (fn, eng) in variants.items():
        for k in range(NB):  # eager warm-up of every batch
            r = fn(k)
            assert "q4_bags" not in name or r == pkg._lib.OK, (name, r)  # (the raw call's status: launched)
        torch.cuda.synchronize()
        eng.check_bounds()
        if name.startswith("q") and "bags" not in name:
            assert eng.route == ("two-launch" if "two_launch" in name else "fused"), (name, eng.route)
        if name in HOT and HOT[name][1]:
            assert (eng.fwd_route if HOT[name][2] else eng.infer_route) == "bags", name
        graphs[name] = graph_of(fn)
        graphs[name].replay()
    torch.cuda.synchronize()
    windows = {name: [] for name in graphs}
    for _ in range(5):
        for name, g in graphs.items():
            t0 = time.perf_counter()
            for _ in range(a.reps):
                g.replay()
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) * 1e6 / (a.reps * NB))
    for name, v in windows.items():
        out[name] = round(statistics.median(v), 2)
        out[name.replace("_us", "_windows_us")] = [round(x, 2) for x in v]
    if a.quantizer:
        import bench
        out["ceiling"] = bench.measured_ceiling(dev, 128)
    print(json.dumps({
        "metric": "inference forward (lookup + interaction), int4 rows against fp32 / bf16 / int8 rows, 1 MI355X",
        "unit": "us per batch", **out,
        "config": {"workload": a.workload, "tables": T, "dim": D, "batch": B, "lookups": L, "indices": "zipf" if w.get("zipf") else "uniform",
                   "launch": f"hipGraph replay ({NB} batches per graph), variants alternating", "windows": 5,
                   "replays_per_window": a.reps},
    }))


if __name__ == "__main__":
    main()
