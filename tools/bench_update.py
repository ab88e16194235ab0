"""The embedding update alone, by optimizer: Descent (dlrm_sgd_update), ADAGrad and RowwiseADAGrad
(dlrm_adagrad_update), SplitDescent (dlrm_split_sgd_update) and StochasticDescent (dlrm_sr_sgd_update), each with
DLRM_UPDATE_PREBUILT on one indexer built once, over a full dt.  SplitDescent and StochasticDescent each run on a
bf16 copy of the tables (the split rule: the truncated high halves, the low halves beside them); on an fp32
workload a Descent-bf16 leg steps another bf16 copy, so the three rules of bf16 tables -- Descent, StochasticDescent
and SplitDescent -- are timed side by side in the same run (bf16_ratio: a leg's time to the Descent leg on bf16
tables).  The stochastic rule moves Descent's bytes: its ratio is the cost of Philox at the write sites plus the
one-thread launch that advances its step, and the sr-step-launch leg times such a one-thread launch alone
(dlrm_sr_sgd_seek, the same kernel shape, in the same captured chain of 200).  The Adagrad rules with the stochastic
store (ADAGrad-sr, RowwiseADAGrad-sr: a seeded optimizer, dlrm_adagrad_create_sr) each step a bf16 copy too, beside
their seedless rules on bf16 tables (on an fp32 workload the legs ADAGrad-bf16 and RowwiseADAGrad-bf16, on a bf16
one ADAGrad and RowwiseADAGrad themselves); sr_cost_us is a stochastic leg's median over its seedless leg's on bf16
tables, the yardstick being StochasticDescent's over Descent's from the same run.

Each leg is a captured graph of 200 launches, replayed until the timed window exceeds 0.5 s; the
legs alternate, five repeats.  One JSON line per run: per shape and leg the median / min / max us
per launch, the leg's algorithmic bytes (gradient rows + twice the touched table rows + twice the
touched state rows or words, from the shapes and the unique-row counts), and each other leg's
time and byte ratios to the Descent leg of the same run.

    python tools/bench_update.py [--workloads kaggle-d128-b2048,kaggle-d16-b2048]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlrm_pkg  # noqa: E402

LAUNCHES, WINDOW_S, REPEATS = 200, 0.5, 5


def bench_shape(pkg, dev, name):
    w = pkg.WORKLOADS[name]
    rows, D, B, L = w["rows"], w["dim"], w["batch"], w["lookups"]
    T = len(rows)
    dtype = torch.float32 if w["dtype"] == "f32" else torch.bfloat16
    esize = 4 if dtype == torch.float32 else 2
    g = torch.Generator(device=dev).manual_seed(7)
    ts = pkg.EmbeddingTableSet([torch.empty((n, D), device=dev).uniform_(-0.05, 0.05, generator=g).to(dtype)
                                for n in rows])
    idx = torch.stack([torch.randint(0, n, (B * L,), device=dev, generator=g, dtype=torch.int32) for n in rows])
    p = pkg.PackedIndices(idx.reshape(T, B, L).contiguous())
    unique = sum(int(torch.unique(idx[t]).numel()) for t in range(T))
    dt = torch.randn((B, (T + 1) * D), device=dev, generator=g) * 1e-3  # x rows first, as dot_back writes it
    ix = pkg.SparseIndexer(T, B * L, dev).build(ts, p, index_base=0)  # once: every leg passes PREBUILT
    grads = pkg.maplookup_pullback(D, ts, p, dt)
    # leg -> (optimizer, tables, their gradient views); the indexer depends on the indices and row counts only
    opts = {"Descent": (pkg.Descent(1e-6), ts, grads), "ADAGrad": (pkg.ADAGrad(1e-6), ts, grads),
            "RowwiseADAGrad": (pkg.RowwiseADAGrad(1e-6), ts, grads)}
    hi = pkg.EmbeddingTableSet([pkg.split_f32(t.data.float())[0] for t in ts])
    opts["SplitDescent"] = (pkg.SplitDescent(1e-6), hi, pkg.maplookup_pullback(D, hi, p, dt))
    if dtype == torch.float32:
        b16 = pkg.EmbeddingTableSet([t.data.clone() for t in hi])
        opts["Descent-bf16"] = (pkg.Descent(1e-6), b16, pkg.maplookup_pullback(D, b16, p, dt))
    sr = pkg.EmbeddingTableSet([t.data.clone() for t in hi])
    sr_opt = pkg.StochasticDescent(1e-6, seed=7)
    opts["StochasticDescent"] = (sr_opt, sr, pkg.maplookup_pullback(D, sr, p, dt))
    opts["sr-step-launch"] = (sr_opt, sr, None)  # (no update: the one-thread launch alone)
    # the Adagrad rules on bf16 tables, round to nearest and stochastic: a bf16 copy per leg
    seedless = {}  # stochastic leg -> its seedless leg on bf16 tables
    for name, rule in (("ADAGrad", pkg.ADAGrad), ("RowwiseADAGrad", pkg.RowwiseADAGrad)):
        seedless[name + "-sr"] = name
        if dtype == torch.float32:
            c = pkg.EmbeddingTableSet([t.data.clone() for t in hi])
            opts[name + "-bf16"] = (rule(1e-6), c, pkg.maplookup_pullback(D, c, p, dt))
            seedless[name + "-sr"] = name + "-bf16"
        c = pkg.EmbeddingTableSet([t.data.clone() for t in hi])
        opts[name + "-sr"] = (rule(1e-6, seed=7), c, pkg.maplookup_pullback(D, c, p, dt))
    seedless["StochasticDescent"] = "Descent-bf16" if dtype == torch.float32 else "Descent"
    graphs = {}
    s = torch.cuda.Stream()
    for leg, (opt, tabs, gr_views) in opts.items():
        def launch(opt=opt, tabs=tabs, gr_views=gr_views):
            if gr_views is None:
                return opt.seek(tabs, 0)
            pkg.update_(opt, tabs, gr_views, ix, index_base=0, prebuilt=True, check_bounds=False)
        launch()  # the state and every first-use allocation, before the capture
        torch.cuda.synchronize()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                for _ in range(LAUNCHES):
                    launch()
        torch.cuda.current_stream().wait_stream(s)
        graphs[leg] = gr
    ts.ctx.check_bounds()
    us = {leg: [] for leg in opts}
    for _ in range(REPEATS):
        for leg, gr in graphs.items():  # the legs alternate
            gr.replay()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n, ms = 0, 0.0
            while ms < WINDOW_S * 1e3:
                t0.record()
                for _ in range(8):
                    gr.replay()
                t1.record()
                t1.synchronize()
                ms += t0.elapsed_time(t1)
                n += 8
            us[leg].append(ms * 1e3 / (n * LAUNCHES))
    ts.ctx.check_bounds()
    grad_bytes = T * B * L * D * 4 if L == 1 else T * B * D * 4
    state_bytes = {"Descent": 0, "ADAGrad": 2 * unique * D * 4, "RowwiseADAGrad": 2 * unique * 4,
                   "SplitDescent": 2 * unique * D * 2, "Descent-bf16": 0, "StochasticDescent": 0}
    table_esize = {"SplitDescent": 2, "Descent-bf16": 2, "StochasticDescent": 2}
    for name in ("ADAGrad", "RowwiseADAGrad"):
        for leg in (name + "-bf16", name + "-sr"):
            state_bytes[leg], table_esize[leg] = state_bytes[name], 2
    out = {"unique_rows": unique, "legs": {}}
    for leg in opts:
        v = us[leg]
        out["legs"][leg] = {"us_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                            "us_max": round(max(v), 3),
                            "bytes": 8 if leg == "sr-step-launch" else
                            grad_bytes + 2 * unique * D * table_esize.get(leg, esize) + state_bytes[leg]}
    base = out["legs"]["Descent"]
    out["descent_spread"] = round((base["us_max"] - base["us_min"]) / base["us_median"], 4)
    for leg in opts:
        if leg == "Descent":
            continue
        out["legs"][leg]["time_ratio"] = round(out["legs"][leg]["us_median"] / base["us_median"], 4)
        out["legs"][leg]["byte_ratio"] = round(out["legs"][leg]["bytes"] / base["bytes"], 4)
    b16_base = out["legs"]["Descent-bf16" if dtype == torch.float32 else "Descent"]["us_median"]
    for leg in ("StochasticDescent", "SplitDescent"):
        out["legs"][leg]["bf16_ratio"] = round(out["legs"][leg]["us_median"] / b16_base, 4)
    for leg, ref in seedless.items():  # what the stochastic store costs each rule on bf16 tables
        out["legs"][leg]["seedless"] = ref
        out["legs"][leg]["sr_cost_us"] = round(out["legs"][leg]["us_median"] - out["legs"][ref]["us_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="kaggle-d128-b2048,kaggle-d16-b2048")
    a = ap.parse_args()
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    res = {"tool": "bench_update", "launches_per_graph": LAUNCHES, "window_s": WINDOW_S, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.workloads.split(","):
        res["shapes"][name] = bench_shape(pkg, dev, name)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
