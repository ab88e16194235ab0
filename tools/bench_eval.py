"""Evaluation batch time on one MI355X: what a user pays per batch of a `DLRMModel.test`.

    python tools/bench_eval.py [--workload kaggle-d128-b2048] [--reps 100]

Model and inputs as tools/bench_full_step.py: kaggle_dlrm's MLPs (criteo.jl:408-433), the workload's tables,
synthetic N(0,1) dense features, Bernoulli(0.25) labels, uniform int32 indices; 8 batches cycled, 8 batches per
hipGraph replay.  Three measurements, each the median of five timed windows of `reps` replays:

    eval_batch_us     DLRMModel.predict + Evaluator.add (the evaluation pass's batch)
    predict_us        DLRMModel.predict alone
    train_forward_us  DLRMModel.forward alone (the training forward: on the step kernels it also builds the indexer)

Prints one JSON line.  No threshold: the numbers are a record, the acceptance conditions are structural.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dlrm_pkg  # noqa: E402

NB = 8


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
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval: needs the GPU (no CPU fallback, no CPU timing)")
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    w = pkg.WORKLOADS[a.workload]
    if w["lookups"] != 1 or w["dtype"] != "f32":
        raise SystemExit("bench_eval: one-hot fp32 workloads only")
    rows, D, B = w["rows"], w["dim"], w["batch"]
    T = len(rows)
    gen = torch.Generator(device=dev).manual_seed(51234)
    tables = [torch.empty((n, D), device=dev).uniform_(-n ** -0.5, n ** -0.5, generator=gen) for n in rows]
    bsz, tsz = pkg.kaggle_mlp_sizes(D, T)
    model = pkg.DLRMModel(pkg.random_mlp(bsz, sigmoid_last=False, generator=gen, device=dev), tables,
                          pkg.random_mlp(tsz, sigmoid_last=True, generator=gen, device=dev), B, 1, index_base=0)
    dense = [torch.randn((B, 13), device=dev, generator=gen) for _ in range(NB)]
    labels = [(torch.rand((B,), device=dev, generator=gen) < 0.25).float() for _ in range(NB)]
    packs = [pkg.PackedIndices(torch.stack([torch.randint(0, n, (B,), device=dev, generator=gen, dtype=torch.int32)
                                            for n in rows]).reshape(T, B, 1).contiguous()) for _ in range(NB)]
    ev = pkg.Evaluator(dev)

    def eval_batch(k):
        ev.add(model.predict(dense[k], packs[k]), labels[k])

    def predict(k):
        model.predict(dense[k], packs[k])

    def train_forward(k):
        model.forward(dense[k], packs[k])

    out = {}
    for name, fn in (("eval_batch_us", eval_batch), ("predict_us", predict), ("train_forward_us", train_forward)):
        for k in range(NB):  # eager warm-up of every batch
            fn(k)
        torch.cuda.synchronize()
        model.hot.check_bounds()
        med, windows = median_us(graph_of(fn), a.reps)
        out[name] = round(med, 2)
        out[name.replace("_us", "_windows_us")] = [round(v, 2) for v in windows]
    ev.reset()
    for k in range(NB):
        eval_batch(k)
    res = ev.result()
    print(json.dumps({
        "metric": "DLRM evaluation batch time (predict + add), 1 MI355X", "unit": "us per batch", **out,
        "dtype": "f32", "data": "synthetic (uniform indices, Bernoulli(0.25) labels, N(0,1) dense)",
        "config": {"workload": a.workload, "tables": T, "dim": D, "batch": B,
                   "launch": f"hipGraph replay ({NB} batches per graph)", "windows": 5, "replays_per_window": a.reps},
        "result_of_8_batches": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in res.items()},
    }))


if __name__ == "__main__":
    main()
