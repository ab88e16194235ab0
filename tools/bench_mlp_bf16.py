"""`DLRMModel.predict` with the fused bf16 MLP chains against the fp32 MLPs, on one MI355X.

    python tools/bench_mlp_bf16.py [--batches 2048,8192] [--dtype f32|bf16] [--reps 50]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_mlp_bf16.py --trace     (kernel times, a run of its own)

The Kaggle model (bottom 13-512-256-D, top W-1024-1024-512-256-1, D = 128, 26 tables), synthetic inputs as
tools/bench_eval.py.  Per batch size, `predict` four ways, 8 batches per hipGraph replay:

    fp32        the fp32 MLPs on hipBLASLt (predict as it was)
    fused       predict(mlp="bf16"): one launch per MLP (csrc/mlp_bf16.hip)
    fused_fp8   predict(mlp="fp8"): one MXFP8 launch per MLP (csrc/mlp_fp8.hip)
    torch_bf16  the yardstick: per-layer torch bf16 `_addmm_activation` on bf16 copies of the weights

The four alternate window by window in one process; each figure is the median and the min .. max of five windows
of `reps` replays.  The tile height is the plan's (printed as mt); DLRM_MLP_MT=16|32 (bf16) and
DLRM_MLP_FP8_MT=16|32|64 (fp8) in the environment override it for the comparison of the tiles.  Prints one JSON line per batch size.  --trace: no timing, 20 eager calls of each
variant at the first batch size, for the profiler.
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


def torch_bf16_mlp(mlp):
    Ws, bs = [w.to(torch.bfloat16) for w in mlp.W], [b.to(torch.bfloat16) for b in mlp.b]

    def run(x):
        for i, (w, b) in enumerate(zip(Ws, bs)):
            last = i == len(Ws) - 1 and mlp.sigmoid_last
            x = torch.addmm(b, x, w.t()) if last else torch._addmm_activation(b, x, w.t())
        return x
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2048,8192")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_bf16: needs the GPU (no CPU fallback, no CPU timing)")
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    rows, D = pkg.KAGGLE_EMBEDDING_SIZES, 128
    T = len(rows)
    tdtype = torch.float32 if a.dtype == "f32" else torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(51234)
    tables = [torch.empty((n, D), device=dev).uniform_(-n ** -0.5, n ** -0.5, generator=gen).to(tdtype) for n in rows]
    bsz, tsz = pkg.kaggle_mlp_sizes(D, T)
    for B in [int(b) for b in a.batches.split(",")]:
        model = pkg.DLRMModel(pkg.random_mlp(bsz, sigmoid_last=False, generator=gen, device=dev), tables,
                              pkg.random_mlp(tsz, sigmoid_last=True, generator=gen, device=dev), B, 1, index_base=0)
        dense = [torch.randn((B, 13), device=dev, generator=gen) for _ in range(NB)]
        packs = [pkg.PackedIndices(torch.stack([torch.randint(0, n, (B,), device=dev, generator=gen, dtype=torch.int32)
                                                for n in rows]).reshape(T, B, 1).contiguous()) for _ in range(NB)]
        bot16, top16 = torch_bf16_mlp(model.bottom), torch_bf16_mlp(model.top)

        def fp32(k):
            return model.predict(dense[k], packs[k])

        def fused(k):
            return model.predict(dense[k], packs[k], mlp="bf16")

        def fused_fp8(k):
            return model.predict(dense[k], packs[k], mlp="fp8")

        def torch_bf16(k):
            x = bot16(dense[k].to(torch.bfloat16))
            return top16(model.hot.infer(x.to(tdtype), packs[k]).to(torch.bfloat16)).float()

        variants = (("fp32", fp32), ("fused", fused), ("fused_fp8", fused_fp8), ("torch_bf16", torch_bf16))
        if a.trace:
            for _, fn in variants:
                for i in range(20):
                    fn(i % NB)
            torch.cuda.synchronize()
            return
        graphs, diff = {}, {}
        ref = fp32(0).clone()
        for name, fn in variants:
            for k in range(NB):
                fn(k)
            torch.cuda.synchronize()
            diff[name] = float((fn(0) - ref).abs().max())
            graphs[name] = graph_of(fn)
            graphs[name].replay()
        torch.cuda.synchronize()
        model.hot.check_bounds()
        windows = {name: [] for name, _ in variants}
        for _ in range(5):
            for name, _ in variants:
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    graphs[name].replay()
                torch.cuda.synchronize()
                windows[name].append((time.perf_counter() - t0) * 1e6 / (a.reps * NB))
        plan = [pkg.mlp_bf16_plan(s, B, pkg._lib.F32 if i == 0 or a.dtype == "f32" else pkg._lib.BF16) for i, s in
                enumerate((bsz, tsz))]
        plan8 = [pkg.mlp_fp8_plan(s, B, pkg._lib.F32 if i == 0 or a.dtype == "f32" else pkg._lib.BF16) for i, s in
                 enumerate((bsz, tsz))]
        print(json.dumps({
            "metric": "DLRMModel.predict per batch, 1 MI355X", "unit": "us", "batch": B, "tables_dtype": a.dtype,
            "mt": [p["mt"] for p in plan], "grid": [p["grid"] for p in plan], "lds_bytes": [p["lds_bytes"] for p in plan],
            "mt_fp8": [p["mt"] for p in plan8], "lds_bytes_fp8": [p["lds_bytes"] for p in plan8],
            **{name: {"median": round(statistics.median(w), 2), "min": round(min(w), 2), "max": round(max(w), 2)}
               for name, w in windows.items()},
            "max_abs_logit_difference_from_fp32": {k: round(v, 5) for k, v in diff.items()},
            "launch": f"hipGraph replay ({NB} batches per graph), 5 windows of {a.reps} replays, variants alternating",
        }), flush=True)


if __name__ == "__main__":
    main()
