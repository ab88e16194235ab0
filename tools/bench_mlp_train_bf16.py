"""`DLRMModel.step` with the MLPs trained on the bf16 MFMA kernels against the fp32 step, on one MI355X (DESIGN.md
section 28).

    python tools/bench_mlp_train_bf16.py [--batches 2048,8192] [--dtype f32|bf16] [--reps 50]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_mlp_train_bf16.py --trace   (kernel times, its own run)

The Kaggle model (bottom 13-512-256-D, top W-1024-1024-512-256-1, D = 128, 26 tables), synthetic inputs as
tools/bench_mlp_bf16.py.  Per batch size, the full step three ways, one step per hipGraph replay:

    fp32        DLRMModel.step as it was: fp32 hipBLASLt GEMMs, relu seams, conversions
    bf16        DLRMModel(..., mlp="bf16").step (csrc/mlp_train.hip)
    torch_bf16  the yardstick, only here: the same step with per-layer torch bf16 `mm` on bf16 copies of the weights
                (one _foreach_copy_ per MLP and step), the relu pullback and bias sums as torch ops, fp32 masters

The three alternate window by window in one process; each figure is the median and the min .. max of five windows of
`reps` replays.  Before the timing, one step of fp32 and bf16 on the same batch, tables and weights gives the largest
logit difference and the loss difference.  Prints one JSON line per batch size.  --trace: no timing, 20 eager steps of
fp32 and bf16 at the first batch size, for the profiler.
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


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return g


class TorchBf16Step:
    """The yardstick: DLRMModel.step with every MLP GEMM a torch bf16 mm."""

    def __init__(self, model):
        self.m = model
        self.w16 = {id(mlp): [torch.empty_like(w, dtype=torch.bfloat16) for w in mlp.W] for mlp in (model.bottom, model.top)}

    def fwd(self, mlp, x):
        W16 = self.w16[id(mlp)]
        torch._foreach_copy_(W16, mlp.W)
        acts = [x]
        for i, w in enumerate(W16):
            z = torch.mm(acts[-1], w.t()) + mlp.b[i].to(torch.bfloat16)
            acts.append(z if i == len(W16) - 1 and mlp.sigmoid_last else torch.relu(z))
        return acts

    def bwd(self, mlp, acts, g, need_dx):
        W16 = self.w16[id(mlp)]
        for i in reversed(range(len(W16))):
            if not (i == len(W16) - 1 and mlp.sigmoid_last):
                g = torch.ops.aten.threshold_backward(g, acts[i + 1], 0.0)
                torch.sum(g, dim=0, dtype=torch.float32, out=mlp.gb[i])
            mlp.gW[i].copy_(torch.mm(g.t(), acts[i]))
            if i > 0 or need_dx:
                g = torch.mm(g, W16[i])
        return g

    def __call__(self, dense, sparse, labels):
        m = self.m
        ab = self.fwd(m.bottom, dense.to(torch.bfloat16))
        out = m.hot.forward(ab[-1].to(m.tdtype), sparse)
        at = self.fwd(m.top, out.to(torch.bfloat16))
        m.head(at[-1].float(), labels)
        dout = self.bwd(m.top, at, m._dz.to(torch.bfloat16), True)
        dx = m.hot.backward(sparse, dout.to(m.tdtype).contiguous())
        self.bwd(m.bottom, ab, dx.to(torch.bfloat16), False)
        m.top.sgd_(m.lr)
        m.bottom.sgd_(m.lr)
        return m.loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2048,8192")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_train_bf16: needs the GPU (no CPU fallback, no CPU timing)")
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    rows, D = pkg.KAGGLE_EMBEDDING_SIZES, 128
    T = len(rows)
    tdtype = torch.float32 if a.dtype == "f32" else torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(51234)
    tables = [torch.empty((n, D), device=dev).uniform_(-n ** -0.5, n ** -0.5, generator=gen).to(tdtype) for n in rows]
    bsz, tsz = pkg.kaggle_mlp_sizes(D, T)
    for B in [int(b) for b in a.batches.split(",")]:
        def model(mlp, tabs):
            g2 = torch.Generator(device=dev).manual_seed(99)
            return pkg.DLRMModel(pkg.random_mlp(bsz, sigmoid_last=False, generator=g2, device=dev), tabs,
                                 pkg.random_mlp(tsz, sigmoid_last=True, generator=g2, device=dev), B, 1, index_base=0, mlp=mlp)

        # (the bf16 model on its own copy of the tables, so that the two first steps start from the same state)
        m32, m16, myd = model(None, tables), model("bf16", [t.clone() for t in tables]), model(None, tables)
        yard = TorchBf16Step(myd)
        dense = torch.randn((B, 13), device=dev, generator=gen)
        labels = (torch.rand((B,), device=dev, generator=gen) < 0.3).float()
        sparse = pkg.PackedIndices(torch.stack([torch.randint(0, n, (B,), device=dev, generator=gen, dtype=torch.int32)
                                                for n in rows]).reshape(T, B, 1).contiguous())
        variants = (("fp32", lambda: m32.step(dense, sparse, labels)), ("bf16", lambda: m16.step(dense, sparse, labels)),
                    ("torch_bf16", lambda: yard(dense, sparse, labels)))
        if a.trace:
            for _, fn in variants[:2]:
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
            return
        l32, l16 = float(variants[0][1]()), float(variants[1][1]())
        dz = float((m32.top._acts[-1].reshape(-1) - m16._z16.reshape(-1)).abs().max())
        graphs = {}
        for name, fn in variants:
            fn()
            torch.cuda.synchronize()
            graphs[name] = graph_of(fn)
            graphs[name].replay()
        torch.cuda.synchronize()
        m16.hot.check_bounds()
        windows = {name: [] for name, _ in variants}
        for _ in range(5):
            for name, _ in variants:
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    graphs[name].replay()
                torch.cuda.synchronize()
                windows[name].append((time.perf_counter() - t0) * 1e6 / a.reps)
        med = {name: statistics.median(w) for name, w in windows.items()}
        print(json.dumps({
            "metric": "DLRMModel.step, 1 MI355X", "unit": "us", "batch": B, "tables_dtype": a.dtype,
            **{name: {"median": round(med[name], 2), "min": round(min(w), 2), "max": round(max(w), 2)}
               for name, w in windows.items()},
            "bf16_over_fp32": round(med["bf16"] / med["fp32"], 4), "bf16_over_torch_bf16": round(med["bf16"] / med["torch_bf16"], 4),
            "first_step_max_abs_logit_difference": round(dz, 6), "first_step_loss": {"fp32": l32, "bf16": l16},
            "wgrad_slabs": [p.plan["slabs"] for p in m16._mlp16],
            "launch": f"hipGraph replay (one step per graph), 5 windows of {a.reps} replays, variants alternating",
        }), flush=True)
        del m32, m16, myd, yard, graphs


if __name__ == "__main__":
    main()
