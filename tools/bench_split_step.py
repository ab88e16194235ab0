"""The whole hot-path training step on split-bf16 tables, three ways, on bf16 copies of a workload's tables:

  (a) descent        Descent on the bf16 tables, the fused and pipelined step (dlrm_step_fwd, dlrm_step_bwd_prepare)
  (b) split-operator SplitDescent on the operator route (HotPath(opt=SplitDescent)): the fused forward,
                     dlrm_interact_bwd_gather writing every dt row, dlrm_split_sgd_update(PREBUILT)
  (c) split-fused    SplitDescent with fused_step=True and the workload's pipeline mode
                     (dlrm_step_fwd, dlrm_split_step_bwd_prepare)

Each leg is a captured graph of STEPS steps over two alternating index batches (an even count, so the
pipelined legs' two indexers are back in the captured state after every replay), replayed until the timed
window exceeds 0.5 s; the legs alternate, five repeats.  One JSON line: per shape and leg the median / min /
max us per step, (c) / (b) and (c) / (a), the spread of (b)'s repeats, and the bytes (c) moves beyond (a)
per step from the shapes: twice the low-half rows of the touched rows.

    python tools/bench_split_step.py [--workloads kaggle-d128-b2048,kaggle-d128-b8192-bf16]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlrm_pkg  # noqa: E402

STEPS, WINDOW_S, REPEATS = 20, 0.5, 5
LR = 1e-6


def _stepper(hp, mode, x, dout, packs):
    """(prime, one graph's worth of steps) of engine `hp` in pipeline `mode` over the alternating batches"""
    if mode == "apply":
        def prime():
            hp.prime(packs[0], x, dout, prev=packs[1])

        def run():
            for k in range(STEPS):
                hp.step_prep(x, packs[k % 2], dout, packs[(k + 1) % 2])
    elif mode == "side":
        def prime():
            hp.prime(packs[0])

        def run():
            for k in range(STEPS):
                hp.step_next(x, packs[k % 2], dout, packs[(k + 1) % 2])
    else:
        def prime():
            pass

        def run():
            for k in range(STEPS):
                hp.step(x, packs[k % 2], dout)
    return prime, run


def bench_shape(pkg, dev, name):
    w = pkg.WORKLOADS[name]
    rows, D, B = w["rows"], w["dim"], w["batch"]
    T = len(rows)
    mode, chunk = pkg.step_pipeline(w), pkg.step_chunk(w)
    wb = dict(w, dtype="bf16")  # (the tables are bf16 here whatever the workload's dtype)
    parts = pkg.step_parts(wb)
    g = torch.Generator(device=dev).manual_seed(11)
    hi = [torch.empty((n, D), device=dev).uniform_(-0.05, 0.05, generator=g).to(torch.bfloat16) for n in rows]
    idx = [torch.stack([torch.randint(0, n, (B,), device=dev, generator=g, dtype=torch.int32) for n in rows])
           for _ in range(2)]
    packs = [pkg.PackedIndices(i.contiguous()) for i in idx]
    unique = [sum(int(torch.unique(i[t]).numel()) for t in range(T)) for i in idx]
    x = (torch.randn((B, D), device=dev, generator=g) * 0.1).to(torch.bfloat16)
    F = T + 1
    dout = (torch.randn((B, D + F * (F - 1) // 2), device=dev, generator=g) * 1e-3).to(torch.bfloat16)
    sets = {leg: pkg.EmbeddingTableSet([t.clone() for t in hi]) for leg in ("descent", "split-operator", "split-fused")}
    del hi
    engines = {
        "descent": (pkg.HotPath(sets["descent"], B, 1, lr=LR, index_base=0, pipeline=mode, chunk=chunk, parts=parts), mode),
        "split-operator": (pkg.HotPath(sets["split-operator"], B, 1, index_base=0, opt=pkg.SplitDescent(LR)), None),
        "split-fused": (pkg.HotPath(sets["split-fused"], B, 1, index_base=0, opt=pkg.SplitDescent(LR), fused_step=True,
                                    pipeline=mode, chunk=chunk, parts=parts), mode),
    }
    graphs = {}
    s = torch.cuda.Stream()
    for leg, (hp, m) in engines.items():
        assert hp.pipeline == m, (leg, hp.pipeline, m)
        prime, run = _stepper(hp, m, x, dout, packs)
        prime()
        run()  # every first-use allocation, before the capture; ends in the state it started from
        torch.cuda.synchronize()
        hp.check_bounds()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                run()
        torch.cuda.current_stream().wait_stream(s)
        graphs[leg] = gr
    us = {leg: [] for leg in engines}
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
            us[leg].append(ms * 1e3 / (n * STEPS))
    for hp, _ in engines.values():
        hp.check_bounds()
    out = {"pipeline": mode, "chunk": chunk, "parts": parts, "unique_rows": unique, "legs": {}}
    for leg, v in us.items():
        out["legs"][leg] = {"us_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                            "us_max": round(max(v), 3)}
    a, b, c = (out["legs"][k] for k in ("descent", "split-operator", "split-fused"))
    out["operator_spread_us"] = round(b["us_max"] - b["us_min"], 3)
    out["fused_minus_operator_us"] = round(c["us_median"] - b["us_median"], 3)
    out["fused_over_operator"] = round(c["us_median"] / b["us_median"], 4)
    out["fused_over_descent"] = round(c["us_median"] / a["us_median"], 4)
    # what (c) moves beyond (a): every touched row's low half, read and written
    out["low_half_bytes_per_step"] = int(2 * statistics.mean(unique) * D * 2)
    # what (b) writes and reads back that (c) does not: the once-hit rows' fp32 dt rows (upper bound: all B*T)
    out["full_dt_bytes"] = B * T * D * 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="kaggle-d128-b2048,kaggle-d128-b8192-bf16")
    a = ap.parse_args()
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    res = {"tool": "bench_split_step", "steps_per_graph": STEPS, "window_s": WINDOW_S, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.workloads.split(","):
        res["shapes"][name] = bench_shape(pkg, dev, name)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
