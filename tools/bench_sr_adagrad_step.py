"""The whole hot-path training step with a seeded Adagrad rule (the stochastic store), three ways per rule, on a
workload's rows as bf16 tables (tools/bench_adagrad_step.py's method and stepper):

  (a) seedless-fused  ADAGrad / RowwiseADAGrad without a seed, adagrad_step=True and the workload's pipeline mode
                      (dlrm_step_fwd, dlrm_adagrad_step_bwd_prepare): the same step with the round-to-nearest store
  (b) seeded-operator the seeded rule on the operator route (HotPath(opt=rule(seed=s))): the fused forward,
                      dlrm_interact_bwd_gather writing every dt row, dlrm_adagrad_update(PREBUILT), the advance
  (c) seeded-fused    the seeded rule with sr_adagrad_step=True and the workload's pipeline mode
                      (dlrm_step_fwd, dlrm_sr_adagrad_step_bwd_prepare, the advance)

Each leg has its own bf16 copy of the tables and is a captured graph of STEPS steps over two alternating index
batches, replayed once to warm up and then until the timed window exceeds 0.5 s; the legs alternate, five repeats.
One JSON line: per shape, rule and leg the median / min / max us per step, (c) / (b), the spread of (b)'s repeats
and whether (c) is below (b) by more than it, and (c) - (a), the cost of the stochastic store in the fused step.

    python tools/bench_sr_adagrad_step.py [--workloads kaggle-d128-b2048,kaggle-d128-b8192-bf16] [--seed S] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlrm_pkg  # noqa: E402
from bench_adagrad_step import EPS, LR, REPEATS, STEPS, WINDOW_S, _stepper  # noqa: E402

LEGS = ("seedless-fused", "seeded-operator", "seeded-fused")


def bench_rule(pkg, w, rowwise, tabs, packs, x, dout, mode, chunk, parts, seed):
    B = w["batch"]
    rule = pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad
    sets = {leg: pkg.EmbeddingTableSet([t.clone() for t in tabs]) for leg in LEGS}
    pipe = dict(pipeline=mode, chunk=chunk, parts=parts)
    engines = {
        "seedless-fused": (pkg.HotPath(sets[LEGS[0]], B, 1, index_base=0, opt=rule(LR, EPS), adagrad_step=True, **pipe), mode),
        "seeded-operator": (pkg.HotPath(sets[LEGS[1]], B, 1, index_base=0, opt=rule(LR, EPS, seed=seed)), None),
        "seeded-fused": (pkg.HotPath(sets[LEGS[2]], B, 1, index_base=0, opt=rule(LR, EPS, seed=seed),
                                     sr_adagrad_step=True, **pipe), mode),
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
    bit = pkg._lib.IX_SINGLES_SR_ROWWISE if rowwise else pkg._lib.IX_SINGLES_SR_ADAGRAD
    fused_bwd = bool(engines["seeded-fused"][0].indexer.state() & bit)
    us = {leg: [] for leg in engines}
    for _ in range(REPEATS):
        for leg, gr in graphs.items():  # the legs alternate
            gr.replay()  # warm-up
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
    out = {"fused_backward": fused_bwd, "legs": {}}
    for leg, v in us.items():
        out["legs"][leg] = {"us_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                            "us_max": round(max(v), 3)}
    a, b, c = (out["legs"][k] for k in LEGS)
    out["operator_spread_us"] = round(b["us_max"] - b["us_min"], 3)
    out["fused_minus_operator_us"] = round(c["us_median"] - b["us_median"], 3)
    out["fused_below_operator_by_more_than_spread"] = bool(b["us_median"] - c["us_median"] > b["us_max"] - b["us_min"])
    out["fused_over_operator"] = round(c["us_median"] / b["us_median"], 4)
    out["seeded_minus_seedless_fused_us"] = round(c["us_median"] - a["us_median"], 3)
    return out


def bench_shape(pkg, dev, name, seed):
    w = pkg.WORKLOADS[name]
    rows, D, B = w["rows"], w["dim"], w["batch"]
    T = len(rows)
    dtype = torch.bfloat16  # (the rules round bf16 tables: an fp32 workload's rows are taken as bf16)
    mode, chunk, parts = pkg.step_pipeline(w), pkg.step_chunk(w), pkg.step_parts(w)
    g = torch.Generator(device=dev).manual_seed(11)
    tabs = [torch.empty((n, D), device=dev).uniform_(-0.05, 0.05, generator=g).to(dtype) for n in rows]
    idx = [torch.stack([torch.randint(0, n, (B,), device=dev, generator=g, dtype=torch.int32) for n in rows])
           for _ in range(2)]
    packs = [pkg.PackedIndices(i.contiguous()) for i in idx]
    x = (torch.randn((B, D), device=dev, generator=g) * 0.1).to(dtype)
    F = T + 1
    dout = (torch.randn((B, D + F * (F - 1) // 2), device=dev, generator=g) * 1e-3).to(dtype)
    out = {"pipeline": mode, "chunk": chunk, "parts": parts, "dtype": str(dtype), "rules": {}}
    for rowwise in (False, True):
        out["rules"]["rowwise" if rowwise else "elementwise"] = bench_rule(pkg, w, rowwise, tabs, packs, x, dout, mode,
                                                                          chunk, parts, seed)
        torch.cuda.empty_cache()
    out["full_dt_bytes"] = B * T * D * 4  # what (b) writes and reads back at most beyond (c)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="kaggle-d128-b2048,kaggle-d128-b8192-bf16")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    res = {"tool": "bench_sr_adagrad_step", "steps_per_graph": STEPS, "window_s": WINDOW_S, "repeats": REPEATS,
           "seed": a.seed, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.workloads.split(","):
        res["shapes"][name] = bench_shape(pkg, dev, name, a.seed)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
