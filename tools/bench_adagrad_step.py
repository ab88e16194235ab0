"""The whole hot-path training step with sparse Adagrad, three ways per rule, on a workload's tables (its dtype):

  (a) descent       Descent, the fused and pipelined step (dlrm_step_fwd, dlrm_step_bwd_prepare)
  (b) rule-operator ADAGrad / RowwiseADAGrad on the operator route (HotPath(opt=rule)): the fused forward,
                    dlrm_interact_bwd_gather writing every dt row, dlrm_adagrad_update(PREBUILT)
  (c) rule-fused    the rule with adagrad_step=True and the workload's pipeline mode
                    (dlrm_step_fwd, dlrm_adagrad_step_bwd_prepare)

Each leg is a captured graph of STEPS steps over two alternating index batches (an even count, so the
pipelined legs' two indexers are back in the captured state after every replay), replayed once to warm up and
then until the timed window exceeds 0.5 s; the legs alternate, five repeats.  The two rules run one after the
other, each beside its own Descent leg.  One JSON line: per shape, rule and leg the median / min / max us per
step, (c) / (b) and (c) / (a), the spread of (b)'s repeats, and the state bytes (c) moves beyond (a) per step
from the shapes (element-wise: a touched row's fp32 state row read and written; row-wise: one word).  At D = 128
the row-wise (c) against the element-wise (c) reads the cost of the row-wise rule's two-wave exchange (one block
barrier per 16 features) against the state bytes it saves.

    python tools/bench_adagrad_step.py [--workloads kaggle-d128-b2048,kaggle-d128-b8192-bf16] [--out FILE]
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
LR, EPS = 1e-6, 1e-8


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


def bench_rule(pkg, dev, w, rowwise, tabs, packs, x, dout, mode, chunk, parts):
    B = w["batch"]
    rule = pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad
    sets = {leg: pkg.EmbeddingTableSet([t.clone() for t in tabs]) for leg in ("descent", "rule-operator", "rule-fused")}
    engines = {
        "descent": (pkg.HotPath(sets["descent"], B, 1, lr=LR, index_base=0, pipeline=mode, chunk=chunk, parts=parts), mode),
        "rule-operator": (pkg.HotPath(sets["rule-operator"], B, 1, index_base=0, opt=rule(LR, EPS)), None),
        "rule-fused": (pkg.HotPath(sets["rule-fused"], B, 1, index_base=0, opt=rule(LR, EPS), adagrad_step=True,
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
    fused_bwd = bool(engines["rule-fused"][0].indexer.state() & pkg._lib.IX_SINGLES_DONE)
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
    a, b, c = (out["legs"][k] for k in ("descent", "rule-operator", "rule-fused"))
    out["operator_spread_us"] = round(b["us_max"] - b["us_min"], 3)
    out["fused_minus_operator_us"] = round(c["us_median"] - b["us_median"], 3)
    out["fused_below_operator_by_more_than_spread"] = bool(b["us_median"] - c["us_median"] > b["us_max"] - b["us_min"])
    out["fused_over_operator"] = round(c["us_median"] / b["us_median"], 4)
    out["fused_over_descent"] = round(c["us_median"] / a["us_median"], 4)
    return out


def bench_shape(pkg, dev, name):
    w = pkg.WORKLOADS[name]
    rows, D, B = w["rows"], w["dim"], w["batch"]
    T = len(rows)
    dtype = torch.bfloat16 if w.get("dtype") == "bf16" else torch.float32
    mode, chunk, parts = pkg.step_pipeline(w), pkg.step_chunk(w), pkg.step_parts(w)
    g = torch.Generator(device=dev).manual_seed(11)
    tabs = [torch.empty((n, D), device=dev).uniform_(-0.05, 0.05, generator=g).to(dtype) for n in rows]
    idx = [torch.stack([torch.randint(0, n, (B,), device=dev, generator=g, dtype=torch.int32) for n in rows])
           for _ in range(2)]
    packs = [pkg.PackedIndices(i.contiguous()) for i in idx]
    unique = [sum(int(torch.unique(i[t]).numel()) for t in range(T)) for i in idx]
    x = (torch.randn((B, D), device=dev, generator=g) * 0.1).to(dtype)
    F = T + 1
    dout = (torch.randn((B, D + F * (F - 1) // 2), device=dev, generator=g) * 1e-3).to(dtype)
    out = {"pipeline": mode, "chunk": chunk, "parts": parts, "dtype": str(dtype), "unique_rows": unique, "rules": {}}
    for rowwise in (False, True):
        r = bench_rule(pkg, dev, w, rowwise, tabs, packs, x, dout, mode, chunk, parts)
        # what (c) moves beyond (a): every touched row's state, read and written
        r["state_bytes_per_step"] = int(2 * statistics.mean(unique) * (1 if rowwise else D) * 4)
        out["rules"]["rowwise" if rowwise else "elementwise"] = r
        torch.cuda.empty_cache()
    # what (b) writes and reads back that (c) does not: the once-hit rows' fp32 dt rows (upper bound: all B*T)
    out["full_dt_bytes"] = B * T * D * 4
    e, rw = (out["rules"][k]["legs"]["rule-fused"]["us_median"] for k in ("elementwise", "rowwise"))
    out["rowwise_fused_minus_elementwise_fused_us"] = round(rw - e, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="kaggle-d128-b2048,kaggle-d128-b8192-bf16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    res = {"tool": "bench_adagrad_step", "steps_per_graph": STEPS, "window_s": WINDOW_S, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.workloads.split(","):
        res["shapes"][name] = bench_shape(pkg, dev, name)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
