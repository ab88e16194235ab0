"""The whole hot-path training step with the stochastic rule, four ways, on bf16 copies of a workload's tables:

  (a) descent        Descent on the bf16 tables, the fused and pipelined step (dlrm_step_fwd, dlrm_step_bwd_prepare)
  (b) sr-operator    StochasticDescent on the operator route (HotPath(opt=StochasticDescent)): the fused forward,
                     dlrm_interact_bwd_gather writing every dt row, dlrm_sr_sgd_update(PREBUILT) and its advance
  (c) sr-fused       StochasticDescent with stochastic_step=True and the workload's pipeline mode
                     (dlrm_step_fwd, dlrm_sr_step_bwd_prepare and the advance)
  (d) sr-fused+1     (c)'s chain with one more one-thread launch per step (dlrm_sr_sgd_seek of a spare handle):
                     (d) - (c) is what the step pays for the advance's launch

Each leg is a captured graph of STEPS steps over two alternating index batches (an even count, so the
pipelined legs' two indexers are back in the captured state after every replay), replayed until the timed
window exceeds 0.5 s; the legs alternate, five repeats.  One JSON line: per shape and leg the median / min /
max us per step, (c) / (b), (c) / (a), the spread of (b)'s repeats, whether (c) beats (b) by more than that
spread, and (d) - (c).

The rule keeps no per-row state and no kernel's time depends on the values, so --share lets every leg step one
copy of the tables (the Terabyte rows: 226 GB as bf16, once); by default each leg has its own.

    python tools/bench_sr_step.py [--workloads kaggle-d128-b2048,kaggle-d128-b8192-bf16] [--share] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlrm_pkg  # noqa: E402

STEPS, WINDOW_S, REPEATS = 20, 0.5, 5
LR = 1e-6
LEGS = ("descent", "sr-operator", "sr-fused", "sr-fused+1")
INIT_ROWS = 1 << 22  # rows initialised per call (no temporary larger than 1 GB beside the tables)


def _stepper(hp, mode, x, dout, packs, after):
    """(prime, one graph's worth of steps) of engine `hp` in pipeline `mode` over the alternating batches;
    after(): called behind every step"""
    if mode == "apply":
        def prime():
            hp.prime(packs[0], x, dout, prev=packs[1])

        def run():
            for k in range(STEPS):
                hp.step_prep(x, packs[k % 2], dout, packs[(k + 1) % 2])
                after()
    elif mode == "side":
        def prime():
            hp.prime(packs[0])

        def run():
            for k in range(STEPS):
                hp.step_next(x, packs[k % 2], dout, packs[(k + 1) % 2])
                after()
    else:
        def prime():
            pass

        def run():
            for k in range(STEPS):
                hp.step(x, packs[k % 2], dout)
                after()
    return prime, run


def _tables(rows, D, dev, g):
    out = []
    for n in rows:
        t = torch.empty((n, D), dtype=torch.bfloat16, device=dev)
        for r0 in range(0, n, INIT_ROWS):
            t[r0:r0 + INIT_ROWS].uniform_(-0.05, 0.05, generator=g)
        out.append(t)
    return out


def _indices(pkg, w, rows, B, dev, g):
    """two index batches: uniform, or the workload's Zipf ranks on fixed rows (as bench.py draws them)"""
    if w.get("zipf"):
        rng = np.random.default_rng(11)
        perms = [pkg.zipf_perm(rng, n) for n in rows]
        return [torch.from_numpy(np.stack([pkg.zipf_rows(rng, n, B, w["zipf"], p) for n, p in zip(rows, perms)])).to(dev)
                for _ in range(2)]
    return [torch.stack([torch.randint(0, n, (B,), device=dev, generator=g, dtype=torch.int32) for n in rows])
            for _ in range(2)]


def bench_shape(pkg, dev, name, share):
    w = pkg.WORKLOADS[name]
    rows, D, B = w["rows"], w["dim"], w["batch"]
    T = len(rows)
    wb = dict(w, dtype="bf16")  # (the tables are bf16 here whatever the workload's dtype)
    mode, chunk, parts = pkg.step_pipeline(wb), pkg.step_chunk(wb), pkg.step_parts(wb)
    g = torch.Generator(device=dev).manual_seed(11)
    base = _tables(rows, D, dev, g)
    idx = _indices(pkg, w, rows, B, dev, g)
    packs = [pkg.PackedIndices(i.contiguous()) for i in idx]
    unique = [sum(int(torch.unique(i[t]).numel()) for t in range(T)) for i in idx]
    once = [sum(int((torch.unique(i[t], return_counts=True)[1] == 1).sum()) for t in range(T)) for i in idx]
    x = (torch.randn((B, D), device=dev, generator=g) * 0.1).to(torch.bfloat16)
    F = T + 1
    dout = (torch.randn((B, D + F * (F - 1) // 2), device=dev, generator=g) * 1e-3).to(torch.bfloat16)
    if share:
        one = pkg.EmbeddingTableSet(base)
        sets = {leg: one for leg in LEGS}
    else:
        sets = {leg: pkg.EmbeddingTableSet([t.clone() for t in base]) for leg in LEGS}
        del base
    sr = lambda: pkg.StochasticDescent(LR, seed=7)  # noqa: E731
    kw = dict(index_base=0, pipeline=mode, chunk=chunk, parts=parts)
    engines = {
        "descent": (pkg.HotPath(sets["descent"], B, 1, lr=LR, **kw), mode),
        "sr-operator": (pkg.HotPath(sets["sr-operator"], B, 1, index_base=0, opt=sr()), None),
        "sr-fused": (pkg.HotPath(sets["sr-fused"], B, 1, opt=sr(), stochastic_step=True, **kw), mode),
        "sr-fused+1": (pkg.HotPath(sets["sr-fused+1"], B, 1, opt=sr(), stochastic_step=True, **kw), mode),
    }
    # the spare handle whose seek is leg (d)'s extra one-thread launch
    spare_ts = pkg.EmbeddingTableSet([torch.zeros((8, 8), dtype=torch.bfloat16, device=dev)])
    spare = pkg.StochasticDescent(LR, seed=1)
    spare.handle_of(spare_ts)
    graphs = {}
    s = torch.cuda.Stream()
    for leg, (hp, m) in engines.items():
        assert hp.pipeline == m, (leg, hp.pipeline, m)
        assert hp.step_api == (leg != "sr-operator"), leg
        after = (lambda: spare.seek(spare_ts, 0)) if leg == "sr-fused+1" else (lambda: None)
        prime, run = _stepper(hp, m, x, dout, packs, after)
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
    steps = {leg: hp.opt.step_of(hp.ts) for leg, (hp, _) in engines.items() if hp.opt is not None}
    out = {"pipeline": mode, "chunk": chunk, "parts": parts, "shared_tables": bool(share), "unique_rows": unique,
           "once_hit_rows": once, "legs": {}, "step_words": steps}
    for leg, v in us.items():
        out["legs"][leg] = {"us_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                            "us_max": round(max(v), 3)}
    a, b, c, d = (out["legs"][k] for k in LEGS)
    out["operator_spread_us"] = round(b["us_max"] - b["us_min"], 3)
    out["fused_minus_operator_us"] = round(c["us_median"] - b["us_median"], 3)
    out["fused_beats_operator_by_more_than_its_spread"] = bool(b["us_median"] - c["us_median"] > b["us_max"] - b["us_min"])
    out["fused_over_operator"] = round(c["us_median"] / b["us_median"], 4)
    out["fused_over_descent"] = round(c["us_median"] / a["us_median"], 4)
    out["fused_minus_descent_us"] = round(c["us_median"] - a["us_median"], 3)
    out["advance_launch_us"] = round(d["us_median"] - c["us_median"], 3)
    # what (b) writes and reads back that (c) does not: the once-hit rows' fp32 dt rows
    out["once_hit_dt_bytes_per_step"] = int(2 * statistics.mean(once) * D * 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="kaggle-d128-b2048,kaggle-d128-b8192-bf16")
    ap.add_argument("--share", action="store_true", help="every leg steps one copy of the tables")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    pkg = dlrm_pkg.load()
    dev = torch.device("cuda:0")
    res = {"tool": "bench_sr_step", "steps_per_graph": STEPS, "window_s": WINDOW_S, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.workloads.split(","):
        res["shapes"][name] = bench_shape(pkg, dev, name, a.share)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
