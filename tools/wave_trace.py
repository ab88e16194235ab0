"""Per-sample wave timelines of the forward and backward bodies (library built with
-DDLRM_WTRACE, tools/wave_trace.sh): BASELINE metric shape, uniform indices.  For each launch
prints, relative to the first wave's start (us): the spread of wave starts, and the p50/p90/max
of each phase.  fwd slots: 0 start, 1 indices returned, 2 first column step landed, 3 last column
step landed, 4 MFMAs done, 5 output stores issued; printed overall and for the first / second
workgroup of a CU (samples < B/2 / >= B/2), with each wave's landing spread (last landed - first
landed) and MFMA tail (MFMAs done - last landed).  bwd slots: 0 start, 1 S built, 2 super-block 0
MFMA done, 3 super-block 1 MFMA done, 4 stores issued.  The split step backward: 0 start, 1 S barrier,
2 MFMAs done, 3 stores issued, 4 stores drained; its tracked schedule (bwd_split_tracked) stamps seven
slots from registers after the wave's last store: 0 start, 1 indices back, 2 first row load issued,
3 first step landed, 4 last step landed, 5 MFMAs done, 6 last store issued.
Modes (arguments): ops (lone operator launches), step (lone step_fwd / step_bwd launches),
metric (the forward and the backward inside the metric step: a graph of 8 consecutive training steps
as bench.py runs them, the stamps of the last step's launches)."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlrm_pkg  # noqa: E402

pkg = dlrm_pkg.load()
lib = pkg._lib.load(os.environ["DLRM_HIP_LIB"])
dev = torch.device("cuda:0")
rows = pkg.KAGGLE_EMBEDDING_SIZES
B, D = 2048, int(os.environ.get("DLRM_WT_D", "128"))  # DLRM_WT_D=16: configs[1]
T = len(rows)
g = torch.Generator(device=dev).manual_seed(1)
ts = pkg.EmbeddingTableSet([torch.empty((n, D), device=dev).uniform_(-0.05, 0.05, generator=g) for n in rows])
packs = [pkg.PackedIndices(torch.stack([torch.randint(0, n, (B,), device=dev, generator=g) for n in rows])
                           .to(torch.int32).reshape(T, B, 1)) for _ in range(4)]
hp = pkg.HotPath(ts, B, 1, lr=0.01, index_base=0)
x = torch.randn((B, D), device=dev, generator=g)
dout = torch.randn((B, hp.width), device=dev, generator=g) * 1e-3
# (a library from before the backward's seven stamps has six slots per kind and no slot count to ask for)
NSLOT = lib.dlrm_debug_wtrace_slots() if hasattr(lib, "dlrm_debug_wtrace_slots") else 6
buf = (ctypes.c_ulonglong * (2 * NSLOT * 8192))()
lib.dlrm_debug_wtrace.restype = ctypes.c_int


FWD = ["start", "indices returned", "first step landed", "last step landed", "mfma done", "stores issued"]
BWD_SPLIT = ["start", "S barrier", "mfma done", "stores issued", "stores drained"]
BWD_TRACKED = ["start", "indices back", "first row load issued", "first step landed", "last step landed", "mfma done",
               "last store issued"]


def pcts(d):
    return f"p50 {np.percentile(d, 50):.2f} p90 {np.percentile(d, 90):.2f} max {d.max():.2f}"


def show(kind, slots, names, sel=None):
    lib.dlrm_debug_wtrace(buf)
    a = np.array(buf, dtype=np.int64).reshape(2, NSLOT, 8192)[kind][:, :B]
    t0 = a[0].min()
    rel = (a - t0) / 100.0  # us
    if sel is not None:
        a, rel = a[:, sel], rel[:, sel]
    print(f"  start spread: p50 {np.percentile(rel[0], 50):.2f} p90 {np.percentile(rel[0], 90):.2f} max {rel[0].max():.2f}")
    # slots a launch never writes (e.g. super-block 1 when D <= 64) are skipped
    used = [s for s in range(slots) if a[s].max() > 0]
    for prev, s in zip(used, used[1:]):
        d = rel[s] - rel[prev]
        print(f"  {names[s]:28s} dur p50 {np.percentile(d, 50):.2f} p90 {np.percentile(d, 90):.2f} max {d.max():.2f}"
              f" | done at p50 {np.percentile(rel[s], 50):.2f} max {rel[s].max():.2f}")
    if kind == 0 and a[3].max() > 0:
        print(f"  {'landing spread (last-first)':28s} {pcts(rel[3] - rel[2])}")
        print(f"  {'mfma tail (done-last landed)':28s} {pcts(rel[4] - rel[3])}")


def show_bwd():
    """The step backward's phases: the tracked schedule's seven slots where the launch stamped them, else
    the kernel text's five."""
    lib.dlrm_debug_wtrace(buf)
    a = np.array(buf, dtype=np.int64).reshape(2, NSLOT, 8192)[1][:, :B] / 100.0
    if NSLOT > 6 and a[6].max() > 0:
        show(1, 7, BWD_TRACKED)
        print(f"  {'landing spread (last-first)':28s} {pcts(a[4] - a[3])}")
        print(f"  {'mfma tail (done-last landed)':28s} {pcts(a[5] - a[4])}")
        print(f"  {'wave life (last store-start)':28s} {pcts(a[6] - a[0])}")
    else:
        show(1, 5, BWD_SPLIT)
        print(f"  {'wave life (stores issued-start)':28s} {pcts(a[3] - a[0])}")


def show_fwd():
    """The forward's six phases: every sample, then the first and the second workgroup of a CU."""
    b = np.arange(B)
    for label, sel in (("all samples", None), (f"samples < {B // 2} (first workgroup of a CU)", b < B // 2),
                       (f"samples >= {B // 2} (second workgroup of a CU)", b >= B // 2)):
        print(f" {label}:")
        show(0, 6, FWD, sel)


for mode in sys.argv[1:] or ["ops"]:
    for k in range(6):  # warm
        hp.step(x, packs[k % 4], dout)
    torch.cuda.synchronize()
    if mode == "ops":
        print("fwd (lookup_interact_fwd, no ys):")
        hp.lookup_interact_fwd(x, packs[1]); torch.cuda.synchronize()
        show_fwd()
        print("bwd_gather (no indexer):")
        hp.interact_bwd(dout, x=x, idx=packs[1]); torch.cuda.synchronize()
        show(1, 5, ["start", "S built", "sb0 mfma", "sb1 mfma", "stores"])
        if os.environ.get("DLRM_BWD_SPLIT", "1") != "0":
            print("  (split backward: slots = start, S barrier, MFMA done, stores issued, stores drained)")
    elif mode == "metric":
        # the engine and the step bench.py times for this shape, 8 steps (two cycles of the four
        # batches, so a replay ends in the state it was captured in) in one graph
        w = dict(pkg.WORKLOADS["kaggle-d128-b2048" if D == 128 else "kaggle-d16-b2048"])
        eng = pkg.HotPath(ts, B, 1, lr=0.01, index_base=0, pipeline=pkg.step_pipeline(w), chunk=pkg.step_chunk(w),
                          parts=pkg.step_parts(w))

        def steps():
            for k in range(8):
                if eng.pipeline == "apply":
                    eng.step_prep(x, packs[k % 4], dout, packs[(k + 1) % 4])
                elif eng.pipeline:
                    eng.step_next(x, packs[k % 4], dout, packs[(k + 1) % 4])
                else:
                    eng.step(x, packs[k % 4], dout)

        def prime():
            if eng.pipeline:
                eng.prime(packs[0], x=x, dout=dout, prev=packs[3])

        prime()
        steps()
        prime()
        cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                steps()
        cur.wait_stream(side)
        for _ in range(4):
            prime()
            gr.replay()
        torch.cuda.synchronize()
        print(f"forward inside the metric step (pipeline {eng.pipeline}; graph of 8 steps, last step's forward):")
        show_fwd()
        print("backward inside the metric step (last step's backward):")
        show_bwd()
    else:
        print("step_fwd:")
        hp.step_fwd(x, packs[2]); torch.cuda.synchronize()
        show_fwd()
        print("step_bwd (BWD_ONLY):")
        hp.step_bwd(dout, x=x, idx=packs[2], flags=pkg._lib.STEP_BWD_ONLY); torch.cuda.synchronize()
        show(1, 5, ["start", "S built", "sb0 mfma", "sb1 mfma", "stores"])
        if os.environ.get("DLRM_BWD_SPLIT", "1") != "0":
            print("  (split backward: slots = start, S barrier, MFMA done, stores issued, stores drained)")
