"""bench.py's plain run, --full and --dump-outputs: a plain run times exactly --steps steps and
leaves every secondary measurement null; --dump-outputs writes the last timed step's arrays as
float32 .npy files under the size cap, identical from run to run."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SECONDARY = ("sustained", "drop_in_chain", "roofline", "cpu_baseline")


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs == "" and (a.steps, a.warmup) == (20, 5)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def host_problem(T=3, N=40, D=8, B=40, width=14):
    g = torch.Generator().manual_seed(5)
    tables = [torch.randn((50 + 7 * t, D), generator=g) for t in range(T)]
    idx = torch.stack([torch.randint(0, 50 + 7 * t, (N,), generator=g, dtype=torch.int32) for t in range(T)])
    idx[0] = torch.randperm(50, generator=g)[:N].to(torch.int32)  # table 0: no row twice
    return torch.randn((B, width), generator=g), torch.randn((B, D), generator=g), tables, idx


def test_dump_outputs_writes_the_step_arrays(tmp_path):
    out, dx, tables, idx = host_problem()
    bench.dump_outputs(str(tmp_path / "d"), out.to(torch.bfloat16), dx, tables, idx)
    got = {p.name: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["dx.npy", "out.npy", "table_rows.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["out.npy"], out.to(torch.bfloat16).float().numpy())
    assert np.array_equal(got["dx.npy"], dx.numpy())
    want = np.stack([tables[t][idx[t].long()].numpy() for t in range(len(tables))])  # every position
    assert np.array_equal(got["table_rows.npy"], want)


def test_dump_outputs_samples_the_same_positions_under_the_cap(tmp_path, monkeypatch):
    out, dx, tables, idx = host_problem()
    T, N, D = len(tables), idx.shape[1], tables[0].shape[1]
    m = 11  # room for 11 of the 40 positions per table beside out and dx
    cap = out.numel() * 4 + dx.numel() * 4 + T * D * 4 * m + 5
    monkeypatch.setattr(bench, "DUMP_CAP", cap)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), out, dx, tables, idx)
    a, b = (np.load(tmp_path / n / "table_rows.npy") for n in ("a", "b"))
    assert a.shape == (T, m, D) and np.array_equal(a, b)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= cap + 3 * 128  # + headers
    # each table's sampled rows are rows of its batch, at the same increasing positions for every table
    pos = [int(np.flatnonzero((tables[0][idx[0].long()].numpy() == r).all(1))[0]) for r in a[0]]
    assert pos == sorted(pos) and len(set(pos)) == m
    for t in range(T):
        assert np.array_equal(a[t], tables[t][idx[t].long()].numpy()[pos])


def run_bench(monkeypatch, capsys, args):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + args)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(gpu, tmp_path, monkeypatch, capsys):
    """Two plain runs with the same arguments (D = 16 Kaggle tables, 4 index batches): the line has
    the headline fields for exactly --steps steps and no secondary measurement; the dumped arrays
    are finite float32 of the step's shapes and equal bit for bit between the runs."""
    w = bench.dlrm_pkg.load().WORKLOADS["kaggle-d16-b2048"]
    T, D, B = len(w["rows"]), w["dim"], w["batch"]
    args = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--nbatch", "4", "--workload", "kaggle-d16-b2048"]
    dumps = []
    for name in ("a", "b"):
        line = run_bench(monkeypatch, capsys, args + ["--dump-outputs", str(tmp_path / name)])
        assert (line["steps"], line["warmup"], line["n_gpus"]) == (6, 2, 1)
        assert line["metric"] == bench.METRIC and line["unit"] == "samples/s" and line["dtype"] == "f32"
        assert line["higher_is_better"] is True and line["ms_per_step"] > 0
        # (the line rounds ms_per_step to 1e-4 ms: half a unit of that, relative to the step)
        assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=5e-5 / line["ms_per_step"] + 1e-6)
        assert all(line[k] is None for k in SECONDARY)
        dumps.append({f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    a, b = dumps
    assert sorted(a) == ["dx", "out", "table_rows"]
    assert a["out"].shape == (B, D + (T + 1) * T // 2) and a["dx"].shape == (B, D)
    assert a["table_rows"].shape == (T, B, D)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0
        assert np.array_equal(a[k], b[k]), k
