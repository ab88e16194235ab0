"""The step backward, bit for bit against the output recorded before its schedule was changed
(tests/golden/bwd_schedule.npz, written by tests/golden/make_bwd_schedule.py at the commit the file names).

The new schedule changes when a wave's row loads are issued, when its MFMAs run and how addresses reach the lanes.
Every accumulator still sums its column steps in ascending order, so dx, dt and the table rows must keep every bit.
The inputs are random floats (N(0, 1) x and tables, 1e-3-scaled dout, lr 0.01), not exactly summable: a reordered
sum would flip bits.  Hence no tolerance: np.array_equal on the bit patterns, every case B <= 6.

Each case runs dlrm_step_fwd (the indexer built in its launch), then dlrm_step_bwd(DLRM_STEP_BWD_ONLY), and compares
dx, the whole of dt (the rows the launch writes -- repeated positions -- and the sentinel everywhere else) and the
table rows of the batch's positions; every other table row must keep its start value.

Cases (make_bwd_schedule.CASES): the metric instantiation (fp32, d = 128, 26 tables) with a partial last block of 4
samples and once-hit and repeated rows in both tile rows and every group of four features, a single sample, F = 17
(tile row 1 holds one feature), F = 9 (one row block), a padded dout leading dimension, one out-of-range index
(error raised, no table row written), index base 1; and two forms that keep the kernel's text: d = 16 (one wave per
sample) and bf16 rows at d = 128.  The split and Adagrad rules keep the kernel's text too (their own suites cover
them); no rule variant takes the new schedule.
"""
import importlib.util
import os

import numpy as np
import pytest

gpu_test = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_bwd_schedule",
                                               os.path.join(_HERE, "golden", "make_bwd_schedule.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


@pytest.fixture(scope="module")
def recorded():
    with np.load(mk.PATH, allow_pickle=False) as z:
        rec = {k: z[k] for k in z.files}
    for v in rec.values():
        v.setflags(write=False)
    return rec


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _want(recorded, name, what):
    return recorded[f"{mk.SAME_AS.get(name, name)}/{what}"]


def test_fixture_is_complete(recorded):
    """Every case has its recorded arrays, of the case's shapes, the file names its commit and stays small."""
    assert len(str(recorded["commit"])) == 40
    assert os.path.getsize(mk.PATH) < 1000 * 1000
    for name, (dtype, d, T, B, form) in mk.CASES.items():
        assert B <= 6
        assert _want(recorded, name, "dx").shape == (B, d), name
        assert _want(recorded, name, "dt").shape == (B, (T + 1) * d), name
        rows = _want(recorded, name, "rows")
        assert rows.shape == (T, B, d) and rows.dtype == (np.float32 if dtype == "f32" else np.uint16), name


def test_metric_case_mixes_once_hit_and_repeated_rows():
    """In the metric case every group of four features (the rows one lane group q stores), in both tile rows, has
    a once-hit row and a repeated one."""
    _, idx, _, _ = mk.inputs("f32_d128_t26_b6")
    once = mk.once_hit(idx)  # [T][B]; table t is feature t + 1
    F = idx.shape[0] + 1
    for g0 in range(0, F, 4):
        ts = [f - 1 for f in range(max(g0, 1), min(g0 + 4, F))]
        if len(ts) < 2:
            continue
        assert once[ts].any() and not once[ts].all(), f"features {g0}..{g0 + 3}"


@gpu_test
@pytest.mark.parametrize("name", list(mk.CASES))
def test_backward_bits_match_the_recorded_commit(pkg, gpu, recorded, name):
    dtype, d, T, B, form = mk.CASES[name]
    dx, dt, rows, after, raised = mk.run_case(pkg, gpu, name)
    # the bounds error is raised exactly as before: by the out-of-range case, and by no other
    assert raised == (form == "oob")
    for what, got in (("dx", dx), ("dt", dt), ("rows", rows)):
        want = _want(recorded, name, what)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want)), \
            f"{name}: {int((_bits(got) != _bits(want)).sum())} of {want.size} {what} elements differ in bits"
    tables, idx, _, _ = mk.inputs(name)
    once = mk.once_hit(idx)
    dt3 = dt.reshape(B, T + 1, d)
    # dt: the x row and (unless a bounds error froze the tables) the once-hit positions' rows keep the sentinel
    assert (dt3[:, 0] == mk.SENTINEL).all()
    for t in range(T):
        for b in range(B):
            kept = (dt3[b, t + 1] == mk.SENTINEL).all()
            assert kept == (bool(once[t, b]) and form != "oob"), (name, t, b)
    # tables: only a once-hit row may change, and with a bounds error none does
    for t in range(T):
        start = tables[t]
        if dtype == "bf16":
            import torch
            start = torch.from_numpy(start).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        same = (_bits(after[t]) == _bits(start)).all(axis=1)
        may = np.zeros(len(start), dtype=bool)
        if form != "oob":
            may[idx[t][once[t]]] = True
        assert same[~may].all(), f"{name}: table {t}: a row that is not once-hit changed"
        # (bf16 rows: a step of lr 0.01 on 1e-3-scaled gradients rounds back to the row's own bf16 bits)
        if form != "oob" and dtype == "f32":
            assert not same[may].any(), f"{name}: table {t}: a once-hit row kept its value"
