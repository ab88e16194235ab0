"""The one-hot forward, bit for bit against the output recorded before its row loads were rolled
into a window (tests/golden/fwd_window.npz, written by tests/golden/make_fwd_window.py at the
commit the file names).

The window changes only when a wave's row loads are issued.  Every Gram accumulator keeps its
order (even and odd column-step partials, each in ascending step order, Z = even + odd), so the
output must keep every bit.  The inputs are random floats, not exactly summable: a reordered sum
would flip bits, which the fused-against-two-operator comparisons cannot see (both forms run the
same body).  Hence no tolerance: np.array_equal on the bit patterns, every case B <= 6.

Cases (make_fwd_window.CASES): the metric instantiation (fp32, d = 128, F = 27) with a partial
last workgroup and unaligned rows (W = 479), with padding (pad_to 8: W = 480, aligned rows; pad_to
64), F = 17 (second 16-row block nearly empty), F = 9 (one block), bf16 (four column steps: the
window clamps), d = 48 and d = 256 on the generic kernel, B = 1; on the metric shape the forward
with ys kept, dlrm_step_fwd with the indexer built in its launch, and one out-of-range index.
"""
import importlib.util
import os

import numpy as np
import pytest

gpu_test = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_fwd_window", os.path.join(_HERE, "golden", "make_fwd_window.py"))
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


def test_fixture_is_complete(recorded):
    """Every case has its recorded output, of the case's shape, and the file names its commit."""
    assert len(str(recorded["commit"])) == 40
    assert os.path.getsize(mk.PATH) < 256 * 1024
    for name, (dtype, d, T, B, pad_to, form) in mk.CASES.items():
        F = T + 1
        W = -(-(d + F * (F - 1) // 2) // pad_to) * pad_to
        assert recorded[name].shape == (B, W), name
        assert recorded[name].dtype == (np.float32 if dtype == "f32" else np.uint16), name


@gpu_test
@pytest.mark.parametrize("name", list(mk.CASES))
def test_forward_bits_match_the_recorded_commit(pkg, gpu, recorded, name):
    dtype, d, T, B, pad_to, form = mk.CASES[name]
    out, ys, raised = mk.run_case(pkg, gpu, name)
    want = recorded[name]
    assert out.dtype == want.dtype and out.shape == want.shape
    assert np.array_equal(_bits(out), _bits(want)), \
        f"{name}: {int((_bits(out) != _bits(want)).sum())} of {want.size} output elements differ in bits"
    # the bounds error is raised exactly as before: by the out-of-range case, and by no other
    assert raised == (form == "oob")
    if form == "ys":
        # ys = [x | the looked-up rows], bit for bit the table rows
        tables, idx, x = mk.inputs(name)
        ref = np.concatenate([x] + [tables[t][idx[t]] for t in range(T)], axis=1)
        assert np.array_equal(_bits(ys), _bits(ref))
    if form in ("ys", "step"):
        # the same inputs as the plain forward: the same output
        assert np.array_equal(_bits(out), _bits(recorded["f32_d128_t26_b6"]))
    if form == "oob":
        # the bad index reads a zero row; no other sample changes
        plain = recorded["f32_d128_t26_b6"]
        keep = np.arange(B) != mk.OOB_SAMPLE
        assert np.array_equal(_bits(out[keep]), _bits(plain[keep]))
        assert not np.array_equal(_bits(out[mk.OOB_SAMPLE]), _bits(plain[mk.OOB_SAMPLE]))
        # the pairs of the zero row are zeros: feature OOB_TABLE + 1 against every other feature
        f = mk.OOB_TABLE + 1
        i, j = np.tril_indices(T + 1, -1)
        assert not out[mk.OOB_SAMPLE, d:][(i == f) | (j == f)].any()
