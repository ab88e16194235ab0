"""Evaluation, the host side: the state layout, argument errors (no device is touched), the numpy
restatement `eval_reference` against a brute-force pair count, and the reference's golden dense step."""
import ctypes
import math
import os

import numpy as np
import pytest

from eval_cases import NAN, SOFT, crafted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def test_eval_layout(lib):
    bins, shift, words = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    assert lib.dlrm_eval_layout(ctypes.byref(bins), ctypes.byref(shift), ctypes.byref(words)) == 0
    assert (bins.value, shift.value, words.value) == (130049, 13, 260106)
    from dlrm_jl_amd import evaluate
    assert (evaluate.BINS, evaluate.SHIFT, evaluate.WORDS) == (130049, 13, 260106)


def test_eval_accumulate_argument_errors_touch_no_device(lib, pkg):
    E_ARG = pkg._lib.E_ARG
    # host memory stands in for every handle and buffer: each call must return before it reads one
    ctx = ctypes.create_string_buffer(8192)  # (an error message is formatted into the ctx)
    buf = (ctypes.c_int64 * 4)()
    a = ctypes.addressof(buf)
    f = lib.dlrm_eval_accumulate
    assert f(None, a, 4, a, 1, 0, a, None) == E_ARG          # null ctx
    assert f(ctx, None, 4, a, 1, 0, a, None) == E_ARG        # null state
    assert f(ctx, a, 4, None, 1, 0, a, None) == E_ARG        # null scores
    assert f(ctx, a, 4, a, 1, 0, None, None) == E_ARG        # null labels
    assert f(ctx, a, 0, a, 1, 0, a, None) == E_ARG           # batch < 1
    assert f(ctx, a, -3, a, 1, 1, a, None) == E_ARG
    assert f(ctx, a, 4, a, 0, 0, a, None) == E_ARG           # scores_ld < 1
    assert f(ctx, a + 4, 4, a, 1, 0, a, None) == E_ARG       # state not 8-byte aligned
    assert b"dlrm_eval_accumulate" in lib.dlrm_last_error(ctx)
    assert lib.dlrm_eval_layout(None, None, None) == E_ARG


def test_eval_reference_against_a_brute_force_pair_count(pkg):
    from dlrm_jl_amd import evaluate
    p, y = crafted()
    n = len(p)
    assert n == 500
    ref = pkg.eval_reference(p, y)
    # the truncated keys, restated per sample in Python
    keys = []
    for v in p:
        v = float(v)
        v = 0.0 if math.isnan(v) else min(max(v, 0.0), 1.0)
        keys.append(int(np.float32(v).view(np.uint32)) >> 13)
    assert keys == list(evaluate.eval_keys(p))
    assert keys[NAN] == 0
    # O(n^2): twice the pairs (negative, positive) ranked right, a tie in a bin counted half
    neg = [i for i in range(n) if y[i] == 0.0]
    pos = [i for i in range(n) if y[i] == 1.0]
    num2 = sum(2 if keys[j] > keys[i] else 1 if keys[j] == keys[i] else 0 for i in neg for j in pos)
    got = evaluate.auc_num2(ref["hist"])
    print("num2", got, "brute force", num2)
    assert got == num2
    assert (ref["total"], ref["positives"], ref["negatives"]) == (n, len(pos), len(neg))
    assert len(pos) + len(neg) == n - 1  # the soft label is in total only
    assert int(ref["hist"].sum()) == n - 1
    assert ref["hist"][0].sum() == len(neg) and ref["hist"][1].sum() == len(pos)
    # accuracy: Python's round is ties-to-even as Julia's; a NaN and the soft label are never equal
    correct = sum(1 for i in range(n) if not math.isnan(float(p[i])) and float(round(float(p[i]))) == float(y[i]))
    assert ref["correct"] == correct
    half = np.float32(0.5)
    for prob, label, want in ((half, 0.0, 1), (half, 1.0, 0), (np.nextafter(half, np.float32(1)), 1.0, 1),
                              (np.float32(0.7), 0.7, 0), (np.float32(np.nan), 1.0, 0), (np.float32(np.nan), 0.0, 0)):
        assert pkg.eval_reference([prob], [label])["correct"] == want, (prob, label)
    soft = pkg.eval_reference(p[SOFT:SOFT + 1], y[SOFT:SOFT + 1])
    assert (soft["total"], soft["correct"], soft["positives"], soft["negatives"]) == (1, 0, 0, 0)
    assert int(soft["hist"].sum()) == 0
    res = evaluate.summarize(ref)
    assert res["auc"] == num2 / (2 * len(pos) * len(neg))
    assert math.isnan(evaluate.summarize(pkg.eval_reference([0.3, 0.6], [1.0, 1.0]))["auc"])  # one class only
    # a perfect and an inverted ranking
    assert evaluate.summarize(pkg.eval_reference([0.1, 0.2, 0.8], [0.0, 0.0, 1.0]))["auc"] == 1.0
    assert evaluate.summarize(pkg.eval_reference([0.9, 0.2, 0.1], [0.0, 1.0, 1.0]))["auc"] == 0.0


@pytest.mark.parametrize("kind", ["single", "multi"])
def test_eval_reference_on_the_golden_dense_step(pkg, kind):
    """The reference's own forward: the log loss of its top MLP's output against its labels is its loss
    (tests/test_dense.py's bound); its labels are soft, so no prediction equals one: accuracy 0/128."""
    from dlrm_jl_amd import evaluate
    with np.load(os.path.join(GOLDEN, f"pytorch_reference_{kind}_dense.npz"), allow_pickle=False) as z:
        prob, labels, loss = z["mlp_top"], z["labels"], float(z["loss"])
    assert np.all((labels != 0.0) & (labels != 1.0))
    res = evaluate.summarize(pkg.eval_reference(prob, labels))
    assert abs(res["logloss"] - loss) <= 1e-5 * abs(loss), (res["logloss"], loss)
    assert (res["correct"], res["total"], res["accuracy"]) == (0, 128, 0.0)
    assert (res["positives"], res["negatives"]) == (0, 0) and math.isnan(res["auc"])
