"""Evaluation: accuracy, log loss and AUC of scores against labels, accumulated on the device.

The reference's `test(model, data; record, strategy)` (src/train/utils.jl:31-46) rounds the model's
predictions, counts the ones equal to their labels and pushes correct / total onto `record`.  Here a
batch is folded into a device-resident integer state by one launch (dlrm_eval_accumulate: no host
synchronisation, graph-capturable), and the host reads the state once, at the end:

    ev = Evaluator(device)
    for labels, dense, sparse in data:
        ev.add(model.predict(dense, sparse), labels)      # logits; is_prob=True for probabilities
    ev.result()   # dict(total, correct, accuracy, logloss, auc, positives, negatives)

State words (include/dlrm_hip.h): 0 total, 1 correct, 2 positives, 3 negatives, 4 batches, 5 loss_sum
(double bits), 6 the last call's mean loss (float bits), 7 zero, then hist[2][BINS]: per class, the count
of probabilities whose float bits, clamped to [0, 1] and shifted right by SHIFT, are k.  Positive float
bits are monotone in the value, so the histogram is an exact ranking of the scores truncated to 10
mantissa bits, and the AUC of that ranking is computed from it in Python integers.

`eval_reference(prob, labels)` restates the counters and the histogram in numpy from given
probabilities: the tests' yardstick for the kernel, as `sr_round` is for the stochastic rule.
"""
import ctypes
import math
import struct

import numpy as np
import torch

from . import _lib
from .runtime import context, ptr, require_device

SHIFT = 13
ONE_BITS = 0x3F800000  # float bits of 1.0
BINS = (ONE_BITS >> SHIFT) + 1
HEADER = 8
WORDS = HEADER + 2 * BINS
_NAMES = ("total", "correct", "positives", "negatives", "batches")


def eval_keys(prob):
    """The histogram bin of every probability: float bits of min(max(p, 0), 1) >> SHIFT (a NaN: bin 0)."""
    p = np.ascontiguousarray(prob, dtype=np.float32).reshape(-1)
    pc = np.fmin(np.fmax(p, np.float32(0.0)), np.float32(1.0))  # fmax / fmin drop a NaN, as fmaxf / fminf do
    bits = np.clip(pc.view(np.int32), 0, ONE_BITS)  # (-0.0f: bin 0)
    return (bits >> SHIFT).astype(np.int64)


def eval_reference(prob, labels):
    """The counters and histogram dlrm_eval_accumulate leaves after these samples, in numpy: dict(total,
    correct, positives, negatives, loss_sum, hist [2][BINS] int64).  correct: rint(p) == y (ties to even,
    so 0.5 predicts 0; a soft label or a NaN is never equal); loss_sum: the float64 sum of bce_loss's terms
    (train.jl:33-41) on the float32 probabilities."""
    p = np.ascontiguousarray(prob, dtype=np.float32).reshape(-1)
    y = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
    if p.shape != y.shape:
        raise ValueError(f"{p.shape[0]} probabilities, {y.shape[0]} labels")
    k = eval_keys(p)
    pos, neg = y == 1.0, y == 0.0
    hist = np.zeros((2, BINS), dtype=np.int64)
    np.add.at(hist[0], k[neg], 1)
    np.add.at(hist[1], k[pos], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p64, y64 = p.astype(np.float64), y.astype(np.float64)
        q64 = (np.float32(1.0) - p).astype(np.float64)  # 1 - p as the kernel forms it, in float32
        terms = -y64 * np.maximum(np.log(p64), -100.0) + (y64 - 1.0) * np.maximum(np.log(q64), -100.0)
    return dict(total=int(p.shape[0]), correct=int(np.count_nonzero(np.rint(p) == y)),
                positives=int(np.count_nonzero(pos)), negatives=int(np.count_nonzero(neg)),
                loss_sum=float(terms.sum()), hist=hist)


def auc_num2(hist):
    """Twice the number of (negative, positive) pairs the ranking orders correctly, ties in a bin counted
    half: num2 = Σ_k neg[k]·(2·pos_above[k] + pos[k]), in Python integers."""
    neg = [int(v) for v in hist[0]]
    pos = [int(v) for v in hist[1]]
    num2, above = 0, 0
    for k in range(len(neg) - 1, -1, -1):
        if neg[k]:
            num2 += neg[k] * (2 * above + pos[k])
        above += pos[k]
    return num2


def summarize(counts):
    """counts (eval_reference's or Evaluator.counts' dict) -> dict(total, correct, accuracy, logloss, auc,
    positives, negatives); auc is nan without both classes, accuracy and logloss without a sample."""
    total, P, N = counts["total"], counts["positives"], counts["negatives"]
    auc = auc_num2(counts["hist"]) / (2 * P * N) if P * N else math.nan
    return dict(total=total, correct=counts["correct"], accuracy=counts["correct"] / total if total else math.nan,
                logloss=counts["loss_sum"] / total if total else math.nan, auc=auc, positives=P, negatives=N)


class Evaluator:
    """The device state of one evaluation pass and its launches.  `add` is one kernel launch on the
    current stream with no synchronisation (capturable in a torch.cuda graph); `counts` / `result`
    copy the state to the host (the pass's one synchronisation).  Two evaluators' states merge by
    integer addition (`merge`).  `add`s on one state from two streams at once are undefined."""

    def __init__(self, device=None):
        self.ctx = context(device)
        self.device = torch.device("cuda", self.ctx.device)
        bins, shift, words = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _lib.check(self.ctx.lib.dlrm_eval_layout(ctypes.byref(bins), ctypes.byref(shift), ctypes.byref(words)))
        if (bins.value, shift.value, words.value) != (BINS, SHIFT, WORDS):
            raise RuntimeError(f"dlrm_eval_layout gives {(bins.value, shift.value, words.value)}, "
                               f"evaluate.py expects {(BINS, SHIFT, WORDS)}")
        self.state = torch.zeros(WORDS, dtype=torch.int64, device=self.device)

    def reset(self):
        self.state.zero_()
        return self

    def add(self, scores, labels, *, is_prob=False, prob=None):
        """Folds a batch in: scores [B] or [B][1] float32 (any row stride), logits unless is_prob;
        labels a contiguous float32 [B]; prob (optional, contiguous float32 [B]) receives the probabilities."""
        dev = self.device
        require_device(scores, dev, "scores")
        require_device(labels, dev, "labels")
        if scores.dim() == 2 and scores.shape[1] == 1:
            B, ld = scores.shape[0], scores.stride(0)
        elif scores.dim() == 1:
            B, ld = scores.shape[0], scores.stride(0)
        else:
            raise ValueError("scores must be [B] or [B][1]")
        if scores.dtype != torch.float32 or B < 1 or ld < 1:
            raise ValueError("scores must be a non-empty float32 vector with a positive stride")
        if labels.shape != (B,) or labels.dtype != torch.float32 or not labels.is_contiguous():
            raise ValueError(f"labels must be a contiguous float32 vector of {B}")
        if prob is not None:
            require_device(prob, dev, "prob")
            if prob.shape != (B,) or prob.dtype != torch.float32 or not prob.is_contiguous():
                raise ValueError(f"prob must be a contiguous float32 vector of {B}")
        ctx = self.ctx
        ctx.check(ctx.lib.dlrm_eval_accumulate(ctx.bind(), ptr(self.state), B, ptr(scores), ld, 1 if is_prob else 0,
                                               ptr(labels), ptr(prob)))
        return self

    def words(self):
        """The raw state on the host (int64 [WORDS]); synchronises."""
        return self.state.cpu().numpy()

    def counts(self):
        """dict(total, correct, positives, negatives, batches, loss_sum, last_loss, hist [2][BINS]); synchronises."""
        return counts_of(self.words())

    def result(self):
        return summarize(self.counts())

    def merge(self, other):
        """Adds another evaluator's state (same or another device) into this one: integer addition of the
        counters and the histogram, a double addition of loss_sum; the last call's loss stays this one's."""
        mine, theirs = self.words().copy(), other.words()
        s = _f64(mine[5]) + _f64(theirs[5])
        keep = mine[6]
        mine += theirs
        mine[5] = struct.unpack("<q", struct.pack("<d", s))[0]
        mine[6], mine[7] = keep, 0
        self.state.copy_(torch.from_numpy(mine))
        return self


def _f64(word):
    return struct.unpack("<d", struct.pack("<q", int(word)))[0]


def counts_of(words):
    """The state's words (int64 [WORDS]) as eval_reference's dict, plus `batches` and `last_loss`."""
    w = np.asarray(words, dtype=np.int64)
    out = {n: int(w[i]) for i, n in enumerate(_NAMES)}
    out["loss_sum"] = _f64(w[5])
    out["last_loss"] = struct.unpack("<f", struct.pack("<I", int(w[6]) & 0xFFFFFFFF))[0]
    out["hist"] = w[HEADER:].reshape(2, BINS).copy()
    return out
