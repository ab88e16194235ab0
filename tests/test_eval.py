"""Evaluation on the GPU: dlrm_eval_accumulate through `Evaluator`, the inference forward `HotPath.infer`,
`DLRMModel.predict` / `test` and `HipTables.infer`.

The yardstick of the counters and the histogram is `eval_reference` (numpy, checked on the CPU against a
brute-force pair count in tests/test_eval_host.py) applied to the probabilities the kernel wrote, which are
themselves held bit for bit to dlrm_bce_head's; integers compare exactly.  The log loss is held to
tests/test_dense.py::test_bce_head_seam's bound, 1e-5·max(1, |loss|), against the float64 restatement.
"""
import os

import numpy as np
import pytest
import torch

from eval_cases import NAN, crafted
from helpers import rand_indices, rand_tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLDAYS = os.path.join(ROOT, "tests", "golden", "dac", "alldays.txt")
ROWS = [2, 8, 40, 5000, 3, 100000]
COUNTERS = ("total", "correct", "positives", "negatives")


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy()


def _logits(gpu, B, ld=1, seed=0):
    """randn·4 with ±120 and 0 in front, as a [B][1] view of row stride ld; labels 0/1 with one soft label."""
    gen = torch.Generator(device=gpu).manual_seed(1000 * seed + B)
    full = torch.randn((B, ld), device=gpu, generator=gen) * 4
    z = full[:, :1]
    z[: min(B, 3), 0] = torch.tensor([120.0, -120.0, 0.0], device=gpu)[: min(B, 3)]
    y = (torch.rand(B, device=gpu, generator=gen) < 0.5).float()
    if B > 3:
        y[3] = 0.3
    return z, y


def _assert_counts(got, want, what=""):
    for n in COUNTERS:
        assert got[n] == want[n], (what, n, got[n], want[n])
    assert np.array_equal(got["hist"], want["hist"]), what


def _assert_logloss(got, want, total, what=""):
    a, b = got["loss_sum"] / total, want["loss_sum"] / total
    print(f"{what} logloss {a!r} float64 restatement {b!r}")
    assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (what, a, b)


# ---- 1. the kernel against dlrm_bce_head and eval_reference
@pytest.mark.parametrize("ld", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 1024, 1025, 2500])
def test_eval_seam_logits(pkg, gpu, B, ld):
    from dlrm_jl_amd.runtime import context, ptr
    z, y = _logits(gpu, B, ld)
    assert z.stride(0) == ld
    prob_h, dz = torch.empty(B, device=gpu), torch.empty((B, 1), device=gpu)
    loss_h = torch.empty((), device=gpu)
    ctx = context(gpu)
    ctx.check(ctx.lib.dlrm_bce_head(ctx.bind(), B, ptr(z), z.stride(0), ptr(y), ptr(prob_h), ptr(dz), ptr(loss_h),
                                    None))
    ev = pkg.Evaluator(gpu)
    prob = torch.full((B,), -1.0, device=gpu)
    ev.add(z, y, prob=prob)
    words = ev.words()
    got = ev.counts()
    assert np.array_equal(_bits(prob), _bits(prob_h))
    loss_bits = int(_bits(loss_h).reshape(-1)[0]) & 0xFFFFFFFF
    assert int(words[6]) == loss_bits  # (the high half is zero)
    assert int(words[7]) == 0 and got["batches"] == 1
    if B & (B - 1) == 0:
        back = np.float32(got["loss_sum"]) * np.float32(1.0 / B)
        assert int(back.view(np.uint32)) == loss_bits
    want = pkg.eval_reference(prob.cpu().numpy(), y.cpu().numpy())
    _assert_counts(got, want)
    assert got["total"] == B and got["positives"] + got["negatives"] == B - (1 if B > 3 else 0)
    _assert_logloss(got, want, B)
    res = ev.result()
    assert res["accuracy"] == want["correct"] / B and res["logloss"] == got["loss_sum"] / B


def test_eval_seam_probabilities(pkg, gpu):
    p, y = crafted()
    pd, yd = torch.from_numpy(p).to(gpu), torch.from_numpy(y).to(gpu)
    ev = pkg.Evaluator(gpu)
    out = torch.zeros(len(p), device=gpu)
    ev.add(pd, yd, is_prob=True, prob=out)
    got = ev.counts()
    _assert_counts(got, pkg.eval_reference(p, y))
    assert np.array_equal(_bits(out), p.view(np.int32))  # (the NaN's bits included)
    assert np.isnan(p[NAN]) and got["hist"][1][0] >= 1  # the NaN: a positive in bin 0
    # without prob the same state
    ev2 = pkg.Evaluator(gpu).add(pd, yd, is_prob=True)
    _assert_counts(ev2.counts(), got)


# ---- 2. accumulation, reset, merge, graph replay
def test_eval_accumulates_resets_merges_and_replays(pkg, gpu):
    ev = pkg.Evaluator(gpu)
    probs, labels = [], []
    for k, B in enumerate((5, 1300, 64)):
        z, y = _logits(gpu, B, seed=k + 1)
        p = torch.empty(B, device=gpu)
        ev.add(z, y, prob=p)
        probs.append(p)
        labels.append(y)
    got = ev.counts()
    want = pkg.eval_reference(torch.cat(probs).cpu().numpy(), torch.cat(labels).cpu().numpy())
    _assert_counts(got, want, "three adds")
    assert got["batches"] == 3 and got["total"] == 1369
    _assert_logloss(got, want, 1369, "three adds")
    # merge: another evaluator's batch
    other = pkg.Evaluator(gpu)
    z, y = _logits(gpu, 700, seed=9)
    p = torch.empty(700, device=gpu)
    other.add(z, y, prob=p)
    ev.merge(other)
    merged = ev.counts()
    want4 = pkg.eval_reference(torch.cat(probs + [p]).cpu().numpy(), torch.cat(labels + [y]).cpu().numpy())
    _assert_counts(merged, want4, "merged")
    assert merged["batches"] == 4
    assert merged["loss_sum"] == got["loss_sum"] + other.counts()["loss_sum"]
    # reset
    ev.reset()
    assert not ev.words().any()
    # one captured add, replayed three times, triples every counter
    ev.add(z, y)  # (eager warm-up)
    once = ev.counts()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            ev.add(z, y)
    torch.cuda.current_stream().wait_stream(s)
    ev.reset()
    for _ in range(3):
        gr.replay()
    thrice = ev.counts()
    for n in COUNTERS + ("batches",):
        assert thrice[n] == 3 * once[n], n
    assert np.array_equal(thrice["hist"], 3 * once["hist"])
    assert thrice["loss_sum"] == 3 * once["loss_sum"]  # (a float's triple is exact in double)
    assert thrice["last_loss"] == once["last_loss"]


# ---- 3. the inference forward
def _hot_inputs(pkg, gpu, T, D, B, L, dtype, seed=0):
    rng = np.random.default_rng(100 * T + D + seed)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    w = [torch.from_numpy(t).to(dtype).to(gpu) for t in rand_tables(rng, rows, D)]
    packs = []
    for _ in range(3):
        i = torch.from_numpy(rand_indices(rng, rows, B, L)).to(torch.int32).to(gpu)
        packs.append(pkg.PackedIndices(i.reshape(T, B, L) if L > 1 else i))
    xs = [torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(dtype) for _ in range(2)]
    F = T + 1
    dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(dtype)
    return w, packs, xs, dout


@pytest.mark.parametrize("T,D,B,L,dtype", [(3, 16, 5, 1, torch.float32), (26, 128, 6, 1, torch.float32),
                                           (26, 128, 6, 1, torch.bfloat16), (4, 32, 7, 3, torch.float32)],
                         ids=["3x16", "26x128", "26x128-bf16", "pooled"])
def test_infer_equals_the_training_forward(pkg, gpu, T, D, B, L, dtype):
    w, packs, xs, _ = _hot_inputs(pkg, gpu, T, D, B, L, dtype)
    ts = pkg.EmbeddingTableSet(w)
    fresh = pkg.HotPath(ts, B, L, index_base=0)
    want = _bits(fresh.forward(xs[0], packs[0]))
    hp = pkg.HotPath(ts, B, L, index_base=0)
    hp.validate(xs[0], packs[0])
    got = _bits(hp.infer(xs[0], packs[0]))
    torch.cuda.synchronize()
    hp.check_bounds()
    assert np.array_equal(got, want)
    assert hp._fwd_x is None and hp._fwd_idx is None
    if hp.indexer is not None:
        assert hp.indexer.state() == 0  # nothing was built
    assert np.array_equal(_bits(hp.infer(xs[0], packs[0])), want)  # (and again, whichever route the first took)


# ---- 4. evaluation between pipelined training steps
def _run_steps(pkg, gpu, w, packs, xs, dout, B, opt, with_infer, **kw):
    ts = pkg.EmbeddingTableSet([t.clone() for t in w])
    hp = pkg.HotPath(ts, B, 1, lr=0.05, index_base=0, pipeline="apply", opt=opt, **kw)
    assert hp.pipeline == "apply"
    seq = [0, 1, 0, 1]
    for k, b in enumerate(seq):
        if with_infer:
            hp.infer(xs[1], packs[2])  # another batch, another x
        nxt = packs[seq[(k + 1) % 4]]
        if k == 0:
            hp.prime(nxt, xs[0], dout, prev=packs[b])
        else:
            hp.step_prep(xs[0], packs[b], dout, nxt)
    torch.cuda.synchronize()
    hp.check_bounds()
    state = [_bits(s) for s in opt.state_of(ts)] if opt is not None else []
    return [_bits(t.data) for t in ts] + state + [_bits(hp.dx), _bits(hp.out)], [_bits(t) for t in w]


@pytest.mark.parametrize("rule", ["descent", "rowwise-adagrad"])
def test_infer_between_pipelined_steps_changes_nothing(pkg, gpu, rule):
    T, D, B = 4, 16, 64
    w, packs, xs, dout = _hot_inputs(pkg, gpu, T, D, B, 1, torch.float32, seed=3)
    runs = []
    for with_infer in (False, True):
        if rule == "descent":
            opt, kw = None, {}
        else:
            opt, kw = pkg.RowwiseADAGrad(0.05, 1e-8), {"adagrad_step": True}
        runs.append(_run_steps(pkg, gpu, w, packs, xs, dout, B, opt, with_infer, **kw))
    (plain, start), (evald, _) = runs
    assert len(plain) == len(evald)
    for a, b in zip(plain, evald):
        assert np.array_equal(a, b)
    assert any((a != b).any() for a, b in zip(plain[:T], start))  # (the steps did train)


# ---- 5. the drop-in chain: an evaluation forward sees the applied updates
def test_hiptables_infer_runs_the_deferred_update_first(pkg, gpu):
    T, D, B = 4, 16, 64
    w, packs, xs, dout = _hot_inputs(pkg, gpu, T, D, B, 1, torch.float32, seed=4)
    ht = pkg.HipTables([t.clone() for t in w], lr=0.05, index_base=0)
    p = packs[0]
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
    out, back = pkg.rrule(pkg.DotInteraction(), xs[0], ys)
    before = _bits(out).copy()
    _, dx, dy = back(dout)
    pkg.update_(pkg.Descent(0.05), ht, pkg.maplookup_pullback(D, ht, p, dy))
    assert ht._pending is not None  # the apply launch is deferred
    got = _bits(ht.infer(xs[0], p)).copy()
    assert ht._pending is None
    ts = ht.ts
    want = _bits(pkg.HotPath(ts, B, 1, index_base=0).forward(xs[0], p))
    assert np.array_equal(got, want)
    assert (got != before).any()  # the step's update is in what the evaluation read


# ---- 6. end to end on the DAC sample
def test_model_test_on_the_dac_sample(pkg, gpu):
    dac = pkg.dac
    data = dac.parse_tsv(ALLDAYS)
    maps = dac.reindex(data)
    maps.reindex_(data)
    D, B, T = 16, 32, 26
    gen = torch.Generator(device=gpu).manual_seed(3)
    tables = [torch.empty((n, D), device=gpu).uniform_(-n ** -0.5, n ** -0.5, generator=gen) for n in maps.sizes()]
    bsz, tsz = pkg.kaggle_mlp_sizes(D, T)
    model = pkg.DLRMModel(pkg.random_mlp(bsz, sigmoid_last=False, generator=gen, device=gpu), tables,
                          pkg.random_mlp(tsz, sigmoid_last=True, generator=gen, device=gpu), B, 1, lr=0.05,
                          index_base=1)
    loader = pkg.DACLoader(data, B, gpu)
    assert len(loader) == 7
    ev, record, probs = pkg.Evaluator(gpu), [], []
    res = model.test(loader, record=record, evaluator=ev, probs=probs)
    model.hot.check_bounds()
    got = ev.counts()
    assert len(probs) == 7 and got["batches"] == 7
    labels = data["label"][:224].astype(np.float32)
    prob = torch.cat(probs).cpu().numpy()
    want = pkg.eval_reference(prob, labels)
    _assert_counts(got, want)
    assert got["total"] == 224
    _assert_logloss(got, want, 224)
    assert record == [got["correct"] / 224] and res["accuracy"] == record[0]
    assert res["positives"] + res["negatives"] == 224 and 0.0 <= res["auc"] <= 1.0
    # the logits are the training forward's: predict == the model call, through the sigmoid
    it = iter(loader)
    b = next(it)
    idx = pkg.PackedIndices(b.sparse.reshape(T, B, 1))
    pz = torch.sigmoid(model.predict(b.dense, idx)).reshape(-1)
    assert torch.allclose(pz, model.forward(b.dense, idx), rtol=1e-6, atol=1e-7)
    assert np.array_equal(_bits(pz), _bits(torch.sigmoid(model.predict(b.dense, b.sparse)).reshape(-1)))
    # one training step, then a second pass: the model is read, not a cache
    model.step(b.dense, idx, b.labels)
    it.close()
    res2 = model.test(loader, record=record)
    assert len(record) == 2 and res2["total"] == 224
    assert res2["logloss"] * 224 != got["loss_sum"]
    loader.close()
