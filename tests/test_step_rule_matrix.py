"""Who completes whose backward: every ordered pair of rules over one split build.

Rule A runs dlrm_step_fwd and its step backward with DLRM_STEP_BWD_ONLY, which steps the build's once-hit rows with A
and leaves their dt rows unwritten.  Rule B then asks to finish that step, once as its step backward with
DLRM_STEP_APPLY_ONLY and once (after a fresh forward and A's backward) as its update with DLRM_UPDATE_PREBUILT.  The
library takes the call exactly when B is A -- for the stochastic rule: bound to the same handle -- and refuses every
other with DLRM_E_STATE before anything is launched: the tables, B's state and B's step word stay as they were.  The
B position has a sixth entry, a second StochasticDescent handle with another seed.

17 bf16 tables, D = 16, B = 8: the row-wise Adagrad rule's split backward exists with 17..32 features only, so this is
the smallest table set at which all five rules have one (asserted: IX_SINGLES_DONE after every A-backward, or a pair
would pass without a once-hit row stepped).  Table 0 has every row hit once, table 1 one row hit twice.

The Python mirror of the refusal is HipTables(opt=...): update_ with another optimizer object raises ValueError.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, D, B, LR = 17, 16, 8, 0.05
A_RULES = ["descent", "split", "adagrad", "rowwise", "stochastic"]
B_RULES = A_RULES + ["stochastic2"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().copy()


@pytest.fixture(scope="module")
def setup(pkg, gpu):
    rng = np.random.default_rng(17)
    rows = [B] + [24] * (T - 1)
    ts = pkg.EmbeddingTableSet([torch.from_numpy(rng.uniform(-1, 1, (n, D)).astype(np.float32)).to(torch.bfloat16).to(gpu)
                                for n in rows])
    idx = np.stack([rng.permutation(24)[:B] for _ in range(T)])  # distinct rows per table ...
    idx[0] = rng.permutation(B)                                  # ... table 0: every row, once
    idx[1][B - 1] = idx[1][0]                                    # ... table 1: one row twice
    p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu))
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(torch.bfloat16)
    F = T + 1
    dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(torch.bfloat16)
    kw = dict(index_base=0)
    eng = {
        "descent": pkg.HotPath(ts, B, 1, lr=LR, **kw),
        "split": pkg.HotPath(ts, B, 1, opt=pkg.SplitDescent(LR), fused_step=True, **kw),
        "adagrad": pkg.HotPath(ts, B, 1, opt=pkg.ADAGrad(LR, 1e-8), adagrad_step=True, **kw),
        "rowwise": pkg.HotPath(ts, B, 1, opt=pkg.RowwiseADAGrad(LR, 1e-8), adagrad_step=True, **kw),
        "stochastic": pkg.HotPath(ts, B, 1, opt=pkg.StochasticDescent(LR, seed=1), stochastic_step=True, **kw),
        "stochastic2": pkg.HotPath(ts, B, 1, opt=pkg.StochasticDescent(LR, seed=2), stochastic_step=True, **kw),
    }
    assert all(e.step_api for e in eng.values())
    return ts, p, x, dout, eng


def _rc(pkg, call):
    try:
        call()
    except pkg._lib.DLRMError as e:
        return e.code
    return pkg._lib.OK


def _snapshot(pkg, ts, e):
    """The tables, and what the engine's optimizer keeps beside them: state tensors and the step word."""
    torch.cuda.synchronize()
    snap = [_bits(t.data) for t in ts]
    if e.opt is not None:
        snap += [s.detach().cpu().numpy().copy() for s in e.opt.state_of(ts)]
        if isinstance(e.opt, pkg.StochasticDescent):
            snap.append(np.array([e.opt.step_of(ts)], dtype=np.uint64))
    return snap


def _a_backward(pkg, ts, p, x, dout, ea):
    ea.step_fwd(x, p)
    ea.step_bwd(dout, x=x, idx=p, flags=pkg._lib.STEP_BWD_ONLY)
    assert ea.indexer.state() & pkg._lib.IX_SINGLES_DONE, "the split backward did not run: the pair would pass vacuously"


@pytest.mark.parametrize("b", B_RULES)
@pytest.mark.parametrize("a", A_RULES)
def test_only_the_same_rule_and_handle_completes_a_backward(pkg, gpu, setup, a, b):
    ts, p, x, dout, eng = setup
    lib = pkg._lib
    ea, eb = eng[a], eng[b]
    want = lib.OK if a == b else lib.E_STATE
    finishers = {
        "step_bwd(APPLY_ONLY)": lambda: eb.step_bwd(dout, x=x, idx=p, flags=lib.STEP_APPLY_ONLY),
        "update(PREBUILT)": lambda: eb.sgd_update(p, True) if eb.opt is None else eb.opt_update(p, True),
    }
    for what, finish in finishers.items():
        _a_backward(pkg, ts, p, x, dout, ea)
        before = _snapshot(pkg, ts, eb)
        home, eb.indexer = eb.indexer, ea.indexer  # B finishes on the build A's backward ran on
        try:
            rc = _rc(pkg, finish)
        finally:
            eb.indexer = home
        print(f"{a} then {b} {what}: rc {rc}")
        assert rc == want, f"{a} then {b} {what}: rc {rc}, expected {want}"
        if rc != lib.OK:
            after = _snapshot(pkg, ts, eb)
            assert all(np.array_equal(u, v) for u, v in zip(before, after)), f"{a} then {b} {what}: refused, yet wrote"
    ts.ctx.check_bounds()


@pytest.mark.parametrize("rule", ["split", "adagrad", "rowwise", "stochastic"])
def test_hiptables_refuse_another_optimizer_object(pkg, gpu, setup, rule):
    ts, p, x, dout, _ = setup
    make = {"split": lambda: pkg.SplitDescent(LR), "adagrad": lambda: pkg.ADAGrad(LR, 1e-8),
            "rowwise": lambda: pkg.RowwiseADAGrad(LR, 1e-8), "stochastic": lambda: pkg.StochasticDescent(LR, seed=1)}[rule]
    opt = make()
    ht = pkg.HipTables([t.data.clone() for t in ts], opt=opt, index_base=0, defer_update=False,
                       stochastic_step=rule == "stochastic")
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
    _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
    _, _, dy = back(dout)
    assert dy.applied
    before = _snapshot(pkg, ht._ts, ht.hotpath(B))
    with pytest.raises(ValueError, match="these HipTables step with"):
        pkg.update_(make(), ht, pkg.maplookup_pullback(D, ht, p, dy))
    after = _snapshot(pkg, ht._ts, ht.hotpath(B))
    assert all(np.array_equal(u, v) for u, v in zip(before, after))
    pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))  # the same object completes it
    ht.check_bounds()
