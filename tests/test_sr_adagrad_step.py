"""The fused training step with the seeded Adagrad rules: dlrm_sr_adagrad_step_bwd / dlrm_sr_adagrad_step_bwd_prepare
through HotPath(opt=ADAGrad | RowwiseADAGrad(eta, eps, seed=s), sr_adagrad_step=True) and HipTables(...,
sr_adagrad_step=True).  Both rules run in every test.

The rules' random bits are a function of (seed, step, table, row, column) alone, so every comparison here is
np.array_equal on bits -- weights, state, dx and out; no case has a tolerance.  Nothing compares the fused kernels
only with themselves.  The first reference is the operator route (HotPath(opt=seeded) without the keyword: fused
forward, dlrm_interact_bwd_gather, dlrm_adagrad_update(PREBUILT)) from the same weights, state, seed and step.  The
second, independent of the stochastic kernels, is the seedless rule of the same kind (dlrm_adagrad_update with a
dlrm_adagrad_create handle) on an fp32 copy of the tables, fed the operator route's full dt through the same indexer
build, followed by the numpy restatement of the store (sr_round / philox4x32_10) with the step the call used; its
state is compared bit for bit, and the copy restarts from the bf16 result each step, as tests/test_sr_adagrad.py does.

Shapes: rows cycled from [2, 8, 40, 5000, 3, 100000] with one-hot lookups and B = 1024 give a multi-slice hot segment
(512 positions on the 2-row table), chunks longer than the inline positions and several hundred once-hit rows.
Which shapes step their once-hit rows inside the backward is `_has_form`.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rand_indices, rand_tables

pytestmark = pytest.mark.gpu

ROWS = [2, 8, 40, 5000, 3, 100000]
ROWS_SMALL = [2, 8, 40, 5000, 3, 300]  # (the state machine test snapshots every table and state many times)
LR, EPS = 0.05, 1e-8
SEED = 12345
BIG_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15  # both halves set
BIG_STEP = (3 << 32) | 0xFFFFFFFE           # >= 2^32, and its low half carries into the high one after two steps
_M32 = 0xFFFFFFFF
KINDS = [False, True]
KIND_IDS = ["elementwise", "rowwise"]
kinds = pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)


def _rule(pkg, rowwise):
    return pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad


def _bit(pkg, rowwise):
    return pkg._lib.IX_SINGLES_SR_ROWWISE if rowwise else pkg._lib.IX_SINGLES_SR_ADAGRAD


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy()


def _nearest(w):
    """round-to-nearest bf16 bits of an fp32 numpy array"""
    return _bits(torch.from_numpy(w).to(torch.bfloat16))


def _has_form(rowwise, D, T, xview=False):
    """Shapes whose step backward has the rule's once-hit write: up to 32 features, x and rows
    16-B aligned, dim 128 or <= 64; row-wise: more than 16 features and dim a power of two >= 8; element-wise: not
    the one-wave form (dim <= 64) with up to 16 features.  Every other shape takes the gather backward and the
    rule's apply."""
    if T > 31 or xview or not (D == 128 or D <= 64):
        return False
    if rowwise:
        return T >= 16 and D >= 8 and D & (D - 1) == 0
    return T >= 16 or D == 128


class _Inputs:
    """Seeded bf16 start weights, index batches, x and dout of one shape."""

    def __init__(self, pkg, gpu, D, T, B, nbatches=3, seed=0, rows=ROWS):
        rng = np.random.default_rng(1000 * D + 10 * T + seed)
        self.rows, self.D, self.T, self.B = [rows[t % len(rows)] for t in range(T)], D, T, B
        self.w = [torch.from_numpy(t).to(torch.bfloat16) for t in rand_tables(rng, self.rows, D)]
        self.idx = [rand_indices(rng, self.rows, B, 1) for _ in range(nbatches)]
        self.packs = [pkg.PackedIndices(torch.from_numpy(i).to(torch.int32).to(gpu)) for i in self.idx]
        self.x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(torch.bfloat16)
        F = T + 1
        self.dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(
            torch.bfloat16)

    def tables(self, pkg, gpu):
        return pkg.EmbeddingTableSet([t.clone().to(gpu) for t in self.w])

    def engine(self, pkg, gpu, rowwise, seed=SEED, first_step=0, **kw):
        """A HotPath on fresh tables at the start weights, its own optimizer (fresh state) at `first_step`."""
        ts = self.tables(pkg, gpu)
        opt = _rule(pkg, rowwise)(LR, EPS, seed=seed)
        hp = pkg.HotPath(ts, self.B, 1, index_base=0, opt=opt, **kw)
        hp.state0 = [s.clone() for s in opt.state_of(ts)]
        if first_step:
            opt.seek(ts, first_step)
        return hp

    def reset(self, hp, first_step=0):
        for t, w in zip(hp.ts, self.w):
            t.data.copy_(w)
        for s, s0 in zip(hp.opt.state_of(hp.ts), hp.state0):
            s.copy_(s0)
        hp.opt.seek(hp.ts, first_step)


def _snap(hp):
    return [_bits(t.data) for t in hp.ts], [_bits(s) for s in hp.opt.state_of(hp.ts)]


def _restated(pkg, w32, touched, seed, step, t):
    """The bits the rule stores in table t for the fp32 results w32 ([rows][D]) at `step`: an untouched row's W' is
    its bf16 value (low half 0), which the store keeps whatever R; a touched row takes R of (seed, step, t, row,
    column): counter (row, t << 16 | column >> 2, step lo, step hi), key (seed lo, seed hi), word column & 3."""
    u = np.ascontiguousarray(w32).view(np.uint32)
    un = np.ones(len(u), dtype=bool)
    un[touched] = False
    assert not (u[un] & 0xFFFF).any()
    want = (u >> 16).astype(np.uint16)
    rows = np.unique(touched)
    d = w32.shape[1]
    blocks = np.arange((d + 3) // 4, dtype=np.uint64)[None, :]
    out = pkg.philox4x32_10([rows.astype(np.uint64)[:, None], np.uint64(t << 16) | blocks, step & _M32, step >> 32],
                            [seed & _M32, seed >> 32])
    r = np.stack(out, axis=-1).reshape(len(rows), -1)[:, :d] & np.uint32(0xFFFF)
    want[rows] = pkg.sr_round(w32[rows], 0, 0, 0, bits=r)
    if len(u) <= 5000:  # ... and the package's own whole-table restatement where that is cheap
        assert np.array_equal(want, pkg.sr_round(w32, seed, step, t))
    return want


_REF = {}


def _reference(pkg, gpu, inp, rowwise, seq, xb=None, key=None, seed=SEED, first_step=0):
    """The operator route over the batches `seq`, checked at every step against the seedless rule on fp32 tables + the
    restated store.  Returns per step (table bits, state bits, out bits, dx bits, elements stored otherwise than
    round-to-nearest would)."""
    key = None if key is None else (key, rowwise)
    if key is not None and key in _REF:
        return _REF[key]
    hop = inp.engine(pkg, gpu, rowwise, seed=seed, first_step=first_step)
    assert not hop.step_api and hop.pipeline is None and not hop.sr_adagrad_step and not hop.adagrad_step
    ref = pkg.EmbeddingTableSet([t.data.float() for t in hop.ts])
    ropt = _rule(pkg, rowwise)(LR, EPS)
    for s, r in zip(hop.opt.state_of(hop.ts), ropt.state_of(ref)):
        assert np.array_equal(_bits(s), _bits(r))  # (both kinds of handle start from the same state)
    steps = []
    for k, b in enumerate(seq):
        p = inp.packs[b]
        assert hop.opt.step_of(hop.ts) == first_step + k
        hop.lookup_interact_fwd(inp.x, p)
        hop.interact_bwd(inp.dout, x=inp.x if xb is None else xb, idx=p, build_indexer=True)
        # the same build for both: the rows' sums are taken in one order
        pkg.update_(ropt, ref, pkg.maplookup_pullback(inp.D, ref, p, hop.dt), hop.indexer, index_base=0, prebuilt=True,
                    check_bounds=False)
        hop.opt_update(p, True)
        torch.cuda.synchronize()
        hop.check_bounds()
        (got, st), odd = _snap(hop), 0
        for t in range(inp.T):
            w32 = ref[t].data.cpu().numpy()
            want = _restated(pkg, w32, inp.idx[b][t], seed, first_step + k, t)
            assert np.array_equal(got[t], want), f"operator route, step {k} table {t}: != seedless rule + sr_round"
            assert np.array_equal(st[t], _bits(ropt.state_of(ref)[t])), f"operator route, step {k} table {t}: state"
            odd += int((want != _nearest(w32)).sum())
            ref[t].data.copy_(hop.ts[t].data.float())  # the next step starts from the bf16 result
        steps.append((got, st, _bits(hop.out), _bits(hop.dx), odd))
    assert hop.opt.step_of(hop.ts) == first_step + len(seq)
    if key is not None:
        _REF[key] = steps
    return steps


def _assert_step(hp, want, what, out=True):
    tabs, state, o, dx, _ = want
    torch.cuda.synchronize()
    hp.check_bounds()
    got, st = _snap(hp)
    for t in range(len(tabs)):
        assert np.array_equal(got[t], tabs[t]), f"{what} table {t}: {(got[t] != tabs[t]).sum()} of {got[t].size} " \
                                                "elements differ from the operator route"
        assert np.array_equal(st[t], state[t]), f"{what} table {t}: {(st[t] != state[t]).sum()} of {st[t].size} state " \
                                                "words differ from the operator route"
    assert np.array_equal(_bits(hp.dx), dx), f"{what}: dx"
    if out:
        assert np.array_equal(_bits(hp.out), o), f"{what}: out"


def _assert_untouched(inp, k, before, after, what):
    for t, n in enumerate(inp.rows):
        un = np.ones(n, dtype=bool)
        un[inp.idx[k][t]] = False
        assert np.array_equal(after[0][t][un], before[0][t][un]), f"{what} table {t}: an untouched row changed"
        assert np.array_equal(after[1][t][un], before[1][t][un]), f"{what} table {t}: an untouched row's state changed"


def _assert_same(a, b):
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert np.array_equal(x, y)


# ---- 1. every kernel form and fallback, 2. padding samples: three plain fused steps against both references
SHAPES = [  # (D, T, B, backward's x is an unaligned view)
    (128, 20, 1024, False),  # the required form: NB = 2, two waves per sample
    (128, 4, 1024, False),   # NB = 1: the element-wise rule's two-wave form; the row-wise rule falls back
    (128, 20, 2112, False),  # B > 2048: 8 columns per lane (element-wise), two waves per sample (row-wise)
    (128, 4, 2112, False),
    (16, 4, 1024, False), (64, 4, 1024, False),    # one wave per sample, NB = 1: both rules fall back
    (16, 20, 1024, False), (64, 20, 1024, False),  # one wave per sample, NB = 2
    (8, 20, 1024, False),    # the row-wise minimum
    (256, 4, 1024, False),   # interact_bwd_update_kernel's shapes: no form with these rules, the fallback
    (16, 33, 1024, False),   # F > 32: no split backward, the gather backward + the rule's apply with once-hit items
    (128, 20, 1024, True),   # x_ld not 16-B aligned in the backward: the same fallback
    (48, 20, 1024, False),   # dim not a power of two: the element-wise rule fuses, the row-wise one falls back
    # padding samples (the row-wise barrier and shuffles in uniform control flow)
    (128, 20, 1022, False),  # two waves, 4 samples per block
    (16, 20, 1022, False),   # one wave, 8 per block
    (128, 20, 2051, False),  # 8 columns per lane, 2 per block (element-wise), odd B
]


@kinds
@pytest.mark.parametrize("D,T,B,xview", SHAPES, ids=[f"d{d}-t{t}-b{b}{'-xview' if v else ''}" for d, t, b, v in SHAPES])
def test_fused_step_equals_operator_route_and_seedless_rule(pkg, gpu, D, T, B, xview, rowwise):
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, D, T, B)
    xb = None
    if xview:
        buf = torch.zeros((B, D + 4), dtype=torch.bfloat16, device=gpu)
        xb = buf[:, :D]
        xb.copy_(inp.x)
        assert (xb.stride(0) * 2) % 16 != 0
    want = _reference(pkg, gpu, inp, rowwise, [0, 1, 2], xb,
                      key=(D, T, B, "plain") if (D, T, B, xview) == (128, 20, 1024, False) else None)
    hp = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True)
    assert hp.step_api and hp.sr_adagrad_step and not hp.adagrad_step
    both = _lib.IX_SINGLES_DONE | _bit(pkg, rowwise)
    every = both | _lib.IX_SINGLES_SR_ADAGRAD | _lib.IX_SINGLES_SR_ROWWISE | _lib.IX_SINGLES_ADAGRAD | \
        _lib.IX_SINGLES_ROWWISE | _lib.IX_SINGLES_STOCHASTIC | _lib.IX_SINGLES_SPLIT
    start = _snap(hp)
    for k in range(3):
        before = _snap(hp) if k else start
        assert hp.opt.step_of(hp.ts) == k
        hp.step_fwd(inp.x, inp.packs[k])
        hp.step_bwd(inp.dout, x=inp.x if xb is None else xb, idx=inp.packs[k])
        _assert_step(hp, want[k], f"step {k}:")
        _assert_untouched(inp, k, before, _snap(hp), f"step {k}:")
        assert hp.indexer.state() & every == (both if _has_form(rowwise, D, T, xview) else 0)
        assert hp.opt.step_of(hp.ts) == k + 1  # (exactly one per step)
    # what keeps the case from passing vacuously
    _, c = np.unique(inp.idx[2][3], return_counts=True)
    assert (c == 1).sum() > 100  # (once-hit rows of the 5000-row table)
    assert all(w[4] > 0 for w in want)  # (some element is stored otherwise than round-to-nearest would)
    assert any((a != b).any() for a, b in zip(want[2][1], start[1]))  # (the state moved)
    plain = pkg.HotPath(inp.tables(pkg, gpu), B, 1, index_base=0, opt=_rule(pkg, rowwise)(LR, EPS), adagrad_step=True)
    plain.step_fwd(inp.x, inp.packs[0])
    plain.step_bwd(inp.dout, x=inp.x if xb is None else xb, idx=inp.packs[0])
    torch.cuda.synchronize()
    plain.check_bounds()
    # (not the seedless fused step in disguise)
    assert any((a != b).any() for a, b in zip([_bits(t.data) for t in plain.ts], want[0][0]))


# ---- 3. both halves of the step and of the seed reach the backward's counter and key
@kinds
@pytest.mark.parametrize("D", [128, 16], ids=["two-waves", "one-wave"])
def test_step_and_seed_above_32_bits(pkg, gpu, D, rowwise):
    inp = _Inputs(pkg, gpu, D, 20, 1024, seed=8, rows=ROWS_SMALL)
    want = _reference(pkg, gpu, inp, rowwise, [0, 1, 2], seed=BIG_SEED, first_step=BIG_STEP)
    hp = inp.engine(pkg, gpu, rowwise, seed=BIG_SEED, first_step=BIG_STEP, sr_adagrad_step=True)
    for k in range(3):
        hp.step(inp.x, inp.packs[k], inp.dout)
        _assert_step(hp, want[k], f"step {k}:")
        assert hp.indexer.state() & _bit(pkg, rowwise)
    assert hp.opt.step_of(hp.ts) == BIG_STEP + 3 and (BIG_STEP + 3) >> 32 == (BIG_STEP >> 32) + 1
    # ... and each half matters: the low halves alone give other tables
    low = _reference(pkg, gpu, inp, rowwise, [0], seed=BIG_SEED & _M32, first_step=BIG_STEP & _M32)
    assert any((a != b).any() for a, b in zip(low[0][0], want[0][0]))


# ---- 4. pipelines
@kinds
@pytest.mark.parametrize("D", [128, 16])
@pytest.mark.parametrize("parts", [16, 32])
@pytest.mark.parametrize("B", [1024, 2048])
def test_pipeline_apply_equals_plain_step(pkg, gpu, B, parts, D, rowwise):
    """Four steps over two alternating batches through prime + step_prep == step, bit for bit, == the references."""
    inp = _Inputs(pkg, gpu, D, 20, B, nbatches=2, seed=1, rows=ROWS_SMALL)
    seq = [0, 1, 0, 1]
    want = _reference(pkg, gpu, inp, rowwise, seq, key=(D, 20, B, "alt"))
    plain = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True, parts=parts)
    hp = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True, pipeline="apply", parts=parts)
    assert hp.pipeline == "apply"
    for k, b in enumerate(seq):
        plain.step(inp.x, inp.packs[b], inp.dout)
        nxt = inp.packs[seq[(k + 1) % 4]]
        if k == 0:
            hp.prime(nxt, inp.x, inp.dout, prev=inp.packs[b])
        else:
            hp.step_prep(inp.x, inp.packs[b], inp.dout, nxt)
        _assert_step(plain, want[k], f"plain step {k}:")
        _assert_step(hp, want[k], f"pipelined step {k}:")
        assert plain.indexer.state() & _bit(pkg, rowwise)
    assert hp._ixs[hp._cur].state() & pkg._lib.IX_PREPARED  # (the last apply launch built the next batch)
    assert plain.opt.step_of(plain.ts) == 4 and hp.opt.step_of(hp.ts) == 4


@kinds
def test_pipeline_apply_above_2048_positions(pkg, gpu, rowwise):
    """The apply launch that carries the scan build (more than 2048 positions per table, int32 indices, B % 4 == 0)."""
    inp = _Inputs(pkg, gpu, 128, 20, 2112, nbatches=2, seed=7, rows=ROWS_SMALL)
    seq = [0, 1, 0]
    want = _reference(pkg, gpu, inp, rowwise, seq)
    hp = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True, pipeline="apply")
    assert hp.pipeline == "apply"
    hp.prime(inp.packs[1], inp.x, inp.dout, prev=inp.packs[0])
    _assert_step(hp, want[0], "step 0:")
    assert hp._ixs[hp._cur].state() & pkg._lib.IX_PREPARED
    for k in (1, 2):
        hp.step_prep(inp.x, inp.packs[seq[k]], inp.dout, inp.packs[1 - seq[k]])
        _assert_step(hp, want[k], f"step {k}:")
    assert hp.opt.step_of(hp.ts) == 3


@kinds
def test_pipeline_side(pkg, gpu, rowwise):
    inp = _Inputs(pkg, gpu, 128, 20, 1024, nbatches=2, seed=2, rows=ROWS_SMALL)
    want = _reference(pkg, gpu, inp, rowwise, [0, 1, 0])
    hp = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True, pipeline="side")
    assert hp.pipeline == "side"
    for k, b in enumerate([0, 1, 0]):
        hp.step_next(inp.x, inp.packs[b], inp.dout, inp.packs[1 - b])
        _assert_step(hp, want[k], f"step {k}:")
        assert hp.indexer.state() & _bit(pkg, rowwise)
    assert hp.opt.step_of(hp.ts) == 3


# ---- 5. flags
@kinds
def test_bwd_only_then_apply_only_and_prebuilt_update(pkg, gpu, rowwise):
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, 128, 20, 1024)
    want = _reference(pkg, gpu, inp, rowwise, [0, 1, 2], key=(128, 20, 1024, "plain"))
    two = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True)
    upd = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True)
    for k in range(2):
        for hp in (two, upd):
            hp.step_fwd(inp.x, inp.packs[k])
            hp.step_bwd(inp.dout, flags=_lib.STEP_BWD_ONLY)
            assert hp.indexer.state() & _bit(pkg, rowwise)
            assert hp.opt.step_of(hp.ts) == k  # (the backward alone does not advance the word)
        two.step_bwd(inp.dout, flags=_lib.STEP_APPLY_ONLY)
        upd.opt_update(inp.packs[k], True)  # dlrm_adagrad_update(PREBUILT): the repeated rows only
        _assert_step(two, want[k], f"step {k}, BWD_ONLY + APPLY_ONLY:")
        _assert_step(upd, want[k], f"step {k}, BWD_ONLY + dlrm_adagrad_update(PREBUILT):")
        assert two.opt.step_of(two.ts) == k + 1 and upd.opt.step_of(upd.ts) == k + 1


# ---- 6. the state machine
def test_cross_rule_combinations_are_refused_and_write_nothing(pkg, gpu):
    """The two seeded rules and a second handle of each (another seed) against each other and against the five
    existing rules, in both orders, and a second backward on one build: DLRM_E_STATE, no table bit, no state word
    and no step word changed.  (20 tables of dim 128: all seven rules have a backward form.)"""
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, 128, 20, 1024, nbatches=1, rows=ROWS_SMALL)
    p, x, dout, B, D = inp.packs[0], inp.x, inp.dout, inp.B, inp.D
    hp = inp.engine(pkg, gpu, False, sr_adagrad_step=True)
    ts = hp.ts
    lib, h = hp.ctx.lib, hp.ctx.bind()
    vp = ctypes.c_void_p
    step = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, vp(x.data_ptr()), x.stride(0), vp(dout.data_ptr()),
            dout.stride(0), hp.padding, vp(hp.dx.data_ptr()), hp.dx.stride(0), vp(hp.dt.data_ptr()), hp.dt.stride(0), LR)
    upd = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, vp(hp.dt.data_ptr()), _lib.F32, hp.dt.stride(0), D, LR)
    ixh = hp.indexer.handle
    PRE, AO, BO = _lib.UPDATE_PREBUILT, _lib.STEP_APPLY_ONLY, _lib.STEP_BWD_ONLY
    split, ada, roww, sgd = pkg.SplitDescent(LR), pkg.ADAGrad(LR, EPS), pkg.RowwiseADAGrad(LR, EPS), \
        pkg.StochasticDescent(LR, seed=SEED)
    seeded = {"sr_adagrad": hp.opt, "sr_rowwise": pkg.RowwiseADAGrad(LR, EPS, seed=SEED),
              "sr_adagrad_2": pkg.ADAGrad(LR, EPS, seed=SEED + 1), "sr_rowwise_2": pkg.RowwiseADAGrad(LR, EPS, seed=SEED + 1)}
    stateful = [split, ada, roww] + list(seeded.values())
    words = [sgd] + list(seeded.values())
    for k, o in enumerate(words):
        o.seek(ts, 7 + k)

    def adagrad_rule(o, new):
        oh = o.handle_of(ts)
        name = "dlrm_sr_adagrad_step_bwd" if new else "dlrm_adagrad_step_bwd"
        return (lambda f: getattr(lib, name)(h, ts.handle, oh, ixh, *step, EPS, f),
                lambda: lib.dlrm_adagrad_update(h, ts.handle, oh, ixh, PRE, *upd, EPS))

    sh, gh = split.handle_of(ts), sgd.handle_of(ts)
    # name -> (the step backward with flags f, the update(PREBUILT), the bit its backward marks a build with)
    rules = {"descent": (lambda f: lib.dlrm_step_bwd(h, ts.handle, ixh, *step, f),
                         lambda: lib.dlrm_sgd_update(h, ts.handle, ixh, PRE, *upd), 0),
             "split": (lambda f: lib.dlrm_split_step_bwd(h, ts.handle, sh, ixh, *step, f),
                       lambda: lib.dlrm_split_sgd_update(h, ts.handle, sh, ixh, PRE, *upd), _lib.IX_SINGLES_SPLIT),
             "adagrad": (*adagrad_rule(ada, False), _lib.IX_SINGLES_ADAGRAD),
             "rowwise": (*adagrad_rule(roww, False), _lib.IX_SINGLES_ROWWISE),
             "stochastic": (lambda f: lib.dlrm_sr_step_bwd(h, ts.handle, gh, ixh, *step, f),
                            lambda: lib.dlrm_sr_sgd_update(h, ts.handle, gh, ixh, PRE, *upd), _lib.IX_SINGLES_STOCHASTIC)}
    for name, o in seeded.items():
        rules[name] = (*adagrad_rule(o, True), _lib.IX_SINGLES_SR_ROWWISE if o.rowwise else _lib.IX_SINGLES_SR_ADAGRAD)
    every = 0
    for _, _, bit in rules.values():
        every |= bit

    def snap():
        torch.cuda.synchronize()
        return ([_bits(t.data) for t in ts] + [_bits(s) for o in stateful for s in o.state_of(ts)],
                [o.step_of(ts) for o in words])

    def unchanged(before, what):
        arrays, steps = snap()
        assert steps == before[1], (what, steps, before[1])
        for a, b in zip(before[0], arrays):
            assert np.array_equal(a, b), what

    for first, (bwd, _, bit) in rules.items():
        hp.step_fwd(x, p)
        assert bwd(BO) == 0, first
        assert hp.indexer.state() & (_lib.IX_SINGLES_DONE | every) == _lib.IX_SINGLES_DONE | bit, first
        before = snap()
        for second, (bwd2, upd2, _) in rules.items():
            if second == first or not (first in seeded or second in seeded):
                continue  # (pairs of two existing rules: tests/test_step_rule_matrix.py)
            what = f"{second} after {first}'s backward"
            assert bwd2(AO) == _lib.E_STATE, what
            assert bwd2(0) == _lib.E_STATE, what  # (a second backward on one build, whichever rule's)
            assert bwd2(BO) == _lib.E_STATE, what
            # (Descent's dlrm_sgd_update and a rule's own family alike)
            assert upd2() == _lib.E_STATE, what
        assert bwd(0) == _lib.E_STATE and bwd(BO) == _lib.E_STATE, first  # a second backward of its own
        unchanged(before, first)
        assert bwd(AO) == 0, first  # its own apply completes it
        torch.cuda.synchronize()
        after = [o.step_of(ts) for o in words]
        moved = [k for k, (a, b) in enumerate(zip(before[1], after)) if a != b]
        own = [k for k, o in enumerate(words) if first in seeded and o is seeded[first] or first == "stochastic" and o is sgd]
        assert moved == own and all(after[k] == before[1][k] + 1 for k in own), (first, before[1], after)

    # argument errors: a plain handle, fp32 tables, a handle made for another dim, both flags
    hp.step_fwd(x, p)
    before = snap()
    new, srh = lib.dlrm_sr_adagrad_step_bwd, hp.opt.handle_of(ts)
    for plain in (ada, roww):
        assert new(h, ts.handle, plain.handle_of(ts), ixh, *step, EPS, 0) == _lib.E_ARG
        assert lib.dlrm_sr_adagrad_step_bwd_prepare(h, ts.handle, plain.handle_of(ts), ixh, *step, EPS, ixh, None, 0) == _lib.E_ARG
    f32 = pkg.EmbeddingTableSet([t.float().to(gpu) for t in inp.w])
    assert new(h, f32.handle, srh, ixh, *step, EPS, 0) == _lib.E_ARG
    other = pkg.EmbeddingTableSet([torch.zeros((n, 16), dtype=torch.bfloat16, device=gpu) for n in inp.rows])
    assert new(h, other.handle, srh, ixh, *step, EPS, 0) == _lib.E_ARG
    assert new(h, ts.handle, srh, ixh, *step, EPS, BO | AO) == _lib.E_ARG
    # ... and dlrm_adagrad_step_bwd still refuses the seeded handle
    assert lib.dlrm_adagrad_step_bwd(h, ts.handle, srh, ixh, *step, EPS, 0) == _lib.E_UNSUPPORTED
    assert not hp.indexer.state() & _lib.IX_SINGLES_DONE
    unchanged(before, "argument errors")
    hp.check_bounds()


# ---- 7. bounds
@kinds
def test_bad_index_in_the_current_batch_writes_nothing_and_the_step_advances(pkg, gpu, rowwise):
    inp = _Inputs(pkg, gpu, 128, 20, 1024, seed=3, rows=ROWS_SMALL)
    bad_np = inp.idx[0].copy()
    bad_np[3, 517] = inp.rows[3] + 2
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    hp = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True)
    before = _snap(hp)
    hp.step(inp.x, bad, inp.dout)
    with pytest.raises(pkg.BoundsError):
        hp.check_bounds()
    _assert_same(before, _snap(hp))  # (no table or state word written: every row went to dt)
    assert hp.indexer.state() & _bit(pkg, rowwise)  # (the backward did run)
    assert hp.opt.step_of(hp.ts) == 1  # (the call returned DLRM_OK and launched)


@kinds
def test_bad_index_in_the_next_batch_only(pkg, gpu, rowwise):
    """pipeline="apply": the current step's rows are written and nothing is raised yet; the step on the bad batch
    raises and writes nothing."""
    inp = _Inputs(pkg, gpu, 128, 20, 1024, seed=4, rows=ROWS_SMALL)
    want = _reference(pkg, gpu, inp, rowwise, [0])
    bad_np = inp.idx[1].copy()
    bad_np[3, 99] = inp.rows[3] + 1
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    hp = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True, pipeline="apply")
    hp.prime(bad, inp.x, inp.dout, prev=inp.packs[0])
    _assert_step(hp, want[0], "apply:")  # (checks bounds: clean)
    before = _snap(hp)
    hp.step_prep(inp.x, bad, inp.dout, inp.packs[0])
    with pytest.raises(pkg.BoundsError):
        hp.check_bounds()
    _assert_same(before, _snap(hp))
    assert hp.opt.step_of(hp.ts) == 2


# ---- 8. graph capture
@kinds
def test_pipelined_step_graph_replay_equals_eager(pkg, gpu, rowwise):
    """A captured pipelined chain of two steps replayed twice == the same four steps run eagerly from the same
    starting step (themselves == the operator route), and the word advanced by steps x replays."""
    S0 = 1000
    inp = _Inputs(pkg, gpu, 128, 20, 1024, nbatches=1, seed=5, rows=ROWS_SMALL)
    want = _reference(pkg, gpu, inp, rowwise, [0, 0, 0, 0], first_step=S0)
    p = inp.packs[0]
    hg = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True, pipeline="apply")
    he = inp.engine(pkg, gpu, rowwise, sr_adagrad_step=True, pipeline="apply")
    hg.prime(p, inp.x, inp.dout, prev=p)  # eager warm-up: one step, and indexer 0 holds p, prepared
    inp.reset(hg, S0)                     # the tables, the state and the step back to the start
    # (two steps per graph: the two indexers are back in the captured state after each replay)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            hg.step_prep(inp.x, p, inp.dout, p)
            hg.step_prep(inp.x, p, inp.dout, p)
    torch.cuda.current_stream().wait_stream(s)
    he.prime(p, inp.x, inp.dout, prev=p)
    inp.reset(he, S0)
    for _ in range(2):
        gr.replay()
        he.step_prep(inp.x, p, inp.dout, p)
        he.step_prep(inp.x, p, inp.dout, p)
    _assert_step(he, want[3], "eager:")
    _assert_step(hg, want[3], "replayed:")
    assert hg.opt.step_of(hg.ts) == S0 + 4 and he.opt.step_of(he.ts) == S0 + 4


# ---- 9. HipTables
@kinds
@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
def test_hiptables_chain_equals_operator_sequence(pkg, gpu, defer, rowwise):
    inp = _Inputs(pkg, gpu, 16, 20, 1024, nbatches=2, seed=6, rows=ROWS_SMALL)
    want = _reference(pkg, gpu, inp, rowwise, [0, 1], key=(16, 20, 1024, "seed6"))
    opt = _rule(pkg, rowwise)(LR, EPS, seed=SEED)
    ht = pkg.HipTables([t.clone().to(gpu) for t in inp.w], opt=opt, index_base=0, defer_update=defer,
                       sr_adagrad_step=True)
    D = inp.D
    for k, p in enumerate(inp.packs):
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
        assert isinstance(ys, pkg.LazyLookup)
        out, back = pkg.rrule(pkg.DotInteraction(), inp.x, ys)
        _, dx, dy = back(inp.dout)
        assert dy.applied and dy.hp.sr_adagrad_step and dy.hp.indexer.state() & _bit(pkg, rowwise)
        assert np.array_equal(_bits(out), want[k][2]) and np.array_equal(_bits(dx), want[k][3])
        with pytest.raises(ValueError):  # another object
            pkg.update_(_rule(pkg, rowwise)(LR, EPS, seed=SEED), ht, pkg.maplookup_pullback(D, ht, p, dy))
        with pytest.raises(ValueError):
            pkg.update_(pkg.Descent(LR), ht, pkg.maplookup_pullback(D, ht, p, dy))
        pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
        assert (ht._pending is not None) == defer
    ts = ht.ts  # (runs a deferred apply, checks bounds)
    torch.cuda.synchronize()
    for t in range(inp.T):
        assert np.array_equal(_bits(ts[t].data), want[1][0][t])
        assert np.array_equal(_bits(opt.state_of(ts)[t]), want[1][1][t])
    assert opt.step_of(ts) == 2
    opt.eta = 2 * LR  # the tables run with the parameters they were built with, and refuse the object once they differ
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, inp.packs[0])
    _, back = pkg.rrule(pkg.DotInteraction(), inp.x, ys)
    with pytest.raises(ValueError):
        pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, inp.packs[0], back(inp.dout)[2]))


def test_sr_adagrad_step_keyword_errors(pkg, gpu):
    bf = [torch.zeros((8, 16), dtype=torch.bfloat16, device=gpu) for _ in range(2)]
    f32 = [torch.zeros((8, 16), dtype=torch.float32, device=gpu) for _ in range(2)]
    for cls in (pkg.ADAGrad, pkg.RowwiseADAGrad):
        for opt in (cls(), pkg.SplitDescent(), pkg.StochasticDescent(0.1, seed=1), None):  # any other optimizer
            with pytest.raises(ValueError, match="sr_adagrad_step"):
                pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=opt, sr_adagrad_step=True)
            with pytest.raises(ValueError, match="sr_adagrad_step"):
                pkg.HipTables(bf, opt=opt, index_base=0, sr_adagrad_step=True)
        sd = lambda: cls(0.1, 1e-8, seed=5)  # noqa: E731
        with pytest.raises(ValueError, match="bfloat16"):  # fp32 tables
            pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=sd(), sr_adagrad_step=True)
        with pytest.raises(ValueError, match="bfloat16"):
            pkg.HipTables(f32, opt=sd(), index_base=0, sr_adagrad_step=True)
        for kw in ({"materialize_ys": True}, {"lookups": 2}):  # the step kernels are unavailable
            with pytest.raises(ValueError):
                pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, kw.pop("lookups", 1), index_base=0, opt=sd(),
                            sr_adagrad_step=True, **kw)
        for kw in ({"fused_step": True}, {"adagrad_step": True}, {"stochastic_step": True}):  # the others stay refused
            with pytest.raises(ValueError, match="fused step"):
                pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=sd(), sr_adagrad_step=True, **kw)
        hp = pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=sd())  # the default route stays
        assert not hp.step_api and not hp.sr_adagrad_step and not hp.adagrad_step and hp.pipeline is None
        for mode in ("apply", "side"):
            hp = pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=sd(), sr_adagrad_step=True, pipeline=mode)
            assert hp.pipeline == mode and hp.sr_adagrad_step and not hp.adagrad_step
        with pytest.raises(ValueError):  # lr beside the optimizer, as for the other rules
            pkg.HipTables(bf, opt=sd(), lr=0.2, index_base=0, sr_adagrad_step=True)
        with pytest.raises(ValueError, match="adagrad_step"):  # the seedless keyword stays refused with a seed
            pkg.HipTables(bf, opt=sd(), index_base=0, adagrad_step=True)
