"""The fused training step with the stochastic rule: dlrm_sr_step_bwd / dlrm_sr_step_bwd_prepare through
HotPath(opt=StochasticDescent, stochastic_step=True) and HipTables(opt=StochasticDescent, stochastic_step=True).

The rule's random bits are a function of (seed, step, table, row, column) alone, so every comparison here is
np.array_equal on bits; no case has a tolerance.  Nothing compares the fused kernels only with themselves.  The
first reference is the operator route (HotPath(opt=StochasticDescent): fused forward, dlrm_interact_bwd_gather,
dlrm_sr_sgd_update(PREBUILT)) with the same seed from the same weights and step.  The second, independent of the
rule's kernels, is fp32 Descent (dlrm_sgd_update) on an fp32 copy of the tables fed the operator route's full dt,
followed by the numpy restatement of the store (sr_round / philox4x32_10) with the step the call used; the copy
restarts from the bf16 result each step, as tests/test_sr_sgd.py::_run does.

Shapes: rows cycled from [2, 8, 40, 5000, 3, 100000] with one-hot lookups give multi- and one-slice hot segments,
chunks longer than the inline positions and several hundred once-hit rows per batch.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rand_indices, rand_tables

pytestmark = pytest.mark.gpu

ROWS = [2, 8, 40, 5000, 3, 100000]
LR = 0.05
SEED = 12345
BIG_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15  # both halves set
BIG_STEP = (3 << 32) | 0xFFFFFFFE           # >= 2^32, and its low half carries into the high one after two steps
_M32 = 0xFFFFFFFF


def _rows(T):
    return [ROWS[t % len(ROWS)] for t in range(T)]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy()


def _nearest(w):
    """round-to-nearest bf16 bits of an fp32 numpy array"""
    return _bits(torch.from_numpy(w).to(torch.bfloat16))


def _has_form(D, T, xview=False):
    """Shapes whose step backward has the stochastic once-hit write: up to 32 features, x
    and rows 16-B aligned, dim 128 or <= 64.  Every other shape takes the gather backward and the rule's apply."""
    return T <= 31 and not xview and (D == 128 or D <= 64)


class _Inputs:
    """Seeded bf16 start weights, index batches, x and dout of one shape."""

    def __init__(self, pkg, gpu, D, T, B, nbatches=3, seed=0):
        rng = np.random.default_rng(1000 * D + 10 * T + seed)
        self.rows, self.D, self.T, self.B = _rows(T), D, T, B
        self.w = [torch.from_numpy(t).to(torch.bfloat16) for t in rand_tables(rng, self.rows, D)]
        self.idx = [rand_indices(rng, self.rows, B, 1) for _ in range(nbatches)]
        self.packs = [pkg.PackedIndices(torch.from_numpy(i).to(torch.int32).to(gpu)) for i in self.idx]
        self.x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(torch.bfloat16)
        F = T + 1
        self.dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(
            torch.bfloat16)

    def tables(self, pkg, gpu):
        return pkg.EmbeddingTableSet([t.clone().to(gpu) for t in self.w])

    def engine(self, pkg, gpu, seed=SEED, first_step=0, **kw):
        """A HotPath on fresh tables at the start weights, its own optimizer at `first_step`."""
        ts = self.tables(pkg, gpu)
        opt = pkg.StochasticDescent(LR, seed=seed)
        hp = pkg.HotPath(ts, self.B, 1, index_base=0, opt=opt, **kw)
        if first_step:
            opt.seek(ts, first_step)
        return hp

    def reset(self, hp, first_step=0):
        for t, w in zip(hp.ts, self.w):
            t.data.copy_(w)
        hp.opt.seek(hp.ts, first_step)


def _snap(hp):
    return [_bits(t.data) for t in hp.ts]


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


def _reference(pkg, gpu, inp, seq, xb=None, key=None, seed=SEED, first_step=0):
    """The operator route over the batches `seq`, checked at every step against fp32 Descent + the restated store.
    Returns per step (table bits, out bits, dx bits, elements stored otherwise than round-to-nearest would)."""
    if key is not None and key in _REF:
        return _REF[key]
    hop = inp.engine(pkg, gpu, seed=seed, first_step=first_step)
    assert not hop.step_api and hop.pipeline is None
    ref = pkg.EmbeddingTableSet([t.data.float() for t in hop.ts])
    steps = []
    for k, b in enumerate(seq):
        p = inp.packs[b]
        assert hop.opt.step_of(hop.ts) == first_step + k
        hop.lookup_interact_fwd(inp.x, p)
        hop.interact_bwd(inp.dout, x=inp.x if xb is None else xb, idx=p, build_indexer=True)
        hop.opt_update(p, True)
        pkg.update_(pkg.Descent(LR), ref, pkg.maplookup_pullback(inp.D, ref, p, hop.dt), index_base=0)
        torch.cuda.synchronize()
        hop.check_bounds()
        got, odd = _snap(hop), 0
        for t in range(inp.T):
            w32 = ref[t].data.cpu().numpy()
            want = _restated(pkg, w32, inp.idx[b][t], seed, first_step + k, t)
            assert np.array_equal(got[t], want), f"operator route, step {k} table {t}: != fp32 Descent + sr_round"
            odd += int((want != _nearest(w32)).sum())
            ref[t].data.copy_(hop.ts[t].data.float())  # the next step starts from the bf16 result
        steps.append((got, _bits(hop.out), _bits(hop.dx), odd))
    assert hop.opt.step_of(hop.ts) == first_step + len(seq)
    if key is not None:
        _REF[key] = steps
    return steps


def _assert_step(hp, want, what, out=True):
    tabs, o, dx, _ = want
    torch.cuda.synchronize()
    hp.check_bounds()
    for t, a in enumerate(_snap(hp)):
        assert np.array_equal(a, tabs[t]), f"{what} table {t}: {(a != tabs[t]).sum()} of {a.size} elements differ from " \
                                           "the operator route"
    assert np.array_equal(_bits(hp.dx), dx), f"{what}: dx"
    if out:
        assert np.array_equal(_bits(hp.out), o), f"{what}: out"


def _assert_untouched(inp, k, before, after, what):
    for t, n in enumerate(inp.rows):
        un = np.ones(n, dtype=bool)
        un[inp.idx[k][t]] = False
        assert np.array_equal(after[t][un], before[t][un]), f"{what} table {t}: an untouched row changed"


# ---- 1. every kernel form: three plain fused steps against both references
SHAPES = [  # (D, T, B, backward's x is an unaligned view)
    (128, 4, 1024, False),   # NB = 1, two waves per sample
    (128, 20, 1024, False),  # NB = 2, two waves per sample
    (128, 4, 2112, False),   # B > 2048: fused forward + in-LDS split build (16 features or fewer: two waves per sample)
    (128, 20, 2112, False),  # ... and 8 columns per lane (more than 16 features)
    (16, 4, 1024, False), (16, 20, 1024, False), (64, 4, 1024, False), (64, 20, 1024, False),  # one wave per sample
    (8, 4, 1024, False),     # one wave per sample again (dim <= 64)
    (256, 4, 1024, False),   # interact_bwd_update_kernel's shapes: no form with this rule, the fallback
    (16, 33, 1024, False),   # F > 32: no split backward, the gather backward + the rule's apply with once-hit items
    (128, 4, 1024, True),    # x_ld not 16-B aligned in the backward: the same fallback
]


@pytest.mark.parametrize("D,T,B,xview", SHAPES, ids=[f"d{d}-t{t}-b{b}{'-xview' if v else ''}" for d, t, b, v in SHAPES])
def test_fused_step_equals_operator_route_and_fp32_descent(pkg, gpu, D, T, B, xview):
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, D, T, B)
    xb = None
    if xview:
        buf = torch.zeros((B, D + 4), dtype=torch.bfloat16, device=gpu)
        xb = buf[:, :D]
        xb.copy_(inp.x)
        assert (xb.stride(0) * 2) % 16 != 0
    want = _reference(pkg, gpu, inp, [0, 1, 2], xb, key=(D, T, B, xview, "plain"))
    hp = inp.engine(pkg, gpu, stochastic_step=True)
    assert hp.step_api and hp.stochastic_step
    both = _lib.IX_SINGLES_DONE | _lib.IX_SINGLES_STOCHASTIC
    for k in range(3):
        before = _snap(hp)
        assert hp.opt.step_of(hp.ts) == k
        hp.step_fwd(inp.x, inp.packs[k])
        hp.step_bwd(inp.dout, x=inp.x if xb is None else xb, idx=inp.packs[k])
        _assert_step(hp, want[k], f"step {k}:")
        _assert_untouched(inp, k, before, _snap(hp), f"step {k}:")
        assert hp.indexer.state() & both == (both if _has_form(D, T, xview) else 0)
        assert hp.opt.step_of(hp.ts) == k + 1  # (exactly one per step)
    # what keeps the case from passing vacuously
    _, c = np.unique(inp.idx[2][3], return_counts=True)
    assert (c == 1).sum() > 100  # (once-hit rows of the 5000-row table)
    assert all(w[3] > 0 for w in want)  # (some element is stored otherwise than round-to-nearest would)
    desc = pkg.HotPath(inp.tables(pkg, gpu), B, 1, lr=LR, index_base=0)
    desc.step_fwd(inp.x, inp.packs[0])
    desc.step_bwd(inp.dout, x=inp.x if xb is None else xb, idx=inp.packs[0])
    torch.cuda.synchronize()
    desc.check_bounds()
    assert any((a != b).any() for a, b in zip(_snap(desc), want[0][0]))  # (not Descent's fused step in disguise)


# ---- 2. both halves of the step and of the seed reach the backward's counter and key
@pytest.mark.parametrize("D", [128, 16], ids=["two-waves", "one-wave"])
def test_step_and_seed_above_32_bits(pkg, gpu, D):
    inp = _Inputs(pkg, gpu, D, 4, 1024, seed=8)
    want = _reference(pkg, gpu, inp, [0, 1, 2], key=(D, "big"), seed=BIG_SEED, first_step=BIG_STEP)
    hp = inp.engine(pkg, gpu, seed=BIG_SEED, first_step=BIG_STEP, stochastic_step=True)
    for k in range(3):
        hp.step(inp.x, inp.packs[k], inp.dout)
        _assert_step(hp, want[k], f"step {k}:")
        assert hp.indexer.state() & pkg._lib.IX_SINGLES_STOCHASTIC
    assert hp.opt.step_of(hp.ts) == BIG_STEP + 3 and (BIG_STEP + 3) >> 32 == (BIG_STEP >> 32) + 1
    # ... and each half matters: the low halves alone give other tables
    low = _reference(pkg, gpu, inp, [0], key=(D, "low"), seed=BIG_SEED & _M32, first_step=BIG_STEP & _M32)
    assert any((a != b).any() for a, b in zip(low[0][0], want[0][0]))


# ---- 3. pipelines
@pytest.mark.parametrize("D", [128, 16])
@pytest.mark.parametrize("parts", [16, 32])
@pytest.mark.parametrize("B", [1024, 2048])
def test_pipeline_apply_equals_plain_step(pkg, gpu, B, parts, D):
    """Four steps over two alternating batches through prime + step_prep == step, bit for bit, == the references."""
    inp = _Inputs(pkg, gpu, D, 4, B, nbatches=2, seed=1)
    seq = [0, 1, 0, 1]
    want = _reference(pkg, gpu, inp, seq, key=(D, 4, B, "alt"))
    plain = inp.engine(pkg, gpu, stochastic_step=True, parts=parts)
    hp = inp.engine(pkg, gpu, stochastic_step=True, pipeline="apply", parts=parts)
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
    assert hp._ixs[hp._cur].state() & pkg._lib.IX_PREPARED  # (the last apply launch built the next batch)
    assert plain.opt.step_of(plain.ts) == 4 and hp.opt.step_of(hp.ts) == 4


@pytest.mark.parametrize("B", [2112, 2110], ids=["scan-build", "rounds-build"])
def test_pipeline_apply_above_2048_positions(pkg, gpu, B):
    """The apply launch that carries a build of more than 2048 positions per table: the scan build (int32
    indices, B % 4 == 0) and the build in rounds (any B)."""
    inp = _Inputs(pkg, gpu, 128, 4, B, nbatches=2, seed=7)
    seq = [0, 1, 0]
    want = _reference(pkg, gpu, inp, seq, key=(128, 4, B, "apply-big"))
    hp = inp.engine(pkg, gpu, stochastic_step=True, pipeline="apply")
    assert hp.pipeline == "apply"
    hp.prime(inp.packs[1], inp.x, inp.dout, prev=inp.packs[0])
    _assert_step(hp, want[0], "step 0:")
    assert hp._ixs[hp._cur].state() & pkg._lib.IX_PREPARED
    for k in (1, 2):
        hp.step_prep(inp.x, inp.packs[seq[k]], inp.dout, inp.packs[1 - seq[k]])
        _assert_step(hp, want[k], f"step {k}:")
    assert hp.opt.step_of(hp.ts) == 3


def test_pipeline_side_large_batch(pkg, gpu):
    inp = _Inputs(pkg, gpu, 128, 4, 2112, nbatches=2, seed=2)
    want = _reference(pkg, gpu, inp, [0, 1, 0], key=(128, 4, 2112, "side"))
    hp = inp.engine(pkg, gpu, stochastic_step=True, pipeline="side")
    assert hp.pipeline == "side"
    for k, b in enumerate([0, 1, 0]):
        hp.step_next(inp.x, inp.packs[b], inp.dout, inp.packs[1 - b])
        _assert_step(hp, want[k], f"step {k}:")
    assert hp.opt.step_of(hp.ts) == 3


# ---- 4. flags
def test_bwd_only_then_apply_only_and_prebuilt_update(pkg, gpu):
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, 128, 4, 1024)
    want = _reference(pkg, gpu, inp, [0, 1, 2], key=(128, 4, 1024, False, "plain"))
    two = inp.engine(pkg, gpu, stochastic_step=True)
    upd = inp.engine(pkg, gpu, stochastic_step=True)
    for k in range(2):
        for hp in (two, upd):
            hp.step_fwd(inp.x, inp.packs[k])
            hp.step_bwd(inp.dout, flags=_lib.STEP_BWD_ONLY)
            assert hp.indexer.state() & _lib.IX_SINGLES_STOCHASTIC
            assert hp.opt.step_of(hp.ts) == k  # (the backward alone does not advance the word)
        two.step_bwd(inp.dout, flags=_lib.STEP_APPLY_ONLY)
        upd.opt_update(inp.packs[k], True)  # dlrm_sr_sgd_update(PREBUILT): the repeated rows only
        _assert_step(two, want[k], f"step {k}, BWD_ONLY + APPLY_ONLY:")
        _assert_step(upd, want[k], f"step {k}, BWD_ONLY + dlrm_sr_sgd_update(PREBUILT):")
        assert two.opt.step_of(two.ts) == k + 1 and upd.opt.step_of(upd.ts) == k + 1


# ---- 5. the state machine
def test_cross_rule_combinations_are_refused_and_write_nothing(pkg, gpu):
    """Every pairing of dlrm_sr_step_bwd with another rule's backward, apply or update, in both directions,
    another stochastic handle and a second backward: DLRM_E_STATE, no table bit and no step word changed.
    (20 tables: every rule, the row-wise one included, has a backward form.)"""
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, 128, 20, 1024, nbatches=1)
    p, x, dout, B, D = inp.packs[0], inp.x, inp.dout, inp.B, inp.D
    hp = inp.engine(pkg, gpu, stochastic_step=True)
    ts = hp.ts
    lib, h = hp.ctx.lib, hp.ctx.bind()
    vp = ctypes.c_void_p
    step = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, vp(x.data_ptr()), x.stride(0), vp(dout.data_ptr()),
            dout.stride(0), hp.padding, vp(hp.dx.data_ptr()), hp.dx.stride(0), vp(hp.dt.data_ptr()), hp.dt.stride(0), LR)
    upd = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, vp(hp.dt.data_ptr()), _lib.F32, hp.dt.stride(0), D, LR)
    sr = hp.opt.handle_of(ts)
    other_opt = pkg.StochasticDescent(LR, seed=SEED)  # (its own handle for the same tables: the same seed, another word)
    osr = other_opt.handle_of(ts)
    assert osr.value != sr.value
    split, ada, roww = pkg.SplitDescent(LR), pkg.ADAGrad(LR), pkg.RowwiseADAGrad(LR)
    sh, ah, rh = split.handle_of(ts), ada.handle_of(ts), roww.handle_of(ts)
    ixh = hp.indexer.handle
    hp.opt.seek(ts, 7)
    other_opt.seek(ts, 11)

    def unchanged(before):
        torch.cuda.synchronize()
        for a, b in zip(before, _snap(hp)):
            assert np.array_equal(a, b)
        assert hp.opt.step_of(ts) == 7 and other_opt.step_of(ts) == 11

    # after a stochastic backward
    hp.step_fwd(x, p)
    hp.step_bwd(dout, flags=_lib.STEP_BWD_ONLY)
    torch.cuda.synchronize()
    both = _lib.IX_SINGLES_DONE | _lib.IX_SINGLES_STOCHASTIC
    assert hp.indexer.state() & (both | _lib.IX_SINGLES_SPLIT | _lib.IX_SINGLES_ADAGRAD | _lib.IX_SINGLES_ROWWISE) == both
    before = _snap(hp)
    AO = _lib.STEP_APPLY_ONLY
    assert lib.dlrm_step_bwd(h, ts.handle, ixh, *step, AO) == _lib.E_STATE
    assert lib.dlrm_split_step_bwd(h, ts.handle, sh, ixh, *step, AO) == _lib.E_STATE
    assert lib.dlrm_adagrad_step_bwd(h, ts.handle, ah, ixh, *step, 1e-8, AO) == _lib.E_STATE
    assert lib.dlrm_adagrad_step_bwd(h, ts.handle, rh, ixh, *step, 1e-8, AO) == _lib.E_STATE
    assert lib.dlrm_sgd_update(h, ts.handle, ixh, _lib.UPDATE_PREBUILT, *upd) == _lib.E_STATE
    assert lib.dlrm_split_sgd_update(h, ts.handle, sh, ixh, _lib.UPDATE_PREBUILT, *upd) == _lib.E_STATE
    assert lib.dlrm_adagrad_update(h, ts.handle, ah, ixh, _lib.UPDATE_PREBUILT, *upd, 1e-8) == _lib.E_STATE
    assert lib.dlrm_adagrad_update(h, ts.handle, rh, ixh, _lib.UPDATE_PREBUILT, *upd, 1e-8) == _lib.E_STATE
    assert lib.dlrm_sr_step_bwd(h, ts.handle, osr, ixh, *step, AO) == _lib.E_STATE  # another stochastic handle
    assert lib.dlrm_sr_sgd_update(h, ts.handle, osr, ixh, _lib.UPDATE_PREBUILT, *upd) == _lib.E_STATE
    assert lib.dlrm_sr_step_bwd(h, ts.handle, sr, ixh, *step, 0) == _lib.E_STATE  # a second backward on one build
    assert lib.dlrm_sr_step_bwd(h, ts.handle, sr, ixh, *step, _lib.STEP_BWD_ONLY) == _lib.E_STATE
    assert lib.dlrm_sr_step_bwd(h, ts.handle, osr, ixh, *step, 0) == _lib.E_STATE
    unchanged(before)
    hp.step_bwd(dout, flags=AO)  # the same handle's apply completes it
    torch.cuda.synchronize()
    assert hp.opt.step_of(ts) == 8
    hp.opt.seek(ts, 7)

    # the other direction: after each other rule's backward, neither stochastic call completes it
    backs = [("dlrm_step_bwd", lambda f: lib.dlrm_step_bwd(h, ts.handle, ixh, *step, f), 0),
             ("dlrm_split_step_bwd", lambda f: lib.dlrm_split_step_bwd(h, ts.handle, sh, ixh, *step, f), _lib.IX_SINGLES_SPLIT),
             ("dlrm_adagrad_step_bwd", lambda f: lib.dlrm_adagrad_step_bwd(h, ts.handle, ah, ixh, *step, 1e-8, f),
              _lib.IX_SINGLES_ADAGRAD),
             ("dlrm_adagrad_step_bwd (row-wise)", lambda f: lib.dlrm_adagrad_step_bwd(h, ts.handle, rh, ixh, *step, 1e-8, f),
              _lib.IX_SINGLES_ROWWISE)]
    for name, call, bit in backs:
        hp.step_fwd(x, p)
        assert call(_lib.STEP_BWD_ONLY) == 0, name
        torch.cuda.synchronize()
        st = hp.indexer.state()
        assert st & _lib.IX_SINGLES_DONE and not st & _lib.IX_SINGLES_STOCHASTIC and st & bit == bit, name
        before = _snap(hp)
        assert lib.dlrm_sr_step_bwd(h, ts.handle, sr, ixh, *step, AO) == _lib.E_STATE, name
        assert lib.dlrm_sr_sgd_update(h, ts.handle, sr, ixh, _lib.UPDATE_PREBUILT, *upd) == _lib.E_STATE, name
        assert lib.dlrm_sr_step_bwd(h, ts.handle, sr, ixh, *step, 0) == _lib.E_STATE, name  # (a second backward)
        unchanged(before)
        assert call(AO) == 0, name  # its own apply completes it

    # argument errors: fp32 tables, a handle made for another dim
    hp.step_fwd(x, p)
    before = _snap(hp)
    f32 = pkg.EmbeddingTableSet([t.float().to(gpu) for t in inp.w])
    assert lib.dlrm_sr_step_bwd(h, f32.handle, sr, ixh, *step, 0) == _lib.E_ARG
    other = pkg.EmbeddingTableSet([torch.zeros((n, 16), dtype=torch.bfloat16, device=gpu) for n in inp.rows])
    assert lib.dlrm_sr_step_bwd(h, other.handle, sr, ixh, *step, 0) == _lib.E_ARG
    assert lib.dlrm_sr_step_bwd(h, ts.handle, sr, ixh, *step, _lib.STEP_BWD_ONLY | AO) == _lib.E_ARG
    unchanged(before)
    hp.check_bounds()


# ---- 6. bounds
def test_bad_index_in_the_current_batch_writes_nothing_and_the_step_advances(pkg, gpu):
    inp = _Inputs(pkg, gpu, 128, 4, 1024, seed=3)
    bad_np = inp.idx[0].copy()
    bad_np[3, 517] = inp.rows[3] + 2
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    hp = inp.engine(pkg, gpu, stochastic_step=True)
    before = _snap(hp)
    hp.step(inp.x, bad, inp.dout)
    with pytest.raises(pkg.BoundsError):
        hp.check_bounds()
    for a, b in zip(before, _snap(hp)):
        assert np.array_equal(a, b)
    assert hp.opt.step_of(hp.ts) == 1  # (the call returned DLRM_OK and launched)


def test_bad_index_in_the_next_batch_only(pkg, gpu):
    """For both pipelines: the current step's rows are written and nothing is raised yet; the step on the bad
    batch raises and writes nothing."""
    inp = _Inputs(pkg, gpu, 128, 4, 1024, seed=4)
    want = _reference(pkg, gpu, inp, [0], key=(128, 4, 1024, "seed4"))
    bad_np = inp.idx[1].copy()
    bad_np[3, 99] = inp.rows[3] + 1
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    for mode in ("apply", "side"):
        hp = inp.engine(pkg, gpu, stochastic_step=True, pipeline=mode)
        if mode == "apply":
            hp.prime(bad, inp.x, inp.dout, prev=inp.packs[0])
        else:
            hp.step_next(inp.x, inp.packs[0], inp.dout, bad)
        _assert_step(hp, want[0], f"{mode}:")  # (checks bounds: clean)
        before = _snap(hp)
        if mode == "apply":
            hp.step_prep(inp.x, bad, inp.dout, inp.packs[0])
        else:
            hp.step_next(inp.x, bad, inp.dout, inp.packs[0])
        with pytest.raises(pkg.BoundsError):
            hp.check_bounds()
        for a, b in zip(before, _snap(hp)):
            assert np.array_equal(a, b)
        assert hp.opt.step_of(hp.ts) == 2


# ---- 7. NaN / Inf
def test_once_hit_nan_and_inf_gradients_follow_the_exponent_all_ones_rule(pkg, gpu):
    """Once-hit rows whose gradient is +Inf (W' = -Inf: stored as -Inf exactly, whatever R) and NaN (stored as a
    NaN with its quiet bit set): sr_bf16's rule for an all-ones exponent, in the backward's write as in the apply's."""
    D, B = 16, 64
    rows = [4, 1000]
    w = [torch.ones((n, D), dtype=torch.bfloat16) for n in rows]
    idx = np.stack([np.arange(B) % 4, 100 + np.arange(B)])  # table 1: every row hit once
    p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu))
    got = []
    for kw in ({"stochastic_step": True}, {}):
        ts = pkg.EmbeddingTableSet([t.clone().to(gpu) for t in w])
        hp = pkg.HotPath(ts, B, 1, index_base=0, opt=pkg.StochasticDescent(LR, seed=SEED), **kw)
        x = torch.ones((B, D), dtype=torch.bfloat16, device=gpu)
        dout = torch.ones((B, hp.width), dtype=torch.bfloat16, device=gpu)
        dout[5] = float("inf")
        dout[6] = float("nan")
        hp.step(x, p, dout)
        torch.cuda.synchronize()
        hp.check_bounds()
        assert bool(hp.indexer.state() & pkg._lib.IX_SINGLES_STOCHASTIC) == bool(kw)
        got.append(_bits(ts[1].data))
    fused, oper = got
    assert np.array_equal(fused, oper)
    assert (fused[105] == 0xFF80).all()                      # 1 - lr * Inf
    assert ((fused[106] & 0x7FC0) == 0x7FC0).all()           # NaN, quiet bit set
    finite = np.ones(1000, dtype=bool)
    finite[[105, 106]] = False
    finite[:100] = finite[164:] = False
    assert ((fused[finite] & 0x7F80) != 0x7F80).all() and (fused[:100] == 0x3F80).all()


# ---- 8. graph capture
def test_pipelined_step_graph_replay_equals_eager(pkg, gpu):
    """A captured pipelined chain of two steps replayed twice == the same four steps run eagerly from the same
    starting step, and the word advanced by steps x replays."""
    S0 = 1000
    inp = _Inputs(pkg, gpu, 128, 4, 1024, nbatches=1, seed=5)
    p = inp.packs[0]
    hg = inp.engine(pkg, gpu, stochastic_step=True, pipeline="apply")
    he = inp.engine(pkg, gpu, stochastic_step=True, pipeline="apply")
    hg.prime(p, inp.x, inp.dout, prev=p)  # eager warm-up: one step, and indexer 0 holds p, prepared
    inp.reset(hg, S0)                     # the tables and the step back to the start
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
    torch.cuda.synchronize()
    hg.check_bounds()
    for a, b in zip(_snap(hg), _snap(he)):
        assert np.array_equal(a, b)
    assert np.array_equal(_bits(hg.dx), _bits(he.dx))
    assert hg.opt.step_of(hg.ts) == S0 + 4 and he.opt.step_of(he.ts) == S0 + 4
    assert any((a != _bits(w)).any() for a, w in zip(_snap(hg), inp.w))  # (the steps did run)


# ---- 9. HipTables
@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
def test_hiptables_chain_equals_operator_sequence(pkg, gpu, defer):
    inp = _Inputs(pkg, gpu, 16, 4, 1024, nbatches=2, seed=6)
    want = _reference(pkg, gpu, inp, [0, 1], key=(16, 4, 1024, "seed6"))
    opt = pkg.StochasticDescent(LR, seed=SEED)
    ht = pkg.HipTables([t.clone().to(gpu) for t in inp.w], opt=opt, index_base=0, defer_update=defer,
                       stochastic_step=True)
    D = inp.D
    for k, p in enumerate(inp.packs):
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
        assert isinstance(ys, pkg.LazyLookup)
        out, back = pkg.rrule(pkg.DotInteraction(), inp.x, ys)
        _, dx, dy = back(inp.dout)
        assert dy.applied and dy.hp.indexer.state() & pkg._lib.IX_SINGLES_STOCHASTIC
        assert np.array_equal(_bits(out), want[k][1]) and np.array_equal(_bits(dx), want[k][2])
        with pytest.raises(ValueError):
            pkg.update_(pkg.StochasticDescent(LR, seed=SEED), ht, pkg.maplookup_pullback(D, ht, p, dy))  # another object
        with pytest.raises(ValueError):
            pkg.update_(pkg.Descent(LR), ht, pkg.maplookup_pullback(D, ht, p, dy))
        pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
        assert (ht._pending is not None) == defer
    ts = ht.ts  # (runs a deferred apply, checks bounds)
    torch.cuda.synchronize()
    for t in range(inp.T):
        assert np.array_equal(_bits(ts[t].data), want[1][0][t])
    assert opt.step_of(ts) == 2


def test_stochastic_step_keyword_errors(pkg, gpu):
    bf = [torch.zeros((8, 16), dtype=torch.bfloat16, device=gpu) for _ in range(2)]
    f32 = [torch.zeros((8, 16), dtype=torch.float32, device=gpu) for _ in range(2)]
    sd = pkg.StochasticDescent
    for opt in (pkg.ADAGrad(), pkg.RowwiseADAGrad(), pkg.SplitDescent(), None):  # any other optimizer
        with pytest.raises(ValueError):
            pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=opt, stochastic_step=True)
        with pytest.raises(ValueError):
            pkg.HipTables(bf, opt=opt, index_base=0, stochastic_step=True)
    with pytest.raises(ValueError, match="bfloat16"):  # fp32 tables
        pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=sd(), stochastic_step=True)
    with pytest.raises(ValueError, match="bfloat16"):
        pkg.HipTables(f32, opt=sd(), index_base=0, stochastic_step=True)
    for kw in ({"materialize_ys": True}, {"lookups": 2}):  # the step kernels are unavailable
        with pytest.raises(ValueError):
            pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, kw.pop("lookups", 1), index_base=0, opt=sd(),
                        stochastic_step=True, **kw)
    for kw in ({"fused_step": True}, {"adagrad_step": True}):  # the other rules' keywords stay refused
        with pytest.raises(ValueError, match="fused step"):
            pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=sd(), stochastic_step=True, **kw)
    hp = pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=sd())  # the default route stays
    assert not hp.step_api and not hp.stochastic_step and hp.pipeline is None
    for mode in ("apply", "side"):
        assert pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=sd(), stochastic_step=True,
                           pipeline=mode).pipeline == mode
    with pytest.raises(ValueError):  # lr beside the optimizer, as for the other rules
        pkg.HipTables(bf, opt=sd(0.1), lr=0.2, index_base=0, stochastic_step=True)
