"""The fused training step with sparse Adagrad: dlrm_adagrad_step_bwd / dlrm_adagrad_step_bwd_prepare through
HotPath(opt=ADAGrad | RowwiseADAGrad, adagrad_step=True) and HipTables(opt=...).

Two references.  Bit equality of tables, state, dx and out with HotPath(opt=rule)'s operator route (the fused
forward, dlrm_interact_bwd_gather, dlrm_adagrad_update(PREBUILT)) over the same batches; and, so that the kernels
are not only compared with each other, the once-hit rows of a step against the rule computed in float64 from
the start values and the row's single dt row (one term: the gradient sum is exact), held to the bounds derived in
tests/test_adagrad.py's docstring (u = 2^-24):
  element-wise: |A - A_ref| <= 2^-22 A_ref,  |w - w_ref| <= 2^-20 |D_ref| + 2^-23 max(|w_ref|, |w_before|)
  row-wise:     |m - m_ref| <= (D + 2) u m_ref,  |w - w_ref| <= (D/2 + 16) u |D_ref| + 2^-23 max(|w_ref|, |w_before|)
  bf16 tables:  the weight bounds plus 2^-8 |w_ref|.

Shapes: rows cycled from [2, 8, 40, 5000, 3, 100000] with one-hot lookups give multi- and one-slice hot segments,
chunks longer than the inline positions and several hundred once-hit rows per batch.  Weights and state start
from seeded random values; the row-wise state starts positive, not zero, so a wrong m shows.

Not every shape steps its once-hit rows inside the backward (F > 32, unaligned x, D off the
forms or off the vector apply's ladder, and the forms that would run below Descent's occupancy -- the row-wise
rule with up to 16 features, the element-wise one-wave form on fp32 tables with up to 16 features).  Those take
the gather backward and the rule's apply with once-hit items, and must give the same bits; `fused_shape` says
which is which and the indexer's state bits are held to it.  The "apply" pipeline, flag, bounds, graph and
HipTables tests use 20 tables so that both rules run their fused forms there; the "side" pipeline runs the
issue's (128, 4, 2112), where the row-wise rule falls back, and the same with 20 tables.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rand_indices, rand_tables

pytestmark = pytest.mark.gpu

ROWS = [2, 8, 40, 5000, 3, 100000]
LR, EPS = 0.05, 1e-8
U = 2.0 ** -24
RULES = [False, True]
RULE_IDS = ["elementwise", "rowwise"]


def _rows(T):
    return [ROWS[t % len(ROWS)] for t in range(T)]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype in (torch.bfloat16, torch.int16) else t.view(torch.int32).numpy()


def _f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


class _Inputs:
    """Seeded start weights and state, index batches, x and dout of one shape."""

    def __init__(self, pkg, gpu, D, T, B, dtype=torch.float32, nbatches=3, seed=0):
        rng = np.random.default_rng(1000 * D + 10 * T + seed)
        self.rows, self.D, self.T, self.B, self.dtype = _rows(T), D, T, B, dtype
        self.w = [torch.from_numpy(t).to(dtype) for t in rand_tables(rng, self.rows, D)]
        # element-wise: eps + a positive random accumulator per element; row-wise: a positive word per row
        self.A = [torch.from_numpy((EPS + rng.uniform(0.0, 0.5, size=(n, D))).astype(np.float32)) for n in self.rows]
        self.m = [torch.from_numpy(rng.uniform(0.01, 0.5, size=(n,)).astype(np.float32)) for n in self.rows]
        self.idx = [rand_indices(rng, self.rows, B, 1) for _ in range(nbatches)]
        self.packs = [pkg.PackedIndices(torch.from_numpy(i).to(torch.int32).to(gpu)) for i in self.idx]
        self.x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(dtype)
        F = T + 1
        self.dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(dtype)

    def start_state(self, rowwise):
        return self.m if rowwise else self.A

    def tables(self, pkg, gpu, rowwise):
        """(table set, optimizer) at the start values"""
        ts = pkg.EmbeddingTableSet([t.to(gpu) for t in self.w])
        opt = (pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad)(LR, EPS)
        for s, s0 in zip(opt.state_of(ts), self.start_state(rowwise)):
            s.copy_(s0)
        return ts, opt

    def engine(self, pkg, gpu, rowwise, **kw):
        ts, opt = self.tables(pkg, gpu, rowwise)
        return pkg.HotPath(ts, self.B, 1, index_base=0, opt=opt, **kw)

    def fused_shape(self, rowwise, xview=False):
        """Whether the shape's step backward steps the once-hit rows with the rule (include/dlrm_hip.h)."""
        D, nb = self.D, (self.T + 1 + 15) // 16
        ok = self.T <= 31 and not xview and (D == 128 or D <= 64)
        if rowwise:  # the vector apply's ladder; the forms of up to 16 features run below Descent's occupancy
            return ok and D >= 8 and D & (D - 1) == 0 and nb == 2
        return ok and not (nb == 1 and D <= 64 and self.dtype == torch.float32)  # (that form: the same)


def _snap(hp):
    return [_bits(t.data) for t in hp.ts], [_bits(s) for s in hp.opt.state_of(hp.ts)]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a[0] + a[1], b[0] + b[1]))


_REF = {}


def _reference(pkg, gpu, inp, rowwise, seq, xb=None, key=None, mutate=None):
    """The operator route over the batches `seq`.  Returns per step (table bits, state bits, out bits, dx bits) and
    step 0's full dt on the host (the float64 check's shapes).  xb: the backward's view of x; mutate(engine): presets before the steps."""
    if key is not None and (key, rowwise) in _REF:
        return _REF[(key, rowwise)]
    hop = inp.engine(pkg, gpu, rowwise)
    assert not hop.step_api
    if mutate is not None:
        mutate(hop)
    steps, dt0 = [], None
    for n, k in enumerate(seq):
        p = inp.packs[k]
        hop.lookup_interact_fwd(inp.x, p)
        hop.interact_bwd(inp.dout, x=inp.x if xb is None else xb, idx=p, build_indexer=True)
        hop.opt_update(p, True)
        torch.cuda.synchronize()
        hop.check_bounds()
        if n == 0 and key is not None and key[1] == "plain" and tuple(key[0][:4]) in F64_SHAPES:
            dt0 = hop.dt.cpu().numpy().copy()  # (kept for the float64 check of these shapes only)
        w, s = _snap(hop)
        steps.append((w, s, _bits(hop.out), _bits(hop.dx)))
    if key is not None:
        _REF[(key, rowwise)] = (steps, dt0)
    return steps, dt0


def _assert_step(hp, want, what, out=True):
    w, s, o, dx = want
    torch.cuda.synchronize()
    hp.check_bounds()
    gw, gs = _snap(hp)
    for t in range(len(gw)):
        assert np.array_equal(gw[t], w[t]), f"{what} table {t}: {(gw[t] != w[t]).sum()} of {gw[t].size} elements != " \
                                            "operator route"
        assert np.array_equal(gs[t], s[t]), f"{what} state {t}: {(gs[t] != s[t]).sum()} of {gs[t].size} words != " \
                                            "operator route"
    assert np.array_equal(_bits(hp.dx), dx), f"{what}: dx"
    if out:
        assert np.array_equal(_bits(hp.out), o), f"{what}: out"


def _assert_untouched(inp, k, before, after, what):
    (w0, s0), (w1, s1) = before, after
    for t, n in enumerate(inp.rows):
        un = np.ones(n, dtype=bool)
        un[inp.idx[k][t]] = False
        assert np.array_equal(w1[t][un], w0[t][un]) and np.array_equal(s1[t][un], s0[t][un]), \
            f"{what} table {t}: an untouched row changed"


# ---- 1. every kernel form: three plain fused steps against the operator route, both rules
F32, BF16 = torch.float32, torch.bfloat16
F64_SHAPES = [(128, 20, 1024, F32), (128, 4, 1024, BF16), (128, 20, 2112, BF16), (16, 4, 1024, F32)]  # (section 2)
SHAPES = [  # (D, T, B, dtype, backward's x is an unaligned view)
    (128, 4, 1024, F32, False), (128, 4, 1024, BF16, False),    # NB = 1, two waves per sample
    (128, 20, 1024, F32, False), (128, 20, 1024, BF16, False),  # NB = 2, two waves per sample
    (128, 4, 1023, F32, False), (128, 4, 1023, BF16, False),    # a padding sample in the last block ...
    (128, 20, 1023, F32, False), (128, 20, 1023, BF16, False),  # ... which must still reach the row-wise barrier
    (128, 4, 2112, F32, False),    # B > 2048, two waves per sample
    (128, 20, 2112, BF16, False),  # ... and 8 columns per lane
    (16, 4, 1024, F32, False), (16, 20, 1024, F32, False), (64, 4, 1024, F32, False), (64, 20, 1024, F32, False),
    (8, 4, 1024, F32, False), (256, 4, 1024, F32, False),  # the smallest ladder size; interact_bwd_update_kernel's form
    (48, 4, 1024, F32, False),   # D off the vector ladder: the row-wise rule falls back
    (16, 33, 1024, F32, False),  # F > 32: the gather backward + the rule's apply with once-hit items
    (128, 4, 1024, F32, True),   # x_ld not 16-B aligned in the backward: the same fallback
]


def _shape_id(s):
    d, t, b, dt, v = s
    return f"d{d}-t{t}-b{b}-{'bf16' if dt == BF16 else 'f32'}{'-xview' if v else ''}"


@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=[_shape_id(s) for s in SHAPES])
def test_fused_adagrad_step_equals_operator_route(pkg, gpu, shape, rowwise):
    D, T, B, dtype, xview = shape
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, D, T, B, dtype)
    xb = None
    if xview:
        buf = torch.zeros((B, D + 1), dtype=dtype, device=gpu)
        xb = buf[:, :D]
        xb.copy_(inp.x)
        assert (xb.stride(0) * xb.element_size()) % 16 != 0
    want, _ = _reference(pkg, gpu, inp, rowwise, [0, 1, 2], xb, key=(shape, "plain"))
    hp = inp.engine(pkg, gpu, rowwise, adagrad_step=True)
    assert hp.step_api and hp.adagrad_step
    fused = inp.fused_shape(rowwise, xview)
    mine, other = ((_lib.IX_SINGLES_ROWWISE, _lib.IX_SINGLES_ADAGRAD) if rowwise else
                   (_lib.IX_SINGLES_ADAGRAD, _lib.IX_SINGLES_ROWWISE))
    for k in range(3):
        before = _snap(hp)
        hp.step_fwd(inp.x, inp.packs[k])
        hp.step_bwd(inp.dout, x=inp.x if xb is None else xb, idx=inp.packs[k])
        _assert_step(hp, want[k], f"step {k}:")
        _assert_untouched(inp, k, before, _snap(hp), f"step {k}:")
        st = hp.indexer.state()
        assert bool(st & _lib.IX_SINGLES_DONE) == fused and bool(st & mine) == fused
        assert not st & other and not st & _lib.IX_SINGLES_SPLIT
    _, c = np.unique(inp.idx[2][3], return_counts=True)
    assert (c == 1).sum() > 100  # (once-hit rows of the 5000-row table)


# ---- 2. once-hit rows against the rule in float64


@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("shape", F64_SHAPES, ids=[_shape_id(s + (False,)) for s in F64_SHAPES])
def test_once_hit_rows_against_float64_rule(pkg, gpu, shape, rowwise):
    D, T, B, dtype = shape
    inp = _Inputs(pkg, gpu, D, T, B, dtype)
    _, dt0 = _reference(pkg, gpu, inp, rowwise, [0, 1, 2], key=(shape + (False,), "plain"))
    hp = inp.engine(pkg, gpu, rowwise, adagrad_step=True)
    hp.step(inp.x, inp.packs[0], inp.dout)
    torch.cuda.synchronize()
    hp.check_bounds()
    assert bool(hp.indexer.state() & pkg._lib.IX_SINGLES_DONE) == inp.fused_shape(rowwise)
    lr, eps = float(np.float32(LR)), float(np.float32(EPS))
    checked = 0
    for t, n in enumerate(inp.rows):
        rows, first, cnt = np.unique(inp.idx[0][t], return_index=True, return_counts=True)
        r, b = rows[cnt == 1], first[cnt == 1]  # once-hit rows and their samples
        if len(r) == 0:
            continue
        G = dt0[b, (t + 1) * D:(t + 2) * D].astype(np.float64)  # the row's single dt row
        w0 = _f64(inp.w[t])[r]
        w1 = _f64(hp.ts[t].data)[r]
        s1 = _f64(hp.opt.state_of(hp.ts)[t])[r]
        if rowwise:
            m_ref = _f64(inp.m[t])[r] + (G * G).mean(axis=1)
            w_ref = w0 - lr * G / (np.sqrt(m_ref) + eps)[:, None]
            s_ref, s_tol, step_rel = m_ref, (D + 2) * U * m_ref, (D / 2 + 16) * U
        else:
            s_ref = _f64(inp.A[t])[r] + G * G
            w_ref = w0 - lr * G / (np.sqrt(s_ref) + eps)
            s_tol, step_rel = 2.0 ** -22 * s_ref, 2.0 ** -20
        w_tol = step_rel * np.abs(w_ref - w0) + 2.0 ** -23 * np.maximum(np.abs(w_ref), np.abs(w0))
        if dtype == BF16:
            w_tol = w_tol + 2.0 ** -8 * np.abs(w_ref)
        werr, serr = np.abs(w1 - w_ref), np.abs(s1 - s_ref)
        print(f"table {t}: {len(r)} once-hit rows, worst weight error/bound "
              f"{np.max(werr / np.maximum(w_tol, 1e-300)):.3f}, state {np.max(serr / np.maximum(s_tol, 1e-300)):.3f}")
        assert (werr <= w_tol).all(), f"table {t} weights: worst error/bound {np.max(werr / np.maximum(w_tol, 1e-300)):.3f}"
        assert (serr <= s_tol).all(), f"table {t} state: worst error/bound {np.max(serr / np.maximum(s_tol, 1e-300)):.3f}"
        assert (np.abs(w1 - w0) > 0).any()  # (the rows were stepped)
        checked += len(r)
    assert checked > 100


# ---- 3. pipelines
@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("D", [128, 16])
@pytest.mark.parametrize("parts", [16, 32])
@pytest.mark.parametrize("B", [1024, 2048])
def test_pipeline_apply_equals_plain_step(pkg, gpu, B, parts, D, rowwise):
    """Four steps over two alternating batches through prime + step_prep == step == the operator route."""
    inp = _Inputs(pkg, gpu, D, 20, B, nbatches=2, seed=1)
    assert inp.fused_shape(rowwise)
    seq = [0, 1, 0, 1]
    want, _ = _reference(pkg, gpu, inp, rowwise, seq, key=(D, 20, B, "alt"))
    plain = inp.engine(pkg, gpu, rowwise, adagrad_step=True, parts=parts)
    hp = inp.engine(pkg, gpu, rowwise, adagrad_step=True, pipeline="apply", parts=parts)
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


@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
def test_pipeline_apply_above_2048_positions(pkg, gpu, rowwise):
    """B = 2112 with pipeline="apply" equals the plain step, whichever of the build-carrying launches or the
    plain-step fallback runs."""
    inp = _Inputs(pkg, gpu, 128, 20, 2112, nbatches=2, seed=7)
    seq = [0, 1, 0]
    want, _ = _reference(pkg, gpu, inp, rowwise, seq, key=(128, 20, 2112, "apply-big"))
    hp = inp.engine(pkg, gpu, rowwise, adagrad_step=True, pipeline="apply")
    assert hp.pipeline == "apply"
    hp.prime(inp.packs[1], inp.x, inp.dout, prev=inp.packs[0])
    _assert_step(hp, want[0], "step 0:")
    for k in (1, 2):
        hp.step_prep(inp.x, inp.packs[seq[k]], inp.dout, inp.packs[1 - seq[k]])
        _assert_step(hp, want[k], f"step {k}:")


@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("T", [4, 20])
def test_pipeline_side_large_batch(pkg, gpu, T, rowwise):
    """(128, 4, 2112), and the same with 20 tables, where the row-wise rule has its fused backward too."""
    inp = _Inputs(pkg, gpu, 128, T, 2112, nbatches=2, seed=2)
    assert inp.fused_shape(rowwise) == (T == 20 or not rowwise)
    want, _ = _reference(pkg, gpu, inp, rowwise, [0, 1, 0], key=(128, T, 2112, "side"))
    hp = inp.engine(pkg, gpu, rowwise, adagrad_step=True, pipeline="side")
    assert hp.pipeline == "side"
    for k, b in enumerate([0, 1, 0]):
        hp.step_next(inp.x, inp.packs[b], inp.dout, inp.packs[1 - b])
        _assert_step(hp, want[k], f"step {k}:")
        assert bool(hp._ixs[1 - hp._cur].state() & pkg._lib.IX_SINGLES_DONE) == inp.fused_shape(rowwise)


# ---- 4. flags
@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
def test_bwd_only_then_apply_only_and_prebuilt_update(pkg, gpu, rowwise):
    _lib = pkg._lib
    shape = (128, 20, 1024, F32, False)
    inp = _Inputs(pkg, gpu, 128, 20, 1024)
    want, _ = _reference(pkg, gpu, inp, rowwise, [0, 1, 2], key=(shape, "plain"))
    two = inp.engine(pkg, gpu, rowwise, adagrad_step=True)
    upd = inp.engine(pkg, gpu, rowwise, adagrad_step=True)
    for hp in (two, upd):
        hp.step_fwd(inp.x, inp.packs[0])
        hp.step_bwd(inp.dout, flags=_lib.STEP_BWD_ONLY)
        assert inp.fused_shape(rowwise)
        assert hp.indexer.state() & (_lib.IX_SINGLES_ROWWISE if rowwise else _lib.IX_SINGLES_ADAGRAD)
    two.step_bwd(inp.dout, flags=_lib.STEP_APPLY_ONLY)
    upd.opt_update(inp.packs[0], True)  # dlrm_adagrad_update(PREBUILT), the same kind of handle: the repeated rows only
    _assert_step(two, want[0], "BWD_ONLY + APPLY_ONLY:")
    _assert_step(upd, want[0], "BWD_ONLY + dlrm_adagrad_update(PREBUILT):")


# ---- 5. the state machine
def test_cross_rule_combinations_are_refused_and_write_nothing(pkg, gpu):
    """After the backward of each of the four rules every other rule's completion is DLRM_E_STATE and writes
    nothing; a second backward on the build too; dlrm_indexer_state names the rule."""
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, 128, 20, 1024, BF16)
    assert inp.fused_shape(True) and inp.fused_shape(False)
    p, x, dout, B, D = inp.packs[0], inp.x, inp.dout, inp.B, inp.D
    ts = pkg.EmbeddingTableSet([t.to(gpu) for t in inp.w])
    split, ada, row = pkg.SplitDescent(LR), pkg.ADAGrad(LR, EPS), pkg.RowwiseADAGrad(LR, EPS)
    for s, s0 in zip(ada.state_of(ts), inp.A):
        s.copy_(s0)
    for s, s0 in zip(row.state_of(ts), inp.m):
        s.copy_(s0)
    hp = pkg.HotPath(ts, B, 1, index_base=0)  # (Descent: the forward and the buffers)
    lib, h = hp.ctx.lib, hp.ctx.bind()
    vp = ctypes.c_void_p
    step = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, vp(x.data_ptr()), x.stride(0), vp(dout.data_ptr()),
            dout.stride(0), hp.padding, vp(hp.dx.data_ptr()), hp.dx.stride(0), vp(hp.dt.data_ptr()), hp.dt.stride(0), LR)
    upd = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, vp(hp.dt.data_ptr()), _lib.F32, hp.dt.stride(0), D, LR)
    sh, ah, rh = split.handle_of(ts), ada.handle_of(ts), row.handle_of(ts)
    ixh = hp.indexer.handle
    # rule -> (its step entry point with a flags argument, its PREBUILT update, its state bit)
    rules = {
        "descent": (lambda f: lib.dlrm_step_bwd(h, ts.handle, ixh, *step, f),
                    lambda: lib.dlrm_sgd_update(h, ts.handle, ixh, _lib.UPDATE_PREBUILT, *upd), 0),
        "split": (lambda f: lib.dlrm_split_step_bwd(h, ts.handle, sh, ixh, *step, f),
                  lambda: lib.dlrm_split_sgd_update(h, ts.handle, sh, ixh, _lib.UPDATE_PREBUILT, *upd),
                  _lib.IX_SINGLES_SPLIT),
        "elementwise": (lambda f: lib.dlrm_adagrad_step_bwd(h, ts.handle, ah, ixh, *step, EPS, f),
                        lambda: lib.dlrm_adagrad_update(h, ts.handle, ah, ixh, _lib.UPDATE_PREBUILT, *upd, EPS),
                        _lib.IX_SINGLES_ADAGRAD),
        "rowwise": (lambda f: lib.dlrm_adagrad_step_bwd(h, ts.handle, rh, ixh, *step, EPS, f),
                    lambda: lib.dlrm_adagrad_update(h, ts.handle, rh, ixh, _lib.UPDATE_PREBUILT, *upd, EPS),
                    _lib.IX_SINGLES_ROWWISE),
    }
    rule_bits = _lib.IX_SINGLES_SPLIT | _lib.IX_SINGLES_ADAGRAD | _lib.IX_SINGLES_ROWWISE

    def snap():
        torch.cuda.synchronize()
        return ([_bits(t.data) for t in ts] + [_bits(s) for s in split.state_of(ts)] +
                [_bits(s) for s in ada.state_of(ts)] + [_bits(s) for s in row.state_of(ts)])

    for name, (step_fn, _, bit) in rules.items():
        hp.step_fwd(x, p)
        assert step_fn(_lib.STEP_BWD_ONLY) == 0, name
        st = hp.indexer.state()
        assert st & _lib.IX_SINGLES_DONE and st & rule_bits == bit, (name, st)
        before = snap()
        for other, (ostep, oupd, _) in rules.items():
            if other == name:
                continue
            assert ostep(_lib.STEP_APPLY_ONLY) == _lib.E_STATE, (name, other)
            assert oupd() == _lib.E_STATE, (name, other)
        assert step_fn(0) == _lib.E_STATE and step_fn(_lib.STEP_BWD_ONLY) == _lib.E_STATE  # a second backward
        for a, b in zip(before, snap()):
            assert np.array_equal(a, b), f"after {name}'s backward a refused call wrote"
        assert step_fn(_lib.STEP_APPLY_ONLY) == 0, name  # its own apply completes it
        assert any(not np.array_equal(a, b) for a, b in zip(before, snap()))
    # argument errors: an optimizer made for another dim
    other = pkg.EmbeddingTableSet([torch.zeros((n, 16), dtype=BF16, device=gpu) for n in inp.rows])
    assert lib.dlrm_adagrad_step_bwd(h, other.handle, ah, ixh, *step, EPS, 0) == _lib.E_ARG
    hp.check_bounds()


# ---- 6. bounds
@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
def test_bad_index_in_the_current_batch_writes_nothing(pkg, gpu, rowwise):
    inp = _Inputs(pkg, gpu, 128, 20, 1024, seed=3)
    bad_np = inp.idx[0].copy()
    bad_np[3, 517] = inp.rows[3] + 2
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    hp = inp.engine(pkg, gpu, rowwise, adagrad_step=True)
    before = _snap(hp)
    hp.step(inp.x, bad, inp.dout)
    with pytest.raises(pkg.BoundsError):
        hp.check_bounds()
    assert _same(before, _snap(hp))


@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
def test_bad_index_in_the_next_batch_only(pkg, gpu, rowwise):
    """Both pipelines: the current step's rows and state are written and nothing is raised yet; the step on the bad
    batch raises and writes nothing."""
    inp = _Inputs(pkg, gpu, 128, 20, 1024, seed=4)
    want, _ = _reference(pkg, gpu, inp, rowwise, [0], key=(128, 20, 1024, "seed4"))
    bad_np = inp.idx[1].copy()
    bad_np[3, 99] = inp.rows[3] + 1
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    for mode in ("apply", "side"):
        hp = inp.engine(pkg, gpu, rowwise, adagrad_step=True, pipeline=mode)
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
        assert _same(before, _snap(hp))


# ---- 7. a zero gradient
def test_zero_gradient_with_zero_rowwise_state(pkg, gpu):
    """Samples whose dout rows are zero have G = 0; with m = 0 for their rows the row-wise step is
    w' = fmaf(-lr / (sqrt(0) + eps), 0, w) = w and m' = 0: the operator route's bits, no NaN."""
    inp = _Inputs(pkg, gpu, 128, 20, 1024, seed=8)
    nz = 256
    inp.dout[:nz] = 0
    hit = [np.unique(inp.idx[0][t][:nz]) for t in range(inp.T)]

    def zero_state(hp):
        for s, r in zip(hp.opt.state_of(hp.ts), hit):
            s[torch.from_numpy(r).to(gpu)] = 0

    want, _ = _reference(pkg, gpu, inp, True, [0], mutate=zero_state)
    hp = inp.engine(pkg, gpu, True, adagrad_step=True)
    zero_state(hp)
    once = 0
    for t in range(inp.T):
        rows, first, cnt = np.unique(inp.idx[0][t], return_index=True, return_counts=True)
        once += ((cnt == 1) & (first < nz)).sum()
    assert once > 20  # (once-hit rows with a zero gradient, stepped inside the backward)
    hp.step(inp.x, inp.packs[0], inp.dout)
    _assert_step(hp, want[0], "zero gradient:")
    assert hp.indexer.state() & pkg._lib.IX_SINGLES_ROWWISE
    for t, s in zip(hp.ts, hp.opt.state_of(hp.ts)):
        assert not torch.isnan(t.data).any() and not torch.isnan(s).any()


# ---- 8. graph capture
@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
def test_pipelined_adagrad_step_graph_replay_equals_eager(pkg, gpu, rowwise):
    inp = _Inputs(pkg, gpu, 128, 20, 1024, nbatches=1, seed=5)
    p = inp.packs[0]
    hg = inp.engine(pkg, gpu, rowwise, adagrad_step=True, pipeline="apply")
    he = inp.engine(pkg, gpu, rowwise, adagrad_step=True, pipeline="apply")

    def restart(hp):  # the tables and the state back to the start
        for t, w in zip(hp.ts, inp.w):
            t.data.copy_(w)
        for s, s0 in zip(hp.opt.state_of(hp.ts), inp.start_state(rowwise)):
            s.copy_(s0)

    hg.prime(p, inp.x, inp.dout, prev=p)  # eager warm-up: one step, and indexer 0 holds p, prepared
    restart(hg)
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
    restart(he)
    for _ in range(2):
        gr.replay()
        he.step_prep(inp.x, p, inp.dout, p)
        he.step_prep(inp.x, p, inp.dout, p)
    torch.cuda.synchronize()
    hg.check_bounds()
    assert _same(_snap(hg), _snap(he))
    assert np.array_equal(_bits(hg.dx), _bits(he.dx))
    assert any((a != _bits(s0)).any() for a, s0 in zip(_snap(hg)[1], inp.start_state(rowwise)))  # (the steps did run)


# ---- 9. HipTables
@pytest.mark.parametrize("rowwise", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
def test_hiptables_chain_equals_operator_sequence(pkg, gpu, defer, rowwise):
    inp = _Inputs(pkg, gpu, 16, 20, 1024, nbatches=2, seed=6)
    want, _ = _reference(pkg, gpu, inp, rowwise, [0, 1], key=(16, 20, 1024, "seed6"))
    rule = pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad
    opt = rule(LR, EPS)
    ht = pkg.HipTables([t.to(gpu) for t in inp.w], opt=opt, index_base=0, defer_update=defer)
    for s, s0 in zip(opt.state_of(ht._ts), inp.start_state(rowwise)):
        s.copy_(s0)
    D = inp.D
    for k, p in enumerate(inp.packs):
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
        assert isinstance(ys, pkg.LazyLookup)
        out, back = pkg.rrule(pkg.DotInteraction(), inp.x, ys)
        _, dx, dy = back(inp.dout)
        assert dy.applied
        assert np.array_equal(_bits(out), want[k][2]) and np.array_equal(_bits(dx), want[k][3])
        with pytest.raises(ValueError):
            pkg.update_(rule(LR, EPS), ht, pkg.maplookup_pullback(D, ht, p, dy))  # another optimizer object
        with pytest.raises(ValueError):
            pkg.update_(pkg.Descent(LR), ht, pkg.maplookup_pullback(D, ht, p, dy))
        for eta, eps in ((2 * LR, EPS), (LR, 2 * EPS)):  # the same object with another eta / eps
            opt.eta, opt.eps = eta, eps
            with pytest.raises(ValueError):
                pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
        opt.eta, opt.eps = LR, EPS
        pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
        assert (ht._pending is not None) == defer
    ts = ht.ts  # (runs a deferred apply, checks bounds)
    torch.cuda.synchronize()
    w, s = want[1][:2]
    for t in range(inp.T):
        assert np.array_equal(_bits(ts[t].data), w[t]) and np.array_equal(_bits(opt.state_of(ts)[t]), s[t])


# ---- 10. keyword errors
def test_adagrad_step_keyword_errors(pkg, gpu):
    bf = [torch.zeros((8, 16), dtype=BF16, device=gpu) for _ in range(2)]
    f32 = [torch.zeros((8, 16), dtype=F32, device=gpu) for _ in range(2)]
    with pytest.raises(ValueError):
        pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=pkg.SplitDescent(), adagrad_step=True)
    with pytest.raises(ValueError):
        pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, adagrad_step=True)
    for rule in (pkg.ADAGrad, pkg.RowwiseADAGrad):
        with pytest.raises(ValueError):  # materialized ys
            pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=rule(), adagrad_step=True, materialize_ys=True)
        with pytest.raises(ValueError):  # pooled lookups
            pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 4, index_base=0, opt=rule(), adagrad_step=True)
        with pytest.raises(ValueError):  # a side-stream indexer
            pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=rule(), adagrad_step=True,
                        overlap_indexer=True)
        with pytest.raises(ValueError):  # the split rule's keyword stays the split rule's
            pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=rule(), fused_step=True)
        with pytest.raises(ValueError):  # a pipeline without the keyword
            pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=rule(), pipeline="apply")
        hp = pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=rule())  # the default route stays
        assert not hp.step_api and not hp.adagrad_step
        for mode in (None, "apply", "side"):
            hp = pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=rule(), adagrad_step=True, pipeline=mode)
            assert hp.step_api and hp.adagrad_step and hp.pipeline == mode
