"""Sparse Adagrad (element-wise and row-wise) embedding update on the GPU: dlrm_adagrad_update
through update_, HotPath(opt=...) and HipTables.

Shapes: rows = [2, 8, 40, 5000] with B = 1024 one-hot lookups gives every item kind of the apply --
two-slice hot segments (~512 hits per row), one-slice hot segments (~128), chunks longer than the
inline positions (~25) and once-hit singles.  Gradients are k/64 with integer |k| <= 512, so every
row sum G is exact in fp32 whatever the summation order: the checks test the rule, not the sum.

Bounds (derived, not measured; u = 2^-24):
  element-wise, fp32: |w - w_ref| <= 2^-20 |D_ref| + 2^-23 max(|w_ref|, |w_before|),
                      |A - A_ref| <= 2^-22 A_ref
      (the step is at most six fp32 operations, with a sqrt and a division that need not be
      correctly rounded; D_ref = w_ref - w_before)
  row-wise, fp32:     |m - m_ref| <= (D + 2) u m_ref   (any order of D non-negative terms)
                      |w - w_ref| <= (D/2 + 16) u |D_ref| + 2^-23 max(|w_ref|, |w_before|)
  bf16 tables:        the weight bounds plus 2^-8 |w_ref| (one bf16 rounding); state bounds as is.
Each step is checked on its own: the reference of the second step starts from the first step's
GPU result (weights and state), so the one-step bounds hold for it too.

bf16 gradients are k/64 with |k| <= 256 (exact in bf16's 8 significant bits), so G stays exact and
the same bounds apply unchanged.  A displaced gradient (grad_offset = 13 in a buffer whose base is
one element past a 16-B boundary: the scalar apply kernels) lives in a guard band of NaNs, which
must neither be read nor written.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import banded, rand_indices, rand_tables

pytestmark = pytest.mark.gpu

ROWS = [2, 8, 40, 5000]
B0 = 1024
LR, EPS = 0.05, 1e-8
U = 2.0 ** -24


def _tables(rng, rows, D, gpu, dtype=torch.float32):
    tabs = [torch.from_numpy(t).to(dtype) for t in rand_tables(rng, rows, D)]
    return [t.to(gpu) for t in tabs]


def _exact_grad(rng, B, width, kmax=512):
    return (rng.integers(-kmax, kmax + 1, size=(B, width)) / 64.0).astype(np.float32)


def _dense_G(idx_t, grad_t, nrows, L):
    """[nrows][D] float64 row sums of one table (exact: multiples of 1/64 below 2^24/64)."""
    G = np.zeros((nrows, grad_t.shape[1]))
    np.add.at(G, idx_t, np.repeat(grad_t.astype(np.float64), L, axis=0))
    return G


def _f32(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy()


DISPLACED_OFFSET = 13


def _update(pkg, opt, ts, idx_np, grad_np, gpu, B, L, indexer=None, prebuilt=False, grad_dtype=torch.float32,
            displaced=False):
    p = pkg.PackedIndices(torch.from_numpy(idx_np).to(torch.int32).to(gpu).reshape(len(idx_np), B, L))
    g = torch.from_numpy(grad_np).to(gpu).to(grad_dtype)
    assert np.array_equal(_f32(g), grad_np)  # (exact in grad_dtype)
    off, band = 0, None
    if displaced:  # columns [0, 13) and everything around the rows: NaN
        off = DISPLACED_OFFSET
        band = banded((B, off + g.shape[1]), grad_dtype, off + g.shape[1], 1, gpu)
        band.view[:, off:].copy_(g)
        band.snapshot()
        g = band.view
    if indexer is not None and prebuilt:
        assert indexer.prepare(ts, p, index_base=0)
    pkg.update_(opt, ts, pkg.maplookup_pullback(off, ts, p, g), indexer, index_base=0, prebuilt=prebuilt)
    if band is not None:
        band.check(0, what="grad")
    return p


def _check_step(rowwise, D, before_w, before_s, after_w, after_s, G, touched, bf16):
    """One table, one step: float64 / torch reference from the `before` values, the bounds of the
    module docstring on touched rows, bit equality on untouched rows."""
    w0 = before_w.astype(np.float64)
    lr, eps = float(np.float32(LR)), float(np.float32(EPS))
    if rowwise:
        m_ref = before_s.astype(np.float64) + (G * G).mean(axis=1)
        w_ref = w0 - lr * G / (np.sqrt(m_ref) + eps)[:, None]
        s_ref, s_tol = m_ref, (D + 2) * U * m_ref
        step_rel = (D / 2 + 16) * U
    else:
        w = torch.from_numpy(before_w.copy()).requires_grad_(True)
        o = torch.optim.Adagrad([w], lr=LR, eps=EPS, initial_accumulator_value=EPS)
        o.state[w]["sum"].copy_(torch.from_numpy(before_s))
        w.grad = torch.from_numpy(G.astype(np.float32))
        o.step()
        w_ref = w.detach().numpy().astype(np.float64)
        s_ref = o.state[w]["sum"].numpy().astype(np.float64)
        s_tol = 2.0 ** -22 * s_ref
        step_rel = 2.0 ** -20
    w_tol = step_rel * np.abs(w_ref - w0) + 2.0 ** -23 * np.maximum(np.abs(w_ref), np.abs(w0))
    if bf16:
        w_tol = w_tol + 2.0 ** -8 * np.abs(w_ref)
    t = touched
    werr = np.abs(after_w.astype(np.float64) - w_ref)
    serr = np.abs(after_s.astype(np.float64) - s_ref)
    assert (werr[t] <= w_tol[t]).all(), f"weights: worst error/bound {np.max(werr[t] / np.maximum(w_tol[t], 1e-300)):.3f}"
    assert (serr[t] <= s_tol[t]).all(), f"state: worst error/bound {np.max(serr[t] / np.maximum(s_tol[t], 1e-300)):.3f}"
    assert t.any()


def _run_and_check(pkg, gpu, rowwise, D, dtype=torch.float32, rows=ROWS, B=B0, L=1, steps=2, seed=0, prepare=False,
                   grad_dtype=torch.float32, displaced=False):
    rng = np.random.default_rng(1000 * D + seed + (7 if rowwise else 0))
    T = len(rows)
    ts = pkg.EmbeddingTableSet(_tables(rng, rows, D, gpu, dtype))
    opt = (pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad)(LR, EPS)
    state = opt.state_of(ts)
    ix = pkg.SparseIndexer(T, B * L, gpu) if prepare else None
    for _ in range(steps):
        idx = rand_indices(rng, rows, B, L)
        grad = _exact_grad(rng, B, T * D, 256 if grad_dtype == torch.bfloat16 else 512)
        w0 = [t.data.clone() for t in ts]
        s0 = [s.clone() for s in state]
        _update(pkg, opt, ts, idx, grad, gpu, B, L, ix, prebuilt=prepare, grad_dtype=grad_dtype, displaced=displaced)
        for t in range(T):
            G = _dense_G(idx[t], grad[:, t * D:(t + 1) * D], rows[t], L)
            touched = np.zeros(rows[t], dtype=bool)
            touched[idx[t]] = True
            _check_step(rowwise, D, _f32(w0[t]), _f32(s0[t]), _f32(ts[t].data), _f32(state[t]), G, touched,
                        dtype == torch.bfloat16)
            un = ~touched
            assert np.array_equal(_bits(ts[t].data)[un], _bits(w0[t])[un]), f"table {t}: an untouched row changed"
            assert np.array_equal(_bits(state[t])[un], _bits(s0[t])[un]), f"table {t}: untouched state changed"


@pytest.mark.parametrize("D", [16, 128, 512, 12])
def test_elementwise_against_torch_adagrad(pkg, gpu, D):
    """ADAGrad == torch.optim.Adagrad(lr, eps, initial_accumulator_value=eps) on dense fp32 copies
    (D = 512: two vectors per lane, several storing waves; D = 12: the any-D fallback kernels)."""
    _run_and_check(pkg, gpu, False, D)


@pytest.mark.parametrize("D", [16, 128, 512, 12])
def test_rowwise_against_float64_formula(pkg, gpu, D):
    _run_and_check(pkg, gpu, True, D)


@pytest.mark.parametrize("rowwise", [False, True])
def test_bf16_tables_fp32_gradients(pkg, gpu, rowwise):
    _run_and_check(pkg, gpu, rowwise, 128, dtype=torch.bfloat16)


@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["tf32", "tbf16"])
@pytest.mark.parametrize("rowwise", [False, True])
def test_bf16_gradients(pkg, gpu, rowwise, dtype, D):
    """grad_dtype = bf16 into fp32 and bf16 tables: the GT = bf16 instantiations of the vector apply
    (chunks, hot slices) for both rules."""
    _run_and_check(pkg, gpu, rowwise, D, dtype=dtype, seed=4, grad_dtype=torch.bfloat16)


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["gf32", "gbf16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["tf32", "tbf16"])
@pytest.mark.parametrize("prepare", [False, True], ids=["built", "prepared"])
@pytest.mark.parametrize("rowwise", [False, True])
def test_displaced_unaligned_gradient(pkg, gpu, rowwise, prepare, dtype, grad_dtype):
    """grad_offset = 13 from a base one element past a 16-B boundary: the scalar apply kernels
    (chunks, hot; with a prepared build also the once-hit singles), which must read nothing before
    grad_offset or outside the rows."""
    _run_and_check(pkg, gpu, rowwise, 16, dtype=dtype, seed=5, prepare=prepare, grad_dtype=grad_dtype, displaced=True)


@pytest.mark.parametrize("rowwise", [False, True])
@pytest.mark.parametrize("form", ["pooled", "big", "prepared"])
def test_other_indexer_forms(pkg, gpu, form, rowwise):
    """Pooled bags (L = 4); 8192 positions per table (above the in-LDS builds); and the wave build
    of SparseIndexer.prepare + prebuilt=True (the apply's item-map path)."""
    if form == "pooled":
        _run_and_check(pkg, gpu, rowwise, 32, B=512, L=4, steps=1, seed=1)
    elif form == "big":
        _run_and_check(pkg, gpu, rowwise, 64, B=2048, L=4, steps=1, seed=2)
    else:
        _run_and_check(pkg, gpu, rowwise, 64, steps=2, seed=3, prepare=True)


@pytest.mark.parametrize("rowwise", [False, True])
def test_bitwise_reproducible(pkg, gpu, rowwise):
    rows, B, D = [3, 10, 100000], 4096, 128
    rng = np.random.default_rng(5)
    tabs = rand_tables(rng, rows, D)
    idx = rand_indices(rng, rows, B, 1)
    grad = rng.standard_normal((B, len(rows) * D)).astype(np.float32)
    got = []
    for _ in range(2):
        ts = pkg.EmbeddingTableSet([torch.from_numpy(t).to(gpu) for t in tabs])
        opt = (pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad)(LR, EPS)
        _update(pkg, opt, ts, idx, grad, gpu, B, 1)
        got.append([_bits(t.data) for t in ts] + [_bits(s) for s in opt.state_of(ts)])
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert not np.array_equal(got[0][2], _bits(torch.from_numpy(tabs[2])))  # (the update did run)


@pytest.mark.parametrize("rowwise", [False, True])
def test_bounds_error_writes_nothing(pkg, gpu, rowwise):
    rng = np.random.default_rng(6)
    rows, B, D = ROWS, 256, 16
    ts = pkg.EmbeddingTableSet(_tables(rng, rows, D, gpu))
    opt = (pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad)(LR, EPS)
    state = opt.state_of(ts)
    w0 = [_bits(t.data) for t in ts]
    s0 = [_bits(s) for s in state]
    idx = rand_indices(rng, rows, B, 1)
    grad = _exact_grad(rng, B, len(rows) * D)
    bad = idx.copy()
    bad[3, B // 2] = rows[3] + 3
    with pytest.raises(pkg.BoundsError):
        _update(pkg, opt, ts, bad, grad, gpu, B, 1)
    for t in range(len(rows)):
        assert np.array_equal(_bits(ts[t].data), w0[t]) and np.array_equal(_bits(state[t]), s0[t])
    _update(pkg, opt, ts, idx, grad, gpu, B, 1)  # the flag is clear again: this one applies
    for t in range(len(rows)):
        touched = np.zeros(rows[t], dtype=bool)
        touched[idx[t]] = True
        changed = (_bits(state[t]).reshape(rows[t], -1) != s0[t].reshape(rows[t], -1)).any(axis=1)
        G = _dense_G(idx[t], grad[:, t * D:(t + 1) * D], rows[t], 1)
        assert np.array_equal(changed, touched & (G != 0).any(axis=1))


def test_state_and_flag_errors(pkg, gpu):
    _lib = pkg._lib
    rows, D, B = [3, 40, 100000, 7], 128, 512
    rng = np.random.default_rng(7)
    ts = pkg.EmbeddingTableSet(_tables(rng, rows, D, gpu))
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
    hp = pkg.HotPath(ts, B, 1, lr=0.5, index_base=0)
    assert hp.step_api
    x = torch.randn((B, D), device=gpu)
    dout = torch.randn((B, hp.width), device=gpu)
    hp.step_fwd(x, p)
    hp.step_bwd(dout, flags=_lib.STEP_BWD_ONLY)
    assert hp.indexer.state() & _lib.IX_SINGLES_DONE
    opt = pkg.ADAGrad()
    w0 = [_bits(t.data) for t in ts]
    args = (ctypes.c_void_p(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, ctypes.c_void_p(hp.dt.data_ptr()), _lib.F32,
            hp.dt.stride(0), D, 0.1, 1e-8)
    lib, h = ts.ctx.lib, ts.ctx.bind()
    # a split backward stepped the once-hit rows with Descent and left their dt rows unwritten
    assert lib.dlrm_adagrad_update(h, ts.handle, opt.handle_of(ts), hp.indexer.handle, _lib.UPDATE_PREBUILT,
                                   *args) == _lib.E_STATE
    assert lib.dlrm_adagrad_update(h, ts.handle, opt.handle_of(ts), hp.indexer.handle, _lib.UPDATE_ATOMIC,
                                   *args) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    for t in range(len(rows)):
        assert np.array_equal(_bits(ts[t].data), w0[t])
    g = torch.zeros((B, len(rows) * D), device=gpu)
    with pytest.raises(ValueError):
        pkg.update_(pkg.ADAGrad(), ts, pkg.maplookup_pullback(0, ts, p, g), index_base=0, deterministic=False)
    with pytest.raises(ValueError):
        pkg.HotPath(ts, B, 1, index_base=0, opt=pkg.ADAGrad(), pipeline="apply")
    hp.check_bounds()


def _engine_inputs(pkg, gpu):
    rows, D, B = [3, 100, 20000], 16, 300
    rng = np.random.default_rng(8)
    tabs = rand_tables(rng, rows, D)
    packs = [pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
             for _ in range(2)]
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu)
    F = len(rows) + 1
    dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu)
    return rows, D, B, tabs, packs, x, dout


def _operator_steps(pkg, gpu, opt, tabs, D, packs, x, dout):
    ts = pkg.EmbeddingTableSet([torch.from_numpy(t).to(gpu) for t in tabs])
    for p in packs:
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ts, p, index_base=0)
        _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
        _, dx, dy = back(dout)
        pkg.update_(opt, ts, pkg.maplookup_pullback(D, ts, p, dy), index_base=0)
    return ts, dx


def _same(pkg, ts_a, opt_a, ts_b, opt_b):
    for a, b in zip(ts_a, ts_b):
        assert np.array_equal(_bits(a.data), _bits(b.data))
    for a, b in zip(opt_a.state_of(ts_a), opt_b.state_of(ts_b)):
        assert np.array_equal(_bits(a), _bits(b))


def test_hotpath_equals_operator_sequence_and_graph(pkg, gpu):
    rows, D, B, tabs, packs, x, dout = _engine_inputs(pkg, gpu)
    ref_opt = pkg.RowwiseADAGrad(LR, EPS)
    ref_ts, ref_dx = _operator_steps(pkg, gpu, ref_opt, tabs, D, packs, x, dout)
    assert (_f32(ref_opt.state_of(ref_ts)[2]) != 0).any()
    # eager engine steps
    opt = pkg.RowwiseADAGrad(LR, EPS)
    hp = pkg.HotPath(pkg.EmbeddingTableSet([torch.from_numpy(t).to(gpu) for t in tabs]), B, 1, index_base=0, opt=opt)
    assert not hp.step_api and hp.pipeline is None
    for p in packs:
        hp.step(x, p, dout)
    torch.cuda.synchronize()
    hp.check_bounds()
    _same(pkg, hp.ts, opt, ref_ts, ref_opt)
    assert np.array_equal(_bits(hp.dx), _bits(ref_dx))
    # the same step, captured after one eager warm-up step and replayed twice == two eager steps
    opt_g = pkg.RowwiseADAGrad(LR, EPS)
    hg = pkg.HotPath(pkg.EmbeddingTableSet([torch.from_numpy(t).to(gpu) for t in tabs]), B, 1, index_base=0, opt=opt_g)
    opt_e = pkg.RowwiseADAGrad(LR, EPS)
    he = pkg.HotPath(pkg.EmbeddingTableSet([torch.from_numpy(t).to(gpu) for t in tabs]), B, 1, index_base=0, opt=opt_e)
    hg.step(x, packs[0], dout)  # warm-up
    for t, w in zip(hg.ts, tabs):  # back to the start
        t.data.copy_(torch.from_numpy(w))
    for s in opt_g.state_of(hg.ts):
        s.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            hg.step(x, packs[0], dout)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        gr.replay()
        he.step(x, packs[0], dout)
    torch.cuda.synchronize()
    hg.check_bounds()
    _same(pkg, hg.ts, opt_g, he.ts, opt_e)
    assert np.array_equal(_bits(hg.dx), _bits(he.dx))


def test_hiptables_chain_equals_plain_update(pkg, gpu):
    rows, D, B, tabs, packs, x, dout = _engine_inputs(pkg, gpu)
    ref_opt = pkg.ADAGrad(LR, EPS)
    ref_ts, ref_dx = _operator_steps(pkg, gpu, ref_opt, tabs, D, packs, x, dout)
    opt = pkg.ADAGrad(LR, EPS)
    ht = pkg.HipTables([torch.from_numpy(t).to(gpu) for t in tabs], lr=None, index_base=0)
    for p in packs:
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
        assert isinstance(ys, pkg.LazyLookup)
        _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
        _, dx, dy = back(dout)
        assert not dy.applied
        pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
    torch.cuda.synchronize()
    _same(pkg, ht.ts, opt, ref_ts, ref_opt)
    assert np.array_equal(_bits(dx), _bits(ref_dx))
    # with the once-hit rows already stepped by the pullback, an Adagrad update! is refused
    ht2 = pkg.HipTables([torch.from_numpy(t).to(gpu) for t in tabs], lr=0.1, index_base=0)
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht2, packs[0])
    _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
    _, _, dy = back(dout)
    if dy.applied:
        with pytest.raises(ValueError, match="once-hit"):
            pkg.update_(pkg.ADAGrad(), ht2, pkg.maplookup_pullback(D, ht2, packs[0], dy))
