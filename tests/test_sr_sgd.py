"""StochasticDescent on the GPU: dlrm_sr_sgd_update through update_, HotPath(opt=...) and HipTables(opt=...).

The reference of every arithmetic check is never the kernel under test: dlrm_sgd_update (Descent) runs on fp32
tables that hold the bf16 weights' values, with the same indexer form, indices and gradient, which yields W' of
every element (an untouched element's W' is its bf16 value, which the store keeps); the numpy sr_round with the
step the call used then gives the bits the bf16 tables must hold, over all rows, after every step.  The fp32
tables are reloaded from the bf16 result between steps.

Shapes (as test_split_sgd.py): rows = [2, 8, 40, 5000] with B = 1024 one-hot lookups gives two-slice and one-slice
hot segments, chunks longer than the inline positions and once-hit singles in one launch; one pooled case
(L = 4, B = 256).  D = 128 and 16 take the vector kernels, D = 12 and 4 the any-D ones.

Where both table dtypes take the vector kernels with the same lane geometry the summation order is the same and
normally distributed gradients are used.  Where the paths may differ (D = 4: the fp32 table takes the vector
kernels, the bf16 table the any-D ones; D = 12; a displaced gradient; other indexer forms) the gradients are k/64
with integer |k| <= 512 (<= 256 as bf16), so every row sum is exact in fp32 whatever the order.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import banded, rand_indices, rand_tables

pytestmark = pytest.mark.gpu

ROWS = [2, 8, 40, 5000]
B0 = 1024
LR = 0.05
SEED = 12345
DISPLACED_OFFSET = 13


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16)


def _nearest(w):
    """round-to-nearest bf16 bits of an fp32 numpy array"""
    return _bits(torch.from_numpy(w).to(torch.bfloat16))


def _exact_grad(rng, B, width, kmax=512):
    return (rng.integers(-kmax, kmax + 1, size=(B, width)) / 64.0).astype(np.float32)


def _tables(pkg, gpu, rng, rows, D):
    """bf16 tables of random weights"""
    return pkg.EmbeddingTableSet([torch.from_numpy(t).to(torch.bfloat16).to(gpu) for t in rand_tables(rng, rows, D)])


def _f32_copy(pkg, ts):
    return pkg.EmbeddingTableSet([t.data.float() for t in ts])


def _grad_arg(g, gpu, displaced):
    """(gradient matrix, column offset, guard band) -- displaced: columns from 13 inside a NaN band whose
    base is one element past a 16-B boundary."""
    if not displaced:
        return g, 0, None
    off = DISPLACED_OFFSET
    band = banded((g.shape[0], off + g.shape[1]), g.dtype, off + g.shape[1], 1, gpu)
    band.view[:, off:].copy_(g)
    band.snapshot()
    return band.view, off, band


def _indexer(pkg, ts, p, form):
    """form: None = update_ builds its own; "build" = dlrm_indexer_build + PREBUILT; "prepare" = the wave build
    (a split indexer, taken whole: its once-hit rows are singles items) + PREBUILT; "prepare16" = the same with the
    other chunk limit and parts per table."""
    if form is None:
        return None
    ix = pkg.SparseIndexer(len(ts), p.B * p.L, ts.device)
    if form == "build":
        ix.build(ts, p, index_base=0)
    else:
        if form == "prepare16":
            ix.set_chunk(16).set_parts(32)
        assert ix.prepare(ts, p, index_base=0)
        assert ix.state() & pkg._lib.IX_SPLIT and not ix.state() & pkg._lib.IX_SINGLES_DONE
    return ix


def _apply(pkg, opt, ts, p, g, off, form=None, check_bounds=None):
    ix = _indexer(pkg, ts, p, form)
    pkg.update_(opt, ts, pkg.maplookup_pullback(off, ts, p, g), ix, index_base=0, prebuilt=form is not None,
                check_bounds=check_bounds)


def _want(pkg, ref, seed, step):
    """the bits the stochastic rule stores for the fp32 results in `ref`"""
    return [pkg.sr_round(r.data.cpu().numpy(), seed, step, t) for t, r in enumerate(ref)]


def _run(pkg, gpu, D, *, rows=ROWS, B=B0, L=1, steps=2, seed=0, exact=False, grad_dtype=torch.float32, form=None,
         displaced=False, first_step=0):
    rng = np.random.default_rng(100 * D + seed)
    T = len(rows)
    ts = _tables(pkg, gpu, rng, rows, D)
    ref = _f32_copy(pkg, ts)
    opt = pkg.StochasticDescent(LR, seed=SEED + seed)
    if first_step:
        opt.seek(ts, first_step)
    assert opt.state_of(ts) == []
    rounded_differently = 0
    for k in range(steps):
        idx = rand_indices(rng, rows, B, L)
        if exact:
            grad = _exact_grad(rng, B, T * D, 256 if grad_dtype == torch.bfloat16 else 512)
        else:
            grad = rng.standard_normal((B, T * D)).astype(np.float32)
        p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu).reshape(T, B, L))
        g = torch.from_numpy(grad).to(gpu).to(grad_dtype)
        if exact:
            assert np.array_equal(g.float().cpu().numpy(), grad)  # (exact in grad_dtype)
        ga, off, band = _grad_arg(g, gpu, displaced)
        w0 = [_bits(t.data) for t in ts]
        assert opt.step_of(ts) == first_step + k
        _apply(pkg, pkg.Descent(LR), ref, p, ga, off, form)
        _apply(pkg, opt, ts, p, ga, off, form)
        if band is not None:
            band.check(0, what="grad")
        want = _want(pkg, ref, SEED + seed, first_step + k)
        for t in range(T):
            got = _bits(ts[t].data)
            assert np.array_equal(got, want[t]), f"step {k} table {t}: {(got != want[t]).sum()} of {got.size} elements differ"
            un = np.ones(rows[t], dtype=bool)
            un[idx[t]] = False
            assert np.array_equal(got[un], w0[t][un]), f"table {t}: an untouched row changed"
            assert (got[~un] != w0[t][~un]).any(), f"table {t}: no touched row changed"
            rounded_differently += int((want[t] != _nearest(ref[t].data.cpu().numpy())).sum())
            ref[t].data.copy_(ts[t].data.float())  # the next step starts from the bf16 result
    assert rounded_differently > 0  # (the reference is not round-to-nearest in disguise)
    assert opt.step_of(ts) == first_step + steps
    return ts


# ---- 1. bit equality with the restated store, the same vector path for both table dtypes
@pytest.mark.parametrize("D", [16, 128])
def test_bit_equal_fp32_gradients(pkg, gpu, D):
    _run(pkg, gpu, D, steps=3)


@pytest.mark.parametrize("D", [16, 128])
def test_bit_equal_bf16_gradients(pkg, gpu, D):
    _run(pkg, gpu, D, seed=1, grad_dtype=torch.bfloat16)


# ---- 2. across kernel paths (exact gradients)
@pytest.mark.parametrize("D", [4, 12])
def test_any_dim_kernels(pkg, gpu, D):
    _run(pkg, gpu, D, seed=2, exact=True)


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["gf32", "gbf16"])
@pytest.mark.parametrize("form", [None, "prepare"], ids=["built", "prepared"])
def test_displaced_gradient_in_a_guard_band(pkg, gpu, form, grad_dtype):
    _run(pkg, gpu, 16, seed=3, exact=True, grad_dtype=grad_dtype, form=form, displaced=True)


@pytest.mark.parametrize("B", [256, 2048], ids=["l4-b256", "l4-b2048"])
def test_pooled_bags(pkg, gpu, B):
    """Pooled bags (L = 4); at B = 2048 the 8192 positions per table are above the in-LDS builds (tables in
    parts: the table index of R is the real table's)."""
    _run(pkg, gpu, 16, B=B, L=4, steps=2 if B == 256 else 1, seed=4, exact=True)


@pytest.mark.parametrize("D", [128, 12])
def test_indexer_forms_give_the_same_bits(pkg, gpu, D):
    """dlrm_indexer_build (PREBUILT), the wave build's split indexer taken whole (PREBUILT) at both chunk limits
    and update_'s own build: each equals the restated store of its own fp32 reference, and all of them are the
    same bits -- R does not depend on the indexer's form, its chunk limit or its parts."""
    got = [[_bits(t.data) for t in _run(pkg, gpu, D, seed=5, exact=True, form=form, first_step=2 ** 32 - 1)]
           for form in (None, "build", "prepare", "prepare16")]
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert np.array_equal(a, b)


# ---- 3. the step: seek, seeds
def test_seek_and_step_round_trip(pkg, gpu):
    rng = np.random.default_rng(11)
    ts = _tables(pkg, gpu, rng, [50], 16)
    opt = pkg.StochasticDescent(LR, seed=1)
    assert opt.step_of(ts) == 0
    for s in (7, 2 ** 40 + 3, 2 ** 64 - 1, 0):
        opt.seek(ts, s)
        assert opt.step_of(ts) == s
    opt.seek(ts, 2 ** 64 - 1)
    p = pkg.PackedIndices(torch.arange(50, dtype=torch.int32, device=gpu).reshape(1, 50, 1))
    g = torch.ones((50, 16), device=gpu)
    _apply(pkg, opt, ts, p, g, 0)
    assert opt.step_of(ts) == 0  # (the 64-bit word wraps)
    with pytest.raises(ValueError):
        opt.seek(ts, -1)
    other = _tables(pkg, gpu, rng, [50], 16)  # the step is per table set
    assert opt.step_of(other) == 0
    _apply(pkg, opt, ts, p, g, 0)
    assert opt.step_of(ts) == 1 and opt.step_of(other) == 0


def test_seeds(pkg, gpu):
    rng = np.random.default_rng(12)
    w = rand_tables(rng, ROWS, 16)
    idx = rand_indices(rng, ROWS, B0, 1)
    p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu).reshape(len(ROWS), B0, 1))
    g = torch.from_numpy(rng.standard_normal((B0, len(ROWS) * 16)).astype(np.float32)).to(gpu)
    got = []
    for seed in (3, 3, 2 ** 63 + 7):
        ts = pkg.EmbeddingTableSet([torch.from_numpy(t).to(torch.bfloat16).to(gpu) for t in w])
        _apply(pkg, pkg.StochasticDescent(LR, seed=seed), ts, p, g, 0)
        got.append([_bits(t.data) for t in ts])
    for a, b, c in zip(*got):
        assert np.array_equal(a, b)      # equal seeds: equal bits
        assert not np.array_equal(a, c)  # different seeds: different bits
    # ... and the same seed at another step differs too
    ts = pkg.EmbeddingTableSet([torch.from_numpy(t).to(torch.bfloat16).to(gpu) for t in w])
    opt = pkg.StochasticDescent(LR, seed=3)
    opt.seek(ts, 1)
    _apply(pkg, opt, ts, p, g, 0)
    assert not np.array_equal(_bits(ts[3].data), got[0][3])


def test_alternates_with_descent(pkg, gpu):
    """No per-row state: a Descent step between two stochastic ones leaves the rule's next step what the
    restatement says (step 1), on the tables as Descent left them."""
    rng = np.random.default_rng(13)
    ts = _tables(pkg, gpu, rng, ROWS, 16)
    opt = pkg.StochasticDescent(LR, seed=9)
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, ROWS, B0, 1)).to(torch.int32).to(gpu).reshape(len(ROWS), B0, 1))
    g = torch.from_numpy(rng.standard_normal((B0, len(ROWS) * 16)).astype(np.float32)).to(gpu)
    _apply(pkg, opt, ts, p, g, 0)
    _apply(pkg, pkg.Descent(LR), ts, p, g, 0)
    ref = _f32_copy(pkg, ts)
    _apply(pkg, pkg.Descent(LR), ref, p, g, 0)
    _apply(pkg, opt, ts, p, g, 0)
    for t, want in enumerate(_want(pkg, ref, 9, 1)):
        assert np.array_equal(_bits(ts[t].data), want)


# ---- 4. the point of the feature
def test_walk_of_small_steps(pkg, gpu):
    """64 x 128 weights 1.5, identity indices, 64 eager steps of lr * G = 2^-9 (a quarter of a bf16 ulp): bitwise
    the restatement's walk, whose mean is near 1.375; Descent on the same input stays at 1.5."""
    n, D, lr, seed = 64, 128, 2.0 ** -6, 12345
    p = pkg.PackedIndices(torch.arange(n, dtype=torch.int32, device=gpu).reshape(1, n, 1))
    g = torch.full((n, D), 2.0 ** -3, dtype=torch.float32, device=gpu)
    ts = pkg.EmbeddingTableSet([torch.full((n, D), 1.5, dtype=torch.bfloat16, device=gpu)])
    plain = pkg.EmbeddingTableSet([torch.full((n, D), 1.5, dtype=torch.bfloat16, device=gpu)])
    opt = pkg.StochasticDescent(lr, seed=seed)
    ix = pkg.SparseIndexer(1, n, gpu)
    for _ in range(64):
        pkg.update_(opt, ts, pkg.maplookup_pullback(0, ts, p, g), ix, index_base=0, check_bounds=False)
        pkg.update_(pkg.Descent(lr), plain, pkg.maplookup_pullback(0, plain, p, g), ix, index_base=0, check_bounds=False)
    ts.ctx.check_bounds()
    w = np.full((n, D), 1.5, dtype=np.float32)
    for s in range(64):
        w = (pkg.sr_round((w - np.float32(2.0 ** -9)).astype(np.float32), seed, s, 0).astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(_bits(ts[0].data), (w.view(np.uint32) >> 16).astype(np.uint16))
    mean = float(ts[0].data.double().mean())
    print(f"mean after 64 steps: {mean:.5f}")
    assert abs(mean - 1.375) <= 2.1e-3
    assert (plain[0].data.float() == 1.5).all()
    assert opt.step_of(ts) == 64


# ---- 5. bounds, state and argument errors
def test_bounds_error_writes_nothing_and_the_step_advances(pkg, gpu):
    rng = np.random.default_rng(7)
    rows, B, D = ROWS, 256, 16
    ts = _tables(pkg, gpu, rng, rows, D)
    opt = pkg.StochasticDescent(LR, seed=5)
    w0 = [_bits(t.data) for t in ts]
    idx = rand_indices(rng, rows, B, 1)
    g = torch.from_numpy(_exact_grad(rng, B, len(rows) * D)).to(gpu)
    bad = idx.copy()
    bad[3, B // 2] = rows[3] + 3
    pb = pkg.PackedIndices(torch.from_numpy(bad).to(torch.int32).to(gpu).reshape(len(rows), B, 1))
    with pytest.raises(pkg.BoundsError):
        _apply(pkg, opt, ts, pb, g, 0)
    for t in range(len(rows)):
        assert np.array_equal(_bits(ts[t].data), w0[t])
    assert opt.step_of(ts) == 1  # (the call returned DLRM_OK and launched)
    p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu).reshape(len(rows), B, 1))
    ref = _f32_copy(pkg, ts)
    _apply(pkg, opt, ts, p, g, 0)  # the flag is clear again: this one applies, with step 1
    _apply(pkg, pkg.Descent(LR), ref, p, g, 0)
    for t, want in enumerate(_want(pkg, ref, 5, 1)):
        assert np.array_equal(_bits(ts[t].data), want)


def test_state_and_flag_errors(pkg, gpu):
    _lib = pkg._lib
    rows, D, B = [3, 40, 100000, 7], 128, 512
    rng = np.random.default_rng(8)
    tabs = [torch.from_numpy(t).to(torch.bfloat16).to(gpu) for t in rand_tables(rng, rows, D)]
    ts = pkg.EmbeddingTableSet(tabs)
    T = len(rows)
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
    hp = pkg.HotPath(ts, B, 1, lr=0.5, index_base=0)
    assert hp.step_api
    x = torch.randn((B, D), device=gpu).to(torch.bfloat16)
    dout = torch.randn((B, hp.width), device=gpu).to(torch.bfloat16)
    hp.step_fwd(x, p)
    hp.step_bwd(dout, flags=_lib.STEP_BWD_ONLY)  # Descent's backward stepped the once-hit rows
    assert hp.indexer.state() & _lib.IX_SINGLES_DONE
    torch.cuda.synchronize()
    opt = pkg.StochasticDescent(seed=4)
    w0 = [_bits(t.data) for t in ts]
    args = (ctypes.c_void_p(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, ctypes.c_void_p(hp.dt.data_ptr()), _lib.F32,
            hp.dt.stride(0), D, 0.1)
    lib, h = ts.ctx.lib, ts.ctx.bind()
    assert lib.dlrm_sr_sgd_update(h, ts.handle, opt.handle_of(ts), hp.indexer.handle, _lib.UPDATE_PREBUILT,
                                  *args) == _lib.E_STATE
    assert lib.dlrm_sr_sgd_update(h, ts.handle, opt.handle_of(ts), hp.indexer.handle, _lib.UPDATE_ATOMIC,
                                  *args) == _lib.E_UNSUPPORTED
    # fp32 tables: neither a handle nor an update
    f32 = pkg.EmbeddingTableSet([t.float() for t in tabs])
    out = ctypes.c_void_p()
    assert lib.dlrm_sr_sgd_create(h, f32.handle, 0, ctypes.byref(out)) == _lib.E_ARG and not out.value
    ix = pkg.SparseIndexer(T, B, gpu)
    f0 = [t.data.clone() for t in f32]
    assert lib.dlrm_sr_sgd_update(h, f32.handle, opt.handle_of(ts), ix.handle, 0, *args) == _lib.E_ARG
    # a handle created for another D
    other = pkg.EmbeddingTableSet([torch.zeros((n, 16), dtype=torch.bfloat16, device=gpu) for n in rows])
    assert lib.dlrm_sr_sgd_update(h, other.handle, opt.handle_of(ts), ix.handle, 0, *args) == _lib.E_ARG
    torch.cuda.synchronize()
    for t in range(T):  # nothing was launched, and the step did not advance
        assert np.array_equal(_bits(ts[t].data), w0[t])
        assert torch.equal(f32[t].data, f0[t])
    assert opt.step_of(ts) == 0
    g = torch.zeros((B, T * D), device=gpu)
    with pytest.raises(ValueError, match="deterministic"):
        pkg.update_(pkg.StochasticDescent(), ts, pkg.maplookup_pullback(0, ts, p, g), index_base=0, deterministic=False)
    with pytest.raises(ValueError, match="bfloat16"):
        pkg.update_(pkg.StochasticDescent(), f32, pkg.maplookup_pullback(0, f32, p, g), index_base=0)
    # the engine: the operator route only
    for kw in ({"pipeline": "apply"}, {"pipeline": "side"}, {"fused_step": True}, {"adagrad_step": True}):
        with pytest.raises(ValueError, match="fused step"):
            pkg.HotPath(ts, B, 1, index_base=0, opt=pkg.StochasticDescent(), **kw)
    with pytest.raises(ValueError, match="bfloat16"):
        pkg.HotPath(f32, B, 1, index_base=0, opt=pkg.StochasticDescent())
    with pytest.raises(ValueError, match="lr"):
        pkg.HipTables(tabs, lr=0.1, index_base=0, opt=pkg.StochasticDescent())
    hp.check_bounds()


# ---- 6. capturable
def test_graph_replays_advance_the_step(pkg, gpu):
    """One update_ captured on one stream and replayed three times from step 0 == three eager calls from step 0."""
    rng = np.random.default_rng(9)
    rows, B, D = ROWS, B0, 128
    w = [torch.from_numpy(t).to(torch.bfloat16) for t in rand_tables(rng, rows, D)]
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu).reshape(len(rows), B, 1))
    g = torch.from_numpy(rng.standard_normal((B, len(rows) * D)).astype(np.float32)).to(gpu)
    te = pkg.EmbeddingTableSet([t.to(gpu) for t in w])
    oe = pkg.StochasticDescent(LR, seed=6)
    ixe = pkg.SparseIndexer(len(rows), B, gpu)
    for _ in range(3):
        pkg.update_(oe, te, pkg.maplookup_pullback(0, te, p, g), ixe, index_base=0, check_bounds=False)
    tg = pkg.EmbeddingTableSet([t.to(gpu) for t in w])
    og = pkg.StochasticDescent(LR, seed=6)
    ixg = pkg.SparseIndexer(len(rows), B, gpu)
    grads = pkg.maplookup_pullback(0, tg, p, g)
    pkg.update_(og, tg, grads, ixg, index_base=0)  # warm-up: the handle, first-use allocations
    for t, t0 in zip(tg, w):  # back to the start
        t.data.copy_(t0)
    og.seek(tg, 0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            pkg.update_(og, tg, grads, ixg, index_base=0, check_bounds=False)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    tg.ctx.check_bounds()
    assert og.step_of(tg) == 3 and oe.step_of(te) == 3
    for a, b, t0 in zip(tg, te, w):
        assert np.array_equal(_bits(a.data), _bits(b.data))
        assert not np.array_equal(_bits(a.data), _bits(t0))


# ---- 7. the engine and the lazy chain: one step each against update_
def _engine_inputs(pkg, gpu):
    rows, D, B = [3, 100, 20000], 16, 300
    rng = np.random.default_rng(10)
    w = [torch.from_numpy(t).to(torch.bfloat16) for t in rand_tables(rng, rows, D)]
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(torch.bfloat16)
    F = len(rows) + 1
    dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(torch.bfloat16)
    return rows, D, B, w, p, x, dout


def _operator_step(pkg, gpu, w, D, p, x, dout):
    ts = pkg.EmbeddingTableSet([t.to(gpu) for t in w])
    opt = pkg.StochasticDescent(LR, seed=21)
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ts, p, index_base=0)
    _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
    _, dx, dy = back(dout)
    pkg.update_(opt, ts, pkg.maplookup_pullback(D, ts, p, dy), index_base=0)
    assert opt.step_of(ts) == 1
    assert any(not np.array_equal(_bits(t.data), _bits(t0)) for t, t0 in zip(ts, w))
    return ts, dx


def test_hotpath_equals_update(pkg, gpu):
    rows, D, B, w, p, x, dout = _engine_inputs(pkg, gpu)
    ref_ts, ref_dx = _operator_step(pkg, gpu, w, D, p, x, dout)
    opt = pkg.StochasticDescent(LR, seed=21)
    hp = pkg.HotPath(pkg.EmbeddingTableSet([t.to(gpu) for t in w]), B, 1, index_base=0, opt=opt)
    assert not hp.step_api and hp.pipeline is None
    hp.step(x, p, dout)
    torch.cuda.synchronize()
    hp.check_bounds()
    assert opt.step_of(hp.ts) == 1
    for a, b in zip(hp.ts, ref_ts):
        assert np.array_equal(_bits(a.data), _bits(b.data))
    assert torch.equal(hp.dx, ref_dx)


def test_hiptables_chain_equals_update(pkg, gpu):
    rows, D, B, w, p, x, dout = _engine_inputs(pkg, gpu)
    ref_ts, ref_dx = _operator_step(pkg, gpu, w, D, p, x, dout)
    opt = pkg.StochasticDescent(LR, seed=21)
    ht = pkg.HipTables([t.to(gpu) for t in w], index_base=0, opt=opt)
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
    assert isinstance(ys, pkg.LazyLookup)
    _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
    _, dx, dy = back(dout)
    assert not dy.applied
    with pytest.raises(ValueError):
        pkg.update_(pkg.StochasticDescent(LR, seed=21), ht, pkg.maplookup_pullback(D, ht, p, dy))  # (another object)
    pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
    torch.cuda.synchronize()
    assert opt.step_of(ht.ts) == 1
    for a, b in zip(ht.ts, ref_ts):
        assert np.array_equal(_bits(a.data), _bits(b.data))
    assert torch.equal(dx, ref_dx)
