"""ADAGrad(seed=...) and RowwiseADAGrad(seed=...) on the GPU: the Adagrad rules with the stochastically rounded store
on bf16 tables (dlrm_adagrad_create_sr + dlrm_adagrad_update), through update_, HotPath(opt=...) and HipTables(opt=...).

The reference of every arithmetic check is never the kernel under test: the seedless rule of the same kind runs
(dlrm_adagrad_update with a dlrm_adagrad_create handle) on fp32 tables that hold the bf16 weights' values, with the
same indexer form, indices, gradient and a copy of the state.  That yields W' of every element (an untouched element's
W' is its bf16 value, which the store keeps) and the state's bits; the numpy sr_round with the step the call used then
gives the bits the bf16 tables must hold, over all rows, after every step.  The fp32 tables are reloaded from the bf16
result between steps.  Both kinds run throughout.

Shapes (as test_adagrad.py): rows = [2, 8, 40, 5000] with B = 1024 one-hot lookups gives two-slice and one-slice hot
segments, chunks longer than the inline positions and once-hit singles in one launch; one pooled case (L = 4, B = 256).
D = 128 and 16 take the vector kernels, D = 12 and 4 the any-D ones.

Where both table dtypes take the vector kernels with the same lane geometry the summation order is the same and
normally distributed gradients are used.  Where the paths may differ (D = 4: the fp32 table takes the vector kernels,
the bf16 table the any-D ones; D = 12; a displaced gradient; pooled bags; other indexer forms) the gradients are k/64
with integer k, so every row sum G is exact in fp32 whatever the order: |k| <= 512 (<= 256 as bf16) for the
element-wise rule, whose other operations are per element; |k| <= 1 for the row-wise rule, so that the sum of the
squares over a row is exact too (asserted: 4096 * sum G^2 is an integer below 2^24).

The walk test's bounds are test_sr_sgd_host.py's (six standard deviations, derived there); its expected mean is the
mean of the same rule's run on fp32 tables (Adagrad's step does not depend on w).
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
SEED = 12345
DISPLACED_OFFSET = 13
KINDS = [False, True]
KIND_IDS = ["elementwise", "rowwise"]
BF16 = torch.bfloat16


def _rule(pkg, rowwise):
    return pkg.RowwiseADAGrad if rowwise else pkg.ADAGrad


def _bits(t):
    """bit patterns of a bf16 (uint16) or fp32 (uint32) tensor"""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def _nearest(w):
    return _bits(torch.from_numpy(w).to(BF16))


def _tables(pkg, gpu, w):
    return pkg.EmbeddingTableSet([torch.from_numpy(t).to(BF16).to(gpu) for t in w])


def _f32_copy(pkg, ts):
    return pkg.EmbeddingTableSet([t.data.float() for t in ts])


def _pack(pkg, gpu, idx, B, L=1):
    return pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu).reshape(idx.shape[0], B, L))


def _exact_grad(rng, B, width, kmax):
    return (rng.integers(-kmax, kmax + 1, size=(B, width)) / 64.0).astype(np.float32)


def _assert_exact(idx, grad, rows, D, L, rowwise):
    """The row sums of k/64 gradients (and, row-wise, the sums of their squares) are exact in fp32 in any order."""
    k = np.rint(grad.astype(np.float64) * 64.0).astype(np.int64)
    assert np.array_equal(k / 64.0, grad.astype(np.float64))
    for t, n in enumerate(rows):
        kg = np.zeros((n, D), dtype=np.int64)
        ka = np.zeros((n, D), dtype=np.int64)
        bag = np.arange(idx.shape[1]) // L
        np.add.at(kg, idx[t], k[bag, t * D:(t + 1) * D])
        np.add.at(ka, idx[t], np.abs(k[bag, t * D:(t + 1) * D]))
        assert ka.max() < 2 ** 24  # every partial sum of G is an integer multiple of 1/64 below 2^24 / 64
        if rowwise:  # ... and so is every partial sum of the non-negative 4096 G^2, each at most the row's total
            assert (kg * kg).sum(axis=1).max() < 2 ** 24


def _grad_arg(g, gpu, displaced):
    """(gradient matrix, column offset, guard band) -- displaced: columns from 13 inside a NaN band whose base is one
    element past a 16-B boundary."""
    if not displaced:
        return g, 0, None
    off = DISPLACED_OFFSET
    band = banded((g.shape[0], off + g.shape[1]), g.dtype, off + g.shape[1], 1, gpu)
    band.view[:, off:].copy_(g)
    band.snapshot()
    return band.view, off, band


def _indexer(pkg, ts, p, form):
    """form: None = update_ builds its own; "build" = dlrm_indexer_build + PREBUILT; "prepare" = the wave build (a
    split indexer, taken whole) + PREBUILT; "prepare16" = the same with the other chunk limit and parts per table."""
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
    """the bits the stochastic store leaves for the fp32 results in `ref`"""
    return [pkg.sr_round(r.data.cpu().numpy(), seed, step, t) for t, r in enumerate(ref)]


def _preset(rng, opt, ropt, ts, ref, rowwise):
    """the same positive random state under both optimizers"""
    for s, r in zip(opt.state_of(ts), ropt.state_of(ref)):
        v = torch.from_numpy((EPS + rng.uniform(0.0, 0.5, size=tuple(s.shape))).astype(np.float32)).to(s.device)
        s.copy_(v)
        r.copy_(v)


def _run(pkg, gpu, rowwise, D, *, rows=ROWS, B=B0, L=1, steps=2, seed=0, exact=False, grad_dtype=torch.float32,
         form=None, displaced=False, first_step=0):
    rng = np.random.default_rng(100 * D + 7 * seed + int(rowwise))
    T = len(rows)
    ts = _tables(pkg, gpu, rand_tables(rng, rows, D))
    ref = _f32_copy(pkg, ts)
    opt = _rule(pkg, rowwise)(LR, EPS, seed=SEED + seed)
    ropt = _rule(pkg, rowwise)(LR, EPS)
    _preset(rng, opt, ropt, ts, ref, rowwise)
    if first_step:
        opt.seek(ts, first_step)
    rounded_differently = 0
    for k in range(steps):
        idx = rand_indices(rng, rows, B, L)
        if exact:
            grad = _exact_grad(rng, B, T * D, 1 if rowwise else (256 if grad_dtype == BF16 else 512))
            _assert_exact(idx, grad, rows, D, L, rowwise)
        else:
            grad = rng.standard_normal((B, T * D)).astype(np.float32)
        p = _pack(pkg, gpu, idx, B, L)
        g = torch.from_numpy(grad).to(gpu).to(grad_dtype)
        if exact:
            assert np.array_equal(g.float().cpu().numpy(), grad)  # (exact in grad_dtype)
        ga, off, band = _grad_arg(g, gpu, displaced)
        w0 = [_bits(t.data) for t in ts]
        s0 = [_bits(s) for s in opt.state_of(ts)]
        assert opt.step_of(ts) == first_step + k
        _apply(pkg, ropt, ref, p, ga, off, form)
        _apply(pkg, opt, ts, p, ga, off, form)
        if band is not None:
            band.check(0, what="grad")  # neither read past nor written
        want = _want(pkg, ref, SEED + seed, first_step + k)
        for t in range(T):
            got, st = _bits(ts[t].data), _bits(opt.state_of(ts)[t])
            assert np.array_equal(got, want[t]), f"step {k} table {t}: {(got != want[t]).sum()} of {got.size} elements differ"
            rst = _bits(ropt.state_of(ref)[t])
            assert np.array_equal(st, rst), f"step {k} table {t}: {(st != rst).sum()} of {st.size} state words differ"
            un = np.ones(rows[t], dtype=bool)
            un[idx[t]] = False
            assert np.array_equal(got[un], w0[t][un]), f"table {t}: an untouched row changed"
            assert np.array_equal(st[un], s0[t][un]), f"table {t}: an untouched row's state changed"
            assert (got[~un] != w0[t][~un]).any(), f"table {t}: no touched row changed"
            assert (st[~un] != s0[t][~un]).any(), f"table {t}: no touched row's state changed"
            rounded_differently += int((want[t] != _nearest(ref[t].data.cpu().numpy())).sum())
            ref[t].data.copy_(ts[t].data.float())  # the next step starts from the bf16 result
    assert rounded_differently > 0  # (the reference is not round-to-nearest in disguise)
    assert opt.step_of(ts) == first_step + steps
    return ts, opt


# ---- 1. bit equality with the restated store, the same vector path for both table dtypes
@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("D", [16, 128])
def test_bit_equal_fp32_gradients(pkg, gpu, D, rowwise):
    _run(pkg, gpu, rowwise, D, steps=3)


@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("D", [16, 128])
def test_bit_equal_bf16_gradients(pkg, gpu, D, rowwise):
    _run(pkg, gpu, rowwise, D, seed=1, grad_dtype=BF16)


# ---- 2. across kernel paths (exact gradients)
@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("D", [4, 12])
def test_any_dim_kernels(pkg, gpu, D, rowwise):
    _run(pkg, gpu, rowwise, D, seed=2, exact=True)


@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("grad_dtype", [torch.float32, BF16], ids=["gf32", "gbf16"])
@pytest.mark.parametrize("form", [None, "prepare"], ids=["built", "prepared"])
def test_displaced_gradient_in_a_guard_band(pkg, gpu, form, grad_dtype, rowwise):
    _run(pkg, gpu, rowwise, 16, seed=3, exact=True, grad_dtype=grad_dtype, form=form, displaced=True)


@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
def test_pooled_bags(pkg, gpu, rowwise):
    _run(pkg, gpu, rowwise, 16, B=256, L=4, seed=4, exact=True)


# ---- 3. indexer forms
@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("D", [128, 12])
def test_indexer_forms_give_the_same_bits(pkg, gpu, D, rowwise):
    """update_'s own build, dlrm_indexer_build (PREBUILT) and the wave build's split indexer taken whole (PREBUILT) at
    both chunk limits: each equals the restated store of its own fp32 reference, and all of them are the same bits,
    weights and state -- R does not depend on the indexer's form, its chunk limit or its parts."""
    got = []
    for form in (None, "build", "prepare", "prepare16"):
        ts, opt = _run(pkg, gpu, rowwise, D, seed=5, exact=True, form=form, first_step=2 ** 32 - 1)
        got.append([_bits(t.data) for t in ts] + [_bits(s) for s in opt.state_of(ts)])
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert np.array_equal(a, b)


# ---- 4. the step word and the seeds
@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
def test_seek_and_step_round_trip(pkg, gpu, rowwise):
    rng = np.random.default_rng(11)
    ts = _tables(pkg, gpu, rand_tables(rng, [50], 16))
    opt = _rule(pkg, rowwise)(LR, EPS, seed=1)
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
    other = _tables(pkg, gpu, rand_tables(rng, [50], 16))  # the step is per table set
    assert opt.step_of(other) == 0
    _apply(pkg, opt, ts, p, g, 0)
    assert opt.step_of(ts) == 1 and opt.step_of(other) == 0


@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
def test_seeds(pkg, gpu, rowwise):
    rng = np.random.default_rng(12)
    w = rand_tables(rng, ROWS, 16)
    p = _pack(pkg, gpu, rand_indices(rng, ROWS, B0, 1), B0)
    g = torch.from_numpy(rng.standard_normal((B0, len(ROWS) * 16)).astype(np.float32)).to(gpu)

    def one(seed, step=0):
        ts = _tables(pkg, gpu, w)
        opt = _rule(pkg, rowwise)(LR, EPS, seed=seed)
        if step:
            opt.seek(ts, step)
        _apply(pkg, opt, ts, p, g, 0)
        return [_bits(t.data) for t in ts], [_bits(s) for s in opt.state_of(ts)]

    a, b, c, d = one(3), one(3), one(2 ** 63 + 7), one(3, step=1)
    for t in range(len(ROWS)):
        assert np.array_equal(a[0][t], b[0][t])      # the same (seed, step): the same bits
        assert not np.array_equal(a[0][t], c[0][t])  # another seed: other bits
        for other in (b, c, d):                      # the state does not depend on either
            assert np.array_equal(a[1][t], other[1][t])
    assert not np.array_equal(a[0][3], d[0][3])      # the same seed at another step: other bits


# ---- 5. capturable
@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
def test_graph_replays_advance_the_step(pkg, gpu, rowwise):
    """One update_ captured on one stream and replayed three times from step 0 == three eager calls from step 0."""
    rng = np.random.default_rng(9)
    rows, B, D = ROWS, B0, 128
    w = rand_tables(rng, rows, D)
    p = _pack(pkg, gpu, rand_indices(rng, rows, B, 1), B)
    g = torch.from_numpy(rng.standard_normal((B, len(rows) * D)).astype(np.float32)).to(gpu)
    te = _tables(pkg, gpu, w)
    oe = _rule(pkg, rowwise)(LR, EPS, seed=6)
    ixe = pkg.SparseIndexer(len(rows), B, gpu)
    for _ in range(3):
        pkg.update_(oe, te, pkg.maplookup_pullback(0, te, p, g), ixe, index_base=0, check_bounds=False)
    tg = _tables(pkg, gpu, w)
    og = _rule(pkg, rowwise)(LR, EPS, seed=6)
    ixg = pkg.SparseIndexer(len(rows), B, gpu)
    grads = pkg.maplookup_pullback(0, tg, p, g)
    s_start = [s.clone() for s in og.state_of(tg)]
    pkg.update_(og, tg, grads, ixg, index_base=0)  # warm-up: the handle, first-use allocations
    for t, t0 in zip(tg, w):  # back to the start
        t.data.copy_(torch.from_numpy(t0).to(BF16))
    for s, s0 in zip(og.state_of(tg), s_start):
        s.copy_(s0)
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
        assert not np.array_equal(_bits(a.data), _nearest(t0))
    for a, b in zip(og.state_of(tg), oe.state_of(te)):
        assert np.array_equal(_bits(a), _bits(b))


# ---- 6. bounds
@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
def test_bounds_error_writes_nothing_and_the_step_advances(pkg, gpu, rowwise):
    rng = np.random.default_rng(7)
    rows, B, D = ROWS, 256, 16
    ts = _tables(pkg, gpu, rand_tables(rng, rows, D))
    opt = _rule(pkg, rowwise)(LR, EPS, seed=5)
    ropt = _rule(pkg, rowwise)(LR, EPS)
    w0 = [_bits(t.data) for t in ts]
    s0 = [_bits(s) for s in opt.state_of(ts)]
    idx = rand_indices(rng, rows, B, 1)
    g = torch.from_numpy(_exact_grad(rng, B, len(rows) * D, 1)).to(gpu)
    bad = idx.copy()
    bad[3, B // 2] = rows[3] + 3
    with pytest.raises(pkg.BoundsError):
        _apply(pkg, opt, ts, _pack(pkg, gpu, bad, B), g, 0)
    for t in range(len(rows)):
        assert np.array_equal(_bits(ts[t].data), w0[t])
        assert np.array_equal(_bits(opt.state_of(ts)[t]), s0[t])
    assert opt.step_of(ts) == 1  # (the call returned DLRM_OK and launched)
    p = _pack(pkg, gpu, idx, B)
    ref = _f32_copy(pkg, ts)
    _apply(pkg, opt, ts, p, g, 0)  # the flag is clear again: this one applies, with step 1
    _apply(pkg, ropt, ref, p, g, 0)
    for t, want in enumerate(_want(pkg, ref, 5, 1)):
        assert np.array_equal(_bits(ts[t].data), want)
        assert np.array_equal(_bits(opt.state_of(ts)[t]), _bits(ropt.state_of(ref)[t]))


# ---- 7. refusals: nothing launched, nothing written, the step word untouched
def test_refusals(pkg, gpu):
    _lib = pkg._lib
    rows = [(ROWS + [3, 100000])[t % 6] for t in range(20)]
    T, D, B = len(rows), 128, 1024  # (20 tables of dim 128: every rule's step backward steps the once-hit rows)
    rng = np.random.default_rng(8)
    w = rand_tables(rng, rows, D)
    ts = _tables(pkg, gpu, w)
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
    x = torch.randn((B, D), device=gpu).to(BF16)
    hp = pkg.HotPath(ts, B, 1, lr=LR, index_base=0)  # (Descent: the forward and the buffers)
    assert hp.step_api
    dout = torch.randn((B, hp.width), device=gpu).to(BF16)
    lib, h, vp = ts.ctx.lib, ts.ctx.bind(), ctypes.c_void_p
    seeded = [pkg.ADAGrad(LR, EPS, seed=4), pkg.RowwiseADAGrad(LR, EPS, seed=4)]
    plain = [pkg.ADAGrad(LR, EPS), pkg.RowwiseADAGrad(LR, EPS)]
    split, sto = pkg.SplitDescent(LR), pkg.StochasticDescent(LR, seed=1)
    for o in seeded:
        o.seek(ts, 41)
    step = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, vp(x.data_ptr()), x.stride(0), vp(dout.data_ptr()),
            dout.stride(0), hp.padding, vp(hp.dx.data_ptr()), hp.dx.stride(0), vp(hp.dt.data_ptr()), hp.dt.stride(0), LR)
    upd = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, vp(hp.dt.data_ptr()), _lib.F32, hp.dt.stride(0), D, LR, EPS)
    ixh = hp.indexer.handle

    def snap():
        torch.cuda.synchronize()
        return ([_bits(t.data) for t in ts] + [_bits(s) for o in seeded + plain + [split] for s in o.state_of(ts)] +
                [np.array([o.step_of(ts) for o in seeded] + [sto.step_of(ts)], dtype=np.uint64)])

    def unchanged(before, what):
        for a, b in zip(before, snap()):
            assert np.array_equal(a, b), f"{what}: a refused call wrote"

    # a SINGLES_DONE indexer, once for each existing rule's mark
    marks = {
        "descent": (lambda f: lib.dlrm_step_bwd(h, ts.handle, ixh, *step, f), 0),
        "split": (lambda f: lib.dlrm_split_step_bwd(h, ts.handle, split.handle_of(ts), ixh, *step, f),
                  _lib.IX_SINGLES_SPLIT),
        "elementwise": (lambda f: lib.dlrm_adagrad_step_bwd(h, ts.handle, plain[0].handle_of(ts), ixh, *step, EPS, f),
                        _lib.IX_SINGLES_ADAGRAD),
        "rowwise": (lambda f: lib.dlrm_adagrad_step_bwd(h, ts.handle, plain[1].handle_of(ts), ixh, *step, EPS, f),
                    _lib.IX_SINGLES_ROWWISE),
        "stochastic": (lambda f: lib.dlrm_sr_step_bwd(h, ts.handle, sto.handle_of(ts), ixh, *step, f),
                       _lib.IX_SINGLES_STOCHASTIC),
    }
    rule_bits = (_lib.IX_SINGLES_SPLIT | _lib.IX_SINGLES_ADAGRAD | _lib.IX_SINGLES_ROWWISE | _lib.IX_SINGLES_STOCHASTIC)
    for name, (step_fn, bit) in marks.items():
        hp.step_fwd(x, p)
        assert step_fn(_lib.STEP_BWD_ONLY) == 0, name
        st = hp.indexer.state()
        assert st & _lib.IX_SINGLES_DONE and st & rule_bits == bit, (name, st)
        before = snap()
        for o in seeded:
            assert lib.dlrm_adagrad_update(h, ts.handle, o.handle_of(ts), ixh, _lib.UPDATE_PREBUILT, *upd) == _lib.E_STATE
        unchanged(before, f"PREBUILT on {name}'s mark")
        assert step_fn(_lib.STEP_APPLY_ONLY) == 0, name  # (its own apply completes the step)
    # the fused step with a stochastic handle, on a fresh build and in every form
    hp.step_fwd(x, p)
    nxt = pkg.SparseIndexer(T, B, gpu)
    before = snap()
    for o in seeded:
        for f in (0, _lib.STEP_BWD_ONLY, _lib.STEP_APPLY_ONLY):
            assert lib.dlrm_adagrad_step_bwd(h, ts.handle, o.handle_of(ts), ixh, *step, EPS, f) == _lib.E_UNSUPPORTED
            assert lib.dlrm_adagrad_step_bwd_prepare(h, ts.handle, o.handle_of(ts), ixh, *step, EPS, nxt.handle,
                                                     vp(p.data.data_ptr()), f) == _lib.E_UNSUPPORTED
        # the atomic flag
        assert lib.dlrm_adagrad_update(h, ts.handle, o.handle_of(ts), ixh, _lib.UPDATE_ATOMIC, *upd) == _lib.E_UNSUPPORTED
    assert not hp.indexer.state() & _lib.IX_SINGLES_DONE and not nxt.state() & _lib.IX_BUILT
    # seek / step on a plain handle
    word = ctypes.c_uint64(77)
    for o in plain:
        assert lib.dlrm_adagrad_seek(h, o.handle_of(ts), 5) == _lib.E_ARG
        assert lib.dlrm_adagrad_step(h, o.handle_of(ts), ctypes.byref(word)) == _lib.E_ARG and word.value == 77
        with pytest.raises(ValueError, match="seed"):
            o.seek(ts, 5)
        with pytest.raises(ValueError, match="seed"):
            o.step_of(ts)
    # fp32 tables: neither a handle nor an update
    f32 = pkg.EmbeddingTableSet([torch.from_numpy(t).to(gpu) for t in w])
    f0 = [t.data.clone() for t in f32]
    ix = pkg.SparseIndexer(T, B, gpu)
    for o, q in zip(seeded, plain):
        out = ctypes.c_void_p()
        ptrs = (ctypes.c_void_p * T)(*[s.data_ptr() for s in q.state_of(ts)])
        assert lib.dlrm_adagrad_create_sr(h, f32.handle, int(o.rowwise), ptrs, 0, ctypes.byref(out)) == _lib.E_ARG
        assert not out.value
        assert lib.dlrm_adagrad_update(h, f32.handle, o.handle_of(ts), ix.handle, 0, *upd) == _lib.E_ARG
        with pytest.raises(ValueError, match="bfloat16"):
            pkg.update_(o, f32, pkg.maplookup_pullback(D, f32, p, hp.dt), index_base=0)
        with pytest.raises(ValueError, match="bfloat16"):
            pkg.HotPath(f32, B, 1, index_base=0, opt=o)
        with pytest.raises(ValueError, match="deterministic"):
            pkg.update_(o, ts, pkg.maplookup_pullback(D, ts, p, hp.dt), index_base=0, deterministic=False)
    unchanged(before, "the refusals")
    for t in range(T):
        assert torch.equal(f32[t].data, f0[t])
    assert [o.step_of(ts) for o in seeded] == [41, 41]
    hp.check_bounds()


# ---- 8. the point of the feature
def test_walk_of_small_steps(pkg, gpu):
    """64 x 128 weights 1.5, every row hit once per step with G = 1, eta = 2^-9, 64 row-wise steps: step k is
    eta / (sqrt(k) + eps), under half a bf16 ulp of the weight (2^-8) every time.  The stochastic store's mean lands
    within 2.1e-3 of the same rule's on fp32 tables (1.47148) and 2048 +- 235 elements move in step 0 (both six
    standard deviations: test_sr_sgd_host.py); the seedless rule on the same bf16 input stays at 1.5."""
    n, D, eta, seed = 64, 128, 2.0 ** -9, 12345
    p = pkg.PackedIndices(torch.arange(n, dtype=torch.int32, device=gpu).reshape(1, n, 1))
    g = torch.ones((n, D), dtype=torch.float32, device=gpu)
    ts = pkg.EmbeddingTableSet([torch.full((n, D), 1.5, dtype=BF16, device=gpu)])
    plain = pkg.EmbeddingTableSet([torch.full((n, D), 1.5, dtype=BF16, device=gpu)])
    exact = pkg.EmbeddingTableSet([torch.full((n, D), 1.5, dtype=torch.float32, device=gpu)])
    opt, popt, eopt = pkg.RowwiseADAGrad(eta, seed=seed), pkg.RowwiseADAGrad(eta), pkg.RowwiseADAGrad(eta)
    ix = pkg.SparseIndexer(1, n, gpu)
    moved0 = None
    for k in range(64):
        for o, t in ((opt, ts), (popt, plain), (eopt, exact)):
            pkg.update_(o, t, pkg.maplookup_pullback(0, t, p, g), ix, index_base=0, check_bounds=False)
        if k == 0:
            moved0 = int((ts[0].data.float() != 1.5).sum())
    ts.ctx.check_bounds()
    want = float(exact[0].data.double().mean())
    mean = float(ts[0].data.double().mean())
    print(f"moved after step 0 = {moved0}, mean after 64 steps = {mean:.5f}, on fp32 tables {want:.5f}")
    assert abs(want - (1.5 - sum(eta / (np.sqrt(k) + 1e-8) for k in range(1, 65)))) <= 1e-5  # (the closed form)
    assert abs(moved0 - 2048) <= 235, moved0
    assert abs(mean - want) <= 2.1e-3, (mean, want)
    assert (plain[0].data.float() == 1.5).all()
    for a, b in ((opt, ts), (popt, plain)):  # the state is the fp32 run's, bit for bit: k after k steps
        assert np.array_equal(_bits(a.state_of(b)[0]), _bits(eopt.state_of(exact)[0]))
    assert opt.step_of(ts) == 64


# ---- 9. the engines: one step each against update_
def _engine_inputs(pkg, gpu):
    rows, D, B = [3, 100, 20000], 16, 300
    rng = np.random.default_rng(10)
    w = rand_tables(rng, rows, D)
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(BF16)
    F = len(rows) + 1
    dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(BF16)
    return rows, D, B, w, p, x, dout


def _operator_step(pkg, gpu, rowwise, w, D, p, x, dout):
    ts = _tables(pkg, gpu, w)
    opt = _rule(pkg, rowwise)(LR, EPS, seed=21)
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ts, p, index_base=0)
    _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
    _, dx, dy = back(dout)
    pkg.update_(opt, ts, pkg.maplookup_pullback(D, ts, p, dy), index_base=0)
    assert opt.step_of(ts) == 1
    assert any(not np.array_equal(_bits(t.data), _nearest(t0)) for t, t0 in zip(ts, w))
    return ts, opt, dx


def _same_as(ts, opt, ref_ts, ref_opt):
    for a, b in zip(ts, ref_ts):
        assert np.array_equal(_bits(a.data), _bits(b.data))
    for a, b in zip(opt.state_of(ts), ref_opt.state_of(ref_ts)):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
def test_hotpath_equals_update(pkg, gpu, rowwise):
    rows, D, B, w, p, x, dout = _engine_inputs(pkg, gpu)
    ref_ts, ref_opt, ref_dx = _operator_step(pkg, gpu, rowwise, w, D, p, x, dout)
    opt = _rule(pkg, rowwise)(LR, EPS, seed=21)
    for kw in ({"adagrad_step": True}, {"pipeline": "apply"}, {"fused_step": True}, {"stochastic_step": True}):
        with pytest.raises(ValueError, match="fused step"):
            pkg.HotPath(_tables(pkg, gpu, w), B, 1, index_base=0, opt=opt, **kw)
    hp = pkg.HotPath(_tables(pkg, gpu, w), B, 1, index_base=0, opt=opt)
    assert not hp.step_api and hp.pipeline is None and not hp.adagrad_step
    hp.step(x, p, dout)
    torch.cuda.synchronize()
    hp.check_bounds()
    assert opt.step_of(hp.ts) == 1
    _same_as(hp.ts, opt, ref_ts, ref_opt)
    assert torch.equal(hp.dx, ref_dx)


@pytest.mark.parametrize("rowwise", KINDS, ids=KIND_IDS)
def test_hiptables_chain_equals_update(pkg, gpu, rowwise):
    rows, D, B, w, p, x, dout = _engine_inputs(pkg, gpu)
    ref_ts, ref_opt, ref_dx = _operator_step(pkg, gpu, rowwise, w, D, p, x, dout)
    opt = _rule(pkg, rowwise)(LR, EPS, seed=21)
    tabs = [torch.from_numpy(t).to(BF16).to(gpu) for t in w]
    with pytest.raises(ValueError, match="adagrad_step"):
        pkg.HipTables(tabs, index_base=0, opt=opt, adagrad_step=True)
    with pytest.raises(ValueError, match="lr"):
        pkg.HipTables(tabs, lr=LR, index_base=0, opt=opt)
    ht = pkg.HipTables(tabs, index_base=0, opt=opt)
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
    assert isinstance(ys, pkg.LazyLookup)
    _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
    _, dx, dy = back(dout)
    assert not dy.applied
    with pytest.raises(ValueError):
        pkg.update_(_rule(pkg, rowwise)(LR, EPS, seed=21), ht, pkg.maplookup_pullback(D, ht, p, dy))  # (another object)
    pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
    torch.cuda.synchronize()
    assert opt.step_of(ht.ts) == 1
    _same_as(ht.ts, opt, ref_ts, ref_opt)
    assert torch.equal(dx, ref_dx)
