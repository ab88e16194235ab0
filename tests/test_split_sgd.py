"""Split-bf16 tables on the GPU: dlrm_split_sgd_update through update_, HotPath(opt=SplitDescent) and
HipTables.

The reference of every arithmetic check is dlrm_sgd_update (Descent) on fp32 tables that hold the
merged values, run on the GPU with the same indexer form, indices and gradient: merge_split(hi, lo)
must have exactly its bits, over all rows, after every step.  Nothing here compares the split kernels
against themselves.

Shapes (as test_adagrad.py): rows = [2, 8, 40, 5000] with B = 1024 one-hot lookups gives two-slice and
one-slice hot segments, chunks longer than the inline positions and once-hit singles in one launch.

Where both table dtypes take the vector kernels with the same lane geometry (everything 16-B aligned,
D * 2 % 16 == 0) the summation order is the same and normally distributed gradients are used.  Where
the paths may differ (D = 4: the fp32 table takes the vector kernels, the split table the any-D ones;
D = 12: three vectors per row, no vector instantiation, the any-D kernels for both; a low half 2 bytes
off a 16-B boundary; a displaced gradient; other indexer forms) the
gradients are k/64 with integer |k| <= 512 (<= 256 as bf16), so every row sum is exact in fp32 whatever
the order and bit equality must still hold.
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
DISPLACED_OFFSET = 13


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype in (torch.bfloat16, torch.int16) else t.view(torch.int32).numpy()


def _exact_grad(rng, B, width, kmax=512):
    return (rng.integers(-kmax, kmax + 1, size=(B, width)) / 64.0).astype(np.float32)


def _pair(pkg, gpu, rng, rows, D):
    """The same random fp32 weights as fp32 tables (the reference) and as split tables."""
    w = [torch.from_numpy(t) for t in rand_tables(rng, rows, D)]
    ref = pkg.EmbeddingTableSet([t.to(gpu) for t in w])
    halves = [pkg.split_f32(t) for t in w]
    ts = pkg.EmbeddingTableSet([h.to(gpu) for h, _ in halves])
    opt = pkg.SplitDescent(LR)
    for s, (_, lo) in zip(opt.state_of(ts), halves):
        assert s.dtype == torch.int16 and s.shape == lo.shape and not s.any()  # (zeros at first use)
        s.copy_(lo)
    return ref, ts, opt


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


def _apply(pkg, opt, ts, p, g, off, prepare):
    ix = None
    if prepare:
        ix = pkg.SparseIndexer(len(ts), p.B * p.L, ts.device)
        assert ix.prepare(ts, p, index_base=0)
    pkg.update_(opt, ts, pkg.maplookup_pullback(off, ts, p, g), ix, index_base=0, prebuilt=prepare)


def _assert_merged_equals(pkg, ts, opt, ref, what=""):
    for t, (m, r) in enumerate(zip(opt.master_of(ts), ref)):
        a, b = _bits(m), _bits(r.data)
        assert np.array_equal(a, b), f"{what} table {t}: {(a != b).sum()} of {a.size} elements differ"


def _run(pkg, gpu, D, *, rows=ROWS, B=B0, L=1, steps=2, seed=0, exact=False, grad_dtype=torch.float32, prepare=False,
         displaced=False):
    rng = np.random.default_rng(100 * D + seed)
    T = len(rows)
    ref, ts, opt = _pair(pkg, gpu, rng, rows, D)
    _assert_merged_equals(pkg, ts, opt, ref, "start:")
    lo = opt.state_of(ts)
    for step in range(steps):
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
        hi0 = [_bits(t.data) for t in ts]
        lo0 = [_bits(s) for s in lo]
        _apply(pkg, pkg.Descent(LR), ref, p, ga, off, prepare)
        _apply(pkg, opt, ts, p, ga, off, prepare)
        if band is not None:
            band.check(0, what="grad")
        _assert_merged_equals(pkg, ts, opt, ref, f"step {step}:")
        changed = 0
        for t in range(T):
            un = np.ones(rows[t], dtype=bool)
            un[idx[t]] = False
            assert np.array_equal(_bits(ts[t].data)[un], hi0[t][un]), f"table {t}: an untouched row's high half changed"
            assert np.array_equal(_bits(lo[t])[un], lo0[t][un]), f"table {t}: an untouched row's low half changed"
            changed += int((_bits(lo[t]) != lo0[t]).any())
            if prepare and L == 1 and t == T - 1:  # the once-hit rows are this launch's too
                r, c = np.unique(idx[t], return_counts=True)
                once = r[c == 1]
                assert len(once) > 100
                moved = (_bits(lo[t])[once] != lo0[t][once]).any(axis=1) | (_bits(ts[t].data)[once] != hi0[t][once]).any(axis=1)
                assert moved.all(), f"{(~moved).sum()} once-hit rows were not updated"
        assert changed == T  # (the update did run)


# ---- 1. bit equality, general gradients, the same vector path for both table dtypes
@pytest.mark.parametrize("D", [8, 16, 128, 512])
def test_bit_equal_fp32_gradients(pkg, gpu, D):
    _run(pkg, gpu, D)


@pytest.mark.parametrize("D", [16, 128])
def test_bit_equal_bf16_gradients(pkg, gpu, D):
    _run(pkg, gpu, D, seed=1, grad_dtype=torch.bfloat16)


# ---- 2. bit equality across kernel paths (exact gradients)
@pytest.mark.parametrize("D", [4, 12])
def test_any_dim_kernels(pkg, gpu, D):
    _run(pkg, gpu, D, seed=2, exact=True)


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16], ids=["gf32", "gbf16"])
@pytest.mark.parametrize("prepare", [False, True], ids=["built", "prepared"])
def test_displaced_unaligned_gradient(pkg, gpu, prepare, grad_dtype):
    _run(pkg, gpu, 16, seed=3, exact=True, grad_dtype=grad_dtype, prepare=prepare, displaced=True)


def test_low_half_off_a_16_byte_boundary(pkg, gpu):
    """lo[t] 2 bytes past a 16-B boundary, through the C entry points: the any-D kernels."""
    _lib = pkg._lib
    rng = np.random.default_rng(21)
    D, B, T = 16, B0, len(ROWS)
    w = [torch.from_numpy(t) for t in rand_tables(rng, ROWS, D)]
    ref = pkg.EmbeddingTableSet([t.to(gpu) for t in w])
    halves = [pkg.split_f32(t) for t in w]
    ts = pkg.EmbeddingTableSet([h.to(gpu) for h, _ in halves])
    bufs = [torch.full((n * D + 16,), 0x7A7A, dtype=torch.int16, device=gpu) for n in ROWS]
    los = [b[1:1 + n * D].view(n, D) for b, n in zip(bufs, ROWS)]
    for s, (_, lo) in zip(los, halves):
        assert s.data_ptr() % 16 == 2
        s.copy_(lo)
    lib, h = ts.ctx.lib, ts.ctx.bind()
    op = ctypes.c_void_p()
    ptrs = (ctypes.c_void_p * T)(*[s.data_ptr() for s in los])
    assert lib.dlrm_split_sgd_create(h, ts.handle, ptrs, ctypes.byref(op)) == 0
    try:
        idx = rand_indices(rng, ROWS, B, 1)
        p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu).reshape(T, B, 1))
        g = torch.from_numpy(_exact_grad(rng, B, T * D)).to(gpu)
        _apply(pkg, pkg.Descent(LR), ref, p, g, 0, False)
        ix = pkg.SparseIndexer(T, B, gpu)
        assert lib.dlrm_split_sgd_update(h, ts.handle, op, ix.handle, 0, ctypes.c_void_p(p.data.data_ptr()), p.itype,
                                         p.stride, 0, B, 1, ctypes.c_void_p(g.data_ptr()), _lib.F32, g.stride(0), 0,
                                         LR) == 0
        ts.ctx.check_bounds()
        for t in range(T):
            assert np.array_equal(_bits(pkg.merge_split(ts[t].data, los[t])), _bits(ref[t].data)), f"table {t}"
            assert (_bits(bufs[t][:1]) == 0x7A7A).all() and (_bits(bufs[t][1 + ROWS[t] * D:]) == 0x7A7A).all()
    finally:
        torch.cuda.synchronize()
        lib.dlrm_split_sgd_destroy(op)


# ---- 3. other indexer forms (exact gradients)
@pytest.mark.parametrize("form", ["pooled", "big", "prepared"])
def test_other_indexer_forms(pkg, gpu, form):
    """Pooled bags (L = 4); 8192 positions per table (above the in-LDS builds); and the wave build of
    SparseIndexer.prepare + prebuilt=True (the item-map path, whose once-hit rows are singles items)."""
    if form == "pooled":
        _run(pkg, gpu, 32, B=512, L=4, steps=1, seed=4, exact=True)
    elif form == "big":
        _run(pkg, gpu, 64, B=2048, L=4, steps=1, seed=5, exact=True)
    else:
        _run(pkg, gpu, 64, steps=2, seed=6, exact=True, prepare=True)


# ---- 4. the point of the feature
def test_small_updates_accumulate(pkg, gpu):
    """Weights 1.0, 16 steps of lr * G = 2^-12 on row 0: half a bf16 ulp of 1.0 is 2^-8, so a bf16 table
    never moves; the split table reaches 1 - 2^-8 exactly."""
    D, lr = 16, 2.0 ** -6
    p = pkg.PackedIndices(torch.zeros((1, 1, 1), dtype=torch.int32, device=gpu))
    g = torch.full((1, D), 2.0 ** -6, dtype=torch.float32, device=gpu)
    plain = pkg.EmbeddingTableSet([torch.ones((4, D), dtype=torch.bfloat16, device=gpu)])
    ts = pkg.EmbeddingTableSet([torch.ones((4, D), dtype=torch.bfloat16, device=gpu)])
    opt = pkg.SplitDescent(lr)
    hi0, lo0 = _bits(ts[0].data), _bits(opt.state_of(ts)[0])
    for _ in range(16):
        pkg.update_(pkg.Descent(lr), plain, pkg.maplookup_pullback(0, plain, p, g), index_base=0)
        pkg.update_(opt, ts, pkg.maplookup_pullback(0, ts, p, g), index_base=0)
    assert (plain[0].data[0].float().cpu() == 1.0).all()
    want = 1.0 - 2.0 ** -8
    assert (opt.master_of(ts)[0][0].cpu() == want).all()
    assert (ts[0].data[0].float().cpu() == want).all()
    assert np.array_equal(_bits(ts[0].data)[1:], hi0[1:])
    assert np.array_equal(_bits(opt.state_of(ts)[0])[1:], lo0[1:])


def test_nan_reads_as_nan_through_the_bf16_table(pkg, gpu):
    """A master weight that is a NaN with its payload in the low half only (high half = Inf's bits):
    after a step the high half alone is a NaN too, as the merged value and the fp32 reference are."""
    D = 16
    w = torch.from_numpy(np.full((4, D), 0x7F800001, dtype=np.uint32).view(np.float32).copy())
    w[1:] = 1.0
    hi, lo = pkg.split_f32(w)
    assert torch.isinf(hi[0].float()).all() and torch.isnan(w[0]).all()
    ref = pkg.EmbeddingTableSet([w.to(gpu)])
    ts = pkg.EmbeddingTableSet([hi.to(gpu)])
    opt = pkg.SplitDescent(LR)
    opt.state_of(ts)[0].copy_(lo)
    p = pkg.PackedIndices(torch.zeros((1, 1, 1), dtype=torch.int32, device=gpu))
    g = torch.ones((1, D), dtype=torch.float32, device=gpu)
    _apply(pkg, pkg.Descent(LR), ref, p, g, 0, False)
    _apply(pkg, opt, ts, p, g, 0, False)
    assert torch.isnan(ref[0].data[0]).all()
    assert torch.isnan(opt.master_of(ts)[0][0]).all()
    assert torch.isnan(ts[0].data[0].float()).all()
    assert np.array_equal(_bits(opt.master_of(ts)[0])[1:], _bits(w)[1:])


# ---- 5. bounds and argument errors
def test_bounds_error_writes_nothing(pkg, gpu):
    rng = np.random.default_rng(7)
    rows, B, D = ROWS, 256, 16
    ref, ts, opt = _pair(pkg, gpu, rng, rows, D)
    hi0 = [_bits(t.data) for t in ts]
    lo0 = [_bits(s) for s in opt.state_of(ts)]
    idx = rand_indices(rng, rows, B, 1)
    g = torch.from_numpy(_exact_grad(rng, B, len(rows) * D)).to(gpu)
    bad = idx.copy()
    bad[3, B // 2] = rows[3] + 3
    pb = pkg.PackedIndices(torch.from_numpy(bad).to(torch.int32).to(gpu).reshape(len(rows), B, 1))
    with pytest.raises(pkg.BoundsError):
        _apply(pkg, opt, ts, pb, g, 0, False)
    for t in range(len(rows)):
        assert np.array_equal(_bits(ts[t].data), hi0[t]) and np.array_equal(_bits(opt.state_of(ts)[t]), lo0[t])
    p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu).reshape(len(rows), B, 1))
    _apply(pkg, opt, ts, p, g, 0, False)  # the flag is clear again: this one applies
    _apply(pkg, pkg.Descent(LR), ref, p, g, 0, False)
    _assert_merged_equals(pkg, ts, opt, ref)


def test_state_and_flag_errors(pkg, gpu):
    _lib = pkg._lib
    rows, D, B = [3, 40, 100000, 7], 128, 512
    rng = np.random.default_rng(8)
    tabs = [torch.from_numpy(t).to(torch.bfloat16).to(gpu) for t in rand_tables(rng, rows, D)]
    ts = pkg.EmbeddingTableSet(tabs)
    p = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
    hp = pkg.HotPath(ts, B, 1, lr=0.5, index_base=0)
    assert hp.step_api
    x = torch.randn((B, D), device=gpu).to(torch.bfloat16)
    dout = torch.randn((B, hp.width), device=gpu).to(torch.bfloat16)
    hp.step_fwd(x, p)
    hp.step_bwd(dout, flags=_lib.STEP_BWD_ONLY)
    assert hp.indexer.state() & _lib.IX_SINGLES_DONE
    torch.cuda.synchronize()
    opt = pkg.SplitDescent()
    lo = opt.state_of(ts)
    hi0 = [_bits(t.data) for t in ts]
    args = (ctypes.c_void_p(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, ctypes.c_void_p(hp.dt.data_ptr()), _lib.F32,
            hp.dt.stride(0), D, 0.1)
    lib, h = ts.ctx.lib, ts.ctx.bind()
    # a split backward wrote the once-hit rows' high halves with a rounded bf16 step
    assert lib.dlrm_split_sgd_update(h, ts.handle, opt.handle_of(ts), hp.indexer.handle, _lib.UPDATE_PREBUILT,
                                     *args) == _lib.E_STATE
    assert lib.dlrm_split_sgd_update(h, ts.handle, opt.handle_of(ts), hp.indexer.handle, _lib.UPDATE_ATOMIC,
                                     *args) == _lib.E_UNSUPPORTED
    # fp32 tables: neither a handle nor an update
    f32 = pkg.EmbeddingTableSet([t.float() for t in tabs])
    T = len(rows)
    ptrs = (ctypes.c_void_p * T)(*[s.data_ptr() for s in lo])
    out = ctypes.c_void_p()
    assert lib.dlrm_split_sgd_create(h, f32.handle, ptrs, ctypes.byref(out)) == _lib.E_ARG and not out.value
    ix = pkg.SparseIndexer(T, B, gpu)
    f0 = [_bits(t.data) for t in f32]
    assert lib.dlrm_split_sgd_update(h, f32.handle, opt.handle_of(ts), ix.handle, 0, *args) == _lib.E_ARG
    # a table with rows and no low half
    ptrs[2] = None
    assert lib.dlrm_split_sgd_create(h, ts.handle, ptrs, ctypes.byref(out)) == _lib.E_ARG and not out.value
    # an optimizer created for another D
    other = pkg.EmbeddingTableSet([torch.zeros((n, 16), dtype=torch.bfloat16, device=gpu) for n in rows])
    assert lib.dlrm_split_sgd_update(h, other.handle, opt.handle_of(ts), ix.handle, 0, *args) == _lib.E_ARG
    torch.cuda.synchronize()
    for t in range(T):  # nothing was launched
        assert np.array_equal(_bits(ts[t].data), hi0[t]) and not lo[t].any()
        assert np.array_equal(_bits(f32[t].data), f0[t])
    g = torch.zeros((B, T * D), device=gpu)
    with pytest.raises(ValueError, match="deterministic"):
        pkg.update_(pkg.SplitDescent(), ts, pkg.maplookup_pullback(0, ts, p, g), index_base=0, deterministic=False)
    with pytest.raises(ValueError, match="bfloat16"):
        pkg.update_(pkg.SplitDescent(), f32, pkg.maplookup_pullback(0, f32, p, g), index_base=0)
    with pytest.raises(ValueError):
        pkg.HotPath(ts, B, 1, index_base=0, opt=pkg.SplitDescent(), pipeline="apply")
    hp.check_bounds()


# ---- 6. reproducible and capturable
def test_bitwise_reproducible(pkg, gpu):
    rows, B, D = [3, 10, 100000], 4096, 128
    rng = np.random.default_rng(9)
    w = [torch.from_numpy(t) for t in rand_tables(rng, rows, D)]
    idx = rand_indices(rng, rows, B, 1)
    p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu).reshape(len(rows), B, 1))
    g = torch.from_numpy(rng.standard_normal((B, len(rows) * D)).astype(np.float32)).to(gpu)
    got = []
    for _ in range(2):
        halves = [pkg.split_f32(t) for t in w]
        ts = pkg.EmbeddingTableSet([h.to(gpu) for h, _ in halves])
        opt = pkg.SplitDescent(LR)
        for s, (_, lo) in zip(opt.state_of(ts), halves):
            s.copy_(lo)
        _apply(pkg, opt, ts, p, g, 0, False)
        got.append([_bits(t.data) for t in ts] + [_bits(s) for s in opt.state_of(ts)])
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert not np.array_equal(got[0][5], _bits(pkg.split_f32(w[2])[1]))  # (the update did run)


def _engine_inputs(pkg, gpu):
    rows, D, B = [3, 100, 20000], 16, 300
    rng = np.random.default_rng(10)
    halves = [pkg.split_f32(torch.from_numpy(t)) for t in rand_tables(rng, rows, D)]
    packs = [pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32).to(gpu))
             for _ in range(2)]
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(torch.bfloat16)
    F = len(rows) + 1
    dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(torch.bfloat16)
    return rows, D, B, halves, packs, x, dout


def _fresh(pkg, gpu, halves):
    """(tables, optimizer) at the start values"""
    tabs = [h.to(gpu) for h, _ in halves]
    opt = pkg.SplitDescent(LR)
    return tabs, opt


def _install(opt, ts, halves):
    for s, (_, lo) in zip(opt.state_of(ts), halves):
        s.copy_(lo)


def _same(ts_a, opt_a, ts_b, opt_b):
    for a, b in zip(ts_a, ts_b):
        assert np.array_equal(_bits(a.data), _bits(b.data))
    for a, b in zip(opt_a.state_of(ts_a), opt_b.state_of(ts_b)):
        assert np.array_equal(_bits(a), _bits(b))


def _operator_steps(pkg, gpu, halves, D, packs, x, dout):
    tabs, opt = _fresh(pkg, gpu, halves)
    ts = pkg.EmbeddingTableSet(tabs)
    _install(opt, ts, halves)
    for p in packs:
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ts, p, index_base=0)
        _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
        _, dx, dy = back(dout)
        pkg.update_(opt, ts, pkg.maplookup_pullback(D, ts, p, dy), index_base=0)
    return ts, opt, dx


def test_hotpath_equals_operator_sequence_and_graph(pkg, gpu):
    rows, D, B, halves, packs, x, dout = _engine_inputs(pkg, gpu)
    ref_ts, ref_opt, ref_dx = _operator_steps(pkg, gpu, halves, D, packs, x, dout)
    assert any((_bits(s) != _bits(lo)).any() for s, (_, lo) in zip(ref_opt.state_of(ref_ts), halves))
    # eager engine steps
    tabs, opt = _fresh(pkg, gpu, halves)
    hp = pkg.HotPath(pkg.EmbeddingTableSet(tabs), B, 1, index_base=0, opt=opt)
    assert not hp.step_api and hp.pipeline is None
    _install(opt, hp.ts, halves)
    for p in packs:
        hp.step(x, p, dout)
    torch.cuda.synchronize()
    hp.check_bounds()
    _same(hp.ts, opt, ref_ts, ref_opt)
    assert np.array_equal(_bits(hp.dx), _bits(ref_dx))
    # the same step, captured after one eager warm-up step and replayed twice == two eager steps
    tabs_g, opt_g = _fresh(pkg, gpu, halves)
    hg = pkg.HotPath(pkg.EmbeddingTableSet(tabs_g), B, 1, index_base=0, opt=opt_g)
    tabs_e, opt_e = _fresh(pkg, gpu, halves)
    he = pkg.HotPath(pkg.EmbeddingTableSet(tabs_e), B, 1, index_base=0, opt=opt_e)
    _install(opt_e, he.ts, halves)
    hg.step(x, packs[0], dout)  # warm-up
    for t, (h, _) in zip(hg.ts, halves):  # back to the start
        t.data.copy_(h)
    _install(opt_g, hg.ts, halves)
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
    _same(hg.ts, opt_g, he.ts, opt_e)
    assert np.array_equal(_bits(hg.dx), _bits(he.dx))


def test_hiptables_chain_equals_plain_update(pkg, gpu):
    rows, D, B, halves, packs, x, dout = _engine_inputs(pkg, gpu)
    ref_ts, ref_opt, ref_dx = _operator_steps(pkg, gpu, halves, D, packs, x, dout)
    tabs, opt = _fresh(pkg, gpu, halves)
    ht = pkg.HipTables(tabs, lr=None, index_base=0)
    _install(opt, ht.ts, halves)
    for p in packs:
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
        assert isinstance(ys, pkg.LazyLookup)
        _, back = pkg.rrule(pkg.DotInteraction(), x, ys)
        _, dx, dy = back(dout)
        assert not dy.applied
        pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
    torch.cuda.synchronize()
    _same(ht.ts, opt, ref_ts, ref_opt)
    assert np.array_equal(_bits(dx), _bits(ref_dx))
