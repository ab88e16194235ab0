"""Layout arguments of the C ABI: `padding`, leading dimensions, displaced and misaligned base
pointers, `out_offset` / `grad_offset`, index views with `table_stride > batch`, and bf16 gradients.

Every output lives in a guard band (helpers.banded): a strided view inside an allocation filled with
a NaN bit pattern, so a store past a row's documented extent shows up as a changed guard element and
a load past an input's extent as a NaN in the result -- without any access outside the allocation.
Inputs whose tail must not be read (x, ys, dout and its padding columns, gradients and the columns
before grad_offset) are banded the same way.

Bars: the ones the parity modules already hold these operators to -- bit equality for copies
(fast_vcat, the lookup), for the fused forms against the operator sequence, and for the Descent
update on exactly representable inputs; rtol 2e-6 (fp32) / 8e-3 (bf16 forward) against the CPU
oracle for the interaction, with the scales of test_interaction_fwd_bwd_vs_oracle /
test_interaction_bf16.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from helpers import (_assert_segments, _dt_written_mask, assert_close, banded, dev_tables, rand_indices, rand_tables,
                     to_np_bits)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# out / dx / dt layouts: (elements added to the leading dimension, elements before each row)
LAYOUTS = {"contig": (0, 0), "ld+4": (4, 0), "ld+3": (3, 0), "ld+1": (1, 0), "lead1": (0, 1)}


def _name(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _to_dev(a, device):
    """numpy float32, or uint16 bf16 bit patterns -> device tensor"""
    a = np.array(a, order="C")  # (a copy: the cached references are read-only)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(device).view(torch.bfloat16)
    return torch.from_numpy(a).to(device)


def _place(a, ld, lead, device):
    """numpy array -> Band whose view holds it (everything around it: NaN)"""
    band = banded(a.shape, BF16 if a.dtype == np.uint16 else F32, ld, lead, device)
    band.view.copy_(_to_dev(a, device))
    return band.snapshot()


def _vals(band):
    """The view as numpy: float32, or uint16 bf16 bit patterns."""
    b = band.bits()
    return b.view(np.uint16) if b.dtype == np.int16 else b.view(np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16)


def _f32(a):
    return oracle.bf16_to_f32(a) if a.dtype == np.uint16 else a


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _check_fwd_out(o, x, ys_tables, ref, d, F):
    """out == [x (bits) | pairs (oracle bar) | zero bits]; ys_tables: the table columns of ys."""
    P = F * (F - 1) // 2
    assert o.shape == ref.shape and o.dtype == ref.dtype
    assert np.array_equal(_bits(o[:, :d]), _bits(x)), "out[:, :d] != x"
    assert np.isfinite(_f32(o)).all(), "a NaN reached out: something outside an input's extent was read"
    if o.dtype == np.uint16:
        r = _f32(ref)
        assert_close(_f32(o), r, rtol=8e-3, scale=float(np.abs(r).max()), what="bf16 fwd")
    else:
        scale = float(np.abs(ys_tables).max() ** 2 * d)
        assert_close(o, ref, rtol=2e-6, scale=scale, what="interaction fwd")
    assert not _bits(o[:, d + P:]).any(), "padding columns are not all-zero bits"


# ------------------------------------------------------------------ 1. interaction forward
# (d, F, B, dtype, pad_to values)
FWD_SHAPES = [
    (128, 27, 9, F32, (1, 8, 64)),    # W = 479 / 480 (the 16-B row store) / 512
    (128, 8, 5, F32, (1, 4, 64)),     # W = 156: the 16-B row store with no padding
    (16, 8, 7, F32, (1, 8, 16, 32)),  # the generic kernel; W = 44 / 48 / 48 / 64
    (32, 17, 6, BF16, (1, 8, 64)),
    (128, 27, 5, BF16, (1, 8, 64)),
    (64, 33, 5, F32, (1, 7, 64)),     # NB = 3; W = 592 / 595 / 640
    (128, 50, 3, F32, (1, 4, 64)),    # W = 1353 > 1024: the unstaged stores
    (8, 100, 3, F32, (1, 8, 64)),     # NB = 7: interact_fwd_scalar
]


@functools.lru_cache(maxsize=None)
def _fwd_case(d, F, B, bf16):
    rng = np.random.default_rng(d * 1000 + F)
    x = rng.standard_normal((B, d)).astype(np.float32)
    ys = np.zeros((B, F * d), dtype=np.float32)
    ys[:, d:] = rng.standard_normal((B, (F - 1) * d)).astype(np.float32)
    if bf16:
        x, ys = oracle.f32_to_bf16(x), oracle.f32_to_bf16(ys)
    return _frozen(x, ys)


@functools.lru_cache(maxsize=None)
def _fwd_ref(d, F, B, bf16, padding):
    x, ys = _fwd_case(d, F, B, bf16)
    ref_ys = ys.copy()
    out = oracle.interact_fwd(x, ref_ys, F, padding)  # (fast_vcat: writes x into ref_ys)
    return _frozen(out, ref_ys)


def _run_fwd(pkg, gpu, d, F, B, dtype, pad_to, out_layout, x_extra=0, ys_extra=0):
    bf16 = dtype == BF16
    x, ys = _fwd_case(d, F, B, bf16)
    _, W, padding = pkg.interact.interaction_sizes(d, F, pad_to)
    ref, ref_ys = _fwd_ref(d, F, B, bf16, padding)
    xb = _place(x, d + x_extra, 0, gpu)
    yb = _place(ys, F * d + ys_extra, 0, gpu)
    extra, lead = LAYOUTS[out_layout]
    ob = banded((B, W), dtype, W + extra, lead, gpu)
    got = pkg.DotInteraction(pad_to=pad_to)(xb.view, yb.view, out=ob.view)
    torch.cuda.synchronize()
    assert got.data_ptr() == ob.view.data_ptr()
    _check_fwd_out(_vals(ob), x, _f32(ys), ref, d, F)
    y = _vals(yb)
    assert np.array_equal(_bits(y[:, :d]), _bits(x)), "fast_vcat: ys[:, :d] != x"
    assert np.array_equal(_bits(y[:, d:]), _bits(ys[:, d:])), "ys[:, d:] changed"
    assert np.array_equal(_bits(y), _bits(ref_ys))
    ob.check(what="out")  # the whole padded row is written, nothing beyond it
    yb.check(d, what="ys")
    xb.check(0, what="x")


def _fwd_params():
    for d, F, B, dtype, pads in FWD_SHAPES:
        for pad_to in pads:
            for layout in ("contig", "ld+4", "ld+3", "lead1"):
                yield pytest.param(d, F, B, dtype, pad_to, layout, id=f"d{d}-F{F}-B{B}-{_name(dtype)}-pad{pad_to}-{layout}")


@pytest.mark.parametrize("d,F,B,dtype,pad_to,layout", list(_fwd_params()))
def test_interact_fwd_padding_and_out_layouts(pkg, gpu, d, F, B, dtype, pad_to, layout):
    """dlrm_interact_fwd with padding and a strided / displaced `out`: x and fast_vcat bit for bit,
    the pairs at the oracle bar, zero padding columns, nothing written past d + P + padding in a row
    (ld = W + 3 rotates the rows through all four 16-B residues; lead1 breaks the base alignment)."""
    _run_fwd(pkg, gpu, d, F, B, dtype, pad_to, layout)


@pytest.mark.parametrize("inputs", ["x_ld+4", "ys_ld+8", "x_ld+1"])
@pytest.mark.parametrize("d,F,B,pads", [(128, 27, 9, (1, 8, 64)), (16, 8, 7, (1, 8, 32))])
def test_interact_fwd_input_layouts(pkg, gpu, d, F, B, pads, inputs):
    """Strided x and ys (16-B aligned rows: the MFMA kernels), and an x of leading dimension d + 1
    (no 16-B alignment: the scalar fallback must give the same answer)."""
    x_extra, ys_extra = {"x_ld+4": (4, 0), "ys_ld+8": (0, 8), "x_ld+1": (1, 0)}[inputs]
    for pad_to in pads:
        for layout in ("contig", "ld+3"):
            _run_fwd(pkg, gpu, d, F, B, F32, pad_to, layout, x_extra, ys_extra)


# ------------------------------------------------------------------ 2. fused forward and the step
STEP_CASES = {
    "d32": ([10, 3000, 7, 100000], 32, 101, F32),
    "d128": ([5, 100000, 3, 77] * 6 + [9, 10], 128, 70, F32),
    "d128-bf16": ([5, 100000, 3, 77] * 6 + [9, 10], 128, 70, BF16),
}


def _hot_inputs(rows, D, B, L, dtype, gpu, seed):
    rng = np.random.default_rng(seed)
    tabs = rand_tables(rng, rows, D)
    idx_np = rand_indices(rng, rows, B, L)
    x_np = rng.standard_normal((B, D)).astype(np.float32)
    if dtype == BF16:
        x_np = oracle.f32_to_bf16(x_np)
    idx = torch.from_numpy(idx_np).reshape(len(rows), B, L).to(torch.int32).to(gpu)
    return rng, tabs, idx_np, x_np, idx


def _two_operators(pkg, tabs_dev, p, x, D, pad_to):
    ys = pkg.maplookup(pkg.PreallocationStrategy(D), tabs_dev, p, index_base=0)
    ys_tables = _f32(to_np_bits(ys))[:, D:].copy()  # (before fast_vcat)
    out = pkg.DotInteraction(pad_to=pad_to)(x, ys)
    return ys, ys_tables, out


def _oracle_fwd(x_np, ys_dev, F, padding):
    ys_np = np.ascontiguousarray(to_np_bits(ys_dev))
    return oracle.interact_fwd(x_np, ys_np, F, padding)


@pytest.mark.parametrize("out_layout", ["ld+4", "ld+3", "lead1"])
@pytest.mark.parametrize("case", ["d32", "d128", "d128-bf16", "pooled-L10", "pooled-L9", "pooled-no-ys"])
def test_fused_forward_padding_and_strided_buffers(pkg, gpu, case, out_layout):
    """dlrm_lookup_interact_fwd with pad_to = 8 into banded `out` and `ys`: ys and out are what
    maplookup + DotInteraction(pad_to = 8) write, bit for bit (the header's promise), out matches the
    oracle, the padding columns are zero bits and the guards are intact.
    Pooled bags: with ys kept, 7 tables x 10 lookups (> 64 rows per sample) take the library's
    two-launch form; 7 x 9 runs the pooled fused kernel, and `pooled-no-ys` calls the ABI with
    ys = NULL at L = 10 (HotPath keeps ys for pooled bags, so the wrapper cannot)."""
    if case.startswith("pooled"):
        rows, D, B, dtype = [1000] * 7, 16, 33, F32
        L = 9 if case == "pooled-L9" else 10
    else:
        (rows, D, B, dtype), L = STEP_CASES[case], 1
    rng, tabs, idx_np, x_np, idx = _hot_inputs(rows, D, B, L, dtype, gpu, len(rows) * D + L)
    tabs_dev = dev_tables(tabs, gpu, dtype)
    hp = pkg.HotPath(pkg.EmbeddingTableSet(tabs_dev), B, L, index_base=0, fused=True, materialize_ys=True, pad_to=8)
    F = hp.F
    assert hp.padding == hp.width - (D + F * (F - 1) // 2) and hp.padding > 0
    xb = _place(x_np, D + 8, 0, gpu)
    extra, lead = LAYOUTS[out_layout]
    ob = banded((B, hp.width), dtype, hp.width + extra, lead, gpu)
    yb = banded((B, F * D), dtype, F * D + 8, 0, gpu)
    hp.out, hp.ys = ob.view, yb.view
    p = pkg.PackedIndices(idx)
    hp.validate(xb.view, p)
    if case == "pooled-no-ys":
        rc = hp.lib.dlrm_lookup_interact_fwd(hp.ctx.bind(), hp.ts.handle, _vp(p.data), p.itype, p.stride, 0, B, L,
                                             _vp(xb.view), xb.ld, None, 0, _vp(ob.view), ob.ld, hp.padding)
        assert rc == pkg._lib.OK
    else:
        hp.forward(xb.view, p)
    ys, ys_tables, out = _two_operators(pkg, tabs_dev, p, xb.view, D, 8)
    torch.cuda.synchronize()
    hp.check_bounds()
    o = _vals(ob)
    assert np.array_equal(_bits(o), _bits(to_np_bits(out))), "fused out != maplookup + DotInteraction"
    _check_fwd_out(o, x_np, ys_tables, _oracle_fwd(x_np, ys, F, hp.padding), D, F)
    ob.check(what="out")
    xb.check(0, what="x")
    if case == "pooled-no-ys":
        yb.check(0, what="ys (not passed)")
    else:
        assert np.array_equal(_bits(_vals(yb)), _bits(to_np_bits(ys))), "fused ys != maplookup + fast_vcat"
        yb.check(what="ys")


@pytest.mark.parametrize("out_layout", ["ld+4", "lead1"])
@pytest.mark.parametrize("case", ["d32", "d128", "d128-bf16"])
def test_step_padding_and_strided_buffers(pkg, gpu, case, out_layout):
    """dlrm_step_fwd / dlrm_step_bwd with pad_to = 8, banded out / dx / dt and a dout whose padding
    columns (and surroundings) are NaN: out is the two-operator result bit for bit; dx, the tables and
    the dt rows the apply reads equal a pad_to = 1 contiguous HotPath given dout[:, :d + P], bit for
    bit; every guard is intact."""
    rows, D, B, dtype = STEP_CASES[case]
    rng, tabs, idx_np, x_np, idx = _hot_inputs(rows, D, B, 1, dtype, gpu, B + D)
    tabs_dev = dev_tables(tabs, gpu, dtype)  # (kept as they are: the forward's reference reads them)
    hp = pkg.HotPath(pkg.EmbeddingTableSet([t.clone() for t in tabs_dev]), B, 1, lr=0.5, index_base=0, pad_to=8)
    assert hp.step_api and hp.padding > 0
    F, W0 = hp.F, hp.width - hp.padding
    dout_np = rng.standard_normal((B, W0)).astype(np.float32)
    if dtype == BF16:
        dout_np = oracle.f32_to_bf16(dout_np)
    xb = _place(x_np, D + 8, 0, gpu)
    db = banded((B, hp.width), dtype, hp.width + 3, 0, gpu)  # padding columns stay NaN
    db.view[:, :W0].copy_(_to_dev(dout_np, gpu))
    db.snapshot()
    extra, lead = LAYOUTS[out_layout]
    ob = banded((B, hp.width), dtype, hp.width + extra, lead, gpu)
    dxb = banded((B, D), F32, D + 4, 0, gpu)       # (the split backward needs 16-B aligned dx and dt)
    dtb = banded((B, F * D), F32, F * D + 4, 0, gpu)
    hp.out, hp.dx, hp.dt = ob.view, dxb.view, dtb.view
    p = pkg.PackedIndices(idx)
    hp.step(xb.view, p, db.view)
    torch.cuda.synchronize()
    hp.check_bounds()
    # the forward: the operator pair on the tables before the step
    ys, ys_tables, out = _two_operators(pkg, tabs_dev, p, xb.view, D, 8)
    o = _vals(ob)
    assert np.array_equal(_bits(o), _bits(to_np_bits(out))), "step out != maplookup + DotInteraction"
    _check_fwd_out(o, x_np, ys_tables, _oracle_fwd(x_np, ys, F, hp.padding), D, F)
    # the backward and the update: a plain engine (pad_to = 1, its own contiguous buffers)
    ref = pkg.HotPath(pkg.EmbeddingTableSet([t.clone() for t in tabs_dev]), B, 1, lr=0.5, index_base=0)
    assert ref.step_api and ref.padding == 0
    ref.step(_to_dev(x_np, gpu), p, _to_dev(dout_np, gpu))
    torch.cuda.synchronize()
    ref.check_bounds()
    assert np.array_equal(_bits(to_np_bits(ref.out)), _bits(o[:, :W0]))
    dx, dt = _vals(dxb), _vals(dtb)
    assert np.array_equal(_bits(dx), _bits(to_np_bits(ref.dx))), "dx"
    m = _dt_written_mask(idx_np, D)
    assert np.isfinite(dt[m]).all()
    assert np.array_equal(_bits(dt)[m], _bits(to_np_bits(ref.dt))[m]), "dt rows of repeated table rows"
    for a, b in zip(hp.ts, ref.ts):
        assert np.array_equal(_bits(to_np_bits(a.data)), _bits(to_np_bits(b.data))), "tables"
    for band, what in ((ob, "out"), (dxb, "dx"), (dtb, "dt")):
        band.check(what=what)
    db.check(0, what="dout")
    xb.check(0, what="x")


def test_step_bwd_refuses_misaligned_dx(pkg, gpu):
    """The split backward needs 16-B aligned dx and dt (the header's rule): a dx displaced by one
    element is DLRM_E_ARG, and neither a table row nor dx / dt nor a guard is written."""
    rows, D, B, dtype = STEP_CASES["d32"]
    rng, tabs, idx_np, x_np, idx = _hot_inputs(rows, D, B, 1, dtype, gpu, 5)
    hp = pkg.HotPath(pkg.EmbeddingTableSet(dev_tables(tabs, gpu, dtype)), B, 1, lr=0.5, index_base=0, pad_to=8)
    assert hp.step_api
    x = _to_dev(x_np, gpu)
    dout = torch.randn((B, hp.width), device=gpu)
    dxb = banded((B, D), F32, D + 3, 1, gpu)  # row stride D + 4, base displaced by 4 bytes
    dtb = banded((B, hp.F * D), F32, hp.F * D + 4, 0, gpu)
    hp.dx, hp.dt = dxb.view, dtb.view
    p = pkg.PackedIndices(idx)
    hp.step_fwd(x, p)
    before = [to_np_bits(t.data).copy() for t in hp.ts]
    rc = hp.lib.dlrm_step_bwd(hp.ctx.bind(), hp.ts.handle, hp.indexer.handle, _vp(p.data), p.itype, p.stride, 0, B,
                              _vp(x), x.stride(0), _vp(dout), dout.stride(0), hp.padding, _vp(dxb.view), dxb.ld,
                              _vp(dtb.view), dtb.ld, 0.5, 0)
    torch.cuda.synchronize()
    assert rc == pkg._lib.E_ARG
    with pytest.raises(pkg.DLRMError):
        hp.step_bwd(dout)
    torch.cuda.synchronize()
    for t, b in zip(hp.ts, before):
        assert np.array_equal(_bits(to_np_bits(t.data)), _bits(b))
    dxb.check(0, what="dx")
    dtb.check(0, what="dt")
    hp.check_bounds()
    # the same build still serves an aligned call
    ok = banded((B, D), F32, D + 4, 0, gpu)
    hp.dx = ok.view
    hp.step_bwd(dout)
    torch.cuda.synchronize()
    hp.check_bounds()
    assert np.isfinite(_vals(ok)).all()
    ok.check(what="dx")
    dtb.check(what="dt")


# ------------------------------------------------------------------ 3. backward
BWD_SHAPES = [(128, 27, 9, F32), (16, 8, 7, F32), (32, 17, 6, BF16), (64, 33, 5, F32), (8, 100, 3, F32)]
BWD_PADDINGS = (0, 1, 33)


@functools.lru_cache(maxsize=None)
def _bwd_case(d, F, B, bf16, padding):
    """dout [B][W + padding] with NaN padding columns, and the oracle's dx, dt for it."""
    _, ref_ys = _fwd_ref(d, F, B, bf16, 0)  # ys after fast_vcat
    W = d + F * (F - 1) // 2
    rng = np.random.default_rng(d * 1000 + F + 1)
    g = rng.standard_normal((B, W)).astype(np.float32)
    if bf16:
        dout = np.full((B, W + padding), 0x7FC1, dtype=np.uint16)
        dout[:, :W] = oracle.f32_to_bf16(g)
    else:
        dout = np.full((B, W + padding), 0x7FC12345, dtype=np.uint32).view(np.float32)
        dout[:, :W] = g
    rdx, rdt = oracle.interact_bwd(dout, ref_ys, d, F, padding)
    assert np.isfinite(rdx).all() and np.isfinite(rdt).all()
    return _frozen(dout, ref_ys, rdx, rdt)


def _check_bwd(dx, dt, dout, ys, rdx, rdt, W, F):
    assert np.isfinite(dx).all() and np.isfinite(dt).all(), "a NaN reached dx / dt: dout was read past d + P"
    if dout.dtype == np.uint16:
        s = float(np.abs(rdt).max())
    else:
        s = float(np.abs(dout[:, :W]).max() * np.abs(ys).max() * F)
    assert_close(dt, rdt, rtol=2e-6, scale=s, what="dt")
    assert_close(dx, rdx, rtol=2e-6, scale=s, what="dx")


def _bwd_params():
    for d, F, B, dtype in BWD_SHAPES:
        for padding in BWD_PADDINGS:
            for dout_extra in (0, 3, 4):
                for layout in ("ld+4", "ld+1", "lead1"):
                    yield pytest.param(d, F, B, dtype, padding, dout_extra, layout,
                                       id=f"d{d}-F{F}-B{B}-{_name(dtype)}-pad{padding}-dout+{dout_extra}-{layout}")


@pytest.mark.parametrize("d,F,B,dtype,padding,dout_extra,layout", list(_bwd_params()))
def test_interact_bwd_padding_and_strided_buffers(pkg, gpu, d, F, B, dtype, padding, dout_extra, layout):
    """dlrm_interact_bwd through dot_back(..., dx=view, dt=view): a dout wider than d + P whose padding
    columns and surroundings are NaN, and dx / dt with an aligned larger leading dimension (the MFMA
    kernels) or an unaligned one (ld + 1, or a base displaced by one element: the scalar kernel)."""
    bf16 = dtype == BF16
    dout, ys, rdx, rdt = _bwd_case(d, F, B, bf16, padding)
    W = d + F * (F - 1) // 2
    db = _place(dout, W + padding + dout_extra, 0, gpu)
    yb = _place(ys, F * d, 0, gpu)
    extra, lead = LAYOUTS[layout]
    dxb = banded((B, d), F32, d + extra, lead, gpu)
    dtb = banded((B, F * d), F32, F * d + extra, lead, gpu)
    pkg.dot_back(pkg.DotInteraction(), db.view, yb.view, d, padding, dx=dxb.view, dt=dtb.view)
    torch.cuda.synchronize()
    _check_bwd(_vals(dxb), _vals(dtb), dout, _f32(ys), rdx, rdt, W, F)
    dxb.check(what="dx")
    dtb.check(what="dt")
    db.check(0, what="dout")
    yb.check(0, what="ys")


@pytest.mark.parametrize("layout", ["ld+4", "lead1"])
@pytest.mark.parametrize("padding", BWD_PADDINGS)
@pytest.mark.parametrize("d,F,B,dtype", BWD_SHAPES)
def test_gather_backward_padding_and_strided_buffers(pkg, gpu, d, F, B, dtype, padding, layout):
    """dlrm_interact_bwd_gather (hp.interact_bwd(dout, x=, idx=)) and dlrm_interact_bwd on the
    materialized ys, both with a NaN-padded strided dout and banded dx / dt, against the oracle.
    Bit equality between the two forms is asserted where test_ys_backward_equals_gather_backward
    promises it: 33 <= F <= 96 with the 16-B aligned layout (the split kernel's load plan and the
    re-gathering MFMA backward share their sums).  The displaced layout takes the scalar kernels,
    which are held to the oracle bar only."""
    T = F - 1
    rng = np.random.default_rng(T * 7 + d)
    rows = [int(r) for r in rng.integers(2, 500, T)]
    tabs = dev_tables(rand_tables(rng, rows, d), gpu, dtype)
    idx = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, 1)).reshape(T, B, 1).to(torch.int32).to(gpu))
    x_np = rng.standard_normal((B, d)).astype(np.float32)
    W = d + F * (F - 1) // 2
    g = rng.standard_normal((B, W)).astype(np.float32) * 1e-2
    if dtype == BF16:
        x_np, g = oracle.f32_to_bf16(x_np), oracle.f32_to_bf16(g)
    x = _to_dev(x_np, gpu)
    ts = pkg.EmbeddingTableSet(tabs)
    a = pkg.HotPath(ts, B, 1, index_base=0, fused=True, materialize_ys=True, deterministic=False)
    h = pkg.HotPath(ts, B, 1, index_base=0, fused=True, materialize_ys=False, deterministic=False)
    a.forward(x, idx)
    db = banded((B, W + padding), dtype, W + padding + 3, 0, gpu)
    db.view[:, :W].copy_(_to_dev(g, gpu))
    db.snapshot()
    extra, lead = LAYOUTS[layout]
    bands = []
    for hp in (a, h):
        hp.padding = padding  # (a plain attribute: any padding, not only what a pad_to yields)
        dxb = banded((B, d), F32, d + extra, lead, gpu)
        dtb = banded((B, F * d), F32, F * d + extra, lead, gpu)
        hp.dx, hp.dt = dxb.view, dtb.view
        bands.append((dxb, dtb))
    a.interact_bwd(db.view)
    h.interact_bwd(db.view, x=x, idx=idx)
    torch.cuda.synchronize()
    a.check_bounds()
    ys_np = np.ascontiguousarray(to_np_bits(a.ys))
    dout_np = np.ascontiguousarray(_vals(db))
    rdx, rdt = oracle.interact_bwd(dout_np, ys_np, d, F, padding)
    for (dxb, dtb), form in zip(bands, ("ys", "gather")):
        _check_bwd(_vals(dxb), _vals(dtb), dout_np, _f32(ys_np), rdx, rdt, W, F)
        dxb.check(what=f"dx ({form})")
        dtb.check(what=f"dt ({form})")
    db.check(0, what="dout")
    if 33 <= F <= 96 and layout == "ld+4":
        assert np.array_equal(bands[0][0].bits(), bands[1][0].bits())
        assert np.array_equal(bands[0][1].bits(), bands[1][1].bits())  # x row included


# ------------------------------------------------------------------ 4. lookup
LOOKUP_ROWS, LOOKUP_B = [5, 1000, 3, 77], 37
# (out_offset P, elements added to the leading dimension, elements before each row)
LOOKUP_FORMS = {"P13": (13, 0, 0), "P4": (4, 0, 0), "P16-ld+3": (16, 3, 0), "P16-lead1": (16, 0, 1)}


def _sentinel_np(shape, dtype):
    if dtype == BF16:
        return np.full(shape, 0x7FC1, dtype=np.uint16)
    return np.full(shape, 0x7FC12345, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("form", list(LOOKUP_FORMS))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("lookups", [1, 3])
@pytest.mark.parametrize("dim", [16, 128])
def test_lookup_out_offset_ld_and_alignment(pkg, gpu, dim, lookups, dtype, form):
    """maplookup(..., out=view): an out_offset that is not 16-B aligned (13 elements; 4 bf16 elements =
    8 bytes), an odd leading dimension, and a displaced base -- all maplookup_scalar; P = 4 in fp32 is
    16 bytes and stays on the vector kernel -- equal the oracle's lookup into an array of the same
    leading dimension bit for bit; columns [0, P) and the guards keep their bits."""
    rows, B = LOOKUP_ROWS, LOOKUP_B
    P, extra, lead = LOOKUP_FORMS[form]
    rng = np.random.default_rng(dim * 10 + lookups)
    tabs = dev_tables(rand_tables(rng, rows, dim), gpu, dtype)
    idx = rand_indices(rng, rows, B, lookups)
    width = P + dim * len(rows)
    ob = banded((B, width), dtype, width + extra, lead, gpu)
    got = pkg.maplookup(pkg.PreallocationStrategy(P), tabs, torch.from_numpy(idx).reshape(len(rows), B, lookups).to(gpu),
                        index_base=0, out=ob.view)
    torch.cuda.synchronize()
    assert got.data_ptr() == ob.view.data_ptr()
    ref = _sentinel_np((B, ob.ld), dtype)
    oracle.maplookup([np.ascontiguousarray(to_np_bits(t)) for t in tabs], idx, 0, B, lookups, ref, P)
    assert np.array_equal(_bits(_vals(ob)), _bits(ref[:, :width]))
    written = np.zeros((B, width), dtype=bool)
    written[:, P:] = True
    ob.check(written, what="out")


@pytest.mark.parametrize("lookups", [1, 3])
@pytest.mark.parametrize("dim", [16, 128])
def test_lookup_through_an_index_view(pkg, gpu, dim, lookups):
    """Indices as columns [1, 1 + B) of a packed [T][B + 8] int32 tensor: the index pointer is 4-B
    aligned only and table_stride > batch * lookups."""
    rows, B = LOOKUP_ROWS, LOOKUP_B
    rng = np.random.default_rng(dim + lookups)
    tabs = dev_tables(rand_tables(rng, rows, dim), gpu)
    idx = rand_indices(rng, rows, B, lookups)
    T = len(rows)
    wide = np.full((T, B + 8, lookups), 1 << 30, dtype=np.int32)  # (out of range: must not be read)
    wide[:, 1:1 + B] = idx.reshape(T, B, lookups)
    packed = pkg.PackedIndices(torch.from_numpy(wide).to(gpu))
    view = pkg.PackedIndices.columns(packed, 1, 1 + B)
    assert view.stride == (B + 8) * lookups and view.data.data_ptr() == packed.data.data_ptr() + 4 * lookups
    out = pkg.maplookup(pkg.PreallocationStrategy(dim), tabs, view, index_base=0)
    ref = np.zeros((B, dim * (T + 1)), dtype=np.float32)
    oracle.maplookup([to_np_bits(t) for t in tabs], idx, 0, B, lookups, ref, dim)
    assert np.array_equal(to_np_bits(out)[:, dim:], ref[:, dim:])


def test_prepare_through_an_index_view(pkg, gpu):
    """SparseIndexer.prepare at B = 2052 (above 2048 positions, B % 4 == 0: the scan build's class)
    on an index view whose pointer is 4-B aligned only and whose table stride is B + 8: the 16-B index
    loads do not apply, and the build in rounds must group the positions exactly."""
    rows, B = [3, 5000, 100000], 2052
    rng = np.random.default_rng(2052)
    idx = rand_indices(rng, rows, B, 1)
    T = len(rows)
    wide = np.full((T, B + 8), 1 << 30, dtype=np.int32)
    wide[:, 1:1 + B] = idx
    packed = pkg.PackedIndices(torch.from_numpy(wide).to(gpu))
    view = pkg.PackedIndices.columns(packed, 1, 1 + B)
    assert view.stride == B + 8 and view.data.data_ptr() % 16 == 4
    ts = pkg.EmbeddingTableSet([torch.zeros((n, 16), device=gpu) for n in rows])
    ix = pkg.SparseIndexer(T, B, gpu)
    assert ix.prepare(ts, view, index_base=0)
    torch.cuda.synchronize()
    _assert_segments(ix, idx, B)
    ts.ctx.check_bounds()


# ------------------------------------------------------------------ 5. Descent with bf16 / displaced gradients
UPD_ROWS = [2, 8, 40, 5000]
# (grad_offset, elements added to the leading dimension, elements before each row)
GRAD_FORMS = {"contig": (0, 0, 0), "off16-ld+8": (16, 8, 0), "off13": (13, 0, 0), "lead1": (0, 0, 1)}


@pytest.mark.parametrize("form", list(GRAD_FORMS))
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=lambda d: "g" + _name(d))
@pytest.mark.parametrize("tdtype", [F32, BF16], ids=lambda d: "t" + _name(d))
@pytest.mark.parametrize("B,L,prepared", [(1024, 1, False), (1024, 1, True), (256, 4, False)])
@pytest.mark.parametrize("D", [4, 16, 128])
def test_descent_grad_dtype_and_layout(pkg, gpu, D, B, L, prepared, tdtype, gdtype, form):
    """update!(Descent) with fp32 and bf16 gradients into fp32 and bf16 tables, from a gradient buffer
    with a grad_offset, a larger leading dimension, and a misaligned offset / base (the scalar apply
    kernels), with the indexer built by the update or prepared (the once-hit `singles` items).
    Gradients are integers in [-8, 8], tables multiples of 1/4 in [-4, 4], lr = 0.5: every fp32
    intermediate is exact in any summation order, so the result equals the oracle's bit for bit --
    for bf16 tables the exact fp32 value rounded once to nearest even."""
    rows, T = UPD_ROWS, len(UPD_ROWS)
    off, extra, lead = GRAD_FORMS[form]
    rng = np.random.default_rng(D * 100 + B + L)
    tabs = [(rng.integers(-16, 17, size=(n, D)) / 4.0).astype(np.float32) for n in rows]
    idx = rand_indices(rng, rows, B, L)
    g = rng.integers(-8, 9, size=(B, T * D)).astype(np.float32)
    width = off + T * D
    grad = _sentinel_np((B, width), gdtype)  # columns [0, grad_offset): NaN, never read
    grad[:, off:] = oracle.f32_to_bf16(g) if gdtype == BF16 else g
    ref = [oracle.f32_to_bf16(t) if tdtype == BF16 else t.copy() for t in tabs]
    start = [r.copy() for r in ref]
    oracle.sgd_update(ref, idx, 0, B, L, grad, off, 0.5)
    ts = pkg.EmbeddingTableSet(dev_tables(tabs, gpu, tdtype))
    for t, s in zip(ts, start):
        assert np.array_equal(_bits(to_np_bits(t.data)), _bits(s))  # (the tables are exact in bf16)
    gb = _place(grad, width + extra, lead, gpu)
    p = pkg.PackedIndices(torch.from_numpy(idx).reshape(T, B, L).to(torch.int32).to(gpu))
    ix = pkg.SparseIndexer(T, B * L, gpu)
    if prepared:
        assert ix.prepare(ts, p, index_base=0)
    pkg.update_(pkg.Descent(0.5), ts, pkg.maplookup_pullback(off, ts, p, gb.view), ix, index_base=0, prebuilt=prepared)
    torch.cuda.synchronize()
    for t in range(T):
        new = to_np_bits(ts[t].data)
        assert np.isfinite(_f32(new)).all()
        assert np.array_equal(_bits(new), _bits(ref[t])), f"table {t}"
        untouched = np.setdiff1d(np.arange(rows[t]), idx[t])
        assert np.array_equal(_bits(new[untouched]), _bits(start[t][untouched]))
    assert any(not np.array_equal(_bits(r), _bits(s)) for r, s in zip(ref, start))  # (the update did run)
    gb.check(0, what="grad")


# ------------------------------------------------------------------ 6. argument validation
def _arg_bands(d, F, B, padding, gpu):
    W = d + F * (F - 1) // 2
    return dict(x=banded((B, d), F32, d, 0, gpu), ys=banded((B, F * d), F32, F * d, 0, gpu),
                out=banded((B, W + padding), F32, W + padding, 0, gpu), dx=banded((B, d), F32, d, 0, gpu),
                dt=banded((B, F * d), F32, F * d, 0, gpu))


def _all_intact(bands):
    torch.cuda.synchronize()
    for name, b in bands.items():
        b.check(0, what=name)


def test_interact_leading_dimensions_one_short(pkg, gpu):
    """dlrm_interact_fwd / dlrm_interact_bwd: a leading dimension one less than the row needs, or a
    negative padding, is DLRM_E_ARG before any launch (every buffer keeps its bits)."""
    _lib = pkg._lib
    d, F, B, padding = 16, 8, 7, 4
    W = d + F * (F - 1) // 2
    ctx = pkg.runtime.context(gpu)
    bands = _arg_bands(d, F, B, padding, gpu)
    x, ys, out, dx, dt = (bands[k] for k in ("x", "ys", "out", "dx", "dt"))

    def fwd(x_ld=d, ys_ld=F * d, out_ld=W + padding, pad=padding):
        return ctx.lib.dlrm_interact_fwd(ctx.bind(), _lib.F32, d, F, B, _vp(x.view), x_ld, _vp(ys.view), ys_ld,
                                         _vp(out.view), out_ld, pad)

    def bwd(dout_ld=W + padding, t_ld=F * d, dx_ld=d, dt_ld=F * d, pad=padding):
        return ctx.lib.dlrm_interact_bwd(ctx.bind(), _lib.F32, d, F, B, _vp(out.view), dout_ld, pad, _vp(ys.view), t_ld,
                                         _vp(dx.view), dx_ld, _vp(dt.view), dt_ld)

    assert fwd(out_ld=W + padding - 1) == _lib.E_ARG
    assert fwd(x_ld=d - 1) == _lib.E_ARG
    assert fwd(ys_ld=F * d - 1) == _lib.E_ARG
    assert fwd(pad=-1) == _lib.E_ARG
    assert bwd(dout_ld=W + padding - 1) == _lib.E_ARG
    assert bwd(dt_ld=F * d - 1) == _lib.E_ARG
    assert bwd(dx_ld=d - 1) == _lib.E_ARG
    assert bwd(t_ld=F * d - 1) == _lib.E_ARG
    assert bwd(pad=-1) == _lib.E_ARG
    _all_intact(bands)


def test_step_fwd_leading_dimensions_one_short(pkg, gpu):
    _lib = pkg._lib
    rows, D, B, padding = [10, 3000, 7], 16, 9, 2
    T, F = len(rows), len(rows) + 1
    W = D + F * (F - 1) // 2
    ts = pkg.EmbeddingTableSet([torch.zeros((n, D), device=gpu) for n in rows])
    ix = pkg.SparseIndexer(T, B, gpu)
    idx = torch.zeros((T, B), dtype=torch.int32, device=gpu)
    bands = _arg_bands(D, F, B, padding, gpu)
    x, out = bands["x"], bands["out"]
    ctx = ts.ctx

    def step_fwd(x_ld=D, out_ld=W + padding, pad=padding):
        return ctx.lib.dlrm_step_fwd(ctx.bind(), ts.handle, ix.handle, _vp(idx), _lib.I32, B, 0, B, _vp(x.view), x_ld,
                                     _vp(out.view), out_ld, pad)

    assert step_fwd(out_ld=W + padding - 1) == _lib.E_ARG
    assert step_fwd(x_ld=D - 1) == _lib.E_ARG
    assert step_fwd(pad=-1) == _lib.E_ARG
    assert not ix.state() & _lib.IX_BUILT
    _all_intact(bands)
    for t in ts:
        assert not t.data.any()
