"""The interaction family, bit for bit, on inputs whose sums are exact in any order.

Why no tolerance is needed.  Every input element here is an integer times a power of two.  If, for
one output element, the sum of the magnitudes of its terms, sum_k |a_k * b_k| (in units of the common
power of two), is below 2^24, then every partial sum of every subset of the terms, taken in any
order and with any grouping (an fmaf chain, the MFMA's k order, parity partials added at the end), is
an integer below 2^24 in magnitude and so a float32 value: no step rounds, and the result is one bit
pattern whatever the kernel's summation order.  (`v_mfma_f32_16x16x4_f32` is an fmaf chain; the bf16
MFMA multiplies bf16 operands exactly and accumulates in fp32, so there are no bits to lose either.)
A bf16 output is that exact value rounded to nearest even exactly once (oracle.f32_to_bf16).  The
reference is plain numpy on int64 / float64 in this module (_gram, _ref_bwd, _ref_step): not the C
oracle and not the code under test.  fp32 results are compared with np.array_equal on the values
(-0 == +0) plus a NaN check, bf16 results on their uint16 bits with +-0 equal.

Input families (all seeded, _rows):
  small     integers in [-8, 8] ([-16, 16] where d <= 16); dout integers in [-8, 8].  Both dtypes,
            every entry point.  sum |a b| <= 256 * 16^2 < 2^24.  In bf16 its point is TIES: an exact
            value whose fp32 low half is 0x8000 (257 -> 256, 259 -> 260).  Conditions, asserted by the
            CPU test on the reference alone: every bf16 forward case with d >= 64 has >= 50 tie
            elements among its pairs, with one rounding down and one up (which separates nearest-even
            from half-away and from truncation); all bf16 forward cases together have >= 1000.  The
            reference produced 14130 ties over the bf16 DotInteraction cases (d=128 F=27 B=5: 278 ties
            in 1755 pairs, 140 down and 138 up; d=256 F=33 B=5: 567 in 2640; d=8 F=17 B=5: 106 in 680;
            d=64 F=16 B=9: 81 in 1080, the fewest of a d >= 64 case); test_fixtures_on_the_cpu prints
            every case's counts (pytest -s).
  wide      fp32 only.  Every third feature row (index % 3 == 0, x included) holds integers in
            [-2047, 2047] (11-12 significant bits: more than a bf16 or tf32-like operand keeps), the
            others integers in [-7, 7].  Forward: an element is compared exactly iff
            sum_k |t_ik t_jk| < 2^24 (int64); the CPU test asserts that the elements left out are
            exactly the wide x wide pairs (36 of 351 at F = 27; at most 12 % of a case's pairs, 11.6 %
            at F = 49) and that every wide x narrow pair is in.  The wide x wide pairs keep the
            assert_close bar of test_interaction_fwd_bwd_vs_oracle.  Backward, nothing left out:
            `wide_dout` (|dout| <= 2047, small T) and `wide_t` (small dout, wide T);
            sum <= 113 * 16 * 2047 < 2^24.
  selector  fp32 only, forward and self_batched_mul.  Odd feature rows have one nonzero element,
            +-2^e with e in [-3, 3], at a seeded column (the columns of a case cover 0..d-1, the last
            one included); even rows (x included) are standard_normal float32.  Z[normal][selector] =
            +-2^e t[k] exactly, with a full 24-bit mantissa; Z[selector][selector] is 0 or a power of
            two.  Those pairs are compared bit for bit (no operand bit lost, the right k of the right
            pair); normal x normal pairs with assert_close.

Which shape reaches which kernel (the rule: DESIGN.md section 22 and csrc/interact_plan.hpp, held row by row by
tests/test_interact_plan_host.py; below, the shapes this module picks from it.  NB = ceil(F / 16) 16-row blocks;
B in {1, 5, 9}: one sample, and a four-sample workgroup plus a tail):
  dlrm_interact_fwd         interact_fwd_kernel<NB = 1..6> for F in {2, 16 | 17, 27, 32 | 33 | 49 | 65 |
                            81, 96}; d = 128: the kernel compiled for it (pad_to = 8 or 64 there:
                            padding columns); d = 256;
                            column tails: fp32 d in {4, 20, 36} (16 columns per MFMA step), bf16 d in
                            {8, 24, 40, 48, 72} (32 per step).  interact_fwd_scalar: F = 97 (NB = 7),
                            fp32 d = 6 / bf16 d = 12 (not a multiple of the 16-B vector), x_ld = d + 1.
  dlrm_lookup_interact_fwd  one-hot T = 26 (NB = 2, table pointers by value) and T = 40 (NB = 3), d in
                            {32, 128}; pooled 7 tables x L = 9 (the pooled fused kernel), L = 10 (the
                            two-launch form) and the ABI call with ys = NULL at L = 10.
  dlrm_step_fwd / _bwd      T = 26, d = 32 (the d <= 64 split branch) and d = 128, B in {5, 70},
                            lr = 2^-4, table elements k/4: out, dx, the dt rows of _dt_written_mask and
                            the TABLES after the step (once-hit rows stepped inside the backward,
                            repeated rows by the apply) equal fmaf(-lr, G, w) computed exactly; bf16
                            tables: that value rounded once.
  dlrm_interact_bwd         interact_bwd_kernel (one wave per sample) at NB = 1, 2, 7 (F in {2, 16, 27,
                            100}) and at NB 3..6 with (d, F) = (32, 40), (16, 65); the split load plan
                            (interact_bwd_split_kernel<YS>) at (64, 33), (128, 49), (256, 65), (128, 96);
                            interact_bwd_scalar: F = 113 (NB = 8), d = 6, a dt of leading dimension + 1.
  dlrm_interact_bwd_gather  T = 26 with the indexer built in the same launch
                            (interact_bwd_index_kernel), T = 40 (the indexer's own launch), d in
                            {16, 128}; then _assert_segments on that indexer.
  dlrm_interact_bwd_blocked d in {64, 128}, T = 26 (interact_bwd_split_kernel<MAPPED>): dx and the rows
                            in the send layout.
  dlrm_self_batched_mul     (F, d) in {(8, 16), (27, 128), (90, 8)}, diagonal included; `_back` on
                            the small family.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

import oracle
from helpers import _assert_segments, _dt_written_mask, assert_close, to_np_bits

gpu_test = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EXACT = float(1 << 24)


def _name(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------ the reference (int64 / float64)
def _pairs(F):
    """(i, j), j < i, in the order of out's pair columns: i = 1..F-1, j = 0..i-1."""
    return np.tril_indices(F, -1)


def _gram(T):
    """T [B][F][d] (int64, or float64 for the selector family) -> Z = T T^T and the bound
    A = |T| |T|^T = sum_k |t_ik t_jk| per element, [B][F][F] each."""
    return T @ T.transpose(0, 2, 1), np.abs(T) @ np.abs(T).transpose(0, 2, 1)


def _ref_bwd(dout, T):
    """dot_back: S = symmetric zero-diagonal unpack of dout's pair columns, dt = S T ([B][F][d]),
    dx = dout[:, :d] + dt[:, 0].  Returns dx, dt and the largest sum of term magnitudes."""
    B, F, d = T.shape
    i, j = _pairs(F)
    S = np.zeros((B, F, F), dtype=dout.dtype)
    S[:, i, j] = dout[:, d:]
    S[:, j, i] = dout[:, d:]
    dt = S @ T
    bound = np.abs(S) @ np.abs(T)
    bound[:, 0] += np.abs(dout[:, :d])
    return dout[:, :d] + dt[:, 0], dt, bound.max() if bound.size else 0


def _f32_exact(v, what=""):
    """An exactly representable float64 / int64 array as float32."""
    v = np.asarray(v)
    f = v.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v.astype(np.float64)), f"{what}: not representable in float32"
    return f


def _bf16_exact(v, what=""):
    f = _f32_exact(v, what)
    h = oracle.f32_to_bf16(f)
    assert np.array_equal(oracle.bf16_to_f32(h), f), f"{what}: not representable in bf16"
    return h


def _is_tie(f):
    """float32 values halfway between two bf16 values"""
    return (np.ascontiguousarray(f, dtype=np.float32).view(np.uint32) & 0xFFFF) == 0x8000


def _tie_counts(exact):
    """(ties, ties rounded down in magnitude, ties rounded up) of exact float32 values under
    round-to-nearest-even"""
    f = np.ascontiguousarray(exact, dtype=np.float32)
    tie = _is_tie(f)
    up = tie & ((oracle.f32_to_bf16(f) & 0x7FFF) > (f.view(np.uint32) >> 16 & 0x7FFF))
    return int(tie.sum()), int((tie & ~up).sum()), int(up.sum())


# ------------------------------------------------------------------ comparing
def assert_f32_equal(got, want, what, where=None):
    """got (float32 from the device) == want (exact, float64 / int64) as values; no NaN (`where`:
    among those elements only)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(want), (what, got.dtype, got.shape, np.shape(want))
    w = _f32_exact(want, what)
    sel = np.ones(got.shape, dtype=bool) if where is None else where
    assert not (sel & np.isnan(got)).any(), f"{what}: NaN"
    bad = sel & (got != w)
    if bad.any():
        at = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(sel.sum())} elements differ, first at {at}: "
                             f"got {got[at]!r}, exact {w[at]!r}")


def assert_bf16_equal(got, want, what):
    """got (uint16 bf16 bits from the device) == the exact `want` rounded once to nearest even, bit
    for bit, except that +-0 are equal."""
    got = np.asarray(got)
    assert got.dtype == np.uint16 and got.shape == np.shape(want), (what, got.dtype, got.shape, np.shape(want))
    w = oracle.f32_to_bf16(_f32_exact(want, what))
    bad = (got != w) & (((got | w) & 0x7FFF) != 0)
    if bad.any():
        at = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements differ, first at {at}: got "
                             f"0x{int(got[at]):04x}, exact {np.asarray(want)[at]!r} -> 0x{int(w[at]):04x}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _host(v, dtype, what=""):
    """exact values -> what the device holds: float32, or uint16 bf16 bits"""
    return _bf16_exact(v, what) if dtype == BF16 else _f32_exact(v, what)


def _dev(a, gpu):
    a = np.array(a, order="C")
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(gpu).view(BF16)
    return torch.from_numpy(a).to(gpu)


def _nan_filled(shape, dtype, gpu):
    return torch.full(shape, float("nan"), dtype=dtype, device=gpu)


# ------------------------------------------------------------------ the input families
def _amp(d):
    return 16 if d <= 16 else 8


@functools.lru_cache(maxsize=None)
def _rows(family, d, F, B):
    """The feature rows T [B][F][d] of a case (row 0: x): int64, or float64 for `selector`."""
    rng = _rng(family, d, F, B)
    if family == "small":
        a = _amp(d)
        return _frozen(rng.integers(-a, a + 1, size=(B, F, d)))
    if family == "wide":
        T = rng.integers(-7, 8, size=(B, F, d))
        T[:, ::3] = rng.integers(-2047, 2048, size=T[:, ::3].shape)
        return _frozen(T)
    assert family == "selector"
    T = rng.standard_normal((B, F, d)).astype(np.float32).astype(np.float64)
    nsel = F // 2
    cols = np.resize(rng.permutation(d), B * nsel).reshape(B, nsel)  # cycles through every column
    vals = rng.choice([-1.0, 1.0], size=(B, nsel)) * 2.0 ** rng.integers(-3, 4, size=(B, nsel))
    T[:, 1::2] = 0.0
    b, s = np.meshgrid(np.arange(B), np.arange(nsel), indexing="ij")
    T[b, 2 * s + 1, cols] = vals
    return _frozen(T)


def _selector_columns(T):
    return np.unique(np.nonzero(T[:, 1::2])[2])


@functools.lru_cache(maxsize=None)
def _fwd_ref(family, d, F, B):
    """(exact pair values [B][P] float64, which of them are compared bit for bit [B][P] or [P])."""
    T = _rows(family, d, F, B)
    Z, A = _gram(T)
    i, j = _pairs(F)
    if family == "selector":
        exact = np.broadcast_to((i % 2 == 1) | (j % 2 == 1), (B, len(i))).copy()
    else:
        exact = A[:, i, j] < (1 << 24)
    return _frozen(Z[:, i, j].astype(np.float64), exact)


def _wide_pairs(F):
    i, j = _pairs(F)
    return (i % 3 == 0) & (j % 3 == 0), (i % 3 == 0) ^ (j % 3 == 0)


def _check_pairs(got, family, d, F, B, dtype, what):
    """The pair columns of an output against the reference, under the family's rule."""
    want, exact = _fwd_ref(family, d, F, B)
    if dtype == BF16:
        assert exact.all()
        assert_bf16_equal(got, want, what)
        return
    assert_f32_equal(got, np.where(exact, want, 0.0), what, where=exact)
    if not exact.all():  # wide x wide, normal x normal: the bar of test_interaction_fwd_bwd_vs_oracle
        scale = float(np.abs(_rows(family, d, F, B)).max() ** 2 * d)
        assert_close(got[~exact], want[~exact], rtol=2e-6, scale=scale, what=what + " (inexact pairs)")


# ------------------------------------------------------------------ dlrm_interact_fwd cases
# (family, d, F, B, pad_to, x_ld - d)
def _fwd(family, shapes):
    return [(family,) + s + (1, 0)[len(s) - 3:] for s in shapes]


FWD_F32 = _fwd("small", [
    (4, 2, 5), (128, 2, 1, 8), (20, 16, 9), (64, 16, 5),                        # NB = 1
    (36, 17, 5), (128, 27, 5, 8), (256, 17, 1), (128, 17, 9, 64),                # NB = 2
    (20, 33, 5), (256, 33, 5), (128, 33, 1, 64),                                 # NB = 3
    (4, 49, 9), (64, 49, 5), (36, 49, 1),                                       # NB = 4
    (36, 65, 5), (128, 65, 5, 64),                                               # NB = 5
    (20, 81, 1), (256, 81, 1), (4, 96, 5), (64, 96, 9),                         # NB = 6
    (8, 97, 5), (64, 97, 1), (6, 5, 9), (6, 27, 1), (128, 27, 5, 8, 1)]) + _fwd("wide", [   # the scalar kernel
    (36, 17, 5), (128, 27, 5, 8), (256, 33, 5), (64, 49, 9), (128, 65, 1, 64), (64, 81, 5), (256, 96, 1),
    (64, 97, 1), (128, 27, 5, 8, 1)]) + _fwd("selector", [
    (4, 2, 5), (20, 17, 5), (128, 32, 9, 64), (128, 33, 9, 64), (36, 49, 5), (256, 65, 9), (64, 81, 5),
    (128, 96, 5, 64), (6, 97, 1), (128, 32, 9, 64, 1)])
FWD_BF16 = _fwd("small", [
    (8, 2, 5), (16, 8, 9), (24, 16, 5), (64, 16, 9), (72, 16, 9),               # NB = 1
    (8, 17, 5), (40, 17, 9), (128, 27, 5, 8), (256, 17, 5), (48, 27, 1), (128, 17, 9, 64),   # NB = 2
    (24, 33, 5), (256, 33, 5), (128, 33, 1, 64),                                 # NB = 3
    (48, 49, 1), (64, 49, 5), (8, 49, 9),                                       # NB = 4
    (72, 65, 5), (128, 65, 1, 64), (40, 65, 1),                                  # NB = 5
    (24, 81, 1), (256, 81, 1), (8, 96, 5), (64, 96, 1),                         # NB = 6
    (8, 97, 5), (64, 97, 1), (12, 5, 9), (12, 27, 5), (128, 27, 5, 8, 1)])      # the scalar kernel
FWD_CASES = [(F32,) + c for c in FWD_F32] + [(BF16,) + c for c in FWD_BF16]


def _fwd_id(c):
    dtype, family, d, F, B, pad_to, x_extra = c
    pad, x_ld = f"-pad{pad_to}" if pad_to > 1 else "", "-x_ld+1" if x_extra else ""
    return f"{_name(dtype)}-{family}-d{d}-F{F}-B{B}{pad}{x_ld}"


def _check_out(o, x_host, d, F, what):
    """out == [x (bits) | pairs (checked by the caller) | zero bits]; returns the pair columns."""
    P = F * (F - 1) // 2
    assert np.array_equal(_bits(o[:, :d]), _bits(x_host)), f"{what}: out[:, :d] is not x's bits"
    assert not _bits(o[:, d + P:]).any(), f"{what}: padding columns are not all-zero bits"
    return o[:, d:d + P]


@gpu_test
@pytest.mark.parametrize("case", FWD_CASES, ids=_fwd_id)
def test_interact_fwd_exact(pkg, gpu, case):
    """DotInteraction(pad_to)(x, ys, out=) on exactly summable inputs: the pairs bit for bit (bf16:
    the exact value rounded once to nearest even), out[:, :d] x's bits, ys after fast_vcat, zero bits
    in the padding columns."""
    dtype, family, d, F, B, pad_to, x_extra = case
    T = _rows(family, d, F, B)
    x_host = _host(T[:, 0], dtype, "x")
    ys_host = _host(T.reshape(B, F * d), dtype, "ys")
    ys0 = ys_host.copy()
    ys0[:, :d] = _host(np.full((B, d), 3.0), dtype)  # fast_vcat must overwrite this with x
    x = _nan_filled((B, d + x_extra), dtype, gpu)[:, :d]
    x.copy_(_dev(x_host, gpu))
    ys = _dev(ys0, gpu)
    _, W, padding = pkg.interact.interaction_sizes(d, F, pad_to)
    assert (padding > 0) == (pad_to > 1)
    out = _nan_filled((B, W), dtype, gpu)
    got = pkg.DotInteraction(pad_to=pad_to)(x, ys, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(_bits(to_np_bits(ys)), _bits(ys_host)), "ys after fast_vcat"
    what = "interact_fwd " + _fwd_id(case)
    _check_pairs(_check_out(to_np_bits(out), x_host, d, F, what), family, d, F, B, dtype, what)


# ------------------------------------------------------------------ tables and indices of the fused forms
@functools.lru_cache(maxsize=None)
def _table_case(T, d, B, L, unit):
    """Tables of 3..50 rows (so rows repeat inside a batch) of `small` integers (in units of
    `unit`: table value = k * unit), indices [T][B*L], x.  Returns (tables int64, idx, x int64)."""
    rng = _rng("tables", T, d, B, L)
    nrows = rng.integers(3, 51, size=T)
    nrows[0], nrows[-1] = 3, 50
    a = 16 if unit != 1 else _amp(d)
    tabs = [rng.integers(-a, a + 1, size=(int(n), d)) for n in nrows]
    idx = np.stack([rng.integers(0, n, size=B * L) for n in nrows])
    x = rng.integers(-a, a + 1, size=(B, d))
    return tuple(_frozen(*tabs)), _frozen(idx), _frozen(x)


def _gathered(tabs, idx, x, B, L, dtype):
    """The feature rows [B][F][d] the forward multiplies: x, then each table's bag sum (bf16: rounded
    once, as the pooled lookup stores it; exact sums here)."""
    rows = [x]
    for t, tab in enumerate(tabs):
        bag = tab[idx[t]].reshape(B, L, -1).sum(axis=1)
        if dtype == BF16:
            bag = oracle.bf16_to_f32(oracle.f32_to_bf16(_f32_exact(bag))).astype(np.int64)
        rows.append(bag)
    return np.stack(rows, axis=1)


def _engine_inputs(pkg, gpu, T, d, B, L, dtype, unit=1.0):
    tabs, idx, x = _table_case(T, d, B, L, unit)
    tabs_dev = [_dev(_host(t * unit, dtype, "table"), gpu) for t in tabs]
    p = pkg.PackedIndices(torch.from_numpy(idx.copy()).to(torch.int32).reshape(T, B, L).to(gpu))
    x_host = _host(x * unit, dtype, "x")
    return tabs, idx, x, tabs_dev, p, x_host


def _check_fwd_exact(o, Tm, x_host, dtype, what):
    """out of a fused forward against the integer reference of the gathered rows Tm."""
    B, F, d = Tm.shape
    got = _check_out(o, x_host, d, F, what)
    Z, A = _gram(Tm)
    i, j = _pairs(F)
    assert A.max() < EXACT
    if dtype == BF16:
        assert_bf16_equal(got, Z[:, i, j], what)
    else:
        assert_f32_equal(got, Z[:, i, j], what)


FUSED_CASES = [(T, d, B, 1, dtype, "hp") for T in (26, 40) for d, B in ((32, 9), (128, 5)) for dtype in (F32, BF16)] + \
              [(7, 16, 9, L, dtype, form) for L, form in ((9, "hp"), (10, "hp"), (10, "no-ys")) for dtype in (F32, BF16)]


@gpu_test
@pytest.mark.parametrize("T,d,B,L,dtype,form", FUSED_CASES,
                         ids=[f"T{c[0]}-d{c[1]}-B{c[2]}-L{c[3]}-{_name(c[4])}-{c[5]}" for c in FUSED_CASES])
def test_fused_forward_exact(pkg, gpu, T, d, B, L, dtype, form):
    """dlrm_lookup_interact_fwd (HotPath(fused=True).forward, pad_to = 8; `no-ys`: the ABI call with
    ys = NULL): out and ys against the integer reference of the gathered (pooled: summed) rows."""
    tabs, idx, x, tabs_dev, p, x_host = _engine_inputs(pkg, gpu, T, d, B, L, dtype)
    hp = pkg.HotPath(pkg.EmbeddingTableSet(tabs_dev), B, L, index_base=0, fused=True, materialize_ys=True, pad_to=8)
    hp.out.fill_(float("nan"))
    hp.ys.fill_(float("nan"))
    xd = _dev(x_host, gpu)
    hp.validate(xd, p)
    if form == "no-ys":
        rc = hp.lib.dlrm_lookup_interact_fwd(hp.ctx.bind(), hp.ts.handle, ctypes.c_void_p(p.data.data_ptr()), p.itype,
                                             p.stride, 0, B, L, ctypes.c_void_p(xd.data_ptr()), xd.stride(0), None, 0,
                                             ctypes.c_void_p(hp.out.data_ptr()), hp.out.stride(0), hp.padding)
        assert rc == pkg._lib.OK
    else:
        hp.forward(xd, p)
    torch.cuda.synchronize()
    hp.check_bounds()
    Tm = _gathered(tabs, idx, x, B, L, dtype)
    _check_fwd_exact(to_np_bits(hp.out), Tm, x_host, dtype, "fused forward out")
    if form != "no-ys":
        want_ys = Tm.reshape(B, -1)
        if dtype == BF16:
            assert_bf16_equal(to_np_bits(hp.ys), want_ys, "fused forward ys")
        else:
            assert_f32_equal(to_np_bits(hp.ys), want_ys, "fused forward ys")


# ------------------------------------------------------------------ the training step
LR = 2.0 ** -4
UNIT = 0.25


def _ref_step(tabs, idx, x, dout, B):
    """One step on tables k/4, x k/4, integer dout, lr = 2^-4, in float64 (exact: every value is an
    integer times 2^-6 far below 2^53): out's pairs, dx, dt, the tables after the step."""
    Tm = _gathered(tabs, idx, x, B, 1, F32).astype(np.float64) * UNIT
    Z, A = _gram(Tm)
    assert A.max() * 16 < EXACT  # (in units of 1/16)
    dx, dt, bound = _ref_bwd(dout.astype(np.float64), Tm)
    assert bound * 4 < EXACT
    new = []
    for t, tab in enumerate(tabs):
        G = np.zeros(tab.shape)
        np.add.at(G, idx[t], dt[:, t + 1])
        Gabs = np.zeros(tab.shape)
        np.add.at(Gabs, idx[t], np.abs(dt[:, t + 1]))
        assert Gabs.max() * 4 < EXACT  # G's partial sums, in units of 1/4
        new.append(tab * UNIT - LR * G)
        assert np.abs(new[-1]).max() * 64 < EXACT  # fmaf(-lr, G, w), in units of 1/64
    i, j = _pairs(Tm.shape[1])
    return Z[:, i, j], dx, dt.reshape(B, -1), new


@gpu_test
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("d,B", [(32, 5), (32, 70), (128, 5), (128, 70)])
def test_step_exact(pkg, gpu, d, B, dtype):
    """dlrm_step_fwd + dlrm_step_bwd (HotPath.step), T = 26: out, dx, the dt rows the apply reads and
    the tables after the step -- once-hit rows (stepped inside the backward) and repeated rows (the
    apply) -- against the integer reference; bf16 out and tables: the exact value rounded once."""
    T = 26
    tabs, idx, x, tabs_dev, p, x_host = _engine_inputs(pkg, gpu, T, d, B, 1, dtype, UNIT)
    F = T + 1
    dout = _rng("step dout", d, B).integers(-8, 9, size=(B, d + F * (F - 1) // 2))
    hp = pkg.HotPath(pkg.EmbeddingTableSet(tabs_dev), B, 1, lr=LR, index_base=0)
    assert hp.step_api
    hp.out.fill_(float("nan"))
    hp.dt.fill_(float("nan"))
    xd, dd = _dev(x_host, gpu), _dev(_host(dout, dtype, "dout"), gpu)
    hp.validate(xd, p, dd)
    hp.step(xd, p, dd)
    torch.cuda.synchronize()
    hp.check_bounds()
    pairs, dx, dt, new = _ref_step(tabs, idx, x, dout, B)
    eq = assert_bf16_equal if dtype == BF16 else assert_f32_equal
    eq(_check_out(to_np_bits(hp.out), x_host, d, F, "step out"), pairs, "step out")
    assert_f32_equal(to_np_bits(hp.dx), dx, "step dx")
    m = _dt_written_mask(idx, d)
    once = sum(int((np.bincount(idx[t]) == 1).sum()) for t in range(T))
    assert once > 0 and m.any(), "the case needs once-hit and repeated rows"
    assert_f32_equal(to_np_bits(hp.dt), np.where(m, dt, 0.0), "step dt", where=m)
    for t in range(T):
        eq(to_np_bits(hp.ts[t].data), new[t], f"table {t} after the step")


# ------------------------------------------------------------------ dlrm_interact_bwd
# (d, F, B, dt_ld - F d)
BWD_SHAPES = [(16, 2, 5, 0), (128, 16, 9, 0), (128, 27, 5, 0), (32, 27, 1, 0), (8, 100, 5, 0), (64, 100, 1, 0),  # one wave
              (64, 33, 5, 0), (128, 49, 9, 0), (256, 65, 5, 0), (128, 96, 1, 0), (64, 81, 9, 0),   # the split load plan
              (32, 40, 5, 0), (16, 65, 9, 0), (32, 49, 1, 0), (16, 96, 5, 0),                      # one wave, NB 3..6
              (8, 113, 1, 0), (6, 5, 9, 0), (128, 27, 5, 1)]                                       # the scalar kernel
BWD_CASES = [(dtype, fam) + s for s in BWD_SHAPES
             for dtype, fam in ((F32, "small"), (BF16, "small"), (F32, "wide_dout"), (F32, "wide_t"))]


@functools.lru_cache(maxsize=None)
def _bwd_case(family, d, F, B):
    """(dout int64 [B][d + P], T int64 [B][F][d], exact dx, exact dt [B][F*d])"""
    T = _rows("wide" if family == "wide_t" else "small", d, F, B)
    a = 2047 if family == "wide_dout" else 8
    dout = _rng("dout", family, d, F, B).integers(-a, a + 1, size=(B, d + F * (F - 1) // 2))
    dx, dt, bound = _ref_bwd(dout, T)
    assert bound < (1 << 24), (family, d, F, bound)
    return _frozen(dout, T, dx, dt.reshape(B, F * d))


def _bwd_id(c):
    dtype, family, d, F, B, extra = c
    return f"{_name(dtype)}-{family}-d{d}-F{F}-B{B}" + ("-dt_ld+1" if extra else "")


@gpu_test
@pytest.mark.parametrize("case", BWD_CASES, ids=_bwd_id)
def test_interact_bwd_exact(pkg, gpu, case):
    """dot_back(dot, dout, t, d, 0, dx=, dt=): fp32 dx and dt, x rows included, bit for bit."""
    dtype, family, d, F, B, extra = case
    dout, T, dx, dt = _bwd_case(family, d, F, B)
    dd = _dev(_host(dout, dtype, "dout"), gpu)
    td = _dev(_host(T.reshape(B, F * d), dtype, "t"), gpu)
    dxb = _nan_filled((B, d), F32, gpu)
    dtb = _nan_filled((B, F * d + extra), F32, gpu)[:, :F * d]
    pkg.dot_back(pkg.DotInteraction(), dd, td, d, 0, dx=dxb, dt=dtb)
    torch.cuda.synchronize()
    assert_f32_equal(to_np_bits(dtb), dt, "dt " + _bwd_id(case))
    assert_f32_equal(to_np_bits(dxb), dx, "dx " + _bwd_id(case))


# ------------------------------------------------------------------ dlrm_interact_bwd_gather / _blocked
@gpu_test
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("T,d,B", [(26, 16, 9), (26, 128, 5), (40, 16, 5), (40, 128, 9)])
def test_gather_backward_exact(pkg, gpu, T, d, B, dtype):
    """dlrm_interact_bwd_gather with an indexer (T = 26: built in the backward's launch; T = 40: its
    own launch): dx, dt bit for bit, and the indexer it built groups the positions exactly."""
    tabs, idx, x, tabs_dev, p, x_host = _engine_inputs(pkg, gpu, T, d, B, 1, dtype)
    F = T + 1
    dout = _rng("gather dout", T, d, B).integers(-8, 9, size=(B, d + F * (F - 1) // 2))
    hp = pkg.HotPath(pkg.EmbeddingTableSet(tabs_dev), B, 1, index_base=0, materialize_ys=False)
    assert not hp.materialize_ys and hp.indexer is not None
    hp.dx.fill_(float("nan"))
    hp.dt.fill_(float("nan"))
    hp.interact_bwd(_dev(_host(dout, dtype, "dout"), gpu), x=_dev(x_host, gpu), idx=p, build_indexer=True)
    torch.cuda.synchronize()
    hp.check_bounds()
    dx, dt, bound = _ref_bwd(dout, _gathered(tabs, idx, x, B, 1, dtype))
    assert bound < (1 << 24)
    assert_f32_equal(to_np_bits(hp.dx), dx, "gather backward dx")
    assert_f32_equal(to_np_bits(hp.dt), dt.reshape(B, -1), "gather backward dt")
    _assert_segments(hp.indexer, idx, B)


@gpu_test
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("d,B", [(64, 9), (128, 5)])
def test_blocked_backward_exact(pkg, gpu, d, B, dtype):
    """dlrm_interact_bwd_blocked (HipShardOps.interact_bwd_send on received [B][D] blocks, identity
    indices), T = 26 over two owners: dx, and every table's dt rows where the send layout
    [owner][B][T_owner][D] puts them; nothing else of the send buffer is written."""
    from dlrm_jl_amd.sharded import HipShardOps
    T = 26
    F = T + 1
    rng = _rng("blocked", d, B)
    a = _amp(d)
    blocks = rng.integers(-a, a + 1, size=(T, B, d))  # table t's row b: sample b's vector
    x = rng.integers(-a, a + 1, size=(B, d))
    dout = rng.integers(-8, 9, size=(B, d + F * (F - 1) // 2))
    owners = [list(range(0, 11)), list(range(11, T))]
    base, ld, off = [0] * T, [0] * T, 0
    for tabs in owners:
        for k, t in enumerate(tabs):
            base[t], ld[t] = off + k * d, len(tabs) * d
        off += len(tabs) * B * d
    ops = HipShardOps([], B, 1, 0.0, device=gpu)
    ops.bind_recv([[_dev(_host(blocks[t], dtype, "block"), gpu) for t in range(T)]])
    gsend = torch.full((T * B * d + 8,), -7.0, dtype=F32, device=gpu)
    dxb = _nan_filled((B, d), F32, gpu)
    ok = ops.interact_bwd_send(_dev(_host(dout, dtype, "dout"), gpu), _dev(_host(x, dtype, "x"), gpu), dxb, gsend,
                               torch.tensor(base, dtype=torch.int64, device=gpu),
                               torch.tensor(ld, dtype=torch.int64, device=gpu), 0)
    torch.cuda.synchronize()
    assert ok, "dlrm_interact_bwd_blocked refused a 16-B aligned shape"
    ops.check_bounds()
    Tm = np.concatenate([x[:, None], blocks.transpose(1, 0, 2)], axis=1)
    dx, dt, bound = _ref_bwd(dout, Tm)
    assert bound < (1 << 24)
    assert_f32_equal(to_np_bits(dxb), dx, "blocked backward dx")
    want = np.full(gsend.shape, -7.0)
    for t in range(T):
        for b in range(B):
            want[base[t] + b * ld[t]: base[t] + b * ld[t] + d] = dt[b, t + 1]
    assert_f32_equal(to_np_bits(gsend), want, "blocked backward send layout")


# ------------------------------------------------------------------ Implementation 2's batched Gram
SBM_SHAPES = [(8, 16, 5), (27, 128, 5), (90, 8, 5)]  # (F, d, B)


@gpu_test
@pytest.mark.parametrize("dtype,family", [(F32, "small"), (BF16, "small"), (F32, "selector")],
                         ids=["f32-small", "bf16-small", "f32-selector"])
@pytest.mark.parametrize("F,d,B", SBM_SHAPES)
def test_self_batched_mul_exact(pkg, gpu, F, d, B, dtype, family):
    """self_batched_mul: the whole F x F Gram, diagonal sum t^2 included, bit for bit (selector: every
    element with a selector row or column; the rest at the bar of test_self_batched_mul_and_rrule); and
    on the small family its rrule dT = (dZ + dZ^T) T."""
    T = _rows(family, d, F, B)
    td = _dev(_host(T, dtype, "t"), gpu)
    z, back = pkg.rrule_self_batched_mul(td)
    torch.cuda.synchronize()
    Z, A = _gram(T)
    got = to_np_bits(z)
    if family == "selector":
        sel = np.arange(F) % 2 == 1
        exact = np.broadcast_to(sel[:, None] | sel[None, :], Z.shape)
        assert_f32_equal(got, np.where(exact, Z, 0.0), "self_batched_mul", where=exact)
        assert_close(got[~exact], Z[~exact], rtol=1e-5, scale=np.sqrt(d), what="self_batched_mul (normal x normal)")
        return
    assert A.max() < (1 << 24)
    (assert_bf16_equal if dtype == BF16 else assert_f32_equal)(got, Z, "self_batched_mul")
    dz = _rng("dz", F, d, B).integers(-8, 9, size=(B, F, F))
    _, dt = back(_dev(_host(dz, dtype, "dz"), gpu))
    torch.cuda.synchronize()
    S = dz + dz.transpose(0, 2, 1)
    assert (np.abs(S) @ np.abs(T)).max() < (1 << 24)
    assert_f32_equal(to_np_bits(dt), S @ T, "self_batched_mul_back")


# ------------------------------------------------------------------ the fixtures, without a GPU
def test_fixtures_on_the_cpu():
    """Every DotInteraction / dot_back case: the C oracle equals the integer reference under the rule
    the GPU tests apply, and the conditions the module docstring states hold -- tie counts of the bf16
    cases, the left-out share of the wide cases, the column coverage of the selector cases."""
    total = total_down = total_up = 0
    for case in FWD_CASES:
        dtype, family, d, F, B, pad_to, x_extra = case
        what = _fwd_id(case)
        T = _rows(family, d, F, B)
        want, exact = _fwd_ref(family, d, F, B)
        P = F * (F - 1) // 2
        assert want.shape == exact.shape == (B, P)
        x = _host(T[:, 0], dtype, "x")
        ys = _host(T.reshape(B, F * d), dtype, "ys")
        ys[:, :d] = 0
        padding = _padding(d, F, pad_to)
        out = oracle.interact_fwd(x, ys, F, padding)
        assert np.array_equal(_bits(ys[:, :d]), _bits(x))
        _check_pairs(_check_out(out, x, d, F, what), family, d, F, B, dtype, "oracle " + what)
        if family == "small":
            assert exact.all(), what
        if dtype == BF16:
            ties, down, up = _tie_counts(_f32_exact(want))
            total, total_down, total_up = total + ties, total_down + down, total_up + up
            print(f"{what}: {ties} ties in {want.size} pairs ({down} down, {up} up)")
            if d >= 64:
                assert ties >= 50 and down >= 1 and up >= 1, (what, ties, down, up)
        if family == "wide":
            ww, wn = _wide_pairs(F)
            assert np.array_equal(~exact, np.broadcast_to(ww, exact.shape)), f"{what}: left out != wide x wide"
            assert exact[:, wn].all(), f"{what}: a wide x narrow pair is not exactly summable"
            assert 0 < ww.sum() <= 0.12 * P, (what, int(ww.sum()), P)
            print(f"{what}: {int(ww.sum())} of {P} pairs left out ({ww.sum() / P:.3f})")
        if family == "selector":
            assert np.array_equal(_selector_columns(T), np.arange(d)), f"{what}: not every column is selected"
            assert (want[exact] != 0).any()
    assert total >= 1000 and total_down >= 1 and total_up >= 1, (total, total_down, total_up)
    down, up = _tie_counts(np.array([257.0, 259.0], dtype=np.float32))[1:]
    assert (down, up) == (1, 1)  # 257 -> 256, 259 -> 260
    print(f"bf16 forward cases: {total} ties in all")
    for case in BWD_CASES:
        dtype, family, d, F, B, extra = case
        dout, T, dx, dt = _bwd_case(family, d, F, B)
        rdx, rdt = oracle.interact_bwd(_host(dout, dtype, "dout"), _host(T.reshape(B, F * d), dtype, "t"), d, F)
        assert_f32_equal(rdx, dx, "oracle dx " + _bwd_id(case))
        assert_f32_equal(rdt, dt, "oracle dt " + _bwd_id(case))


def _padding(d, F, pad_to):
    """process_batches' padding (interact.jl:449-456), restated: the CPU test imports no GPU package"""
    unpadded = F * (F - 1) // 2 + d
    return -unpadded % pad_to
