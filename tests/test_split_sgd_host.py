"""Split-bf16 tables: split_f32 / merge_split, the SplitDescent class and the host side of the three
C entry points (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch


def _u32(bits):
    """uint32 bit patterns -> float32 tensor"""
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def _bits32(t):
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


def _bits16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# values just below a bf16 rounding boundary: the low half is 0x8000..0xffff, so round-to-nearest
# moves the high half up where truncation keeps it (1.0 + 2^-8 + ..., negative, tiny and huge)
BOUNDARY = [0x3F80FFFF, 0x3F808001, 0xBF80C000, 0x00018000, 0x7F7EFFFF, 0x4049FFFF, 0xC2F6E979]
SPECIAL = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFFFFFFF]


def test_round_trip_every_bit(pkg):
    rng = np.random.default_rng(0)
    bits = np.concatenate([rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32),
                           np.array(SPECIAL + BOUNDARY, dtype=np.uint32)])
    w = _u32(bits)
    hi, lo = pkg.split_f32(w)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.int16 and hi.shape == w.shape == lo.shape
    assert np.array_equal(_bits16(hi), (bits >> 16).astype(np.uint16))
    assert np.array_equal(_bits16(lo), (bits & 0xFFFF).astype(np.uint16))
    back = pkg.merge_split(hi, lo)
    assert back.dtype == torch.float32
    assert np.array_equal(_bits32(back), bits)


def test_two_dimensional_and_strided(pkg):
    w = torch.randn((7, 12))
    hi, lo = pkg.split_f32(w)
    assert hi.shape == (7, 12)
    assert np.array_equal(_bits32(pkg.merge_split(hi, lo)), _bits32(w))
    v = w[:, 2:10]  # a strided view
    assert np.array_equal(_bits32(pkg.merge_split(*pkg.split_f32(v))), _bits32(v))


def test_high_half_is_the_truncation_not_the_rounding(pkg):
    w = _u32(BOUNDARY)
    hi, _ = pkg.split_f32(w)
    top = (np.array(BOUNDARY, dtype=np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(_bits16(hi), top)
    rounded = _bits16(w.to(torch.bfloat16))
    assert (rounded != top).all()
    # ... and the truncation lies toward zero, less than one bf16 ulp away
    f = hi.float().numpy().astype(np.float64)
    x = w.numpy().astype(np.float64)
    assert (np.abs(f) <= np.abs(x)).all()
    ulp = np.abs(_u32(((top.astype(np.uint32) + 1) << 16)).numpy().astype(np.float64) - f)
    assert (np.abs(x - f) < ulp).all()


def test_type_errors(pkg):
    with pytest.raises(TypeError):
        pkg.split_f32(torch.zeros(4, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        pkg.merge_split(torch.zeros(4), torch.zeros(4, dtype=torch.int16))
    with pytest.raises(TypeError):
        pkg.merge_split(torch.zeros(4, dtype=torch.bfloat16), torch.zeros(5, dtype=torch.int16))


def test_optimizer_class(pkg):
    o = pkg.SplitDescent()
    assert o.eta == 0.1 and repr(o) == "SplitDescent(0.1)"
    assert repr(pkg.SplitDescent(0.5)) == "SplitDescent(0.5)"
    for name in ("SplitDescent", "split_f32", "merge_split"):
        assert name in pkg.__all__


def test_update_rejects_fp32_tables(pkg):
    tables = [torch.zeros((4, 8), dtype=torch.float32)]
    with pytest.raises(ValueError, match="bfloat16"):
        pkg.update_(pkg.SplitDescent(), tables, [], index_base=0)


def test_update_is_deterministic_only(pkg):
    tables = [torch.zeros((4, 8), dtype=torch.bfloat16)]
    with pytest.raises(ValueError, match="deterministic"):
        pkg.update_(pkg.SplitDescent(), tables, [], index_base=0, deterministic=False)


def test_entry_points_reject_null_arguments(pkg):
    """Argument validation runs on the host before any HIP call."""
    _lib = pkg._lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.dlrm_split_sgd_create(None, None, None, ctypes.byref(out)) == _lib.E_ARG
    assert lib.dlrm_split_sgd_create(None, None, None, None) == _lib.E_ARG
    assert not out.value
    assert lib.dlrm_split_sgd_update(None, None, None, None, 0, None, 0, 0, 0, 1, 1, None, 0, 0, 0, 0.1) == _lib.E_ARG
    assert lib.dlrm_split_sgd_update(None, None, None, None, _lib.UPDATE_PREBUILT, None, 0, 0, 0, 1, 1, None, 0, 0, 0,
                                     0.1) == _lib.E_ARG
    assert lib.dlrm_split_sgd_destroy(None) == 0
