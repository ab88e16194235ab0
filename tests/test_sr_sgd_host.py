"""StochasticDescent on the host: the Philox restatement against known answers, sr_round on hand-made bit
patterns, the statistics of a walk of small steps, the class's errors and the C entry points' NULL-argument
returns (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

# (counter, key, output) of Philox4x32-10: the Random123 known answers
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32).reshape(1, -1).copy()


def _sr(pkg, bits, r):
    return pkg.sr_round(_f32(bits), 0, 0, 0, bits=np.asarray(r, dtype=np.uint32).reshape(1, -1))[0]


def test_philox_known_answers(pkg):
    for counter, key, want in KAT:
        got = [int(x) for x in pkg.philox4x32_10(counter, key)]
        assert got == want, ([hex(x) for x in got], [hex(x) for x in want])
    # ... and vectorised: the three blocks at once
    got = pkg.philox4x32_10([np.array([k[0][i] for k in KAT], dtype=np.uint32) for i in range(4)], KAT[0][1])
    assert [int(x[0]) for x in got] == KAT[0][2]


def test_sr_bits_layout(pkg):
    """Column c takes the low 16 bits of word c & 3 of the block with counter (row, table << 16 | c >> 2, step)."""
    seed, step, table = (0x299F31D0 << 32) | 0xA4093822, (0x03707344 << 32) | 0x13198A2E, 0x85A3
    r = pkg.sr_bits((3, 12), seed, step, table, row0=0x243F6A88 - 1)
    assert r.shape == (3, 12) and r.dtype == np.uint32 and (r < 65536).all()
    for c in range(12):
        blk = pkg.philox4x32_10([0x243F6A88, (table << 16) | (c >> 2), 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])
        assert int(r[1, c]) == int(blk[c & 3]) & 0xFFFF
    # the third known answer is block 0x08D3 of table 0x85A3, row 0x243F6A88: columns 4 * 0x08D3 ..
    blk = pkg.sr_bits((1, 4 * 0x08D3 + 4), seed, step, table, row0=0x243F6A88)[0, 4 * 0x08D3:]
    assert [int(x) for x in blk] == [x & 0xFFFF for x in KAT[2][2]]
    # a width that is no multiple of 4, and independence of the shape asked for
    assert np.array_equal(pkg.sr_bits((3, 6), seed, step, table, row0=7), pkg.sr_bits((5, 12), seed, step, table, row0=7)[:3, :6])
    assert not np.array_equal(pkg.sr_bits((3, 8), 1, 0, 0), pkg.sr_bits((3, 8), 2, 0, 0))
    assert not np.array_equal(pkg.sr_bits((3, 8), 1, 0, 0), pkg.sr_bits((3, 8), 1, 1, 0))
    assert not np.array_equal(pkg.sr_bits((3, 8), 1, 0, 0), pkg.sr_bits((3, 8), 1, 0, 1))


def test_sr_round_bit_patterns(pkg):
    # a bf16 value (low half 0) is kept, whatever R
    assert list(_sr(pkg, [0x3FC00000, 0x3FC00000, 0xBFC00000], [0, 0xFFFF, 0xFFFF])) == [0x3FC0, 0x3FC0, 0xBFC0]
    # low half 0xffff: R = 0 keeps the lower neighbour, R = 1 rounds up; low half 1 needs R = 0xffff
    assert list(_sr(pkg, [0x3FC0FFFF, 0x3FC0FFFF, 0x3FC00001, 0x3FC00001], [0, 1, 0xFFFE, 0xFFFF])) == \
        [0x3FC0, 0x3FC1, 0x3FC0, 0x3FC1]
    # negative values round away from zero (the magnitude grows)
    assert list(_sr(pkg, [0xBFC08000, 0xBFC08000], [0x7FFF, 0x8000])) == [0xBFC0, 0xBFC1]
    # a carry into the exponent: 1.99.. -> 2.0
    assert list(_sr(pkg, [0x3FFFFFFF, 0x3FFFFFFF], [0, 1])) == [0x3FFF, 0x4000]
    # the largest subnormal's neighbour is the smallest normal
    assert list(_sr(pkg, [0x007FFFFF], [1])) == [0x0080]
    # a finite value above the largest finite bf16 can reach Inf, its upper neighbour
    assert list(_sr(pkg, [0x7F7F0001, 0x7F7F0001, 0xFF7FFFFF], [0xFFFE, 0xFFFF, 1])) == [0x7F7F, 0x7F80, 0xFF80]
    # Inf, NaN and both zeros: unchanged behaviour, whatever R (a NaN keeps its quiet bit)
    assert list(_sr(pkg, [0x7F800000, 0xFF800000, 0x00000000, 0x80000000], [0xFFFF] * 4)) == [0x7F80, 0xFF80, 0x0000, 0x8000]
    assert list(_sr(pkg, [0x7F800001, 0x7FC12345, 0xFFFFFFFF, 0x7FBFFFFF], [0xFFFF, 0, 0xFFFF, 0xFFFF])) == \
        [0x7FC0, 0x7FC1, 0xFFFF, 0x7FFF]
    # the probability is (low half) / 65536 exactly: over every R
    r = np.arange(65536, dtype=np.uint32)
    up = _sr(pkg, np.full(65536, 0x3FBFC000, dtype=np.uint32), r)
    assert int((up == 0x3FC0).sum()) == 0xC000 and int((up == 0x3FBF).sum()) == 0x4000


def test_sr_round_types(pkg):
    with pytest.raises(TypeError):
        pkg.sr_round(np.zeros((2, 4), dtype=np.float64), 0, 0, 0)
    with pytest.raises(TypeError):
        pkg.sr_round(np.zeros(4, dtype=np.float32), 0, 0, 0)
    a = pkg.sr_round(torch.full((2, 4), 1.5), 0, 0, 0)
    assert a.dtype == np.uint16 and (a == 0x3FC0).all()


def _walk(pkg, seed, steps=64, rows=64, D=128):
    """rows x D weights 1.5, `steps` steps of lr * G = 2^-9 with the restated store: (moved after step 0, mean)."""
    w = np.full((rows, D), 1.5, dtype=np.float32)
    step = np.float32(2.0 ** -9)
    moved0 = None
    for s in range(steps):
        wp = (w - step).astype(np.float32)  # (exact: fmaf(-lr, G, w) with lr * G = 2^-9)
        if s == 0:
            assert (wp.view(np.uint32) == 0x3FBFC000).all()
        h = pkg.sr_round(wp, seed, s, 0)
        w = (h.astype(np.uint32) << 16).view(np.float32)
        if s == 0:
            moved0 = int((w != 1.5).sum())
    return moved0, float(w.astype(np.float64).mean())


def test_walk_is_unbiased_where_nearest_rounding_stalls(pkg):
    """64 x 128 elements at 1.5, lr * G = 2^-9: every W' of step 0 is 0x3FBFC000, a quarter of a bf16 ulp (2^-7)
    below 1.5, so an element moves down with probability 1/4.
      * moved after step 0: within 2048 +- 235 (six binomial standard deviations, sqrt(8192 * 3 / 16) = 39.2);
      * mean after 64 steps: within 2.1e-3 of 1.5 - 64 * 2^-9 = 1.375 (six standard deviations of the mean at a
        per-step variance of at most 1/4 ulp^2: 6 * 4 * 2^-7 / sqrt(8192)).
    Round-to-nearest stays at 1.5 exactly: the failure the rule removes."""
    moved0, mean = _walk(pkg, 12345)
    print(f"seed 12345: moved after step 0 = {moved0}, mean after 64 steps = {mean:.5f}")
    assert abs(moved0 - 2048) <= 235, moved0
    assert abs(mean - 1.375) <= 2.1e-3, mean
    w = torch.full((64, 128), 1.5, dtype=torch.bfloat16)
    for _ in range(64):
        w = (w.float() - 2.0 ** -9).to(torch.bfloat16)
    assert (w.float() == 1.5).all()


def test_optimizer_class(pkg):
    o = pkg.StochasticDescent()
    assert o.eta == 0.1 and o.seed == 0 and repr(o) == "StochasticDescent(0.1, seed=0)"
    o = pkg.StochasticDescent(0.5, seed=2 ** 63 + 7)
    assert o.seed == 2 ** 63 + 7 and repr(o) == f"StochasticDescent(0.5, seed={2 ** 63 + 7})"
    for bad in (1.0, "7", None, True):
        with pytest.raises(TypeError):
            pkg.StochasticDescent(0.1, seed=bad)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            pkg.StochasticDescent(0.1, seed=bad)
    for name in ("StochasticDescent", "sr_round"):
        assert name in pkg.__all__


def test_update_rejects_fp32_tables_and_the_atomic_mode(pkg):
    with pytest.raises(ValueError, match="bfloat16"):
        pkg.update_(pkg.StochasticDescent(), [torch.zeros((4, 8), dtype=torch.float32)], [], index_base=0)
    with pytest.raises(ValueError, match="deterministic"):
        pkg.update_(pkg.StochasticDescent(), [torch.zeros((4, 8), dtype=torch.bfloat16)], [], index_base=0,
                    deterministic=False)
    with pytest.raises(TypeError, match="StochasticDescent"):  # (the message that lists the rules names it)
        pkg.update_(object(), [torch.zeros((4, 8), dtype=torch.bfloat16)], [], index_base=0)


def test_entry_points_reject_null_arguments(pkg):
    """Argument validation runs on the host before any HIP call."""
    _lib = pkg._lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.dlrm_sr_sgd_create(None, None, 0, ctypes.byref(out)) == _lib.E_ARG
    assert lib.dlrm_sr_sgd_create(None, None, 0, None) == _lib.E_ARG
    assert not out.value
    assert lib.dlrm_sr_sgd_update(None, None, None, None, 0, None, 0, 0, 0, 1, 1, None, 0, 0, 0, 0.1) == _lib.E_ARG
    assert lib.dlrm_sr_sgd_update(None, None, None, None, _lib.UPDATE_PREBUILT, None, 0, 0, 0, 1, 1, None, 0, 0, 0,
                                  0.1) == _lib.E_ARG
    assert lib.dlrm_sr_sgd_seek(None, None, 0) == _lib.E_ARG
    step = ctypes.c_uint64(77)
    assert lib.dlrm_sr_sgd_step(None, None, ctypes.byref(step)) == _lib.E_ARG and step.value == 77
    assert lib.dlrm_sr_sgd_destroy(None) == 0
