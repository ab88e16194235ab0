"""The fused MXFP8 MLP chain on the CPU: `mx_quantize` on known values, csrc/mlp_fp8_plan.hpp through
dlrm_mlp_fp8_plan (pure host) against a restatement, and the ABI's argument checks, which run before any HIP call."""
import numpy as np
import pytest

KAGGLE_BOTTOM, KAGGLE_TOP = [13, 512, 256, 128], [479, 1024, 1024, 512, 256, 1]


def _block(pkg, **at):
    """A block of 32 zeros with v[i] = value for every i=value given; its (codes, byte, values)."""
    v = np.zeros(32)
    for i, val in at.items():
        v[int(i[1:])] = val
    c, s, d = pkg.mx_quantize(v)
    return c, int(s[0]), d


def test_mx_quantize_known_values(pkg):
    c, s, d = _block(pkg, i0=14.0, i1=-3.0)
    assert s == 3 - 8 + 127 and d[0] == 14.0 and d[1] == -3.0 and c[0] == 0x7E and c[1] == 0xEC  # 448, -96 scaled
    c, s, d = _block(pkg, i5=15.0)
    assert s == 3 - 8 + 127 and d[5] == 14.0 and c[5] == 0x7E  # 480 saturates to 448
    c, s, d = _block(pkg)
    assert s == 0 and not c.any() and not d.any()
    c, s, d = _block(pkg, i0=256.0, i1=2.0 ** -10, i2=3 * 2.0 ** -10, i3=2.0 ** -9)
    # X = 0 and the subnormal step is 2^-9: 2^-10 is a tie between codes 0 and 1 and rounds to zero, 3 2^-10 a tie
    # between codes 1 and 2 and rounds up (a value 2^-18 of the block maximum: e4m3 spans 2^8 .. 2^-9)
    assert s == 127 and list(d[:4]) == [256.0, 0.0, 2.0 ** -8, 2.0 ** -9] and list(c[:4]) == [0x78, 0, 2, 1]
    c, s, d = _block(pkg, i0=1.0, i1=(256 + 16) / 256, i2=(256 + 48) / 256, i3=(256 + 24) / 256)
    # at 256 the step is 32: 272 is a tie -> 256 (even), 304 a tie -> 320 (even), 280 -> 288
    assert list(d[:4] * 256) == [256.0, 256.0, 320.0, 288.0]
    for m in (1.0, 1.75, 1.99, 3e-5, 7e4):
        assert _block(pkg, i7=m)[1] == int(np.floor(np.log2(m))) - 8 + 127
    assert pkg.mx_quantize(np.ones((3, 40)))[0].shape == (3, 64) and pkg.mx_quantize(np.ones((3, 40)))[1].shape == (3, 2)


def _ceil(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("sizes,batch", [(KAGGLE_BOTTOM, 2048), (KAGGLE_TOP, 2048), (KAGGLE_TOP, 8192),
                                         (KAGGLE_TOP, 16384), ([32, 16], 1)])
@pytest.mark.parametrize("dtypes", [(0, 0), (1, 1)])
def test_plan(pkg, sizes, batch, dtypes):
    p = pkg.mlp_fp8_plan(sizes, batch, *dtypes)
    assert p["rc"] == pkg._lib.OK
    kp, npad = [_ceil(k, 128) for k in sizes[:-1]], [_ceil(n, 16) for n in sizes[1:]]
    assert p["kp"] == kp and p["np"] == npad
    off, want = 0, []
    for k, n in zip(kp, npad):
        want.append([off, off + n * k])
        off += n * k + n * k // 32
    for l, n in enumerate(npad):
        want[l].append(off)
        off += 4 * n
    assert [list(o) for o in p["offsets"]] == want and p["packed_bytes"] == off
    assert all(o % 64 == 0 for t in p["offsets"] for o in t)
    assert p["mt"] == (32 if batch >= 4096 else 16)  # the committed rule
    assert p["grid"] == (batch + p["mt"] - 1) // p["mt"]
    wmax = max(kp)
    assert p["lds_bytes"] == 2 * p["mt"] * (wmax + 16 + wmax // 32) <= 160 * 1024 - 8192


def test_plan_refuses(pkg):
    L = pkg._lib
    assert pkg.mlp_fp8_plan([13, 1025, 1], 64)["rc"] == L.E_UNSUPPORTED  # padded width 1040
    assert pkg.mlp_fp8_plan([1040, 16], 64)["rc"] == L.E_UNSUPPORTED
    assert pkg.mlp_fp8_plan([13, 1024, 1], 64)["rc"] == L.OK
    assert pkg.mlp_fp8_plan([8] * 10, 64)["rc"] == L.E_UNSUPPORTED  # 9 layers
    assert pkg.mlp_fp8_plan([8] * 9, 64)["rc"] == L.OK
    assert pkg.mlp_fp8_plan([13], 64)["rc"] == L.E_ARG  # an empty chain
    assert pkg.mlp_fp8_plan([13, 0, 1], 64)["rc"] == L.E_ARG
    assert pkg.mlp_fp8_plan([13, 1], -1)["rc"] == L.E_ARG
    assert pkg.mlp_fp8_plan([13, 1], 64, 2, 0)["rc"] == L.E_ARG  # a dtype that is neither fp32 nor bf16


def test_null_arguments_are_rejected_without_a_device(pkg):
    lib, E = pkg._lib.load(), pkg._lib.E_ARG
    assert lib.dlrm_mlp_fp8_plan(1, None, 64, 0, 0, None, None, None, None, None, None, None) == E
    assert lib.dlrm_mlp_fp8_create(None, 1, None, None) == E
    assert lib.dlrm_mlp_fp8_pack(None, None, None, None, None) == E
    assert lib.dlrm_mlp_fp8_infer(None, None, 1, None, 0, 16, None, 0, 16, 0) == E
    assert lib.dlrm_mlp_fp8_destroy(None) == 0
