"""int4 row quantization on the CPU: the numpy restatement `quantize_rows4` / `dequantize_rows4` / `pack_rows4` /
`unpack_rows4` (the yardstick of tests/test_q4.py), the derived error bound, the ABI's argument checks and
csrc/q4_plan.hpp on the host.

The bound, per element of a finite row:  |v - w| <= (0.5 + 2^-10) * scale + 2^-22 * max(|lo|, |hi|).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import q8_cases

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
DIMS = (1, 2, 6, 16, 128)


@pytest.mark.parametrize("d", DIMS)
def test_bound_and_codes_of_every_family(pkg, d):
    fams = q8_cases.families(d)
    fams["integers"] = np.random.default_rng(d).integers(0, 16, size=(12, d)).astype(F)
    if d > 1:
        fams["integers"][:, 0], fams["integers"][:, -1] = 0, 15
    worst = 0.0
    for name, w in fams.items():
        q, scale, bias = pkg.quantize_rows4(w)
        assert q.dtype == np.uint8 and scale.dtype == F and bias.dtype == F and q.max() <= 15
        v = pkg.dequantize_rows4(q, scale, bias)
        err = np.abs(v.astype(np.float64) - w.astype(np.float64))
        bound = pkg.q4_bound(w, scale)
        assert (err <= bound[:, None]).all(), (name, d, float((err / np.maximum(bound[:, None], 1e-300)).max()))
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0, None]).max()))
        const = w.min(axis=1) == w.max(axis=1)
        assert (q.min(axis=1) == 0).all() and (q.max(axis=1)[~const] == 15).all(), (name, "codes 0 and 15")
        assert np.array_equal(bias, w.min(axis=1))
        assert (scale[const] == 0).all() and (q[const] == 0).all() and np.array_equal(v[const], w[const])
        if name == "integers" and d > 1:
            assert (scale == 1).all() and np.array_equal(q, w.astype(np.uint8)) and np.array_equal(v, w)
    print(f"d={d}: worst |v - w| / bound = {worst:.4f}")


@pytest.mark.parametrize("d", (1, 2, 5, 6, 16, 17, 48, 128))
def test_pack_and_unpack_round_trip(pkg, d):
    rng = np.random.default_rng(d)
    q = rng.integers(0, 16, size=(9, d)).astype(np.uint8)
    scale, bias = rng.standard_normal(9).astype(F), rng.standard_normal(9).astype(F)
    img = pkg.pack_rows4(q, scale, bias)
    S = 8 + 8 * ((d + 15) // 16)
    assert img.shape == (9, S) and img.dtype == np.uint8
    assert np.array_equal(img[:, :4].copy().view(F)[:, 0], scale) and np.array_equal(img[:, 4:8].copy().view(F)[:, 0], bias)
    for c in range(d):  # code c: byte 8 + c // 2, low nibble for even c
        assert np.array_equal((img[:, 8 + c // 2] >> (4 * (c % 2))) & 15, q[:, c]), c
    if d % 2:
        assert (img[:, 8 + d // 2] >> 4 == 0).all()  # the pad nibble
    assert (img[:, 8 + (d + 1) // 2:] == 0).all()  # the pad bytes
    q2, s2, b2 = pkg.unpack_rows4(img, d)
    assert np.array_equal(q2, q) and np.array_equal(s2, scale) and np.array_equal(b2, bias)
    assert not pkg.pack_rows4(np.zeros((1, d), np.uint8), F(0), F(0)).any()  # a zero row is all-zero bytes


def test_row_bytes_and_null_arguments_without_a_device(pkg):
    lib, E = pkg._lib.load(), pkg._lib.E_ARG
    for d in (1, 15, 16, 17, 128, 144, 1000):
        assert lib.dlrm_q4_row_bytes(d) == 8 + 8 * ((d + 15) // 16)
    assert lib.dlrm_q4_row_bytes(0) == E and lib.dlrm_q4_row_bytes(-3) == E
    assert lib.dlrm_q4_tables_create(None, 1, 16, None, None, None) == E
    assert lib.dlrm_q4_quantize(None, None, None) == E
    assert lib.dlrm_q4_dequantize(None, None, None) == E
    assert lib.dlrm_q4_maplookup(None, None, None, 0, 0, 0, 1, 1, 0, None, 0, 0) == E
    assert lib.dlrm_q4_lookup_interact_fwd(None, None, None, 0, 0, 0, 1, 1, 0, None, 16, None, 17, 0) == E
    assert lib.dlrm_q4_tables_destroy(None) == 0


def _fused(dtype, d, T, L, x_addr, x_ld):
    return L == 1 and 1 <= T <= 31 and d % 16 == 0 and x_addr % 16 == 0 and x_ld % (4 if dtype == 0 else 8) == 0


PLAN_CASES = [  # dtype d T lookups x_address x_ld rows16: both sides of each limit of the fused condition
    (0, 128, 26, 1, 4096, 128, 1), (1, 128, 26, 1, 4096, 128, 1), (0, 16, 31, 1, 4096, 16, 1), (0, 16, 32, 1, 4096, 16, 1),
    (0, 16, 1, 1, 4096, 16, 1), (0, 16, 0, 1, 4096, 16, 1), (0, 16, 7, 2, 4096, 16, 1), (0, 144, 7, 1, 4096, 144, 0),
    (0, 8, 7, 1, 4096, 8, 1), (1, 24, 7, 1, 4096, 24, 1), (0, 16, 7, 1, 4100, 16, 1), (0, 16, 7, 1, 4104, 16, 1),
    (0, 16, 7, 1, 4096, 18, 1), (1, 16, 7, 1, 4096, 20, 1), (1, 16, 7, 1, 4096, 24, 1), (0, 6, 7, 1, 4096, 8, 1),
]


def test_plan_header_alone_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "plan")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-o", exe,
                    os.path.join(HERE, "q4_plan_print.cpp")], check=True)
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in PLAN_CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = [tuple(int(v) for v in out[k:k + 3]) for k in range(0, len(out), 3)]
    want = [(int(_fused(*c[:6])), int(c[1] % 16 == 0 and c[6] == 1), 8 + 8 * ((c[1] + 15) // 16)) for c in PLAN_CASES]
    assert got == want
    assert 0 < sum(w[0] for w in want) < len(want)
