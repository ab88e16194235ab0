"""int8 row quantization on the CPU: the numpy restatement `quantize_rows` / `dequantize_rows` (the yardstick of
tests/test_q8.py), the derived error bound, the ABI's argument checks and csrc/q8_plan.hpp on the host.

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
DIMS = (1, 6, 16, 128)


def _ulps(a, b):
    ia = np.ascontiguousarray(a, dtype=F).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=F).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("d", DIMS)
def test_bound_and_codes_of_every_family(pkg, d):
    worst = 0.0
    for name, w in q8_cases.families(d).items():
        q, scale, bias = pkg.quantize_rows(w)
        assert q.dtype == np.uint8 and scale.dtype == F and bias.dtype == F
        v = pkg.dequantize_rows(q, scale, bias)
        assert v.dtype == F and v.shape == w.shape
        err = np.abs(v.astype(np.float64) - w.astype(np.float64))
        m = np.maximum(np.abs(w.min(axis=1)), np.abs(w.max(axis=1))).astype(np.float64)
        bound = (0.5 + 2.0 ** -10) * scale.astype(np.float64) + 2.0 ** -22 * m
        assert (err <= bound[:, None]).all(), (name, d, float((err / np.maximum(bound[:, None], 1e-300)).max()))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz, None]).max()))
        assert (q.min(axis=1) == 0).all(), (name, "code 0 in every row")
        const = w.min(axis=1) == w.max(axis=1)
        assert (q.max(axis=1)[~const] == 255).all(), (name, "code 255 in every non-constant row")
        assert np.array_equal(bias, w.min(axis=1))
        # constant rows: scale 0, exact
        assert (scale[const] == 0).all() and (q[const] == 0).all()
        assert np.array_equal(v[const], w[const])
    print(f"d={d}: worst |v - w| / bound = {worst:.4f}")


@pytest.mark.parametrize("d", DIMS)
def test_idempotence(pkg, d):
    """Quantizing a dequantized fp32 table gives the same codes, and scale and bias within 1 ulp.  The bound, not bit
    equality, is the claim; over these families scale and bias do come out bit-equal (the printed count is 0)."""
    moved = 0
    for name, w in q8_cases.families(d).items():
        q, scale, bias = pkg.quantize_rows(w)
        v = pkg.dequantize_rows(q, scale, bias)
        q2, scale2, bias2 = pkg.quantize_rows(v)
        assert np.array_equal(q2, q), name
        assert (_ulps(scale2, scale) <= 1).all(), name
        assert (_ulps(bias2, bias) <= 1).all(), name
        moved += int((_ulps(scale2, scale) != 0).sum() + (_ulps(bias2, bias) != 0).sum())
    print(f"d={d}: {moved} scale / bias values moved by one ulp")


def test_exact_sum_inputs(pkg):
    rng = np.random.default_rng(3)
    for d in (2, 16, 128):
        k = rng.integers(0, 256, size=(9, d))
        k[:, 0], k[:, -1] = 0, 255  # the full range: scale is exactly 1
        for step, off in ((1.0, 0.0), (1.0, 37.0), (0.25, 0.0), (0.25, -8.0)):
            w = (k.astype(F) * F(step) + F(off)).astype(F)
            q, scale, bias = pkg.quantize_rows(w)
            assert (scale == F(step)).all() and np.array_equal(bias, w.min(axis=1))
            assert np.array_equal(q, k.astype(np.uint8))
            assert np.array_equal(pkg.dequantize_rows(q, scale, bias), w)
    # the same off zero: integers lo .. lo + 255
    w = np.array([[3, 258, 100, 3 + 17]], dtype=F)
    q, scale, bias = pkg.quantize_rows(w)
    assert scale[0] == F(1.0) and bias[0] == F(3.0) and np.array_equal(pkg.dequantize_rows(q, scale, bias), w)


def test_bf16_consumer_rounds_once(pkg):
    w = q8_cases.families(16)["normal"]
    q, scale, bias = pkg.quantize_rows(w)
    v = pkg.dequantize_rows(q, scale, bias)
    b = pkg.dequantize_rows(q, scale, bias, dtype="bfloat16")
    assert ((b.view(np.uint32) & 0xFFFF) == 0).all()
    assert (np.abs(b.astype(np.float64) - v) <= np.abs(v) * 2.0 ** -8).all()
    import torch
    assert np.array_equal(b, torch.from_numpy(v).to(torch.bfloat16).float().numpy())
    assert np.array_equal(pkg.dequantize_rows(q, scale, bias, dtype=torch.bfloat16), b)


def test_null_and_shape_arguments_are_rejected_without_a_device(pkg):
    lib, E = pkg._lib.load(), pkg._lib.E_ARG
    assert lib.dlrm_q8_tables_create(None, 1, 16, None, None, None, None) == E
    assert lib.dlrm_q8_tables_create(None, -1, 0, None, None, None, None) == E
    assert lib.dlrm_q8_quantize(None, None, None) == E
    assert lib.dlrm_q8_dequantize(None, None, None) == E
    assert lib.dlrm_q8_maplookup(None, None, None, 0, 0, 0, 1, 1, 0, None, 0, 0) == E
    assert lib.dlrm_q8_lookup_interact_fwd(None, None, None, 0, 0, 0, 1, 1, 0, None, 16, None, 17, 0) == E
    assert lib.dlrm_q8_tables_destroy(None) == 0


# ---- csrc/q8_plan.hpp on the host
def _fused(dtype, d, T, L, q_align, x_addr, x_ld):
    vec = 4 if dtype == 0 else 8
    return (L == 1 and 1 <= T <= 31 and d % vec == 0 and q_align >= vec and x_addr % 16 == 0 and x_ld % vec == 0)


PLAN_CASES = [  # dtype d T lookups q_align x_address x_ld rows16
    (0, 128, 26, 1, 16, 4096, 128, 1), (1, 128, 26, 1, 16, 4096, 128, 1),
    (0, 16, 31, 1, 16, 4096, 16, 1), (0, 16, 32, 1, 16, 4096, 16, 1), (0, 16, 40, 1, 16, 4096, 16, 1),
    (0, 16, 1, 1, 16, 4096, 16, 1), (0, 16, 0, 1, 16, 4096, 16, 1),
    (0, 16, 7, 9, 16, 4096, 16, 1), (0, 16, 7, 10, 16, 4096, 16, 1),
    (0, 4, 7, 1, 4, 4096, 4, 1), (0, 6, 7, 1, 2, 4100, 6, 0), (0, 6, 7, 1, 16, 4096, 8, 1),
    (1, 8, 7, 1, 8, 4096, 8, 1), (1, 4, 7, 1, 8, 4096, 8, 1), (1, 8, 7, 1, 4, 4096, 8, 1), (1, 16, 7, 1, 16, 4096, 20, 1),
    (0, 16, 7, 1, 2, 4096, 16, 1), (0, 16, 7, 1, 16, 4100, 16, 1), (0, 16, 7, 1, 16, 4096, 18, 1),
    (0, 48, 7, 1, 16, 4096, 48, 1), (0, 48, 7, 1, 8, 4096, 48, 1), (0, 48, 7, 1, 16, 4096, 48, 0), (0, 24, 7, 1, 16, 4096, 24, 1),
]


def test_plan_header_alone_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(HERE, "q8_plan_print.cpp")
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in PLAN_CASES)
    for name, flags in (("plan", ["-O1"]), ("plan_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                         "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, src], check=True)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
        got = [(int(a), int(b)) for a, b in zip(out[::2], out[1::2])]
        want = [(int(_fused(*c[:7])), int(c[1] % 16 == 0 and c[4] >= 16 and c[7] == 1)) for c in PLAN_CASES]
        assert got == want, name
    fused = [c for c in PLAN_CASES if _fused(*c[:7])]
    assert 0 < len(fused) < len(PLAN_CASES)
