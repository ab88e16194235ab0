"""The fused bf16 MLP chain on the CPU: csrc/mlp_plan.hpp through dlrm_mlp_bf16_plan (pure host) and the ABI's
argument checks, which run before any HIP call."""
import pytest

CHAINS = [  # sizes, batch
    ([13, 512, 256, 128], 2048), ([479, 1024, 1024, 512, 256, 1], 2048), ([479, 1024, 1024, 512, 256, 1], 8192),
    ([13, 48, 1024, 32, 1], 33), ([32, 16], 1), ([1024, 1024], 65), ([1, 1, 1, 1, 1, 1, 1, 1, 1], 16),
]


def _ceil(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("sizes,batch", CHAINS)
@pytest.mark.parametrize("dtypes", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_plan(pkg, sizes, batch, dtypes):
    p = pkg.mlp_bf16_plan(sizes, batch, *dtypes)
    assert p["rc"] == pkg._lib.OK
    assert p["kp"] == [_ceil(k, 32) for k in sizes[:-1]]
    assert p["np"] == [_ceil(n, 16) for n in sizes[1:]]
    assert p["mt"] in (16, 32)
    wmax = max(p["kp"])
    assert p["lds_bytes"] == 2 * p["mt"] * (wmax + 8) * 2 <= 160 * 1024
    assert p["grid"] == (batch + p["mt"] - 1) // p["mt"]
    assert p["packed_bytes"] == sum(n * k * 2 + n * 4 for k, n in zip(p["kp"], p["np"]))


def test_plan_refuses(pkg):
    L = pkg._lib
    assert pkg.mlp_bf16_plan([13, 1025, 1], 64)["rc"] == L.E_UNSUPPORTED  # padded width 1040
    assert pkg.mlp_bf16_plan([1040, 16], 64)["rc"] == L.E_UNSUPPORTED
    assert pkg.mlp_bf16_plan([16, 1030], 64)["rc"] == L.E_UNSUPPORTED
    assert pkg.mlp_bf16_plan([13, 1024, 1], 64)["rc"] == L.OK
    assert pkg.mlp_bf16_plan([8] * 10, 64)["rc"] == L.E_UNSUPPORTED  # 9 layers
    assert pkg.mlp_bf16_plan([8] * 9, 64)["rc"] == L.OK
    assert pkg.mlp_bf16_plan([13], 64)["rc"] == L.E_ARG  # an empty chain
    assert pkg.mlp_bf16_plan([13, 0, 1], 64)["rc"] == L.E_ARG
    assert pkg.mlp_bf16_plan([13, 1], -1)["rc"] == L.E_ARG
    assert pkg.mlp_bf16_plan([13, 1], 64, 2, 0)["rc"] == L.E_ARG
    assert L.load().dlrm_mlp_bf16_plan(1, None, 64, 0, 0, None, None, None, None, None, None) == L.E_ARG


def test_null_arguments_are_rejected_without_a_device(pkg):
    lib, E = pkg._lib.load(), pkg._lib.E_ARG
    assert lib.dlrm_mlp_bf16_create(None, 1, None, None) == E
    assert lib.dlrm_mlp_bf16_pack(None, None, None, None, None) == E
    assert lib.dlrm_mlp_bf16_infer(None, None, 1, None, 0, 16, None, 0, 16, 0) == E
    assert lib.dlrm_mlp_bf16_destroy(None) == 0
