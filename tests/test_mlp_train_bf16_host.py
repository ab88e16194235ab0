"""bf16 MLP training on the CPU: csrc/mlp_train_plan.hpp through dlrm_mlp_train_plan (pure host) and the ABI's
argument checks, which return before any HIP call."""
import pytest

BOTTOM, TOP = [13, 512, 256, 128], [479, 1024, 1024, 512, 256, 1]


def _al(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("sizes,batch,ld,slabs,slab_rows", [
    (BOTTOM, 2048, [64, 512, 256, 128], [32, 8, 32], [64, 256, 64]),
    (TOP, 2048, [512, 1024, 1024, 512, 256, 64], [2, 1, 2, 8, 32], [1024, 2048, 1024, 256, 64]),
    (BOTTOM, 8192, [64, 512, 256, 128], [32, 8, 32], [256, 1024, 256]),
    (TOP, 8192, [512, 1024, 1024, 512, 256, 64], [2, 1, 2, 8, 32], [4096, 8192, 4096, 1024, 256]),
    ([13, 1], 130, [64, 64], [3], [64]),
])
def test_plan(pkg, sizes, batch, ld, slabs, slab_rows):
    p = pkg.mlp_train_plan(sizes, batch)
    n = len(sizes) - 1
    ldt = (batch + 63) // 64 * 64
    assert p["rc"] == 0 and p["ld"] == ld and p["ldt"] == ldt
    assert p["slabs"] == slabs and p["slab_rows"] == slab_rows
    assert p["tile"] == [[64, 64, 64]] * 3
    for l in range(n):
        nt, kt = ld[l + 1] // 64, ld[l] // 64
        assert p["grid"][l] == [[nt, ldt // 64, 1], [kt, ldt // 64, 1], [nt, kt, slabs[l]]]
    K, N = sizes[:-1], sizes[1:]
    assert p["w_bytes"] == sum(_al(N[l] * ld[l] * 2) + _al(K[l] * ld[l + 1] * 2) for l in range(n))
    assert p["a_bytes"] == sum(_al(batch * ld[l] * 2) + _al(K[l] * ldt * 2) for l in range(n))
    assert p["g_bytes"] == sum(_al(batch * ld[l + 1] * 2) + _al(N[l] * ldt * 2) for l in range(n))
    assert p["p_bytes"] == max(256, sum(_al(slabs[l] * N[l] * K[l] * 4) + _al(slabs[l] * N[l] * 4)
                                        for l in range(n) if slabs[l] > 1))
    offs = [p[k][l] for k in ("w_off", "wt_off", "a_off", "at_off", "g_off", "gt_off", "p_off", "pb_off") for l in range(n)]
    assert all(o % 256 == 0 for o in offs)
    assert p["wt_off"][0] == _al(N[0] * ld[0] * 2) and p["at_off"][0] == _al(batch * ld[0] * 2)


def test_one_layer_13_to_1_sizes(pkg):
    p = pkg.mlp_train_plan([13, 1], 130)
    assert (p["w_bytes"], p["a_bytes"], p["g_bytes"], p["p_bytes"]) == (2048, 21760, 17152, 512)


def test_plan_errors(pkg):
    L = pkg._lib
    rc = lambda sizes, batch: pkg.mlp_train_plan(sizes, batch)["rc"]
    assert rc([13, 8193, 1], 64) == L.E_UNSUPPORTED and rc([13, 8192, 1], 64) == L.OK
    assert rc([8] * 10, 64) == L.E_UNSUPPORTED and rc([8] * 9, 64) == L.OK  # 9 layers, 8 layers
    assert rc([13], 64) == L.E_ARG and rc([13, 0, 1], 64) == L.E_ARG and rc([13, 1], 0) == L.E_ARG
    assert L.load().dlrm_mlp_train_plan(1, None, 64, None) == L.E_ARG


def test_null_arguments(pkg):
    lib, E = pkg._lib.load(), pkg._lib.E_ARG
    assert lib.dlrm_mlp_train_create(None, 1, None, 64, None) == E
    assert lib.dlrm_mlp_train_refresh(None, None, None, None, None) == E
    assert lib.dlrm_mlp_train_forward(None, None, 1, None, 0, 16, None, None, None, None, 0, 16, 0) == E
    assert lib.dlrm_mlp_train_backward(None, None, 1, None, 0, 16, None, 0, 0, None, None, None, None, None, None, None,
                                       1, None, 0, 0) == E
    assert lib.dlrm_mlp_train_destroy(None) == 0

    # a dtype that is neither fp32 nor bf16 is refused first, whatever else is passed
    U = pkg._lib.E_UNSUPPORTED
    assert lib.dlrm_mlp_train_forward(None, None, 1, None, 7, 16, None, None, None, None, 0, 16, 0) == U
    assert lib.dlrm_mlp_train_forward(None, None, 1, None, 0, 16, None, None, None, None, 2, 16, 0) == U
    assert lib.dlrm_mlp_train_backward(None, None, 1, None, 2, 16, None, 0, 0, None, None, None, None, None, None, None,
                                       1, None, 0, 0) == U
