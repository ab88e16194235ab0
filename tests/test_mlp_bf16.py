"""The fused bf16 MLP chain on the GPU (csrc/mlp_bf16.hip) against `mlp_bf16_reference` (numpy float64).

1. One layer within a derived bound.  Products of bf16 values are exact in fp32, so only the additions round: with r
   the reference and S = sum_k |a_k w_k| + |b|, an fp32 output satisfies |y - r| <= (K + 2) 2^-23 S (one 2^-23 per
   addition, whatever the MFMA's internal order and rounding); a bf16 output adds its one rounding:
   |y - r| <= e + 2^-8 (|r| + e).
2. Chains bit for bit on inputs whose every sum is a small integer in any order.
3. The wiring of DLRMModel.predict(mlp="bf16").
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mlp(pkg, gpu, Ws, bs, sigmoid_last=False):
    return pkg.DenseMLP([torch.from_numpy(w).to(gpu) for w in Ws], [torch.from_numpy(b).to(gpu) for b in bs],
                        sigmoid_last=sigmoid_last)


@functools.lru_cache(maxsize=None)
def _layer_case(pkg, B, K, N):
    rng = np.random.default_rng(1000 * K + N + B)
    x = rng.standard_normal((B, K)).astype(np.float32)
    W = rng.standard_normal((N, K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r, S = pkg.mlp_bf16_reference(x, [W], [b], False)
    return x, W, b, r, S


@pytest.mark.parametrize("last_relu", [False, True])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,N", [(13, 1), (32, 16), (479, 80), (64, 272), (1024, 1024)])
@pytest.mark.parametrize("B", [1, 33])
def test_one_layer_within_the_bound(pkg, gpu, B, K, N, x_dtype, out_dtype, last_relu):
    x, W, b, r, S = _layer_case(pkg, B, K, N)
    chain = pkg.Bf16MLP(_mlp(pkg, gpu, [W], [b]))
    y = chain.infer(torch.from_numpy(x).to(gpu).to(x_dtype), out_dtype=out_dtype, last_relu=last_relu)
    assert y.dtype == out_dtype and y.shape == (B, N)
    y = y.float().cpu().numpy().astype(np.float64)
    if last_relu:
        r = np.maximum(r, 0.0)
    bound = (K + 2) * 2.0 ** -23 * S
    if out_dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (np.abs(r) + bound)
    err = np.abs(y - r)
    print(f"B={B} K={K} N={N}: worst |y - r| / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()


CHAINS = [  # sizes, x dtype, out dtype, last relu
    ([13, 48, 1024, 32, 1], torch.float32, torch.float32, False),
    ([479, 1024, 1024, 16], torch.bfloat16, torch.float32, False),
    ([13, 512, 256, 128], torch.float32, torch.bfloat16, True),
    ([32, 16], torch.float32, torch.float32, False),
]


@functools.lru_cache(maxsize=None)
def _chain_case(pkg, ci, B):
    sizes, _, _, last_relu = CHAINS[ci]
    rng = np.random.default_rng(7 + ci)
    x = rng.integers(0, 3, size=(B, sizes[0])).astype(np.float32)
    Ws, bs = [], []
    for K, N in zip(sizes[:-1], sizes[1:]):
        W = np.zeros((N, K), np.float32)
        for n in range(N):
            W[n, rng.choice(K, 3, replace=False)] = rng.choice([-1.0, 1.0], 3)
        Ws.append(W)
        bs.append(rng.integers(0, 2, size=N).astype(np.float32))
    acts = []
    r, _ = pkg.mlp_bf16_reference(x, Ws, bs, last_relu, acts)
    # what makes the comparison exact, and not vacuous: asserted on the reference alone
    for a in acts + [r]:
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 256
    for a in acts:
        assert np.count_nonzero(a) >= a.size / 4
    return x, Ws, bs, r


# (4100: the plan's 32-row tile, with a partly filled last tile; the smaller batches take the 16-row tile)
@pytest.mark.parametrize("ci,B", [(ci, B) for ci in range(len(CHAINS)) for B in (1, 33, 65)] + [(0, 4100), (2, 4100)])
def test_chains_bit_for_bit_on_exactly_summable_inputs(pkg, gpu, ci, B):
    sizes, x_dtype, out_dtype, last_relu = CHAINS[ci]
    assert pkg.mlp_bf16_plan(sizes, B)["mt"] == (32 if B == 4100 else 16)
    x, Ws, bs, r = _chain_case(pkg, ci, B)
    chain = pkg.Bf16MLP(_mlp(pkg, gpu, Ws, bs))
    xw = torch.full((B, sizes[0] + 5), 3.0, dtype=x_dtype, device=gpu)  # x_ld > K
    xw[:, :sizes[0]] = torch.from_numpy(x).to(gpu).to(x_dtype)
    ow = torch.full((B, sizes[-1] + 3), -7.0, dtype=out_dtype, device=gpu)  # out_ld > N
    chain.infer(xw[:, :sizes[0]], out=ow[:, :sizes[-1]], last_relu=last_relu)
    got = ow.float().cpu().numpy()
    assert np.array_equal(got[:, :sizes[-1]], r.astype(np.float32))
    assert (got[:, sizes[-1]:] == -7.0).all()


@pytest.mark.parametrize("tdtype", [torch.float32, torch.bfloat16])
def test_predict_wiring(pkg, gpu, tdtype):
    T, D, B = 3, 16, 64
    rows = [50, 7, 1000]
    width = pkg.interaction_sizes(D, T + 1)[1]

    def model():
        gen = torch.Generator(device=gpu).manual_seed(5)
        tabs = [torch.empty((n, D), device=gpu).uniform_(-0.5, 0.5, generator=gen).to(tdtype) for n in rows]
        return pkg.DLRMModel(pkg.random_mlp([13, 32, D], sigmoid_last=False, generator=gen, device=gpu), tabs,
                             pkg.random_mlp([width, 48, 1], sigmoid_last=True, generator=gen, device=gpu), B, 1, lr=0.1)

    rng = np.random.default_rng(11)
    dense = torch.empty((B, 13), dtype=torch.float32, device=gpu)
    ibuf = torch.empty((T, B), dtype=torch.int32, device=gpu)
    sparse = pkg.PackedIndices(ibuf)
    labels = torch.from_numpy(rng.integers(0, 2, B).astype(np.float32)).to(gpu)

    def fill():
        dense.copy_(torch.from_numpy(rng.standard_normal((B, 13)).astype(np.float32)))
        ibuf.copy_(torch.from_numpy(np.stack([rng.integers(0, n, B) for n in rows])).to(torch.int32))

    def by_hand(m):
        x = pkg.Bf16MLP(m.bottom).infer(dense, out_dtype=tdtype)
        return pkg.Bf16MLP(m.top).infer(m.hot.infer(x, sparse), last_relu=False).clone()

    fill()
    a, b = model(), model()
    z0 = a.predict(dense, sparse, mlp="bf16").clone()
    assert z0.dtype == torch.float32 and z0.shape == (B, 1)
    assert torch.equal(z0, by_hand(a))
    assert not torch.equal(z0, a.predict(dense, sparse))  # (the fp32 MLPs: other bits)
    # a captured graph replays what the eager call computes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        zg = a.predict(dense, sparse, mlp="bf16")
    for _ in range(3):
        fill()
        graph.replay()
        assert torch.equal(zg, a.predict(dense, sparse, mlp="bf16"))
    # the inference leaves the training state alone
    la, lb = a.step(dense, sparse, labels).clone(), b.step(dense, sparse, labels).clone()
    assert torch.equal(la, lb)
    for p, q in zip(a.bottom.params() + a.top.params() + [a.tables[t].data for t in range(T)],
                    b.bottom.params() + b.top.params() + [b.tables[t].data for t in range(T)]):
        assert torch.equal(p, q)
    # the packed weights are the last repack's
    z1 = a.predict(dense, sparse, mlp="bf16").clone()
    a.repack()
    z2 = a.predict(dense, sparse, mlp="bf16").clone()
    assert not torch.equal(z1, z2)
    assert torch.equal(z2, by_hand(a))
    a.hot.check_bounds()
