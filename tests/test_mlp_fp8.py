"""The fused MXFP8 MLP chain on the GPU (csrc/mlp_fp8.hip) against `mlp_fp8_reference` (numpy float64).

1. One layer within a derived bound.  Products of e4m3 values and their power-of-two block scalings are exact in
   fp32, so only the additions round: with r the reference and S = sum_k |a_k w_k| + |b| over the dequantised
   operands, an fp32 output satisfies |y - r| <= (K + 2) 2^-23 S, times the measured factor of the instruction's
   internal accumulation (MFMA_FACTOR below); a bf16 output adds its one rounding:
   |y - r| <= e + 2^-8 (|r| + e).  One wrong scale, lane or rounding moves a result by about 2^-4 of a term.
2. Chains bit for bit on inputs whose every sum is a small integer that MXFP8 holds exactly.
3. The hidden re-quantisation bit for bit where it is lossy: an exact first layer, a signed selection as the second.
4. The wiring of DLRMModel.predict(mlp="fp8").
"""
import functools
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# The block-scaled MFMA does not keep one fp32 ulp per addition: against (K + 2) 2^-23 S the MI355X gives a worst
# |y - r| / bound of 8.26 (K = 13), 5.93 (K = 32), 0.84 (K = 128), 0.10 (K = 479), 0.035 (K = 1024) on fp32 outputs --
# an error of about 2^-16 S whatever K, the instruction's internal alignment of its 128 products; a wrong e4m3 step
# would be a ratio in the thousands.  The bound carries the next power of two above the worst ratio.
MFMA_FACTOR = 16


def _mlp(pkg, gpu, Ws, bs, sigmoid_last=False):
    return pkg.DenseMLP([torch.from_numpy(w).to(gpu) for w in Ws], [torch.from_numpy(b).to(gpu) for b in bs],
                        sigmoid_last=sigmoid_last)


@functools.lru_cache(maxsize=None)
def _layer_case(pkg, B, K, N, x_dtype):
    rng = np.random.default_rng(1000 * K + N + B)
    x = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).to(x_dtype)
    W = rng.standard_normal((N, K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r, S = pkg.mlp_fp8_reference(x.float().numpy(), [W], [b], False)
    return x, W, b, r, S


@pytest.mark.parametrize("last_relu", [False, True])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,N", [(13, 1), (32, 16), (479, 80), (128, 272), (1024, 1024)])
@pytest.mark.parametrize("B", [1, 33])
def test_one_layer_within_the_bound(pkg, gpu, B, K, N, x_dtype, out_dtype, last_relu):
    x, W, b, r, S = _layer_case(pkg, B, K, N, x_dtype)
    chain = pkg.Fp8MLP(_mlp(pkg, gpu, [W], [b]))
    y = chain.infer(x.to(gpu), out_dtype=out_dtype, last_relu=last_relu)
    assert y.dtype == out_dtype and y.shape == (B, N)
    y = y.float().cpu().numpy().astype(np.float64)
    if last_relu:
        r = np.maximum(r, 0.0)
    bound = MFMA_FACTOR * (K + 2) * 2.0 ** -23 * S
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
    """x in 0..2, a +1 and a -1 per weight row, biases 0 / 1: an activation grows by one per layer and stays below 15,
    so every value has at most four significant bits and no block maximum saturates."""
    sizes, _, _, last_relu = CHAINS[ci]
    rng = np.random.default_rng(7 + ci)
    x = rng.integers(0, 3, size=(B, sizes[0])).astype(np.float32)
    Ws, bs = [], []
    for K, N in zip(sizes[:-1], sizes[1:]):
        W = np.zeros((N, K), np.float32)
        for n in range(N):
            W[n, rng.choice(K, 2, replace=False)] = [1.0, -1.0]
        Ws.append(W)
        bs.append(rng.integers(0, 2, size=N).astype(np.float32))
    acts = []
    r, _ = pkg.mlp_fp8_reference(x, Ws, bs, last_relu, acts)
    # what makes the comparison exact, and not vacuous: asserted on the reference alone.  Every hidden activation
    # survives the quantisation unchanged (it equals the chain computed without any), and a quarter is non-zero.
    a = x.astype(np.float64)
    for W, b, q in zip(Ws, bs, acts):
        a = np.maximum(a @ W.T.astype(np.float64) + b, 0.0)
        assert np.array_equal(a, q) and np.count_nonzero(a) >= a.size / 4
    return x, Ws, bs, r


# (4100: the plan's 32-row tile, with a partly filled last tile; the smaller batches take the 16-row tile)
@pytest.mark.parametrize("ci,B", [(ci, B) for ci in range(len(CHAINS)) for B in (1, 33, 65)] + [(0, 4100), (2, 4100)])
def test_chains_bit_for_bit_on_exactly_summable_inputs(pkg, gpu, ci, B):
    sizes, x_dtype, out_dtype, last_relu = CHAINS[ci]
    assert pkg.mlp_fp8_plan(sizes, B)["mt"] == (32 if B == 4100 else 16)
    _run_chain(pkg, gpu, ci, B)


def _run_chain(pkg, gpu, ci, B):
    sizes, x_dtype, out_dtype, last_relu = CHAINS[ci]
    x, Ws, bs, r = _chain_case(pkg, ci, B)
    chain = pkg.Fp8MLP(_mlp(pkg, gpu, Ws, bs))
    xw = torch.full((B, sizes[0] + 5), 3.0, dtype=x_dtype, device=gpu)  # x_ld > K
    xw[:, :sizes[0]] = torch.from_numpy(x).to(gpu).to(x_dtype)
    ow = torch.full((B, sizes[-1] + 3), -7.0, dtype=out_dtype, device=gpu)  # out_ld > N
    chain.infer(xw[:, :sizes[0]], out=ow[:, :sizes[-1]], last_relu=last_relu)
    got = ow.float().cpu().numpy()
    assert np.array_equal(got[:, :sizes[-1]], r.astype(np.float32))
    assert (got[:, sizes[-1]:] == -7.0).all()


def test_forced_64_row_tile_in_a_process_of_its_own(gpu):
    """DLRM_MLP_FP8_MT is read once per process: the 64-row tile (no batch takes it by the rule) runs two chains, the
    last tile partly filled, in a child."""
    code = ("import sys, torch; sys.path[:0] = [%r, %r]; import dlrm_pkg, test_mlp_fp8 as t; pkg = dlrm_pkg.load(); "
            "assert pkg.mlp_fp8_plan([13, 1], 80)['mt'] == 64; "
            "[t._run_chain(pkg, torch.device('cuda:0'), ci, 80) for ci in (0, 2)]; print('tile64 ok')"
            % (os.path.dirname(HERE), HERE))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DLRM_MLP_FP8_MT="64"), capture_output=True,
                         text=True)
    assert res.returncode == 0 and "tile64 ok" in res.stdout, res.stderr[-2000:]


@functools.lru_cache(maxsize=None)
def _requant_case(pkg, B, H):
    """Layer 1: x in 0..14 and, per block of 32 hidden features, weights and biases that are integers times a power
    of two 2^-p, so a row's terms share the grid 2^-p and every partial sum is below 2^24 grid steps: exact in fp32
    in any order, with up to 13 significant bits.  Feature 0 is the constant 3968 2^-p (no weights), the maximum of its
    block, which saturates (496 -> 448).  Layer 2: a signed permutation, no bias."""
    K = 40
    rng = np.random.default_rng(31 + H + B)
    x = rng.integers(0, 15, size=(B, K)).astype(np.float32)
    grid = 2.0 ** -(3.0 * (np.arange(H) // 32) - 6)
    W1 = (rng.integers(-7, 8, size=(H, K)) * grid[:, None]).astype(np.float32)
    b1 = (rng.integers(0, 500, size=H) * grid).astype(np.float32)
    W1[0], b1[0] = 0.0, 3968 * grid[0]
    W2 = np.zeros((H, H), np.float32)
    W2[np.arange(H), rng.permutation(H)] = rng.choice([-1.0, 1.0], H)
    b2 = np.zeros(H, np.float32)
    acts = []
    r, _ = pkg.mlp_fp8_reference(x, [W1, W2], [b1, b2], False, acts)
    x64, W64 = x.astype(np.float64), W1.astype(np.float64)
    assert np.array_equal(pkg.mx_quantize(x64)[2][:, :K], x64) and np.array_equal(pkg.mx_quantize(W64)[2][:, :K], W64)
    assert ((np.abs(x64) @ np.abs(W64).T + b1) / grid < 2.0 ** 24).all()
    h = np.maximum(x64 @ W64.T + b1, 0.0)
    assert np.array_equal(h / grid, np.rint(h / grid))
    assert (h != acts[0]).mean() >= 0.25 and (acts[0][:, 0] == 3584 * grid[0]).all()
    assert len(np.unique(pkg.mx_quantize(h)[1])) >= H // 32  # blocks of varied magnitude
    return x, [W1, W2], [b1, b2], r


@pytest.mark.parametrize("H", [64, 272])
@pytest.mark.parametrize("B", [1, 33])
def test_hidden_requantisation_bit_for_bit(pkg, gpu, B, H):
    x, Ws, bs, r = _requant_case(pkg, B, H)
    y = pkg.Fp8MLP(_mlp(pkg, gpu, Ws, bs)).infer(torch.from_numpy(x).to(gpu), last_relu=False)
    assert np.array_equal(y.cpu().numpy(), r.astype(np.float32))


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

    def by_hand(m, hot):
        x = pkg.Fp8MLP(m.bottom).infer(dense, out_dtype=tdtype)
        return pkg.Fp8MLP(m.top).infer(hot.infer(x, sparse), last_relu=False).clone()

    fill()
    a, b = model(), model()
    z0 = a.predict(dense, sparse, mlp="fp8").clone()
    assert z0.dtype == torch.float32 and z0.shape == (B, 1)
    assert torch.equal(z0, by_hand(a, a.hot))
    assert not torch.equal(z0, a.predict(dense, sparse, mlp="bf16"))  # (the bf16 chains: other bits)
    q4 = a.quantize(bits=4)
    assert torch.equal(a.predict(dense, sparse, mlp="fp8", q4=q4), by_hand(a, a._q4_engine(q4)))
    # a captured graph replays what the eager call computes.  (A chain handle frees device memory when it is
    # collected, and a DenseMLP and its chain refer to each other: dead ones must not be collected inside the capture.)
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        zg = a.predict(dense, sparse, mlp="fp8")
    for _ in range(3):
        fill()
        graph.replay()
        assert torch.equal(zg, a.predict(dense, sparse, mlp="fp8"))
    # the inference leaves the training state alone
    la, lb = a.step(dense, sparse, labels).clone(), b.step(dense, sparse, labels).clone()
    assert torch.equal(la, lb)
    for p, q in zip(a.bottom.params() + a.top.params() + [a.tables[t].data for t in range(T)],
                    b.bottom.params() + b.top.params() + [b.tables[t].data for t in range(T)]):
        assert torch.equal(p, q)
    # the packed weights are the last repack's
    z1 = a.predict(dense, sparse, mlp="fp8").clone()
    a.repack(mlp="fp8")
    z2 = a.predict(dense, sparse, mlp="fp8").clone()
    assert not torch.equal(z1, z2)
    assert torch.equal(z2, by_hand(a, a.hot))
    a.hot.check_bounds()
