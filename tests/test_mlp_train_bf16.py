"""bf16 MLP training on the GPU (csrc/mlp_train.hip) against numpy float64.

1. Every product within its bound, on the operands the kernels themselves stored (W16, the saved a_{l-1}, the stored
   g_l), so each layer is judged alone.  Products of bf16 values are exact in fp32 and only the additions round: an
   fp32 result of a contraction over n terms with S = sum |u v| (+ |b|) satisfies |y - r| <= (n + 2) 2^-23 S whatever
   the summation tree (tiles, slabs); a bf16 result adds its one rounding: |y - r| <= e + 2^-8 (|r| + e).
2. Bit for bit on inputs whose every sum is an integer below 2^24.
3. The wiring and the determinism of DLRMModel(..., mlp="bf16").
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
SINGLE = [[13, 1], [32, 16], [479, 80], [64, 272], [1024, 1024]]
# sizes, sigmoid-last, dx dtype (None: not needed)
CASES = ([(s, False, torch.float32) for s in SINGLE] +
         [([13, 48, 16], False, None), ([479, 64, 80, 1], True, torch.float32), ([479, 64, 80, 1], True, torch.bfloat16)])


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def nz(t):
    return bool((t != 0).any())


def within(y, r, e, bf16):
    return bool((np.abs(y - r) <= (e + 2.0 ** -8 * (np.abs(r) + e) if bf16 else e)).all())


@functools.lru_cache(maxsize=None)
def _inputs(sizes, B):
    rng = np.random.default_rng(sum(sizes) + B)
    Ws = [rng.standard_normal((n, k)).astype(np.float32) / np.float32(np.sqrt(k)) for k, n in zip(sizes[:-1], sizes[1:])]
    bs = [rng.standard_normal(n).astype(np.float32) for n in sizes[1:]]
    return (rng.standard_normal((B, sizes[0])).astype(np.float32), Ws, bs,
            (rng.standard_normal((B, sizes[-1])) / B).astype(np.float32))


def _train(pkg, gpu, Ws, bs, sigmoid_last, B):
    mlp = pkg.DenseMLP([torch.from_numpy(w).to(gpu) for w in Ws], [torch.from_numpy(b).to(gpu) for b in bs],
                       sigmoid_last=sigmoid_last)
    mlp.flatten()  # the gW views of the flat buffer: rows of 13 or 479 floats are not 16-B aligned
    return mlp, mlp.train_bf16(B)


@pytest.mark.parametrize("B", [1, 33, 130])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_every_product_within_its_bound(pkg, gpu, ci, B):
    sizes, sigmoid_last, dx_dtype = CASES[ci]
    n = len(sizes) - 1
    x, Ws, bs, dy = _inputs(tuple(sizes), B)
    mlp, tr = _train(pkg, gpu, Ws, bs, sigmoid_last, B)
    if B == 130:  # spans more than one slab wherever the plan cuts slabs (a layer of 256 tiles has none)
        assert sizes == [1024, 1024] or (tr.plan["slabs"][0] > 1 and tr.plan["slab_rows"][0] < B)
    Bp = (B + 63) // 64 * 64
    out = tr.forward(torch.from_numpy(x).to(gpu), out_dtype=torch.float32 if sigmoid_last else torch.bfloat16)
    mlp.gb[-1].fill_(-7.0)
    dx = tr.backward(torch.from_numpy(dy).to(gpu), need_dx=dx_dtype is not None, dx_dtype=dx_dtype)
    torch.cuda.synchronize()
    assert (dx is None) == (dx_dtype is None)

    # operands: exact roundings, both forms, zero padding
    assert torch.equal(tr.a[0][:B, :sizes[0]], torch.from_numpy(x).to(gpu).bfloat16())
    for l in range(n):
        K, N = sizes[l], sizes[l + 1]
        assert torch.equal(tr.W16[l][:, :K], mlp.W[l].bfloat16()) and torch.equal(tr.W16T[l][:, :N], tr.W16[l][:, :K].t())
        assert not nz(tr.W16[l][:, K:]) and not nz(tr.W16T[l][:, N:])
        for row, col, width in ((tr.a[l], tr.aT[l], K), (tr.g[l], tr.gT[l], N)):
            assert torch.equal(col[:, :B], row[:B, :width].t())
            assert not nz(row[:B, width:]) and not nz(col[:, B:Bp])

    a = [f64(t[:B, :k]) for t, k in zip(tr.a, sizes)]
    g = [f64(t[:B, :k]) for t, k in zip(tr.g, sizes[1:])]
    W16 = [f64(t[:, :k]) for t, k in zip(tr.W16, sizes)]
    yout = f64(out)
    # forward
    for l in range(n):
        b = bs[l].astype(np.float64)
        r = a[l] @ W16[l].T + b
        e = (sizes[l] + 2) * U * (np.abs(a[l]) @ np.abs(W16[l]).T + np.abs(b))
        if l < n - 1 or not sigmoid_last:
            r = np.maximum(r, 0.0)
        assert within(a[l + 1] if l < n - 1 else yout, r, e, l < n - 1 or not sigmoid_last), f"forward {l}"
    # g_n
    gn = torch.from_numpy(dy).to(gpu).bfloat16()
    assert torch.equal(tr.g[-1][:B, :sizes[-1]], gn if sigmoid_last else gn * (out > 0))
    # wgrad, gb, dgrad
    for l in range(n):
        e = (B + 2) * U * (np.abs(g[l]).T @ np.abs(a[l]))
        assert within(f64(mlp.gW[l]), g[l].T @ a[l], e, False), f"wgrad {l}"
        if l == n - 1 and sigmoid_last:
            assert (mlp.gb[l] == -7.0).all()
        else:
            assert within(f64(mlp.gb[l]), g[l].sum(0), (B + 2) * U * np.abs(g[l]).sum(0), False), f"gb {l}"
        if l == 0 and dx is None:
            continue
        r = g[l] @ W16[l]
        e = (sizes[l + 1] + 2) * U * (np.abs(g[l]) @ np.abs(W16[l]))
        if l == 0:
            assert dx.dtype == dx_dtype and within(f64(dx), r, e, dx_dtype == torch.bfloat16), "dx"
        else:
            mask = a[l] > 0
            assert not g[l - 1][~mask].any()  # masked elements are exactly zero
            assert within(g[l - 1], r * mask, e, True), f"dgrad {l}"


@pytest.mark.parametrize("B", [33, 130])
@pytest.mark.parametrize("K,N", SINGLE)
def test_bit_for_bit_on_exactly_summable_inputs(pkg, gpu, K, N, B):
    rng = np.random.default_rng(K + N + B)
    x, dy = rng.integers(-4, 5, (B, K)), rng.integers(-4, 5, (B, N))
    W, b = rng.integers(-2, 3, (N, K)), rng.integers(-2, 3, N)
    out = np.maximum(x @ W.T + b, 0)  # int64: every sum is below 2^24
    gl = dy * (out > 0)
    mlp, tr = _train(pkg, gpu, [W.astype(np.float32)], [b.astype(np.float32)], False, B)
    xg, dyg = torch.from_numpy(x.astype(np.float32)).to(gpu), torch.from_numpy(dy.astype(np.float32)).to(gpu)

    def exact(t, ref):
        return torch.equal(t, torch.from_numpy(ref.astype(np.float32)).to(gpu).to(t.dtype))

    for dt in (torch.float32, torch.bfloat16):  # (a bf16 result is the rounding of the exact value)
        mlp.flat_grad.fill_(3.0)
        assert exact(tr.forward(xg.to(dt), out_dtype=dt), out)
        assert exact(tr.backward(dyg.to(dt), dx_dtype=dt), gl @ W)
        assert exact(mlp.gW[0], gl.T @ x) and exact(mlp.gb[0], gl.sum(0))


@pytest.mark.parametrize("tdtype", [torch.float32, torch.bfloat16])
def test_step_wiring_and_determinism(pkg, gpu, tdtype):
    T, D, B, rows = 3, 16, 33, [50, 7, 1000]
    width = pkg.interaction_sizes(D, T + 1)[1]

    def model(mlp):
        gen = torch.Generator(device=gpu).manual_seed(5)
        tabs = [torch.empty((n, D), device=gpu).uniform_(-0.5, 0.5, generator=gen).to(tdtype) for n in rows]
        return pkg.DLRMModel(pkg.random_mlp([13, 32, D], sigmoid_last=False, generator=gen, device=gpu), tabs,
                             pkg.random_mlp([width, 48, 1], sigmoid_last=True, generator=gen, device=gpu), B, 1, lr=0.1,
                             mlp=mlp)

    def state(m):
        return [m.loss] + m.bottom.params() + m.top.params() + [m.tables[t].data for t in range(T)]

    rng = np.random.default_rng(11)
    dense = torch.from_numpy(rng.standard_normal((B, 13)).astype(np.float32)).to(gpu)
    sparse = pkg.PackedIndices(torch.from_numpy(np.stack([rng.integers(0, n, B) for n in rows])).to(torch.int32).to(gpu))
    labels = torch.from_numpy(rng.integers(0, 2, B).astype(np.float32)).to(gpu)

    a, b, c, plain = model("bf16"), model("bf16"), model("bf16"), model(None)
    plain.step(dense, sparse, labels)
    assert plain.bottom._train16 is None and plain.top._train16 is None
    for _ in range(2):
        a.step(dense, sparse, labels)
    # the kernel's own logits give the loss; W16 follows the updated master
    z = a._z16.reshape(-1)
    ref = pkg.bce_loss(torch.sigmoid(z.double()), labels.double())
    assert abs(float(a.loss) - float(ref)) <= 1e-6 * abs(float(ref))
    for tr in a._mlp16:
        for l, w in enumerate(tr.mlp.W):
            assert torch.equal(tr.W16[l][:, :w.shape[1]], w.bfloat16())
    assert not torch.equal(a.loss, plain.loss)  # (two bf16 steps against one fp32 step: other bits)
    # a second model from the same seed: the same bits
    for _ in range(2):
        b.step(dense, sparse, labels)
    assert all(torch.equal(p, q) for p, q in zip(state(a), state(b)))
    # a captured step, replayed, is the eager step: loss, every MLP parameter, every table, replay after replay
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            c.step(dense, sparse, labels)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(3):
        graph.replay()
        if k == 2:
            a.step(dense, sparse, labels)
        torch.cuda.synchronize()
        if k >= 1:
            assert all(torch.equal(p, q) for p, q in zip(state(a), state(c))), k
    a.hot.check_bounds()
