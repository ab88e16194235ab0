"""dlrm_q4_bags_interact_fwd / `Q4Inference(bags=True)`: bits against the two-launch route and `HotPath.infer` over the
dequantized set, the int64 Gram of integer rows, limits, bounds, graph capture and `DLRMModel.predict(..., q4=)`."""
import numpy as np
import pytest
import torch

from helpers import rand_indices
from test_q4 import DTYPES, IDS, ROWS, _bits, _indices, _rand_set, _tables

pytestmark = pytest.mark.gpu


def _run(pkg, gpu, q4, deq, rng, rows, D, B, L, dtype, x_off=0):
    idx = _indices(pkg, gpu, rng, rows, B, L)
    xw = torch.from_numpy(rng.standard_normal((B, D + 16 + x_off)).astype(np.float32)).to(gpu).to(dtype)
    x = xw[:, x_off:x_off + D]
    eng = pkg.Q4Inference(q4, B, L, bags=True, d=D, dtype=dtype)
    two = pkg.Q4Inference(q4, B, L, bags=True, d=D, dtype=dtype)
    probe = torch.full((B, eng.width + 5), 3.25, dtype=dtype, device=gpu)
    rc = eng.bags_fused(x, idx, probe)
    torch.cuda.synchronize()
    # the rest of the row is kept; refused: nothing was launched
    assert (probe[:, eng.width:] == 3.25).all() and (rc == pkg._lib.OK or (probe == 3.25).all())
    got = _bits(eng.infer(x, idx)).copy()
    two.route = "two-launch"  # the forced fallback
    slow = _bits(two.infer(x, idx)).copy()
    want = _bits(pkg.HotPath(deq, B, L).infer(x, idx))
    torch.cuda.synchronize()
    eng.check_bounds()
    assert two.route == "two-launch" and (rc != pkg._lib.OK or np.array_equal(_bits(probe[:, :eng.width]), got))
    return rc, eng.route, got, slow, want

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T,L,D,B", [(1, 2, 16, 1), (15, 5, 48, 5), (16, 2, 128, 5), (32, 9, 144, 1), (48, 1, 256, 5),
                                     (64, 9, 256, 5), (95, 2, 16, 5)])
def test_bags_equal_two_launch_and_infer_of_the_dequantized_set(pkg, gpu, T, L, D, B, dtype):
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, dtype)
    rc, route, got, slow, want = _run(pkg, gpu, q4, q4.dequantize(dtype), rng, rows, D, B, L, dtype)
    assert rc == pkg._lib.OK and route == "bags" and np.array_equal(slow, want) and np.array_equal(got, want)

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bags_on_exactly_summable_rows(pkg, gpu, dtype):
    """Integer rows 0 .. 15 plus an offset quantize to themselves (scale 1); bags of 9 sum within +-135, exact in bf16;
    the Gram stays below 2^24: the output is the int64 Gram, rounded once where the output is bf16."""
    T, D, B, L = 40, 128, 5, 9
    rng = np.random.default_rng(12)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ws = []
    for t, n in enumerate(rows):
        k = rng.integers(0, 16, size=(n, D))
        k[:, 0], k[:, -1] = 0, 15  # every row spans 15: scale 1
        ws.append((k - (8 if t % 2 else 0)).astype(np.float32))
    q4 = pkg.Quantized4TableSet.from_tables(_tables(pkg, gpu, ws, dtype))
    idx = rand_indices(rng, rows, B, L).reshape(T, B, L)
    x = rng.integers(-8, 9, size=(B, D))
    eng = pkg.Q4Inference(q4, B, L, bags=True, dtype=dtype)
    got = eng.infer(torch.from_numpy(x.astype(np.float32)).to(gpu).to(dtype),
                    pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu)))
    assert eng.route == "bags"
    pooled = [ws[t].astype(np.int64)[idx[t]].sum(axis=1) for t in range(T)]
    feat = np.stack([x] + pooled, axis=1)
    gram = np.einsum("bid,bjd->bij", feat, feat)
    assert max(np.abs(p).max() for p in pooled) <= 135 and np.abs(gram).max() < 2 ** 24
    want = np.concatenate([x] + [gram[:, i, :i] for i in range(1, T + 1)], axis=1).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(torch.from_numpy(want).to(dtype)))

@pytest.mark.parametrize("T,D,dtype,x_off,ok", [
    (95, 16, torch.float32, 0, True), (96, 16, torch.float32, 0, False), (7, 16, torch.float32, 0, True),
    (7, 24, torch.bfloat16, 0, False), (7, 16, torch.bfloat16, 8, True), (7, 16, torch.bfloat16, 4, False)])
def test_bags_route_on_both_sides_of_each_limit(pkg, gpu, T, D, dtype, x_off, ok):
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, dtype, seed=1)
    rc, route, got, slow, want = _run(pkg, gpu, q4, q4.dequantize(dtype), rng, rows, D, 5, 2, dtype, x_off)
    assert rc == (pkg._lib.OK if ok else pkg._lib.E_UNSUPPORTED) and route == ("bags" if ok else "two-launch") \
        and np.array_equal(slow, want) and np.array_equal(got, want)
    plain = pkg.Q4Inference(q4, 5, 2, d=D, dtype=dtype)  # without the keyword nothing changes
    plain.infer(torch.zeros((5, D), dtype=dtype, device=gpu), _indices(pkg, gpu, rng, rows, 5, 2))
    assert plain.route == "two-launch"

def test_an_index_out_of_range_in_a_bag_is_a_zero_row_and_raises(pkg, gpu):
    T, D, B, L, base, b0, t0, k0 = 20, 16, 5, 5, 1, 3, 4, 3
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, torch.float32, seed=2)
    clean = (rand_indices(rng, rows, B, L) + base).reshape(T, B, L)
    bad = clean.copy()
    bad[t0, b0, k0] = base + rows[t0]  # one past the last row
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu)
    eng = pkg.Q4Inference(q4, B, L, bags=True, dtype=torch.float32, index_base=base)
    hot = pkg.HotPath(q4.dequantize(torch.float32), B, L, index_base=base)
    outs = []
    for k, idx in enumerate((clean, bad)):
        packed = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int64).to(gpu))
        outs.append(_bits(eng.infer(x, packed)).copy())
        torch.cuda.synchronize()
        eng.check_bounds() if k == 0 else pytest.raises(pkg.BoundsError, eng.check_bounds)
        assert eng.route == "bags"
    want = _bits(hot.infer(x, packed)).copy()  # the same bad index: that lookup's row replaced by zeros
    torch.cuda.synchronize()
    pytest.raises(pkg.BoundsError, hot.check_bounds)
    touched = np.zeros(outs[0].shape, dtype=bool)  # the Gram entries of feature t0 + 1 of sample b0
    for i in range(1, T + 1):
        touched[b0, [D + i * (i - 1) // 2 + j for j in range(i) if t0 + 1 in (i, j)]] = True
    assert touched.sum() == T and np.array_equal(outs[1][~touched], outs[0][~touched]) and np.array_equal(outs[1], want)

def test_bags_replay_from_a_captured_graph(pkg, gpu):
    T, D, B, L = 40, 128, 9, 3
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, torch.bfloat16, seed=3)
    x = torch.empty((B, D), dtype=torch.bfloat16, device=gpu)
    ibuf = torch.empty((T, B, L), dtype=torch.int32, device=gpu)
    idx = pkg.PackedIndices(ibuf)
    eng, eager = (pkg.Q4Inference(q4, B, L, bags=True, dtype=torch.bfloat16) for _ in range(2))

    def fill():
        x.copy_(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)))
        ibuf.copy_(torch.from_numpy(rand_indices(rng, rows, B, L)).to(torch.int32).reshape(T, B, L))

    fill()
    eng.infer(x, idx)  # (the route is chosen here; the bags route allocates nothing)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.infer(x, idx)
    for _ in range(3):
        fill()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(eng.out).copy(), _bits(eager.infer(x, idx)))
    assert eng.route == eager.route == "bags"

def test_pooled_model_predicts_on_quantized_tables_in_one_launch(pkg, gpu):
    D, B, T, L = 16, 8, 5, 3
    gen = torch.Generator(device=gpu).manual_seed(4)
    rows = ROWS[:T]
    tables = [torch.empty((n, D), device=gpu).uniform_(-1, 1, generator=gen) for n in rows]
    bsz, tsz = pkg.kaggle_mlp_sizes(D, T)
    model = pkg.DLRMModel(pkg.random_mlp(bsz, sigmoid_last=False, generator=gen, device=gpu), tables,
                          pkg.random_mlp(tsz, sigmoid_last=True, generator=gen, device=gpu), B, L, lr=0.05)
    rng = np.random.default_rng(6)
    dense = torch.from_numpy(rng.standard_normal((B, bsz[0])).astype(np.float32)).to(gpu)
    sparse = _indices(pkg, gpu, rng, rows, B, L)
    q4 = model.quantize(bits=4)
    got = _bits(model.predict(dense, sparse, q4=q4)).copy()
    assert model._q4[1].route == "bags"
    for t, back in enumerate(q4.dequantize(torch.float32)):
        model.tables[t].data.copy_(back.data)
    assert np.array_equal(got, _bits(model.predict(dense, sparse)))
    model.hot.check_bounds()
