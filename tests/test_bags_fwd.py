"""dlrm_bags_interact_fwd / `HotPath(bags=True)`: bits against dlrm_maplookup + dlrm_interact_fwd with and without ys, a
float64 bound, the int64 Gram of integer rows, both sides of each limit, bounds, graph capture, the training forward."""
import numpy as np
import pytest
import torch

from helpers import rand_indices
from test_q4 import DTYPES, IDS, ROWS, _bits, _tables

pytestmark = pytest.mark.gpu
PROBE = 3.25

def _setup(pkg, gpu, T, D, B, L, dtype, seed=0, x_off=0, base=0):
    """(table set, [T][B][L] indices, the same packed, x: a [B][D] view x_off elements into rows of D + 24)."""
    rng = np.random.default_rng(1000 * T + D + seed)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ts = _tables(pkg, gpu, [rng.standard_normal((n, D)).astype(np.float32) for n in rows], dtype)
    idx = (rand_indices(rng, rows, B, L) + base).reshape(T, B, L)
    xw = torch.from_numpy(rng.standard_normal((B, D + 24)).astype(np.float32)).to(gpu).to(dtype)
    return ts, idx, pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu)), xw[:, x_off:x_off + D]

def _two_launch(pkg, ts, B, L, x, pidx):
    """(out, ys) bits of dlrm_maplookup + dlrm_interact_fwd: the forced route of an engine without the keyword."""
    ref = pkg.HotPath(ts, B, L)
    ref.infer_route = "two-launch"
    return _bits(ref.infer(x, pidx)).copy(), _bits(ref._infer_ys).copy()

def _raw(hp, x, pidx, ys_pad=8):
    """The entry point into probe-filled buffers, with ys and without: [(rc, out, ys or None)]."""
    full = lambda n: torch.full((hp.B, n), PROBE, dtype=x.dtype, device=x.device)
    bufs = [(full(hp.width + 5), full(hp.F * hp.D + ys_pad)), (full(hp.width + 5), None)]
    res = [(hp.bags_interact_fwd(x, pidx, ys, out), out, ys) for out, ys in bufs]
    torch.cuda.synchronize()
    return res

def _check_float64(ts, idx, ys_bits, out_bits, D, dtype):
    """Pooled sums and Gram in float64.  A bag of L fp32 adds: L 2^-24 sum|row|; the Gram, on the pooled operands as
    the kernel rounds them (ys): e = (d + 2) 2^-23 S, S = sum|u v|, per fp32 result; bf16 results e + 2^-8 (|r| + e)."""
    T, B, L = idx.shape
    back, wide = (lambda b: torch.from_numpy(b).view(dtype).double().numpy()), dtype == torch.float32
    feat, got = back(ys_bits).reshape(B, T + 1, D), back(out_bits)
    rows = np.stack([ts[t].data.double().cpu().numpy()[idx[t]] for t in range(T)], axis=1)  # [B][T][L][D]
    r, e = rows.sum(axis=2), L * 2.0 ** -24 * np.abs(rows).sum(axis=2)
    assert (np.abs(feat[:, 1:] - r) <= (e if wide else e + 2.0 ** -8 * (np.abs(r) + e))).all()
    r = np.einsum("bid,bjd->bij", feat, feat)
    e = (D + 2) * 2.0 ** -23 * np.einsum("bid,bjd->bij", np.abs(feat), np.abs(feat))
    bound = e if wide else e + 2.0 ** -8 * (np.abs(r) + e)
    for i in range(1, T + 1):
        lo = D + i * (i - 1) // 2
        assert (np.abs(got[:, lo:lo + i] - r[:, i, :i]) <= bound[:, i, :i]).all(), i

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T,L,D,B", [(1, 2, 16, 1), (15, 5, 48, 5), (16, 2, 128, 5), (32, 9, 136, 1), (48, 1, 256, 5),
                                     (64, 9, 256, 5), (95, 2, 16, 5)])
def test_bags_equal_the_two_launches_with_and_without_ys(pkg, gpu, T, L, D, B, dtype):
    ts, idx, pidx, x = _setup(pkg, gpu, T, D, B, L, dtype)
    want, want_ys = _two_launch(pkg, ts, B, L, x, pidx)
    hp = pkg.HotPath(ts, B, L, bags=True)
    W, Y = hp.width, hp.F * D
    for rc, out, ys in _raw(hp, x, pidx):
        assert rc == pkg._lib.OK and np.array_equal(_bits(out[:, :W]), want) and (out[:, W:] == PROBE).all()
        assert ys is None or (np.array_equal(_bits(ys[:, :Y]), want_ys) and (ys[:, Y:] == PROBE).all())
    assert np.array_equal(_bits(hp.infer(x, pidx)), want) and hp.infer_route == "bags"
    hp.check_bounds()
    if (T, L) == (64, 9):
        _check_float64(ts, idx, want_ys, want, D, dtype)

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bags_on_exactly_summable_rows(pkg, gpu, dtype):
    """Integer rows in [-8, 7] and x in [-8, 8]: bags of 9 sum within +-72, exact in bf16, and the Gram stays below
    2^24: the output is the int64 Gram, rounded once where the output is bf16."""
    T, D, B, L = 40, 128, 5, 9
    rng = np.random.default_rng(12)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ws = [rng.integers(-8, 8, size=(n, D)) for n in rows]
    idx, x = rand_indices(rng, rows, B, L).reshape(T, B, L), rng.integers(-8, 9, size=(B, D))
    hp = pkg.HotPath(_tables(pkg, gpu, [w.astype(np.float32) for w in ws], dtype), B, L, bags=True)
    got = hp.infer(torch.from_numpy(x.astype(np.float32)).to(gpu).to(dtype),
                   pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu)))
    feat = np.stack([x] + [ws[t][idx[t]].sum(axis=1) for t in range(T)], axis=1)
    gram = np.einsum("bid,bjd->bij", feat, feat)
    assert hp.infer_route == "bags" and np.abs(feat[:, 1:]).max() <= 72 and np.abs(gram).max() < 2 ** 24
    want = np.concatenate([x] + [gram[:, i, :i] for i in range(1, T + 1)], axis=1).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(torch.from_numpy(want).to(dtype)))

@pytest.mark.parametrize("T,D,dtype,x_off,ys_pad,ok", [
    (95, 16, torch.float32, 0, 8, True), (96, 16, torch.float32, 0, 8, False), (7, 12, torch.float32, 0, 8, True),
    (7, 12, torch.bfloat16, 0, 8, False), (7, 16, torch.float32, 4, 8, True), (7, 16, torch.float32, 1, 8, False),
    (7, 16, torch.float32, 0, 6, False)])
def test_bags_on_both_sides_of_each_limit(pkg, gpu, T, D, dtype, x_off, ys_pad, ok):
    """T = 95 / 96; d = 12 in fp32 / bf16; x 16 B / 4 B past a 16-B boundary; a ys leading dimension off a vector."""
    B, L = 5, 2
    ts, idx, pidx, x = _setup(pkg, gpu, T, D, B, L, dtype, seed=1, x_off=x_off)
    want, want_ys = _two_launch(pkg, ts, B, L, x, pidx)
    hp = pkg.HotPath(ts, B, L, bags=True)
    (rc, out, ys), (rc0, out0, _) = _raw(hp, x, pidx, ys_pad)
    assert rc == (pkg._lib.OK if ok else pkg._lib.E_UNSUPPORTED)
    if ok:
        assert np.array_equal(_bits(out[:, :hp.width]), want) and np.array_equal(_bits(ys[:, :hp.F * D]), want_ys)
    else:  # nothing was launched
        assert (out == PROBE).all() and (ys == PROBE).all() and (rc0 == pkg._lib.OK or (out0 == PROBE).all())
    assert np.array_equal(_bits(hp.infer(x, pidx)), want) and (hp.infer_route == "bags") == (rc0 == pkg._lib.OK)
    plain = pkg.HotPath(ts, B, L)  # without the keyword nothing changes
    assert np.array_equal(_bits(plain.infer(x, pidx)), want) and plain.infer_route in ("fused", "two-launch")

def test_an_index_out_of_range_in_a_bag_is_a_zero_row_and_raises(pkg, gpu):
    T, D, B, L, base, b0, t0, k0 = 20, 16, 5, 5, 1, 3, 4, 3
    ts, clean, _, x = _setup(pkg, gpu, T, D, B, L, torch.float32, seed=2, base=base)
    bad = clean.copy()
    bad[t0, b0, k0] = base + len(ts[t0])  # one past the last row
    hp, plain = pkg.HotPath(ts, B, L, bags=True, index_base=base), pkg.HotPath(ts, B, L, index_base=base)
    outs = []
    for k, idx in enumerate((clean, bad)):
        packed = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int64).to(gpu))
        outs.append(_bits(hp.infer(x, packed)).copy())
        torch.cuda.synchronize()
        hp.check_bounds() if k == 0 else pytest.raises(pkg.BoundsError, hp.check_bounds)
        assert hp.infer_route == "bags"
    want = _bits(plain.infer(x, packed)).copy()  # the same bad index: that lookup's row replaced by zeros
    torch.cuda.synchronize()
    pytest.raises(pkg.BoundsError, plain.check_bounds)
    touched = np.zeros(outs[0].shape, dtype=bool)  # the Gram entries of feature t0 + 1 of sample b0
    for i in range(1, T + 1):
        touched[b0, [D + i * (i - 1) // 2 + j for j in range(i) if t0 + 1 in (i, j)]] = True
    assert touched.sum() == T and np.array_equal(outs[1][~touched], outs[0][~touched]) and np.array_equal(outs[1], want)

def test_bags_replay_from_a_captured_graph(pkg, gpu):
    T, D, B, L = 40, 128, 9, 3
    ts, _, _, _ = _setup(pkg, gpu, T, D, B, L, torch.bfloat16, seed=3)
    rng, rows = np.random.default_rng(3), [len(t) for t in ts]
    x, ibuf = torch.empty((B, D), dtype=torch.bfloat16, device=gpu), torch.empty((T, B, L), dtype=torch.int32, device=gpu)
    idx = pkg.PackedIndices(ibuf)
    eng, eager = (pkg.HotPath(ts, B, L, bags=True) for _ in range(2))

    def fill():
        x.copy_(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)))
        ibuf.copy_(torch.from_numpy(rand_indices(rng, rows, B, L)).to(torch.int32).reshape(T, B, L))

    fill()
    eng.infer(x, idx)  # (the bags route allocates nothing)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.infer(x, idx)
    for _ in range(3):
        fill()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(eng.out).copy(), _bits(eager.infer(x, idx)))
    assert eng.infer_route == eager.infer_route == "bags"

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_training_step_on_the_bags_forward(pkg, gpu, dtype):
    """A pooled operator-route step (ys kept) on the bags forward against the same step without: out, dx, the tables.
    (bags=True alone keeps the two launches there: the forward with ys measured slower)"""
    T, D, B, L = 40, 32, 5, 3
    res = []
    for bags in (True, False):
        ts, _, pidx, x = _setup(pkg, gpu, T, D, B, L, dtype, seed=4)
        hp = pkg.HotPath(ts, B, L, lr=0.05, pad_to=8, bags=True, bags_forward=bags)
        dout = torch.from_numpy(np.random.default_rng(5).standard_normal((B, hp.width)).astype(np.float32)).to(gpu).to(dtype)
        dx = hp.step(x, pidx, dout)
        torch.cuda.synchronize()
        hp.check_bounds()
        assert not hp.step_api and hp.fwd_route == ("bags" if bags else "fused")
        res.append([_bits(hp.out), _bits(hp.ys), _bits(dx)] + [_bits(t.data) for t in ts])
    assert all(np.array_equal(a, b) for a, b in zip(*res))
