"""int4 row-quantized tables on the GPU: the quantizer's byte image and the dequantizer against the numpy restatement
(`quantize_rows4` / `pack_rows4` / `dequantize_rows4`, checked on the CPU in tests/test_q4_host.py), the dequantizing
gather against dlrm_maplookup over the dequantized set, `Q4Inference.infer` against `HotPath.infer` over the
dequantized set (both routes), bounds, graph capture and `DLRMModel.test(..., q4=)`.  Every check is an equality of
bits.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import q8_cases
from helpers import rand_indices

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLDAYS = os.path.join(ROOT, "tests", "golden", "dac", "alldays.txt")
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
ROWS = [2, 8, 40, 5000, 3, 1000]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _tables(pkg, gpu, ws, dtype, off=0):
    """The rows as a table set; off: every table starts `off` elements past a 256-B boundary."""
    ts = []
    for w in ws:
        buf = torch.zeros(w.size + off + 64, dtype=dtype, device=gpu)
        buf[off:off + w.size] = torch.from_numpy(w).reshape(-1).to(gpu).to(dtype)
        ts.append(buf[off:off + w.size].view(w.shape))
    return pkg.EmbeddingTableSet(ts)


def _rand_set(pkg, gpu, T, D, dtype, seed=0):
    rng = np.random.default_rng(1000 * T + D + seed)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ts = _tables(pkg, gpu, [rng.standard_normal((n, D)).astype(np.float32) for n in rows], dtype)
    return rng, rows, pkg.Quantized4TableSet.from_tables(ts)


def _indices(pkg, gpu, rng, rows, B, L=1, itype=torch.int32, base=0):
    idx = torch.from_numpy(rand_indices(rng, rows, B, L) + base).to(itype).to(gpu)
    return pkg.PackedIndices(idx.reshape(len(rows), B, L))


# ---- 1. the quantizer's byte image and the dequantizer against numpy
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,off", [(1, 0), (6, 0), (16, 0), (48, 0), (128, 0), (144, 0), (16, 1)])
def test_quantizer_equals_numpy(pkg, gpu, D, off, dtype):
    """off = 1: source rows at a non-16-B address take the element-wise kernels, with the same results."""
    nrows = [1, 3, 105, 1000]
    ws = q8_cases.mixed(D, nrows, seed=off)
    if dtype == torch.bfloat16:
        ws = [q8_cases.bf16_values(w) for w in ws]
    q4 = pkg.Quantized4TableSet.from_tables(_tables(pkg, gpu, ws, dtype, off))
    S = 8 + 8 * ((D + 15) // 16)
    assert q4.nrows() == nrows and q4.dim == D and q4.nbytes == 1109 * S
    backs = [q4.dequantize(dt) for dt in DTYPES]
    torch.cuda.synchronize()
    for t, w in enumerate(ws):
        q, scale, bias = pkg.quantize_rows4(w)
        assert np.array_equal(q4.rows[t].cpu().numpy(), pkg.pack_rows4(q, scale, bias)), (t, "byte image")
        for dt, back in zip(DTYPES, backs):
            want = pkg.dequantize_rows4(q, scale, bias, dtype=dt)
            assert np.array_equal(back[t].data.float().cpu().numpy().view(np.int32), want.view(np.int32)), (t, dt)


# ---- 2. the gather against dlrm_maplookup over the dequantized set
@pytest.mark.parametrize("L", [1, 9])
@pytest.mark.parametrize("T,D", [(7, 6), (7, 16), (7, 128), (26, 6), (26, 16), (26, 128)])
def test_gather_equals_maplookup_of_the_dequantized_set(pkg, gpu, T, D, L):
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, torch.float32)
    lib, ctx = q4.ctx.lib, q4.ctx
    k = 0
    for dtype in DTYPES:
        deq = q4.dequantize(dtype)
        for B in (1, 5, 70):
            itype, base = (torch.int32, torch.int64)[k % 2], (k // 2) % 2
            k += 1
            idx = _indices(pkg, gpu, rng, rows, B, L, itype, base)
            ld = D + T * D + 8  # out_offset = d, and a row longer than what is written
            got = torch.full((B, ld), -7.5, dtype=dtype, device=gpu)
            want = got.clone()
            ctx.check(lib.dlrm_q4_maplookup(ctx.bind(), q4.handle, _ptr(idx.data), idx.itype, idx.stride, base, B, L,
                                            (pkg._lib.F32 if dtype == torch.float32 else pkg._lib.BF16), _ptr(got), ld, D))
            ctx.check(lib.dlrm_maplookup(ctx.bind(), deq.handle, _ptr(idx.data), idx.itype, idx.stride, base, B, L,
                                         _ptr(want), ld, D))
            torch.cuda.synchronize()
            ctx.check_bounds()
            g = _bits(got)
            assert np.array_equal(g, _bits(want)), (dtype, B, itype, base)  # (the kept rest of each row included)
            assert (got[:, :D] == -7.5).all() and (got[:, D + T * D:] == -7.5).all() and (got[:, D:D + T * D] != -7.5).any()


# ---- 3. the forward against HotPath.infer over the dequantized set
def _forward(pkg, gpu, q4, deq, rng, rows, D, B, L, dtype, x_off=0):
    """(fused route's output or None, its raw status, the two-launch route's output, HotPath.infer's)."""
    T = len(rows)
    idx = _indices(pkg, gpu, rng, rows, B, L)
    xw = torch.from_numpy(rng.standard_normal((B, D + 16 + x_off)).astype(np.float32)).to(gpu).to(dtype)
    x = xw[:, x_off:x_off + D]
    eng = pkg.Q4Inference(q4, B, L, d=D, dtype=dtype)
    two = pkg.Q4Inference(q4, B, L, d=D, dtype=dtype)
    probe = torch.full((B, eng.width + 5), 3.25, dtype=dtype, device=gpu)
    rc = eng.fused(x, idx, probe)
    torch.cuda.synchronize()
    assert (probe[:, eng.width:] == 3.25).all()  # the rest of the row is kept
    if rc != pkg._lib.OK:
        assert (probe == 3.25).all()  # refused: nothing was launched
    eng.infer(x, idx)
    assert eng.route == ("fused" if rc == pkg._lib.OK else "two-launch")
    two.route = "two-launch"  # the forced fallback
    slow = _bits(two.infer(x, idx)).copy()
    want = _bits(pkg.HotPath(deq, B, L).infer(x, idx))
    torch.cuda.synchronize()
    eng.check_bounds()
    assert two.route == "two-launch"
    return (_bits(probe[:, :eng.width]) if rc == pkg._lib.OK else None), rc, slow, want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [16, 32, 128, 144])
@pytest.mark.parametrize("T", [7, 17, 26])
def test_forward_equals_infer_of_the_dequantized_set(pkg, gpu, T, D, dtype):
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, dtype)
    deq = q4.dequantize(dtype)
    for B in (1, 5):
        fused, rc, slow, want = _forward(pkg, gpu, q4, deq, rng, rows, D, B, 1, dtype)
        assert rc == pkg._lib.OK
        assert np.array_equal(slow, want), ("two-launch", B)
        assert np.array_equal(fused, want), ("fused", B)


@pytest.mark.parametrize("T,D,L,dtype,x_off,ok", [
    (31, 16, 1, torch.float32, 0, True), (32, 16, 1, torch.float32, 0, False), (1, 16, 1, torch.bfloat16, 0, True),
    (7, 16, 2, torch.float32, 0, False), (7, 8, 1, torch.float32, 0, False), (7, 24, 1, torch.bfloat16, 0, False),
    (7, 16, 1, torch.float32, 1, False), (7, 16, 1, torch.bfloat16, 4, False), (7, 16, 1, torch.bfloat16, 8, True)])
def test_forward_routes_on_both_sides_of_each_limit(pkg, gpu, T, D, L, dtype, x_off, ok):
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, dtype, seed=1)
    fused, rc, slow, want = _forward(pkg, gpu, q4, q4.dequantize(dtype), rng, rows, D, 5, L, dtype, x_off)
    assert rc == (pkg._lib.OK if ok else pkg._lib.E_UNSUPPORTED)
    assert np.array_equal(slow, want) and (fused is None or np.array_equal(fused, want))


def test_forward_on_exactly_summable_rows(pkg, gpu):
    """Rows of integers 0 .. 15 (plus an integer offset) quantize to themselves (scale 1), x holds integers in
    [-8, 8], and every sum of the Gram stays below 2^24: the output is the int64 Gram, exactly."""
    T, D, B = 26, 128, 5
    rng = np.random.default_rng(11)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ws = []
    for t, n in enumerate(rows):
        k = rng.integers(0, 16, size=(n, D))
        k[:, 0], k[:, -1] = 0, 15
        ws.append((k - (8 if t % 2 else 0)).astype(np.float32))
    q4 = pkg.Quantized4TableSet.from_tables(_tables(pkg, gpu, ws, torch.float32))
    for t, w in enumerate(ws):
        q, scale, bias = pkg.unpack_rows4(q4.rows[t].cpu().numpy(), D)
        assert (scale == 1.0).all() and np.array_equal(bias, w.min(axis=1)) and np.array_equal(q + bias[:, None], w)
    idx = rand_indices(rng, rows, B, 1)
    x = rng.integers(-8, 9, size=(B, D))
    eng = pkg.Q4Inference(q4, B, 1, dtype=torch.float32)
    got = eng.infer(torch.from_numpy(x.astype(np.float32)).to(gpu),
                    pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu))).cpu().numpy()
    assert eng.route == "fused"
    feat = np.stack([x] + [ws[t][idx[t]].astype(np.int64) for t in range(T)], axis=1)
    gram = np.einsum("bid,bjd->bij", feat, feat)
    assert np.abs(gram).max() < 2 ** 24
    want = np.concatenate([x] + [gram[:, i, :i] for i in range(1, T + 1)], axis=1)
    assert np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows_starting_in_every_8_byte_residue_of_a_line(pkg, gpu, dtype):
    """D = 128 rows of 72 bytes from a base 8 bytes past a 128-B boundary: 16 consecutive rows start in all 16
    residues, half of them cross a line, and half of the 16-byte loads are 8-B but not 16-B aligned."""
    T, D, N = 3, 128, 16
    rng = np.random.default_rng(5)
    ts = _tables(pkg, gpu, [rng.standard_normal((N, D)).astype(np.float32) for _ in range(T)], dtype)
    bufs = [torch.zeros(N * 72 + 256, dtype=torch.uint8, device=gpu) for _ in range(T)]
    assert all(b.data_ptr() % 128 == 0 for b in bufs)
    q4 = pkg.Quantized4TableSet.from_arrays([b[8:8 + N * 72].view(N, 72) for b in bufs], D).quantize_from(ts)
    assert sorted((8 + 72 * r) % 128 for r in range(N)) == list(range(0, 128, 8))
    idx = pkg.PackedIndices(torch.arange(N, dtype=torch.int32, device=gpu).repeat(T, 1))
    x = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(gpu).to(dtype)
    eng = pkg.Q4Inference(q4, N, 1, dtype=dtype)
    got = _bits(eng.infer(x, idx))
    assert eng.route == "fused"
    assert np.array_equal(got, _bits(pkg.HotPath(q4.dequantize(dtype), N, 1).infer(x, idx)))


# ---- 4. bounds, once per route
@pytest.mark.parametrize("route", ["fused", "two-launch"])
def test_an_index_out_of_range_is_a_zero_row_and_raises(pkg, gpu, route):
    T, D, B, base, b0, t0 = 26, 16, 5, 1, 3, 4
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, torch.float32, seed=2)
    clean = rand_indices(rng, rows, B, 1) + base
    bad = clean.copy()
    bad[t0, b0] = base + rows[t0]  # one past the last row
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu)
    eng = pkg.Q4Inference(q4, B, 1, dtype=torch.float32, index_base=base)
    eng.route = None if route == "fused" else "two-launch"
    outs = []
    for k, idx in enumerate((clean, bad)):
        outs.append(_bits(eng.infer(x, pkg.PackedIndices(torch.from_numpy(idx).to(torch.int64).to(gpu)))).copy())
        torch.cuda.synchronize()
        if k == 0:
            eng.check_bounds()
        else:
            with pytest.raises(pkg.BoundsError):
                eng.check_bounds()
        assert eng.route == route
    eng.check_bounds()  # the flag was cleared by the read
    i0 = t0 + 1
    zero = np.zeros(outs[0].shape, dtype=bool)
    for i in range(1, T + 1):
        for j in range(i):
            zero[b0, D + i * (i - 1) // 2 + j] = i0 in (i, j)
    assert (outs[1].view(np.float32)[zero] == 0).all() and zero.sum() == T and np.array_equal(outs[1][~zero], outs[0][~zero])


# ---- 5. graph capture
def test_infer_replays_from_a_captured_graph(pkg, gpu):
    T, D, B = 26, 128, 9
    rng, rows, q4 = _rand_set(pkg, gpu, T, D, torch.float32, seed=3)
    x = torch.empty((B, D), dtype=torch.float32, device=gpu)
    ibuf = torch.empty((T, B), dtype=torch.int32, device=gpu)
    idx = pkg.PackedIndices(ibuf)
    eng, eager = pkg.Q4Inference(q4, B, 1, dtype=torch.float32), pkg.Q4Inference(q4, B, 1, dtype=torch.float32)

    def fill():
        x.copy_(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)))
        ibuf.copy_(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32))

    fill()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        eng.infer(x, idx)
    torch.cuda.current_stream(gpu).wait_stream(side)
    assert eng.route == "fused"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.infer(x, idx)
    for _ in range(3):
        fill()
        graph.replay()
        torch.cuda.synchronize()
        got = _bits(eng.out).copy()
        assert np.array_equal(got, _bits(eager.infer(x, idx)))
    eng.check_bounds()


# ---- 6. the quantized model's metrics
def test_model_test_with_quantized_tables(pkg, gpu):
    dac = pkg.dac
    data = dac.parse_tsv(ALLDAYS)
    maps = dac.reindex(data)
    maps.reindex_(data)
    D, B, T = 16, 32, 26
    gen = torch.Generator(device=gpu).manual_seed(3)
    tables = [torch.empty((n, D), device=gpu).uniform_(-n ** -0.5, n ** -0.5, generator=gen) for n in maps.sizes()]
    bsz, tsz = pkg.kaggle_mlp_sizes(D, T)
    model = pkg.DLRMModel(pkg.random_mlp(bsz, sigmoid_last=False, generator=gen, device=gpu), tables,
                          pkg.random_mlp(tsz, sigmoid_last=True, generator=gen, device=gpu), B, 1, lr=0.05,
                          index_base=1)
    loader = pkg.DACLoader(data, B, gpu)
    first = [(dense.clone(), sparse.clone()) for _, dense, sparse in loader][0]
    q4 = model.quantize(bits=4)
    assert isinstance(model.quantize(), pkg.QuantizedTableSet)  # the default is as before
    assert q4.nrows() == list(maps.sizes()) and q4.nbytes == sum(maps.sizes()) * 16
    ev, probs = pkg.Evaluator(gpu), []
    res = model.test(loader, evaluator=ev, probs=probs, q4=q4)
    model.hot.check_bounds()
    got = ev.counts()
    assert len(probs) == 7 and got["total"] == 224 and model._q4[1].route == "fused"
    # the reference: the same model with the dequantized rows as its tables, scored without q4
    for t, back in enumerate(q4.dequantize(torch.float32)):
        model.tables[t].data.copy_(back.data)
    want_p = []
    model.test(loader, probs=want_p)
    assert np.array_equal(_bits(torch.cat(probs)), _bits(torch.cat(want_p)))
    want = pkg.eval_reference(torch.cat(want_p).cpu().numpy(), data["label"][:224].astype(np.float32))
    for n in ("total", "correct", "positives", "negatives"):
        assert got[n] == want[n], n
    assert np.array_equal(got["hist"], want["hist"]) and res["accuracy"] == got["correct"] / 224
    with pytest.raises(ValueError):
        model.predict(*first, q8=model.quantize(), q4=q4)
