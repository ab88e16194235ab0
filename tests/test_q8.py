"""int8 row-quantized tables on the GPU: the quantizer and the dequantizer against the numpy restatement
(`quantize_rows` / `dequantize_rows`, checked on the CPU in tests/test_q8_host.py), the dequantizing gather against
dlrm_maplookup over the dequantized set, `Q8Inference.infer` against `HotPath.infer` over the dequantized set (both
routes, bit for bit), bounds, 64-bit row offsets, graph capture and `DLRMModel.test(..., q8=)`.

Everything here is an equality of bits: the dequantizer is the yardstick, and it is held to numpy float32.
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


def _f32bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _tables(pkg, gpu, ws, dtype):
    return pkg.EmbeddingTableSet([torch.from_numpy(w).to(gpu).to(dtype) for w in ws])


def _rand_set(pkg, gpu, T, D, dtype, seed=0):
    rng = np.random.default_rng(1000 * T + D + seed)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ws = [rng.standard_normal((n, D)).astype(np.float32) for n in rows]
    ts = _tables(pkg, gpu, ws, dtype)
    return rng, rows, ts, pkg.QuantizedTableSet.from_tables(ts)


def _offset_codes(gpu, rows, D, off):
    """Code arrays whose pointers sit `off` bytes past a 256-B boundary."""
    out = []
    for n in rows:
        buf = torch.zeros(n * D + 256, dtype=torch.uint8, device=gpu)
        assert buf.data_ptr() % 256 == 0
        out.append(buf[off:off + n * D].view(n, D))
    return out


def _check_quantized(pkg, q8, ws, what):
    for t, w in enumerate(ws):
        q, scale, bias = pkg.quantize_rows(w)
        sb = q8.sbs[t].cpu().numpy()
        assert np.array_equal(q8.qs[t].cpu().numpy(), q), (what, t, "codes")
        assert np.array_equal(_f32bits(sb[:, 0]), _f32bits(scale)), (what, t, "scale")
        assert np.array_equal(sb[:, 1], bias), (what, t, "bias")  # by value: the sign of a zero minimum is not pinned
    for dt in DTYPES:
        back = q8.dequantize(dt)
        for t, w in enumerate(ws):
            sb = q8.sbs[t].cpu().numpy()
            want = pkg.dequantize_rows(q8.qs[t].cpu().numpy(), sb[:, 0], sb[:, 1], dtype=dt)
            got = back[t].data.float().cpu().numpy()
            assert np.array_equal(_f32bits(got), _f32bits(want)), (what, t, dt, "dequantize")


# ---- 1. the quantizer and the dequantizer against numpy
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [1, 6, 16, 48, 128, 256])
def test_quantizer_equals_numpy(pkg, gpu, D, dtype):
    ws = q8_cases.mixed(D, [1, 3, 105, 1000])
    if dtype == torch.bfloat16:
        ws = [q8_cases.bf16_values(w) for w in ws]
    ts = _tables(pkg, gpu, ws, dtype)
    q8 = pkg.QuantizedTableSet.from_tables(ts)
    assert q8.nrows() == [1, 3, 105, 1000] and q8.dim == D and q8.nbytes == 1109 * (D + 8)
    torch.cuda.synchronize()
    _check_quantized(pkg, q8, ws, f"D={D}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unaligned_codes_take_the_scalar_kernels_with_the_same_results(pkg, gpu, dtype):
    D, rows = 16, [3, 105]
    ws = q8_cases.mixed(D, rows, seed=2)
    if dtype == torch.bfloat16:
        ws = [q8_cases.bf16_values(w) for w in ws]
    ts = _tables(pkg, gpu, ws, dtype)
    sbs = [torch.empty((n, 2), dtype=torch.float32, device=gpu) for n in rows]
    q8 = pkg.QuantizedTableSet.from_arrays(_offset_codes(gpu, rows, D, 3), sbs).quantize_from(ts)
    torch.cuda.synchronize()
    _check_quantized(pkg, q8, ws, "offset 3")


def test_mismatched_sets_are_refused(pkg, gpu):
    ts = _tables(pkg, gpu, [np.zeros((4, 16), np.float32), np.zeros((5, 16), np.float32)], torch.float32)
    q8 = pkg.QuantizedTableSet.from_tables(ts)
    for other in ([np.zeros((4, 16), np.float32)], [np.zeros((4, 16), np.float32), np.zeros((6, 16), np.float32)],
                  [np.zeros((4, 32), np.float32), np.zeros((5, 32), np.float32)]):
        with pytest.raises(pkg.DLRMError) as e:
            q8.quantize_from(_tables(pkg, gpu, other, torch.float32))
        assert e.value.code == pkg._lib.E_ARG


# ---- 2. the gather against dlrm_maplookup over the dequantized set
@pytest.mark.parametrize("L", [1, 9, 10])
@pytest.mark.parametrize("T,D", [(7, 6), (7, 16), (7, 128), (26, 6), (26, 16), (26, 128)])
def test_gather_equals_maplookup_of_the_dequantized_set(pkg, gpu, T, D, L):
    rng, rows, _, q8 = _rand_set(pkg, gpu, T, D, torch.float32)
    lib, ctx = q8.ctx.lib, q8.ctx
    k = 0
    for dtype in DTYPES:
        deq = q8.dequantize(dtype)
        for B in (1, 5, 70):
            itype = (torch.int32, torch.int64)[k % 2]
            base = (k // 2) % 2
            k += 1
            idx = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, L) + base).to(itype).to(gpu)
                                    .reshape(T, B, L))
            ld = D + T * D + 8  # out_offset = d, and a row longer than what is written
            sentinel = torch.full((B, ld), -7.5, dtype=dtype, device=gpu)
            got, want = sentinel.clone(), sentinel.clone()
            ctx.check(lib.dlrm_q8_maplookup(ctx.bind(), q8.handle, _ptr(idx.data), idx.itype, idx.stride, base, B, L,
                                            (pkg._lib.F32 if dtype == torch.float32 else pkg._lib.BF16), _ptr(got), ld, D))
            ctx.check(lib.dlrm_maplookup(ctx.bind(), deq.handle, _ptr(idx.data), idx.itype, idx.stride, base, B, L,
                                         _ptr(want), ld, D))
            torch.cuda.synchronize()
            ctx.check_bounds()
            g, w = _bits(got), _bits(want)
            assert np.array_equal(g, w), (dtype, B, itype, base)
            keep = _bits(sentinel)
            assert np.array_equal(g[:, :D], keep[:, :D]) and np.array_equal(g[:, D + T * D:], keep[:, D + T * D:])
            assert (g[:, D:D + T * D] != keep[:, D:D + T * D]).any()


# ---- 3. the forward against HotPath.infer over the dequantized set
def _forward_pair(pkg, gpu, q8, deq, rng, rows, T, D, B, L, dtype, pad_to, x_off=0, wide=True):
    """(got, want, engine, raw status of the fused call): Q8Inference.infer into a row longer than the output,
    from an x inside longer rows; HotPath.infer of a fresh engine over the dequantized set."""
    idx = pkg.PackedIndices(torch.from_numpy(rand_indices(rng, rows, B, L)).to(torch.int32).to(gpu).reshape(T, B, L))
    xw = torch.from_numpy(rng.standard_normal((B, D + 16 + x_off)).astype(np.float32)).to(gpu).to(dtype)
    x = xw[:, x_off:x_off + D] if (wide or x_off) else xw[:, :D].contiguous()
    eng = pkg.Q8Inference(q8, B, L, d=D, dtype=dtype, index_base=0, pad_to=pad_to)
    hp = pkg.HotPath(deq, B, L, index_base=0, pad_to=pad_to)
    assert hp.width == eng.width and hp.padding == eng.padding
    out = torch.full((B, eng.width + 5), 3.25, dtype=dtype, device=gpu)
    probe = torch.full((B, eng.width), 3.25, dtype=dtype, device=gpu)
    rc = eng.fused(x, idx, probe)
    if rc != pkg._lib.OK:  # refused: nothing was launched
        torch.cuda.synchronize()
        assert (probe == 3.25).all()
    got = eng.infer(x, idx, out)
    want = hp.infer(x, idx)
    torch.cuda.synchronize()
    eng.check_bounds()
    g, w = _bits(got), _bits(want)
    assert np.array_equal(g[:, eng.width:], _bits(torch.full((B, 5), 3.25, dtype=dtype)))  # the rest of the row is kept
    if eng.padding:
        assert (g[:, eng.width - eng.padding:eng.width] == 0).all()  # padding columns: all-zero bits
    return g[:, :eng.width], w, eng, rc


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [16, 32, 128])
def test_forward_equals_infer_of_the_dequantized_set(pkg, gpu, D, dtype):
    T = 26
    rng, rows, _, q8 = _rand_set(pkg, gpu, T, D, dtype)
    deq = q8.dequantize(dtype)
    for B in (1, 5, 9, 70):
        for pad_to in (1, 8):
            got, want, eng, rc = _forward_pair(pkg, gpu, q8, deq, rng, rows, T, D, B, 1, dtype, pad_to)
            assert rc == pkg._lib.OK and eng.route == "fused"
            assert np.array_equal(got, want), (B, pad_to)


FALLBACK = [  # T, D, L, dtype, x offset (elements)
    (40, 16, 1, torch.float32, 0), (32, 16, 1, torch.float32, 0), (7, 16, 9, torch.float32, 0),
    (7, 16, 10, torch.bfloat16, 0), (7, 6, 1, torch.float32, 1), (7, 16, 1, torch.float32, 1),
    (7, 4, 1, torch.bfloat16, 0), (7, 16, 2, torch.float32, 0),
]
FUSED = [(31, 16, 1, torch.float32, 0), (17, 8, 1, torch.bfloat16, 0), (7, 4, 1, torch.float32, 0),
         (16, 16, 1, torch.float32, 0), (1, 16, 1, torch.bfloat16, 0), (15, 72, 1, torch.float32, 0)]


@pytest.mark.parametrize("T,D,L,dtype,x_off", FALLBACK + FUSED,
                         ids=[f"{'two' if k < len(FALLBACK) else 'fused'}-T{c[0]}-D{c[1]}-L{c[2]}-{IDS[DTYPES.index(c[3])]}-x{c[4]}"
                              for k, c in enumerate(FALLBACK + FUSED)])
def test_forward_routes_on_both_sides_of_each_limit(pkg, gpu, T, D, L, dtype, x_off):
    fused = (T, D, L, dtype, x_off) in FUSED
    rng, rows, _, q8 = _rand_set(pkg, gpu, T, D, dtype, seed=1)
    deq = q8.dequantize(dtype)
    for B in (5, 9):
        got, want, eng, rc = _forward_pair(pkg, gpu, q8, deq, rng, rows, T, D, B, L, dtype, 1, x_off=x_off)
        assert rc == (pkg._lib.OK if fused else pkg._lib.E_UNSUPPORTED)
        assert eng.route == ("fused" if fused else "two-launch")
        assert np.array_equal(got, want), B


@pytest.mark.parametrize("off,dtype,fused", [(4, torch.float32, True), (4, torch.bfloat16, False),
                                             (8, torch.bfloat16, True), (2, torch.float32, False)])
def test_forward_with_code_rows_at_small_alignments(pkg, gpu, off, dtype, fused):
    T, D, B = 7, 16, 9
    rng = np.random.default_rng(off)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ts = _tables(pkg, gpu, [rng.standard_normal((n, D)).astype(np.float32) for n in rows], dtype)
    sbs = [torch.empty((n, 2), dtype=torch.float32, device=gpu) for n in rows]
    q8 = pkg.QuantizedTableSet.from_arrays(_offset_codes(gpu, rows, D, off), sbs).quantize_from(ts)
    got, want, eng, rc = _forward_pair(pkg, gpu, q8, q8.dequantize(dtype), rng, rows, T, D, B, 1, dtype, 1)
    assert rc == (pkg._lib.OK if fused else pkg._lib.E_UNSUPPORTED)
    assert eng.route == ("fused" if fused else "two-launch")
    assert np.array_equal(got, want)


def test_forward_on_exactly_summable_rows(pkg, gpu):
    """tests/test_interaction_exact.py's small-integer family: rows of integers lo .. lo + 255 quantize to the
    integers themselves (scale 1), x holds integers in [-8, 8], and every sum of the Gram stays below 2^24: the
    output is the int64 Gram, exactly."""
    T, D, B = 26, 16, 5
    rng = np.random.default_rng(11)
    rows = [ROWS[t % len(ROWS)] for t in range(T)]
    ws = []
    for t, n in enumerate(rows):
        k = rng.integers(0, 256, size=(n, D))
        k[:, 0], k[:, -1] = 0, 255
        ws.append((k - (128 if t % 2 else 0)).astype(np.float32))
    ts = _tables(pkg, gpu, ws, torch.float32)
    q8 = pkg.QuantizedTableSet.from_tables(ts)
    for t, w in enumerate(ws):
        sb = q8.sbs[t].cpu().numpy()
        assert (sb[:, 0] == 1.0).all() and np.array_equal(sb[:, 1], w.min(axis=1))
        assert np.array_equal(q8.qs[t].cpu().numpy().astype(np.int64), (w - w.min(axis=1, keepdims=True)).astype(np.int64))
    idx = rand_indices(rng, rows, B, 1)
    x = rng.integers(-8, 9, size=(B, D))
    eng = pkg.Q8Inference(q8, B, 1, dtype=torch.float32)
    got = eng.infer(torch.from_numpy(x.astype(np.float32)).to(gpu),
                    pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu))).cpu().numpy()
    assert eng.route == "fused"
    F = T + 1
    feat = np.empty((B, F, D), dtype=np.int64)
    feat[:, 0] = x
    for t in range(T):
        feat[:, t + 1] = ws[t][idx[t]].astype(np.int64)
    gram = np.einsum("bid,bjd->bij", feat, feat)
    assert np.abs(gram).max() < 2 ** 24
    pairs = np.stack([gram[:, i, j] for i in range(1, F) for j in range(i)], axis=1)
    want = np.concatenate([x, pairs], axis=1)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


# ---- 4. bounds, once per route
@pytest.mark.parametrize("T,route", [(26, "fused"), (40, "two-launch")])
def test_an_index_out_of_range_is_a_zero_row_and_raises(pkg, gpu, T, route):
    D, B, base, b0, t0 = 16, 5, 1, 3, 4
    rng, rows, _, q8 = _rand_set(pkg, gpu, T, D, torch.float32, seed=2)
    clean = rand_indices(rng, rows, B, 1) + base
    bad = clean.copy()
    bad[t0, b0] = base - 1  # negative after the base
    x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu)
    eng = pkg.Q8Inference(q8, B, 1, dtype=torch.float32, index_base=base)
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
    F, i0 = T + 1, t0 + 1
    zero = np.zeros(outs[0].shape, dtype=bool)
    for i in range(1, F):
        for j in range(i):
            if i == i0 or j == i0:
                zero[b0, D + i * (i - 1) // 2 + j] = True
    vals = outs[1].view(np.float32)
    assert (vals[zero] == 0).all() and zero.sum() == T
    assert np.array_equal(outs[1][~zero], outs[0][~zero])
    if route == "two-launch":
        ys = eng.ys.cpu().numpy()
        assert (ys[b0, i0 * D:(i0 + 1) * D] == 0).all()


# ---- 5. row offsets past 2^31
def test_large_table_offsets(pkg, gpu):
    N, D = 2 ** 27 + 5, 16
    ts = q8 = None
    try:
        w = torch.empty((N, D), dtype=torch.bfloat16, device=gpu)
        q = torch.empty((N, D), dtype=torch.uint8, device=gpu)
        sb = torch.empty((N, 2), dtype=torch.float32, device=gpu)
    except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
        pytest.skip(f"no room for a {N} x {D} table: {e}")
    try:
        w.normal_(generator=torch.Generator(device=gpu).manual_seed(5))
        pick = [0, 1, 2, N - 3, N - 2, N - 1]
        w[N - 1, 0], w[N - 1, D - 1] = -4.0, 6.0  # the last row's extremes in its first and last column
        ts = pkg.EmbeddingTableSet([w])
        q8 = pkg.QuantizedTableSet.from_arrays([q], [sb]).quantize_from(ts)
        ctx, lib = q8.ctx, q8.ctx.lib
        idx = pkg.PackedIndices(torch.tensor([pick], dtype=torch.int64, device=gpu))
        out = torch.empty((6, D), dtype=torch.float32, device=gpu)
        ctx.check(lib.dlrm_q8_maplookup(ctx.bind(), q8.handle, _ptr(idx.data), idx.itype, idx.stride, 0, 6, 1,
                                        pkg._lib.F32, _ptr(out), D, 0))
        torch.cuda.synchronize()
        ctx.check_bounds()
        src = w[pick].float().cpu().numpy()
        qq, scale, bias = pkg.quantize_rows(src)
        assert np.array_equal(q[pick].cpu().numpy(), qq)
        got_sb = sb[pick].cpu().numpy()
        assert np.array_equal(_f32bits(got_sb[:, 0]), _f32bits(scale)) and np.array_equal(got_sb[:, 1], bias)
        assert np.array_equal(_f32bits(out.cpu().numpy()), _f32bits(pkg.dequantize_rows(qq, scale, bias)))
    finally:
        del w, q, sb, ts, q8
        torch.cuda.empty_cache()


# ---- 6. graph capture
@pytest.mark.parametrize("T,route", [(26, "fused"), (40, "two-launch")])
def test_infer_replays_from_a_captured_graph(pkg, gpu, T, route):
    D, B = 32, 9
    rng, rows, _, q8 = _rand_set(pkg, gpu, T, D, torch.float32, seed=3)
    x = torch.empty((B, D), dtype=torch.float32, device=gpu)
    ibuf = torch.empty((T, B), dtype=torch.int32, device=gpu)
    idx = pkg.PackedIndices(ibuf)
    eng, eager = pkg.Q8Inference(q8, B, 1, dtype=torch.float32), pkg.Q8Inference(q8, B, 1, dtype=torch.float32)

    def fill():
        x.copy_(torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)))
        ibuf.copy_(torch.from_numpy(rand_indices(rng, rows, B, 1)).to(torch.int32))

    fill()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        eng.infer(x, idx)  # (allocates the fallback's ys before the capture)
    torch.cuda.current_stream(gpu).wait_stream(side)
    assert eng.route == route
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.infer(x, idx)
    for _ in range(3):
        fill()
        graph.replay()
        torch.cuda.synchronize()
        got = _bits(eng.out).copy()
        want = _bits(eager.infer(x, idx))
        assert np.array_equal(got, want)
    eng.check_bounds()


# ---- 7. the quantized model's metrics next to the trained one's
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
    assert len(loader) == 7
    batches = [(dense.clone(), sparse.clone()) for _, dense, sparse in loader]
    dense0, sparse0 = batches[0]
    before = _bits(model.predict(dense0, sparse0)).copy()
    q8 = model.quantize()
    assert q8.nrows() == list(maps.sizes()) and q8.nbytes == sum(maps.sizes()) * (D + 8)
    ev, record, probs = pkg.Evaluator(gpu), [], []
    res = model.test(loader, record=record, evaluator=ev, probs=probs, q8=q8)
    model.hot.check_bounds()
    got = ev.counts()
    assert len(probs) == 7 and got["batches"] == 7 and got["total"] == 224
    labels = data["label"][:224].astype(np.float32)
    prob = torch.cat(probs).cpu().numpy()
    want = pkg.eval_reference(prob, labels)
    for n in ("total", "correct", "positives", "negatives"):
        assert got[n] == want[n], n
    assert np.array_equal(got["hist"], want["hist"])
    assert record == [got["correct"] / 224] and res["accuracy"] == record[0]
    # the probabilities are predict(..., q8=)'s, through the sigmoid; and they are the quantized model's
    for k, (dense, sparse) in enumerate(batches):
        pz = torch.sigmoid(model.predict(dense, sparse, q8=q8)).reshape(-1)
        assert np.array_equal(_bits(pz), _bits(probs[k])), k
    assert model._q8[1].route == "fused"
    # predict without q8 is what it was
    assert np.array_equal(_bits(model.predict(dense0, sparse0)), before)
    assert (before != _bits(model.predict(dense0, sparse0, q8=q8))).any()
