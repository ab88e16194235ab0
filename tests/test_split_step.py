"""The fused training step on split-bf16 tables: dlrm_split_step_bwd / dlrm_split_step_bwd_prepare through
HotPath(opt=SplitDescent, fused_step=True) and HipTables(opt=SplitDescent).

Nothing compares the split kernels only with themselves.  The reference of the tables is the fp32 Descent
trajectory: fp32 tables that hold the merged master weights, stepped by dlrm_sgd_update with the full dt that
dlrm_interact_bwd_gather computes from the bf16 high halves.  After every fused split step
merge_split(hi, lo) must have exactly those bits on every row, untouched rows keep their bits in both arrays,
and out / dx equal the operator route's.  The second check is bit equality of hi, lo, dx and out with
HotPath(opt=SplitDescent)'s default (operator) route.

Shapes: rows cycled from [2, 8, 40, 5000, 3, 100000] with B = 1024 one-hot lookups give multi- and one-slice hot
segments, chunks longer than the inline positions and several hundred once-hit rows per batch.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rand_indices, rand_tables

pytestmark = pytest.mark.gpu

ROWS = [2, 8, 40, 5000, 3, 100000]
LR = 0.05


def _rows(T):
    return [ROWS[t % len(ROWS)] for t in range(T)]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype in (torch.bfloat16, torch.int16) else t.view(torch.int32).numpy()


class _Inputs:
    """Seeded start weights (fp32 and their halves), index batches, x and dout of one shape."""

    def __init__(self, pkg, gpu, D, T, B, nbatches=3, seed=0):
        rng = np.random.default_rng(1000 * D + 10 * T + seed)
        self.rows, self.D, self.T, self.B = _rows(T), D, T, B
        self.w = [torch.from_numpy(t) for t in rand_tables(rng, self.rows, D)]
        self.halves = [pkg.split_f32(t) for t in self.w]
        self.idx = [rand_indices(rng, self.rows, B, 1) for _ in range(nbatches)]
        self.packs = [pkg.PackedIndices(torch.from_numpy(i).to(torch.int32).to(gpu)) for i in self.idx]
        self.x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(gpu).to(torch.bfloat16)
        F = T + 1
        self.dout = torch.from_numpy(rng.standard_normal((B, D + F * (F - 1) // 2)).astype(np.float32)).to(gpu).to(
            torch.bfloat16)

    def split_tables(self, pkg, gpu):
        """(table set, optimizer) at the start values"""
        ts = pkg.EmbeddingTableSet([h.to(gpu) for h, _ in self.halves])
        opt = pkg.SplitDescent(LR)
        for s, (_, lo) in zip(opt.state_of(ts), self.halves):
            s.copy_(lo)
        return ts, opt

    def engine(self, pkg, gpu, **kw):
        ts, opt = self.split_tables(pkg, gpu)
        return pkg.HotPath(ts, self.B, 1, index_base=0, opt=opt, **kw)


def _snap(hp):
    return [_bits(t.data) for t in hp.ts], [_bits(s) for s in hp.opt.state_of(hp.ts)]


_REF = {}


def _reference(pkg, gpu, inp, seq, xb=None, key=None):
    """The operator route (fused forward, dlrm_interact_bwd_gather, dlrm_split_sgd_update(PREBUILT)) over the
    batches `seq`, and beside it the fp32 Descent trajectory from the operator route's full dt.  Returns per step
    (fp32 table bits, hi bits, lo bits, out bits, dx bits).  xb: the backward's view of x."""
    if key is not None and key in _REF:
        return _REF[key]
    hop = inp.engine(pkg, gpu)
    assert not hop.step_api
    ref = pkg.EmbeddingTableSet([t.to(gpu) for t in inp.w])
    steps = []
    for k in seq:
        p = inp.packs[k]
        hop.lookup_interact_fwd(inp.x, p)
        hop.interact_bwd(inp.dout, x=inp.x if xb is None else xb, idx=p, build_indexer=True)
        hop.opt_update(p, True)
        pkg.update_(pkg.Descent(LR), ref, pkg.maplookup_pullback(inp.D, ref, p, hop.dt), index_base=0)
        torch.cuda.synchronize()
        hop.check_bounds()
        hi, lo = _snap(hop)
        steps.append(([_bits(t.data) for t in ref], hi, lo, _bits(hop.out), _bits(hop.dx)))
    if key is not None:
        _REF[key] = steps
    return steps


def _assert_step(pkg, hp, want, what, out=True):
    f32, hi, lo, o, dx = want
    torch.cuda.synchronize()
    hp.check_bounds()
    ghi, glo = _snap(hp)
    for t, m in enumerate(hp.opt.master_of(hp.ts)):
        a = _bits(m)
        assert np.array_equal(a, f32[t]), f"{what} table {t}: {(a != f32[t]).sum()} of {a.size} merged elements differ " \
                                          "from the fp32 Descent trajectory"
        assert np.array_equal(ghi[t], hi[t]) and np.array_equal(glo[t], lo[t]), f"{what} table {t}: != operator route"
    assert np.array_equal(_bits(hp.dx), dx), f"{what}: dx"
    if out:
        assert np.array_equal(_bits(hp.out), o), f"{what}: out"


def _assert_untouched(inp, k, before, after, what):
    (hi0, lo0), (hi1, lo1) = before, after
    for t, n in enumerate(inp.rows):
        un = np.ones(n, dtype=bool)
        un[inp.idx[k][t]] = False
        assert np.array_equal(hi1[t][un], hi0[t][un]) and np.array_equal(lo1[t][un], lo0[t][un]), \
            f"{what} table {t}: an untouched row changed"


# ---- 1. every kernel form: three plain fused steps against both references
SHAPES = [  # (D, T, B, backward's x is an unaligned view)
    (128, 4, 1024, False),   # NB = 1, two waves per sample
    (128, 20, 1024, False),  # NB = 2, two waves per sample
    (128, 4, 2112, False),   # B > 2048: fused forward + in-LDS split build (16 features or fewer: two waves per sample)
    (128, 20, 2112, False),  # ... and 8 columns per lane (more than 16 features)
    (16, 4, 1024, False), (16, 20, 1024, False), (64, 4, 1024, False), (64, 20, 1024, False),  # one wave per sample
    (8, 4, 1024, False), (256, 4, 1024, False),  # interact_bwd_update_kernel's form
    (16, 33, 1024, False),   # F > 32: no split backward, the gather backward + the split apply with once-hit items
    (128, 4, 1024, True),    # x_ld not 16-B aligned in the backward: the same fallback
]


@pytest.mark.parametrize("D,T,B,xview", SHAPES, ids=[f"d{d}-t{t}-b{b}{'-xview' if v else ''}" for d, t, b, v in SHAPES])
def test_fused_split_step_equals_fp32_descent_and_operator_route(pkg, gpu, D, T, B, xview):
    inp = _Inputs(pkg, gpu, D, T, B)
    xb = None
    if xview:
        buf = torch.zeros((B, D + 4), dtype=torch.bfloat16, device=gpu)
        xb = buf[:, :D]
        xb.copy_(inp.x)
        assert (xb.stride(0) * 2) % 16 != 0
    want = _reference(pkg, gpu, inp, [0, 1, 2], xb, key=(D, T, B, xview, "plain"))
    hp = inp.engine(pkg, gpu, fused_step=True)
    assert hp.step_api and hp.split_step
    for k in range(3):
        before = _snap(hp)
        hp.step_fwd(inp.x, inp.packs[k])
        hp.step_bwd(inp.dout, x=inp.x if xb is None else xb, idx=inp.packs[k])
        _assert_step(pkg, hp, want[k], f"step {k}:")
        _assert_untouched(inp, k, before, _snap(hp), f"step {k}:")
        st = hp.indexer.state()
        split_bwd = T <= 31 and not xview
        assert bool(st & pkg._lib.IX_SINGLES_DONE) == split_bwd and bool(st & pkg._lib.IX_SINGLES_SPLIT) == split_bwd
    r, c = np.unique(inp.idx[2][3], return_counts=True)
    assert (c == 1).sum() > 100  # (once-hit rows of the 5000-row table)


# ---- 2. pipelines
@pytest.mark.parametrize("D", [128, 16])
@pytest.mark.parametrize("parts", [16, 32])
@pytest.mark.parametrize("B", [1024, 2048])
def test_pipeline_apply_equals_plain_step(pkg, gpu, B, parts, D):
    """Four steps over two alternating batches through prime + step_prep == step, bit for bit, == the fp32
    reference."""
    inp = _Inputs(pkg, gpu, D, 4, B, nbatches=2, seed=1)
    seq = [0, 1, 0, 1]
    want = _reference(pkg, gpu, inp, seq, key=(D, 4, B, "alt"))
    plain = inp.engine(pkg, gpu, fused_step=True, parts=parts)
    hp = inp.engine(pkg, gpu, fused_step=True, pipeline="apply", parts=parts)
    assert hp.pipeline == "apply"
    for k, b in enumerate(seq):
        plain.step(inp.x, inp.packs[b], inp.dout)
        nxt = inp.packs[seq[(k + 1) % 4]]
        if k == 0:
            hp.prime(nxt, inp.x, inp.dout, prev=inp.packs[b])
        else:
            hp.step_prep(inp.x, inp.packs[b], inp.dout, nxt)
        _assert_step(pkg, plain, want[k], f"plain step {k}:")
        _assert_step(pkg, hp, want[k], f"pipelined step {k}:")
    assert hp._ixs[hp._cur].state() & pkg._lib.IX_PREPARED  # (the last apply launch built the next batch)


@pytest.mark.parametrize("B", [2112, 2110], ids=["scan-build", "rounds-build"])
def test_pipeline_apply_above_2048_positions(pkg, gpu, B):
    """The apply launch that carries a build of more than 2048 positions per table: the scan build (int32
    indices, B % 4 == 0) and the build in rounds (any B)."""
    inp = _Inputs(pkg, gpu, 128, 4, B, nbatches=2, seed=7)
    seq = [0, 1, 0]
    want = _reference(pkg, gpu, inp, seq, key=(128, 4, B, "apply-big"))
    hp = inp.engine(pkg, gpu, fused_step=True, pipeline="apply")
    assert hp.pipeline == "apply"
    hp.prime(inp.packs[1], inp.x, inp.dout, prev=inp.packs[0])
    _assert_step(pkg, hp, want[0], "step 0:")
    assert hp._ixs[hp._cur].state() & pkg._lib.IX_PREPARED
    for k in (1, 2):
        hp.step_prep(inp.x, inp.packs[seq[k]], inp.dout, inp.packs[1 - seq[k]])
        _assert_step(pkg, hp, want[k], f"step {k}:")


def test_pipeline_side_large_batch(pkg, gpu):
    inp = _Inputs(pkg, gpu, 128, 4, 2112, nbatches=2, seed=2)
    want = _reference(pkg, gpu, inp, [0, 1, 0], key=(128, 4, 2112, "side"))
    hp = inp.engine(pkg, gpu, fused_step=True, pipeline="side")
    assert hp.pipeline == "side"
    for k, b in enumerate([0, 1, 0]):
        hp.step_next(inp.x, inp.packs[b], inp.dout, inp.packs[1 - b])
        _assert_step(pkg, hp, want[k], f"step {k}:")


# ---- 3. flags
def test_bwd_only_then_apply_only_and_prebuilt_update(pkg, gpu):
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, 128, 4, 1024)
    want = _reference(pkg, gpu, inp, [0, 1, 2], key=(128, 4, 1024, False, "plain"))
    two = inp.engine(pkg, gpu, fused_step=True)
    upd = inp.engine(pkg, gpu, fused_step=True)
    for hp in (two, upd):
        hp.step_fwd(inp.x, inp.packs[0])
        hp.step_bwd(inp.dout, flags=_lib.STEP_BWD_ONLY)
        assert hp.indexer.state() & _lib.IX_SINGLES_SPLIT
    two.step_bwd(inp.dout, flags=_lib.STEP_APPLY_ONLY)
    upd.opt_update(inp.packs[0], True)  # dlrm_split_sgd_update(PREBUILT): the repeated rows only
    _assert_step(pkg, two, want[0], "BWD_ONLY + APPLY_ONLY:")
    _assert_step(pkg, upd, want[0], "BWD_ONLY + dlrm_split_sgd_update(PREBUILT):")


# ---- 4. the state machine
def test_cross_rule_combinations_are_refused_and_write_nothing(pkg, gpu):
    _lib = pkg._lib
    inp = _Inputs(pkg, gpu, 128, 4, 1024)
    p, x, dout, B, D = inp.packs[0], inp.x, inp.dout, inp.B, inp.D
    hp = inp.engine(pkg, gpu, fused_step=True)
    lib, h = hp.ctx.lib, hp.ctx.bind()
    vp = ctypes.c_void_p
    step = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, vp(x.data_ptr()), x.stride(0), vp(dout.data_ptr()),
            dout.stride(0), hp.padding, vp(hp.dx.data_ptr()), hp.dx.stride(0), vp(hp.dt.data_ptr()), hp.dt.stride(0), LR)
    upd = (vp(p.data.data_ptr()), p.itype, p.stride, 0, B, 1, vp(hp.dt.data_ptr()), _lib.F32, hp.dt.stride(0), D, LR)
    sh = hp.opt.handle_of(hp.ts)
    ada = pkg.RowwiseADAGrad(LR)
    # after a split backward
    hp.step_fwd(x, p)
    hp.step_bwd(dout, flags=_lib.STEP_BWD_ONLY)
    torch.cuda.synchronize()
    assert hp.indexer.state() & (_lib.IX_SINGLES_DONE | _lib.IX_SINGLES_SPLIT) == _lib.IX_SINGLES_DONE | _lib.IX_SINGLES_SPLIT
    before = _snap(hp)
    ixh = hp.indexer.handle
    assert lib.dlrm_step_bwd(h, hp.ts.handle, ixh, *step, _lib.STEP_APPLY_ONLY) == _lib.E_STATE
    assert lib.dlrm_sgd_update(h, hp.ts.handle, ixh, _lib.UPDATE_PREBUILT, *upd) == _lib.E_STATE
    assert lib.dlrm_adagrad_update(h, hp.ts.handle, ada.handle_of(hp.ts), ixh, _lib.UPDATE_PREBUILT, *upd,
                                   1e-8) == _lib.E_STATE
    assert lib.dlrm_split_step_bwd(h, hp.ts.handle, sh, ixh, *step, 0) == _lib.E_STATE  # a second backward on one build
    assert lib.dlrm_split_step_bwd(h, hp.ts.handle, sh, ixh, *step, _lib.STEP_BWD_ONLY) == _lib.E_STATE
    torch.cuda.synchronize()
    after = _snap(hp)
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a, b)
    hp.step_bwd(dout, flags=_lib.STEP_APPLY_ONLY)  # the split apply completes it
    # after a Descent backward on the same tables
    hp.step_fwd(x, p)
    assert lib.dlrm_step_bwd(h, hp.ts.handle, ixh, *step, _lib.STEP_BWD_ONLY) == 0
    torch.cuda.synchronize()
    st = hp.indexer.state()
    assert st & _lib.IX_SINGLES_DONE and not st & _lib.IX_SINGLES_SPLIT
    before = _snap(hp)
    assert lib.dlrm_split_step_bwd(h, hp.ts.handle, sh, ixh, *step, _lib.STEP_APPLY_ONLY) == _lib.E_STATE
    assert lib.dlrm_split_sgd_update(h, hp.ts.handle, sh, ixh, _lib.UPDATE_PREBUILT, *upd) == _lib.E_STATE
    torch.cuda.synchronize()
    after = _snap(hp)
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a, b)
    # argument errors: fp32 tables, an optimizer made for another dim
    f32 = pkg.EmbeddingTableSet([t.to(gpu) for t in inp.w])
    assert lib.dlrm_split_step_bwd(h, f32.handle, sh, ixh, *step, 0) == _lib.E_ARG
    other = pkg.EmbeddingTableSet([torch.zeros((n, 16), dtype=torch.bfloat16, device=gpu) for n in inp.rows])
    assert lib.dlrm_split_step_bwd(h, other.handle, sh, ixh, *step, 0) == _lib.E_ARG
    hp.check_bounds()


# ---- 5. bounds
def test_bad_index_in_the_current_batch_writes_nothing(pkg, gpu):
    inp = _Inputs(pkg, gpu, 128, 4, 1024, seed=3)
    bad_np = inp.idx[0].copy()
    bad_np[3, 517] = inp.rows[3] + 2
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    hp = inp.engine(pkg, gpu, fused_step=True)
    before = _snap(hp)
    hp.step(inp.x, bad, inp.dout)
    with pytest.raises(pkg.BoundsError):
        hp.check_bounds()
    after = _snap(hp)
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a, b)


def test_bad_index_in_the_next_batch_only(pkg, gpu):
    """The split counterpart of test_step_next_bad_index_in_next_batch_only, for both pipelines: the current
    step's rows are written and nothing is raised yet; the step on the bad batch raises and writes nothing."""
    inp = _Inputs(pkg, gpu, 128, 4, 1024, seed=4)
    want = _reference(pkg, gpu, inp, [0], key=(128, 4, 1024, "seed4"))
    bad_np = inp.idx[1].copy()
    bad_np[3, 99] = inp.rows[3] + 1
    bad = pkg.PackedIndices(torch.from_numpy(bad_np).to(torch.int32).to(gpu))
    for mode in ("apply", "side"):
        hp = inp.engine(pkg, gpu, fused_step=True, pipeline=mode)
        if mode == "apply":
            hp.prime(bad, inp.x, inp.dout, prev=inp.packs[0])
        else:
            hp.step_next(inp.x, inp.packs[0], inp.dout, bad)
        _assert_step(pkg, hp, want[0], f"{mode}:")  # (checks bounds: clean)
        before = _snap(hp)
        if mode == "apply":
            hp.step_prep(inp.x, bad, inp.dout, inp.packs[0])
        else:
            hp.step_next(inp.x, bad, inp.dout, inp.packs[0])
        with pytest.raises(pkg.BoundsError):
            hp.check_bounds()
        after = _snap(hp)
        for a, b in zip(before[0] + before[1], after[0] + after[1]):
            assert np.array_equal(a, b)


# ---- 6. NaN
def test_once_hit_nan_reads_as_nan_through_the_bf16_table(pkg, gpu):
    """A once-hit row whose master weight is a NaN with its payload in the low half only (high half = Inf's
    bits): the backward's split write sets the high half's quiet bit, so the bf16 table alone reads NaN."""
    D, B = 16, 64
    rows = [4, 1000]
    w = [torch.ones((n, D)) for n in rows]
    w[1][7] = torch.from_numpy(np.full((D,), 0x7F800001, dtype=np.uint32).view(np.float32).copy())
    halves = [pkg.split_f32(t) for t in w]
    assert torch.isinf(halves[1][0][7].float()).all()
    ts = pkg.EmbeddingTableSet([h.to(gpu) for h, _ in halves])
    opt = pkg.SplitDescent(LR)
    for s, (_, lo) in zip(opt.state_of(ts), halves):
        s.copy_(lo)
    idx = np.stack([np.arange(B) % 4, 100 + np.arange(B)])
    idx[1, 5] = 7  # row 7 of table 1: hit once
    p = pkg.PackedIndices(torch.from_numpy(idx).to(torch.int32).to(gpu))
    hp = pkg.HotPath(ts, B, 1, index_base=0, opt=opt, fused_step=True)
    x = torch.ones((B, D), dtype=torch.bfloat16, device=gpu)
    dout = torch.ones((B, hp.width), dtype=torch.bfloat16, device=gpu)
    hp.step(x, p, dout)
    torch.cuda.synchronize()
    hp.check_bounds()
    assert hp.indexer.state() & pkg._lib.IX_SINGLES_SPLIT
    assert torch.isnan(opt.master_of(ts)[1][7]).all()
    assert torch.isnan(ts[1].data[7].float()).all()
    assert not torch.isnan(ts[1].data[8].float()).any()


# ---- 7. graph capture
def test_pipelined_split_step_graph_replay_equals_eager(pkg, gpu):
    inp = _Inputs(pkg, gpu, 128, 4, 1024, nbatches=1, seed=5)
    p = inp.packs[0]
    hg = inp.engine(pkg, gpu, fused_step=True, pipeline="apply")
    he = inp.engine(pkg, gpu, fused_step=True, pipeline="apply")
    hg.prime(p, inp.x, inp.dout, prev=p)  # eager warm-up: one step, and indexer 0 holds p, prepared
    for t, (h, _) in zip(hg.ts, inp.halves):  # the tables back to the start
        t.data.copy_(h)
    for s, (_, lo) in zip(hg.opt.state_of(hg.ts), inp.halves):
        s.copy_(lo)
    # (two steps per graph: the two indexers are back in the captured state after each replay)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            hg.step_prep(inp.x, p, inp.dout, p)
            hg.step_prep(inp.x, p, inp.dout, p)
    torch.cuda.current_stream().wait_stream(s)
    he.prime(p, inp.x, inp.dout, prev=p)
    for t, (h, _) in zip(he.ts, inp.halves):
        t.data.copy_(h)
    for s_, (_, lo) in zip(he.opt.state_of(he.ts), inp.halves):
        s_.copy_(lo)
    for _ in range(2):
        gr.replay()
        he.step_prep(inp.x, p, inp.dout, p)
        he.step_prep(inp.x, p, inp.dout, p)
    torch.cuda.synchronize()
    hg.check_bounds()
    for a, b in zip(_snap(hg)[0] + _snap(hg)[1], _snap(he)[0] + _snap(he)[1]):
        assert np.array_equal(a, b)
    assert np.array_equal(_bits(hg.dx), _bits(he.dx))
    assert any((a != _bits(lo)).any() for a, (_, lo) in zip(_snap(hg)[1], inp.halves))  # (the steps did run)


# ---- 8. HipTables
@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
def test_hiptables_chain_equals_operator_sequence(pkg, gpu, defer):
    inp = _Inputs(pkg, gpu, 16, 4, 1024, nbatches=2, seed=6)
    want = _reference(pkg, gpu, inp, [0, 1], key=(16, 4, 1024, "seed6"))
    opt = pkg.SplitDescent(LR)
    ht = pkg.HipTables([h.to(gpu) for h, _ in inp.halves], opt=opt, index_base=0, defer_update=defer)
    for s, (_, lo) in zip(opt.state_of(ht._ts), inp.halves):
        s.copy_(lo)
    D = inp.D
    for k, p in enumerate(inp.packs):
        ys = pkg.maplookup(pkg.PreallocationStrategy(D), ht, p)
        assert isinstance(ys, pkg.LazyLookup)
        out, back = pkg.rrule(pkg.DotInteraction(), inp.x, ys)
        _, dx, dy = back(inp.dout)
        assert dy.applied
        assert np.array_equal(_bits(out), want[k][3]) and np.array_equal(_bits(dx), want[k][4])
        with pytest.raises(ValueError):
            pkg.update_(pkg.SplitDescent(LR), ht, pkg.maplookup_pullback(D, ht, p, dy))  # another optimizer object
        with pytest.raises(ValueError):
            pkg.update_(pkg.Descent(LR), ht, pkg.maplookup_pullback(D, ht, p, dy))
        pkg.update_(opt, ht, pkg.maplookup_pullback(D, ht, p, dy))
        assert (ht._pending is not None) == defer
    ts = ht.ts  # (runs a deferred apply, checks bounds)
    torch.cuda.synchronize()
    f32, hi, lo = want[1][:3]
    for t in range(inp.T):
        assert np.array_equal(_bits(ts[t].data), hi[t]) and np.array_equal(_bits(opt.state_of(ts)[t]), lo[t])
        assert np.array_equal(_bits(opt.master_of(ts)[t]), f32[t])


# ---- 9. keyword errors
def test_fused_step_keyword_errors(pkg, gpu):
    bf = [torch.zeros((8, 16), dtype=torch.bfloat16, device=gpu) for _ in range(2)]
    f32 = [torch.zeros((8, 16), dtype=torch.float32, device=gpu) for _ in range(2)]
    with pytest.raises(ValueError):
        pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=pkg.ADAGrad(), fused_step=True)
    with pytest.raises(ValueError):
        pkg.HotPath(pkg.EmbeddingTableSet(f32), 32, 1, index_base=0, opt=pkg.SplitDescent(), fused_step=True)
    with pytest.raises(ValueError):
        pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, fused_step=True)
    hp = pkg.HotPath(pkg.EmbeddingTableSet(bf), 32, 1, index_base=0, opt=pkg.SplitDescent())  # the default route stays
    assert not hp.step_api and not hp.split_step
