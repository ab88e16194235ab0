"""One dlrm_indexer across builds of different forms, sizes and table sets.

An indexer holds about twenty device arrays and a host record that ten build forms share; what keeps a later build
right is a set of "zero at rest" invariants the kernels restore themselves (hent by the hash alloc pass, hot_cnt by a
segment's last-arriving slice, a build_arrive word by its sub-list's last wave, counts / hstate by block 0 of the next
insert, single[] rewritten only by split builds) and the record begin_build / record_build keep (vshift, has_map,
build_err, split, prepared, singles_*).  The other modules build each form on a fresh indexer; here every script of
tests/sequence_cases.py runs its steps on ONE indexer, through the real entry points (dlrm_indexer_build,
dlrm_indexer_build_split, dlrm_indexer_prepare by ctypes; dlrm_step_fwd and dlrm_step_bwd_prepare through a HotPath of
the step's batch whose indexer is replaced by the shared one), and after every build check_build asks:

  1. the return code and the dlrm_indexer_state bits the form implies: BUILT, SPLIT where split, PREPARED from the two
     preparing sites, no SINGLES bit;
  2. helpers._assert_segments on every table: exact;
  3. the exact update: dlrm_sgd_update(PREBUILT) of zeroed tables with lr = 1 and a gradient of k / 64, |k| <= K
     integers with N K < 2^24 -- every partial sum in any order is exact in fp32 -- must leave EVERY row of every table,
     touched or not, at minus the float64 scatter-add (np.array_equal), with check_bounds clean;
  4. history independence: the same PREBUILT update of a fixed random table set with a standard-normal gradient on the
     reused indexer and on a fresh one (same capacity, set_chunk / set_parts and build call) gives the same bits.  No
     tolerance: the order of summation is fixed by the positions alone, not by what the indexer held before;
  5. dlrm_indexer_bytes is what it was at creation (the table-set test: grown once, by the partial rows of D = 512).

A stale has_map, a hot_cnt left at 1, a single[] flag beyond the new N or a CNT_OFF of an earlier wave build makes a
later update skip or double-step rows: 3 sees it on every row, 4 on any order that moved.

The tests set no DLRM_* environment knob (knobs() is read once per process).  Not reached: the scan build with 8 waves
per workgroup -- its T * 2^vshift / 4 workgroups must exceed the compute units, 17 tables of 64 parts.
"""
import numpy as np
import pytest
import torch

import oracle
import sequence_cases as sc
from helpers import _assert_segments, to_np_bits

pytestmark = pytest.mark.gpu


class Tables:
    """A table set of `rows` x dim, its fixed random contents, and the HotPaths that step it."""

    def __init__(self, pkg, dev, rows, dim=sc.DIM, dtype=torch.float32):
        self.pkg, self.dev, self.rows, self.D, self.dtype = pkg, dev, rows, dim, dtype
        rng = np.random.default_rng(len(rows) * 1000 + dim)
        self.fixed = [torch.from_numpy(rng.standard_normal((n, dim), dtype=np.float32)).to(dev).to(dtype) for n in rows]
        self.ts = pkg.EmbeddingTableSet([torch.zeros((n, dim), dtype=dtype, device=dev) for n in rows])
        self._hp = {}

    def zero(self):
        for t in self.ts:
            t.data.zero_()

    def restore(self):
        for t, f in zip(self.ts, self.fixed):
            t.data.copy_(f)

    def bits(self):
        return [to_np_bits(t.data).copy() for t in self.ts]

    def hotpath(self, B, pipeline):
        """(HotPath of batch B, its own indexer, x, dout): x and dout zero, so a step moves no table."""
        if (B, pipeline) not in self._hp:
            hp = self.pkg.HotPath(self.ts, B, 1, lr=1.0, index_base=0, pipeline=pipeline)
            assert hp.step_api and (pipeline is None or hp.pipeline == pipeline)
            self._hp[B, pipeline] = (hp, hp.indexer, torch.zeros((B, self.D), dtype=self.dtype, device=self.dev),
                                     torch.zeros((B, hp.width), dtype=self.dtype, device=self.dev))
        return self._hp[B, pipeline]


def pack(pkg, dev, st, idx):
    t = torch.from_numpy(idx).to(torch.int64 if st.i64 else torch.int32).to(dev)
    return pkg.PackedIndices(t.reshape(idx.shape[0], st.N // st.L, st.L) if st.L > 1 else t)


def run_site(pkg, tb, ix, st, p, cur=None):
    """The step's entry point once, building `ix` from the PackedIndices p.  cur: in_apply -- the batch whose step
    carries the build (its own indexer is the HotPath's).  Returns the library's return code."""
    ptr, ts = pkg.runtime.ptr, tb.ts
    B = st.N // st.L
    ix.set_chunk(st.chunk)
    ix.set_parts(st.parts)
    if st.site in ("build", "build_split", "prepare"):
        args = (ts.ctx.bind(), ix.handle, ts.handle, ptr(p.data), p.itype, p.stride, 0, B)
        if st.site == "build":
            return ts.ctx.lib.dlrm_indexer_build(*args, st.L)
        if st.site == "build_split":
            return ts.ctx.lib.dlrm_indexer_build_split(*args)
        return ts.ctx.lib.dlrm_indexer_prepare(*args)
    hp, own, x, dout = tb.hotpath(B, "apply" if st.site == "in_apply" else None)
    try:
        if st.site == "step_fwd":
            hp.indexer = ix
            hp.step_fwd(x, p)
            return pkg._lib.OK
        assert st.site == "in_apply" and cur is not None
        hp.indexer, hp._ixs = own, [own, ix]
        hp.step_fwd(x, cur)
        hp.step_bwd(dout, x=x, idx=cur, prepare=(ix, p))
        return pkg._lib.OK
    finally:
        hp.indexer = own


def prebuilt_update(pkg, tb, ix, p, grad):
    """dlrm_sgd_update(PREBUILT) with lr = 1: w -= the sum of grad's rows over the row's positions."""
    lib, ts = pkg._lib, tb.ts
    ts.ctx.check(ts.ctx.lib.dlrm_sgd_update(ts.ctx.bind(), ts.handle, ix.handle, lib.UPDATE_PREBUILT,
                                            pkg.runtime.ptr(p.data), p.itype, p.stride, 0, p.B, p.L,
                                            pkg.runtime.ptr(grad), lib.F32, grad.stride(0), 0, 1.0))


def new_indexer(pkg, tb, cap):
    return pkg.SparseIndexer(len(tb.rows), cap, tb.dev)


def check_build(pkg, tb, ix, cap, st, key, idx, p, nbytes, cur=None):
    """Items 1 to 5 of the module docstring for the build `ix` holds: made by step `st` from idx [T][N] = p.
    key: (name, step, draw) of the inputs."""
    lib, ts, N, L, D = pkg._lib, tb.ts, st.N, st.L, tb.D
    B, T = N // L, len(tb.rows)
    # 1. the record
    want = lib.IX_BUILT | (0 if st.form == "sorted" else lib.IX_SPLIT) | (lib.IX_PREPARED if st.form == "wave" else 0)
    assert ix.state() == want, (key, hex(ix.state()), hex(want))
    ts.ctx.check_bounds()
    # 2. the segments
    _assert_segments(ix, idx, N)
    # 3. the exact update, every row
    kk = sc.draw_exact(*key, B, T * D, N)
    tb.zero()
    prebuilt_update(pkg, tb, ix, p, torch.from_numpy(kk.astype(np.float32) / 64).to(tb.dev))
    ts.ctx.check_bounds()
    for t, n in enumerate(tb.rows):
        ref = (0.0 - sc.scatter_sums(idx[t], kk[:, t * D:(t + 1) * D], n, L) / 64).astype(np.float32)
        got = to_np_bits(ts[t].data)
        if tb.dtype == torch.bfloat16:  # the exact step, rounded once
            ref, got = oracle.bf16_to_f32(oracle.f32_to_bf16(ref)), oracle.bf16_to_f32(got)
        bad = np.flatnonzero((got != ref).any(axis=1))
        assert bad.size == 0, (key, f"table {t}: {bad.size} rows differ, first {bad[:8]}, positions per row "
                               f"{np.bincount(idx[t], minlength=n)[bad[:8]]}")
    # 4. the same bits as a fresh indexer
    grad = torch.from_numpy(sc.draw_normal(*key, B, T * D)).to(tb.dev)
    tb.restore()
    prebuilt_update(pkg, tb, ix, p, grad)
    reused = tb.bits()
    fresh = new_indexer(pkg, tb, cap)
    assert run_site(pkg, tb, fresh, st, p, cur) == lib.OK
    tb.restore()
    prebuilt_update(pkg, tb, fresh, p, grad)
    ts.ctx.check_bounds()
    for t, (a, b) in enumerate(zip(reused, tb.bits())):
        assert np.array_equal(a, b), (key, f"table {t}: {(a != b).any(axis=1).sum()} rows differ from a fresh indexer's")
    # 5. nothing grew
    assert ix.nbytes() == nbytes, key


def run_step(pkg, tb, ix, cap, name, k, st, nbytes, last=None):
    """Step k of script `name` on the shared indexer, check_build after each of its builds.  Returns what the indexer
    holds afterwards as (step, key, idx, p) -- `last` where the call was refused."""
    for draw in range(2 if st.hot else 1):
        key = (name, k, draw)
        idx = sc.draw_indices(*key, tb.rows, st.N)
        p = pack(pkg, tb.dev, st, idx)
        cur = pack(pkg, tb.dev, st, sc.draw_indices(name, k, draw + 2, tb.rows, st.N)) if st.site == "in_apply" else None
        rc = run_site(pkg, tb, ix, st, p, cur)
        assert rc == st.rc, (key, rc)
        if rc:  # refused: the indexer is as it was, and its previous build still passes
            assert rc == pkg._lib.E_UNSUPPORTED and last is not None
            check_build(pkg, tb, ix, cap, *last, nbytes)
            return last
        check_build(pkg, tb, ix, cap, st, key, idx, p, nbytes, cur)
        last = (st, key, idx, p)
    return last


@pytest.mark.parametrize("name", [s.name for s in sc.SCRIPTS])
def test_script(pkg, gpu, name):
    script = sc.BY_NAME[name]
    tb = Tables(pkg, gpu, script.rows)
    ix = new_indexer(pkg, tb, script.cap)
    nbytes, last = ix.nbytes(), None
    for k, st in enumerate(script.steps):
        last = run_step(pkg, tb, ix, script.cap, name, k, st, nbytes, last)


def _bad(idx, rows):
    """One index past the end of the 3-row table and one negative in the 5000-row table."""
    bad = idx.copy()
    bad[0, idx.shape[1] // 3] = rows[0]
    bad[len(rows) - 1, 17] = -1
    return bad


@pytest.mark.parametrize("cap", [8192, 32768])
@pytest.mark.parametrize("history", list(sc.HISTORIES))
def test_interrupted_history(pkg, gpu, history, cap):
    """A build that ended otherwise than by its apply, then a clean build of another form on the same indexer."""
    lib = pkg._lib
    first, then = sc.HISTORIES[history][cap]
    name = f"{history}-{cap}"
    tb = Tables(pkg, gpu, sc.ROWS)
    ix = new_indexer(pkg, tb, cap)
    nbytes = ix.nbytes()
    idx = sc.draw_indices(name, 0, 0, sc.ROWS, first.N)
    if history.startswith("bounds"):
        # the build skips and flags two positions (dlrm_indexer_build: on the ctx's word; dlrm_indexer_prepare: on
        # prep_err[0], which the apply folds in); every kernel of the PREBUILT update sees the flag and writes no row,
        # so hot_cnt and partial stay at rest
        p = pack(pkg, gpu, first, _bad(idx, sc.ROWS))
        assert run_site(pkg, tb, ix, first, p) == lib.OK
        tb.restore()
        before = tb.bits()
        prebuilt_update(pkg, tb, ix, p, torch.from_numpy(sc.draw_normal(name, 0, 0, first.N, len(sc.ROWS) * sc.DIM)).to(gpu))
        with pytest.raises(pkg.BoundsError):
            tb.ts.ctx.check_bounds()
        for a, b in zip(before, tb.bits()):
            assert np.array_equal(a, b)
    else:
        p = pack(pkg, gpu, first, idx)
        cur = pack(pkg, gpu, first, sc.draw_indices(name, 0, 2, sc.ROWS, first.N)) if first.site == "in_apply" else None
        assert run_site(pkg, tb, ix, first, p, cur) == lib.OK
        want = lib.IX_BUILT | lib.IX_SPLIT | (lib.IX_PREPARED if first.form == "wave" else 0)
        if history == "bwd_without_apply":
            # the backward steps the once-hit rows; its apply never comes
            hp, own, x, dout = tb.hotpath(first.N, None)
            hp.indexer = ix
            try:
                hp.step_bwd(dout, x=x, idx=p, flags=lib.STEP_BWD_ONLY)
            finally:
                hp.indexer = own
            want |= lib.IX_SINGLES_DONE
        assert ix.state() == want, hex(ix.state())
        tb.ts.ctx.check_bounds()
    # the clean build: BUILT (+ SPLIT / PREPARED) only, every row stepped -- the once-hit rows too
    last = run_step(pkg, tb, ix, cap, name, 1, then, nbytes)
    assert last[0] is then


def _partial_rows(T, cap):
    """abi.cpp partial_rows: per table (times the 8 parts of the builds without an item map up to 8192 positions)
    cap / kHotSlice + cap / (kMinChunk + 1) + 1 slices."""
    return T * (8 if cap <= 8192 else 1) * (cap // sc.HOT_SLICE + cap // (sc.MIN_CHUNK + 1) + 1)


def test_another_table_set_on_the_same_indexer(pkg, gpu):
    """D = 16, 512, 512, 16, bf16 128, 512 on one indexer: the partial rows are regrown once (ensure_partials,
    D > kPartialDim), dlrm_indexer_bytes grows by partial rows x 512 x 4 then and never again."""
    cap, st = sc.TABLE_SET_CAP, sc.TABLE_SET_STEP
    sets = {}
    ix = None
    for k, (dtype, dim) in enumerate(sc.TABLE_SETS):
        if (dtype, dim) not in sets:
            sets[dtype, dim] = Tables(pkg, gpu, sc.ROWS, dim, getattr(torch, dtype))
        tb = sets[dtype, dim]
        if ix is None:
            ix = new_indexer(pkg, tb, cap)
            nbytes = ix.nbytes()
        grown = nbytes + _partial_rows(len(sc.ROWS), cap) * 512 * 4
        seen512 = any(d == 512 for _, d in sc.TABLE_SETS[:k + 1])
        key = ("tables", k, 0)
        idx = sc.draw_indices(*key, sc.ROWS, st.N)
        p = pack(pkg, gpu, st, idx)
        assert run_site(pkg, tb, ix, st, p) == pkg._lib.OK
        assert ix.nbytes() == (grown if any(d == 512 for _, d in sc.TABLE_SETS[:k]) else nbytes)  # (grown on use)
        check_build(pkg, tb, ix, cap, st, key, idx, p, grown if seen512 else nbytes)
