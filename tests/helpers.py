"""Shared test helpers: seeded inputs and comparison criteria.

Tolerances (stated here once, used by every parity test):
  * integer / index / copy work (one-hot lookup, unique rows, segment positions): bit-exact.
  * fp32 reductions in a different order than the checker (interaction MFMA k order,
    chunked hot-row sums): |a - b| <= 1e-5 * (|b| + scale) elementwise, where `scale` is the
    magnitude of the summed terms, AND Julia's isapprox default on the whole array,
    norm(a - b) <= sqrt(eps(Float32)) * max(norm(a), norm(b)) (the reference's own criterion,
    test/integration.jl, src/validation.jl).
  * bf16 outputs: one bf16 rounding (2^-8 relative) of the fp32 result.
  * interaction on exactly summable inputs: bit-exact, bf16 rounded once to nearest even
    (tests/test_interaction_exact.py).
"""
import numpy as np

SQRT_EPS_F32 = float(np.sqrt(np.finfo(np.float32).eps))


def julia_isapprox(a, b, rtol=SQRT_EPS_F32):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(a), np.linalg.norm(b))


def assert_close(a, b, rtol=1e-5, scale=None, what=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    s = np.abs(b).max() if scale is None else scale
    s = max(float(s), 1e-30)
    err = np.abs(a - b)
    bound = rtol * (np.abs(b) + s)
    bad = err > bound
    assert not bad.any(), f"{what}: {bad.sum()} elements off, max err {err.max():.3e} (bound rtol={rtol})"
    assert julia_isapprox(a, b), f"{what}: fails Julia isapprox"


def rand_tables(rng, rows, dim, scale=1.0):
    return [(rng.uniform(-scale, scale, size=(n, dim))).astype(np.float32) for n in rows]


def rand_indices(rng, rows, batch, lookups, zipf=None):
    out = np.empty((len(rows), batch * lookups), dtype=np.int64)
    for t, n in enumerate(rows):
        if zipf is None:
            out[t] = rng.integers(0, n, size=batch * lookups)
        else:
            z = rng.zipf(zipf, size=batch * lookups) - 1
            out[t] = np.minimum(z, n - 1)
    return out


# ---- device <-> numpy, shared by the GPU parity modules (torch and the oracle are imported on use:
# the CPU-only tests import this module too)
def dev_tables(tables, device, dtype=None):
    import torch
    import oracle
    if dtype == torch.bfloat16:
        return [torch.from_numpy(oracle.bf16_to_f32(oracle.f32_to_bf16(t))).to(device).to(torch.bfloat16)
                for t in tables]
    return [torch.from_numpy(t).to(device) for t in tables]


def to_np_bits(t):
    """device tensor -> numpy (bf16 as uint16 bit patterns, fp32 as float32)"""
    import torch
    t = t.detach().cpu()
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def to_np_f32(t):
    return t.detach().float().cpu().numpy()


def _dt_written_mask(idx, D):
    """[B][F*D] bool: the dt entries dlrm_step_bwd must write -- the rows of positions whose table
    row is hit more than once (once-hit rows are updated in place; the x rows' gradient is dx, and
    the split step backward leaves dt's x rows unwritten)."""
    T, B = idx.shape
    keep = np.ones((B, T + 1), dtype=bool)
    keep[:, 0] = False
    for t in range(T):
        _, inv, cnt = np.unique(idx[t], return_inverse=True, return_counts=True)
        keep[:, t + 1] = cnt[inv] > 1
    return np.repeat(keep, D, axis=1)


def _assert_segments(ix, idx, N):
    """One segment per distinct row (segment order unspecified), holding exactly that row's
    positions in ascending order (vectorised: large-N builds have ~N segments per table)."""
    for t in range(idx.shape[0]):
        got_rows, pos, seg = ix.segments(t)
        got_rows, pos, seg = np.asarray(got_rows, dtype=np.int64), np.asarray(pos), np.asarray(seg)
        order = np.argsort(idx[t], kind="stable")
        urows, starts, counts = np.unique(idx[t][order], return_index=True, return_counts=True)
        assert len(got_rows) == len(urows) and seg[-1] == N and len(seg) == len(urows) + 1
        assert np.array_equal(np.sort(got_rows), urows)
        k = np.searchsorted(urows, got_rows)
        assert np.array_equal(np.diff(seg), counts[k])
        want = order[np.repeat(starts[k] - seg[:-1], counts[k]) + np.arange(N)]
        assert np.array_equal(pos, want)


# ---- guard bands: strided, displaced views whose surroundings must survive a call
SENTINEL_F32 = 0x7FC12345  # NaNs with a payload: compared as integers
SENTINEL_BF16 = 0x7FC1


class Band:
    """A [rows][width] view inside a sentinel-filled allocation (see `banded`)."""

    def __init__(self, buf, view, base, stride, sentinel):
        self.buf, self.view, self.base, self.stride, self.sentinel = buf, view, base, stride, sentinel
        self.kept = None

    def snapshot(self):
        """After filling the view with an input: `check` then holds the allocation to these bits."""
        self.kept = self.buf.cpu().numpy().copy()
        return self

    @property
    def ld(self):
        return self.stride

    def bits(self):
        """The view's bit patterns as a numpy integer array [rows][width]."""
        rows, width = self.view.shape
        flat = self.buf.cpu().numpy()
        at = self.base + np.arange(rows)[:, None] * self.stride + np.arange(width)[None, :]
        return flat[at]

    def check(self, written=None, what="buffer"):
        """Every element outside what the call may write still holds the sentinel bits (after a
        `snapshot`: the snapshot's bits, i.e. the input in the view and the sentinel around it).
        written: None = the whole view; an int n = the view's first n columns; a [rows][width] bool
        array = those elements.  (0: nothing -- an input, or an output of a refused call.)"""
        rows, width = self.view.shape
        flat = self.buf.cpu().numpy()
        may = np.zeros((rows, width), dtype=bool)
        if written is None:
            may[:] = True
        elif isinstance(written, (int, np.integer)):
            may[:, :int(written)] = True
        else:
            may[:] = written
        intact = np.ones(flat.shape, dtype=bool)
        at = self.base + np.arange(rows)[:, None] * self.stride + np.arange(width)[None, :]
        intact[at[may]] = False
        bad = np.flatnonzero(intact & (flat != (self.sentinel if self.kept is None else self.kept)))
        assert bad.size == 0, (f"{what}: {bad.size} elements overwritten, first at flat offset {bad[0]} "
                               f"(view base {self.base}, row stride {self.stride}, width {width})")


def banded(shape, dtype, ld, lead, device):
    """A [rows][width] view of `dtype` (fp32 or bf16) with row stride lead + ld inside a larger
    allocation: a guard row (rounded up to 16 bytes, so lead = 0 keeps the view's base 16-B aligned
    and lead = 1 breaks the alignment) before and after the rows, `lead` elements before each row's
    first and ld - width after its last.  Everything starts as a NaN with a payload (fp32 0x7FC12345,
    bf16 0x7FC1): an input read past its view poisons the result, and Band.check finds a stray write
    without any access outside the allocation.  Returns the Band (`.view` is the tensor to pass)."""
    import torch
    rows, width = shape
    assert ld >= width and lead >= 0
    stride = lead + ld
    guard = -(-max(stride, 8) // 8) * 8
    if dtype == torch.bfloat16:
        ity, sentinel = torch.int16, SENTINEL_BF16
    elif dtype == torch.float32:
        ity, sentinel = torch.int32, SENTINEL_F32
    else:
        raise TypeError(dtype)
    buf = torch.full((2 * guard + rows * stride,), sentinel, dtype=ity, device=device)
    base = guard + lead
    view = torch.as_strided(buf.view(dtype), (rows, width), (stride, 1), base)
    return Band(buf, view, base, stride, sentinel)
