"""Sparse embedding gradients and the SGD scatter update.

Mirrors EmbeddingTables' training API as DLRM.jl calls it:
  * the maplookup pullback -> one `SparseEmbeddingUpdate(delta, indices)` per table
    (test/model/embedding_update.jl:35-40, test/train/backprop.jl:147-158);
  * `SparseIndexer()` per table (src/train/train.jl:276-281);
  * `update!(Descent(lr), tables, grads, indexers; num_splits, nthreads)`
    (src/train/train.jl:283-290) -> `update_` here (Python has no `!`).
The deterministic GPU path dedupes each table's indices with a stable sort and writes every
touched row once; `deterministic=False` uses float atomics instead.
"""
import ctypes

import torch

from . import _lib
from .embedding import EmbeddingTableSet, PackedIndices, as_table_set
from .runtime import context, dtype_code, ptr, require_device


class Descent:
    """Flux.Descent(η): plain SGD, w .-= η * g (default η = 0.1 as in Flux)."""

    def __init__(self, eta=0.1):
        self.eta = float(eta)

    def __repr__(self):
        return f"Descent({self.eta})"


class _StatefulOpt:
    """An optimizer with device state per table row.  The state is kept per table set (as Flux keys
    its IdDict by parameter): allocated on the tables' device at first use, and exposed by
    `state_of(tables)` so a caller can read, save or preset it."""

    def __init__(self):
        self._state = {}  # the tables' data pointers -> (table set, [state tensors], the C handle)

    def _init_state(self, table):
        raise NotImplementedError

    def _create(self, ts, ptrs, out):
        """The C constructor's return code (handle into `out`)."""
        raise NotImplementedError

    def _destroy(self, lib, handle):
        raise NotImplementedError

    def launch(self, ts, indexer, flags, idx, index_base, grad, grad_offset):
        """The C update's return code: `grad` columns from `grad_offset`, indices `idx` (PackedIndices)."""
        raise NotImplementedError

    # The rule's fused training step (HotPath, HipTables): the keyword that opts an engine in, the library's pair of
    # entry points (the step backward and its _prepare form), and `step_params`, the scalars they take after the
    # buffers (fixed: the ones an owner fixed for both launches of a step, HipTables' deferred apply among them;
    # None: the optimizer's own, read at the call).
    step_keyword = None
    step_entry = None
    # (a seeded Adagrad optimizer's fused step: a keyword and a pair of its own, `_AdagradBase`; None everywhere else)
    sr_step_keyword = None
    sr_step_entry = None
    no_atomic = None  # why the rule has no atomic mode (none of these has one)

    def step_params(self, fixed=None):
        return fixed or (self.eta,)

    def check_tables(self, dtype):
        """Raises ValueError when the rule cannot step tables of element type `dtype`."""

    def _entry(self, tables):
        ts = as_table_set(tables)
        key = tuple(t.data.data_ptr() for t in ts)  # (the parameters themselves: any table set over them)
        ent = self._state.get(key)
        if ent is None:
            state = [self._init_state(t.data) for t in ts]
            T = len(ts)
            ptrs = (ctypes.c_void_p * T)(*[s.data_ptr() for s in state])
            h = ctypes.c_void_p()
            ts.ctx.check(self._create(ts, ptrs, ctypes.byref(h)))
            ent = self._state[key] = (ts, state, h)
        return ent

    def state_of(self, tables):
        """The state tensors of `tables` (a table set), one per table: fp32 [nrows][D] accumulators
        (ADAGrad), fp32 [nrows] row accumulators (RowwiseADAGrad) or int16 [nrows][D] low halves
        (SplitDescent); none for StochasticDescent, whose state is the handle's step (a seeded Adagrad optimizer has both:
        its step is `step_of`).  Write into them to
        preset the state."""
        return self._entry(tables)[1]

    def handle_of(self, tables):
        return self._entry(tables)[2]

    def __del__(self):
        try:
            for ts, _, h in self._state.values():
                self._destroy(ts.ctx.lib, h)
        except Exception:
            pass


class _AdagradBase(_StatefulOpt):
    """Sparse Adagrad over embedding tables (dlrm_adagrad_*).

    seed (None: round to nearest, the rule as it always was): an integer in [0, 2^64) makes the store of every written
    weight stochastic, on bfloat16 tables only (dlrm_adagrad_create_sr).  The gradient sum, the state update and the
    fp32 result of every element are the seedless rule's, bit for bit, and so is the state written; the bfloat16
    stored is that result rounded up or down as StochasticDescent rounds (`sr_round` restates it), so a step below
    half an ulp of the weight accumulates instead of vanishing.  The step is a counter on the device, per table set:
    0 at first use, one more after every update (a captured update advances it on every replay); `seek(tables, step)`
    sets it and `step_of(tables)` reads it (synchronising).  A seeded optimizer's fused training step is
    `sr_adagrad_step=True` (dlrm_sr_adagrad_step_bwd; `sr_step_keyword` / `sr_step_entry`): without it `HotPath` and
    `HipTables` take the optimizer on the operator route, and `adagrad_step=True` is refused with it."""
    rowwise = False
    no_atomic = "an atomic add never holds the row's whole gradient sum, which the rule squares"
    step_keyword = "adagrad_step"
    step_entry = ("dlrm_adagrad_step_bwd", "dlrm_adagrad_step_bwd_prepare")

    def __init__(self, eta=0.1, eps=1e-8, seed=None):
        super().__init__()
        name = type(self).__name__
        if seed is not None:
            if isinstance(seed, bool) or not isinstance(seed, int):
                raise TypeError(f"{name}: seed is None or an integer in [0, 2^64), not {type(seed).__name__}")
            if not 0 <= seed < 2 ** 64:
                raise ValueError(f"{name}: seed is None or an integer in [0, 2^64)")
            # the stochastic store's fused step is not the seedless rule's: a keyword and entry points of its own
            # (dlrm_adagrad_step_bwd refuses a seeded handle), opt-in as every rule's
            self.step_keyword = self.step_entry = None
            self.sr_step_keyword = "sr_adagrad_step"
            self.sr_step_entry = ("dlrm_sr_adagrad_step_bwd", "dlrm_sr_adagrad_step_bwd_prepare")
        self.eta = float(eta)
        self.eps = float(eps)
        self.seed = seed

    def step_params(self, fixed=None):
        return fixed or (self.eta, self.eps)

    def check_tables(self, dtype):
        if self.seed is not None and dtype != torch.bfloat16:
            raise ValueError(f"{type(self).__name__} with a seed needs bfloat16 tables (fp32: nothing to round), not {dtype}")

    def _init_state(self, table):
        self.check_tables(table.dtype)
        return self._zero_state(table)

    def _create(self, ts, ptrs, out):
        lib = ts.ctx.lib
        if self.seed is None:
            return lib.dlrm_adagrad_create(ts.ctx.bind(), ts.handle, int(self.rowwise), ptrs, out)
        return lib.dlrm_adagrad_create_sr(ts.ctx.bind(), ts.handle, int(self.rowwise), ptrs, _as_i64(self.seed), out)

    def _destroy(self, lib, handle):
        lib.dlrm_adagrad_destroy(handle)

    def launch(self, ts, indexer, flags, idx, index_base, grad, grad_offset):
        ctx = ts.ctx
        return ctx.lib.dlrm_adagrad_update(ctx.bind(), ts.handle, self.handle_of(ts), indexer.handle, flags,
                                           ptr(idx.data), idx.itype, idx.stride, index_base, idx.B, idx.L, ptr(grad),
                                           dtype_code(grad.dtype), grad.stride(0), grad_offset, self.eta, self.eps)

    def _seeded(self, what):
        if self.seed is None:
            raise ValueError(f"{type(self).__name__}.{what}: the optimizer has no seed, so no step (seed=... makes "
                             "its store stochastic)")

    def seek(self, tables, step):
        """With a seed: the next update of `tables` uses `step` (asynchronous, in stream order)."""
        self._seeded("seek")
        ts, _, h = self._entry(tables)
        if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < 2 ** 64:
            raise ValueError(f"{type(self).__name__}.seek: step is an integer in [0, 2^64)")
        ts.ctx.check(ts.ctx.lib.dlrm_adagrad_seek(ts.ctx.bind(), h, _as_i64(step)))

    def step_of(self, tables):
        """With a seed: the step the next update of `tables` will use (synchronises)."""
        self._seeded("step_of")
        ts, _, h = self._entry(tables)
        out = ctypes.c_uint64()
        ts.ctx.check(ts.ctx.lib.dlrm_adagrad_step(ts.ctx.bind(), h, ctypes.byref(out)))
        return out.value

    def __repr__(self):
        tail = "" if self.seed is None else f", seed={self.seed}"
        return f"{type(self).__name__}({self.eta}, {self.eps}{tail})"


class ADAGrad(_AdagradBase):
    """Flux.ADAGrad(η, ϵ): A .+= g.^2; w .-= η .* g ./ (sqrt.(A) .+ ϵ), A starting at ϵ.  On
    embedding tables only the rows a batch touches change (an untouched row has g = 0).  seed: the stochastically
    rounded store on bfloat16 tables (see _AdagradBase)."""

    def _zero_state(self, table):
        return torch.full(table.shape, self.eps, dtype=torch.float32, device=table.device)


class RowwiseADAGrad(_AdagradBase):
    """Row-wise Adagrad: one fp32 accumulator per table row, m[r] += mean_c(g[r][c]^2);
    w[r] .-= η .* g[r] ./ (sqrt(m[r]) + ϵ), m starting at 0.  seed: the stochastically rounded store on bfloat16
    tables (see _AdagradBase): with bfloat16 rows and this rule's one word per row, the Adagrad that fits the largest
    table sets."""
    rowwise = True

    def _zero_state(self, table):
        return torch.zeros((table.shape[0],), dtype=torch.float32, device=table.device)


def split_f32(w):
    """(hi, lo) of an fp32 tensor: hi = the top 16 bits of every element as bfloat16 (the
    truncation of w, not `w.to(bfloat16)`, which rounds), lo = the bottom 16 bits as int16.  Pure
    bit operations, any device; `merge_split(hi, lo)` has exactly the bits of `w`."""
    if w.dtype != torch.float32:
        raise TypeError("split_f32 expects a float32 tensor")
    u = w.view(torch.int32)
    hi = (u >> 16).to(torch.int16).view(torch.bfloat16)  # (arithmetic shifts: both halves fit int16 as they are)
    lo = ((u << 16) >> 16).to(torch.int16)
    return hi, lo


def merge_split(hi, lo):
    """The fp32 tensor whose top 16 bits are `hi` (bfloat16) and bottom 16 bits `lo` (int16)."""
    if hi.dtype != torch.bfloat16 or lo.dtype != torch.int16 or hi.shape != lo.shape:
        raise TypeError("merge_split expects a bfloat16 tensor and an int16 tensor of the same shape")
    u = (hi.view(torch.int16).to(torch.int32) << 16) | (lo.to(torch.int32) & 0xFFFF)
    return u.view(torch.float32)


class SplitDescent(_StatefulOpt):
    """Flux.Descent(η) on split-bf16 tables (dlrm_split_sgd_*): every weight has an fp32 master value
    whose high 16 bits are the bf16 table element and whose low 16 bits live in an int16 state array
    of the same shape.  The step is Descent's on the fp32 value, exactly; the lookup, the
    interaction and its backward keep reading the bf16 table (the master value truncated).

    `state_of(tables)` returns the low halves, zeros at first use (right for tables that were bf16
    all along); write `split_f32(w)[1]` into them to start from fp32 weights `w`.  Do not step such
    tables with Descent, an Adagrad optimizer or a `HotPath` without `opt=`: those round the high
    half and leave the low one behind."""

    no_atomic = "an atomic add on one half of a weight cannot carry into the other"
    step_keyword = "fused_step"
    step_entry = ("dlrm_split_step_bwd", "dlrm_split_step_bwd_prepare")

    def __init__(self, eta=0.1):
        super().__init__()
        self.eta = float(eta)

    def check_tables(self, dtype):
        if dtype != torch.bfloat16:
            raise ValueError(f"SplitDescent needs bfloat16 tables (the high halves), not {dtype}")

    def _init_state(self, table):
        self.check_tables(table.dtype)
        return torch.zeros(table.shape, dtype=torch.int16, device=table.device)

    def _create(self, ts, ptrs, out):
        return ts.ctx.lib.dlrm_split_sgd_create(ts.ctx.bind(), ts.handle, ptrs, out)

    def _destroy(self, lib, handle):
        lib.dlrm_split_sgd_destroy(handle)

    def launch(self, ts, indexer, flags, idx, index_base, grad, grad_offset):
        ctx = ts.ctx
        return ctx.lib.dlrm_split_sgd_update(ctx.bind(), ts.handle, self.handle_of(ts), indexer.handle, flags,
                                             ptr(idx.data), idx.itype, idx.stride, index_base, idx.B, idx.L, ptr(grad),
                                             dtype_code(grad.dtype), grad.stride(0), grad_offset, self.eta)

    def master_of(self, tables):
        """The fp32 master weights of `tables`, one new tensor per table (checkpoints, tests)."""
        ts, lo, _ = self._entry(tables)
        return [merge_split(t.data, s) for t, s in zip(ts, lo)]

    def __repr__(self):
        return f"SplitDescent({self.eta})"


_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in numpy: `counter` = four uint32 arrays (or scalars) that
    broadcast together, `key` = two; returns the four output words as uint32 arrays."""
    import numpy as np
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in counter]
    k = [int(key[0]) & _M32, int(key[1]) & _M32]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & np.uint64(_M32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & np.uint64(_M32)]
        k = [(k[0] + 0x9E3779B9) & _M32, (k[1] + 0xBB67AE85) & _M32]
    shape = np.broadcast(*c).shape
    return [np.broadcast_to(x, shape).astype(np.uint32) for x in c]


def sr_bits(shape, seed, step, table, row0=0):
    """The 16 random bits R of every element of rows row0.. of table `table` at `step` under `seed`, as a
    uint32 array of `shape` = (rows, columns): key = the seed's halves, counter = (row, table << 16 |
    column >> 2, the step's halves), column c takes the low 16 bits of output word c & 3."""
    import numpy as np
    n, d = shape
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    rows = (np.arange(n, dtype=np.uint64) + np.uint64(row0))[:, None]
    blocks = np.arange((d + 3) // 4, dtype=np.uint64)[None, :]
    out = philox4x32_10([rows, (np.uint64(int(table)) << np.uint64(16)) | blocks, step & _M32, step >> 32],
                        [seed & _M32, seed >> 32])
    r = np.stack(out, axis=-1).reshape(n, -1)[:, :d]  # (word c & 3 of block c >> 2)
    return r & np.uint32(0xFFFF)


def sr_round(w_f32, seed, step, table, *, row0=0, bits=None):
    """The stochastic rule's store, restated in numpy: the bfloat16 bit patterns (uint16 array) that
    StochasticDescent writes for the fp32 results `w_f32` ([rows][D] float32 numpy array or CPU tensor: the
    W' of every element of rows row0.. of table `table`) at `step` under `seed`.  u = bits(W'): Inf and NaN
    round to nearest (a NaN keeps its quiet bit), anything else is (u + R) >> 16.  bits: R given instead of
    drawn (tests)."""
    import numpy as np
    w = w_f32.detach().cpu().numpy() if isinstance(w_f32, torch.Tensor) else np.asarray(w_f32)
    if w.dtype != np.float32 or w.ndim != 2:
        raise TypeError("sr_round expects a two-dimensional float32 array")
    u = np.ascontiguousarray(w).view(np.uint32)
    r = sr_bits(w.shape, seed, step, table, row0) if bits is None else np.asarray(bits, dtype=np.uint32) & np.uint32(0xFFFF)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    nan = special & ((u & np.uint32(0x007FFFFF)) != 0)
    sr = ((u.astype(np.uint64) + r) >> np.uint64(16)).astype(np.uint16)
    nearest = np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), u >> np.uint32(16)).astype(np.uint16)  # (Inf: exact)
    return np.where(special, nearest, sr)


class StochasticDescent(_StatefulOpt):
    """Flux.Descent(η) on bfloat16 tables with a stochastically rounded store (dlrm_sr_sgd_*): the fp32 result
    of every touched element's step is rounded up or down with probability proportional to its distance to
    each bfloat16 neighbour, so the stored weight equals the fp32 step in expectation and updates below half
    an ulp accumulate instead of vanishing -- at no memory beside the table (SplitDescent is exact and takes 2
    more bytes per element).

    The random bits are a function of (seed, step, table, row, column) alone (Philox4x32-10; `sr_round`
    restates a step on the host).  The step is a counter on the device, per table set: 0 at first use, one
    more after every update (a captured update advances it on every replay); `seek(tables, step)` sets it and
    `step_of(tables)` reads it (synchronising).  There is no per-row state, so the rule may be alternated
    freely with Descent on the same tables.  `HotPath` / `HipTables` take it on the operator route
    (`pipeline=None`) unless built with `stochastic_step=True`, the fused step with this rule (dlrm_sr_step_bwd):
    the step backward rounds the once-hit rows itself, both launches of a step read the same value of the
    counter, and it advances after the apply."""

    def __init__(self, eta=0.1, seed=0):
        super().__init__()
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError(f"StochasticDescent: seed is an integer in [0, 2^64), not {type(seed).__name__}")
        if not 0 <= seed < 2 ** 64:
            raise ValueError("StochasticDescent: seed is an integer in [0, 2^64)")
        self.eta = float(eta)
        self.seed = seed

    no_atomic = "the rule rounds each row's complete step once, an atomic add would round every addend"
    step_keyword = "stochastic_step"
    step_entry = ("dlrm_sr_step_bwd", "dlrm_sr_step_bwd_prepare")

    def check_tables(self, dtype):
        if dtype != torch.bfloat16:
            raise ValueError(f"StochasticDescent needs bfloat16 tables (fp32: nothing to round), not {dtype}")

    def _entry(self, tables):
        ts = as_table_set(tables)
        key = tuple(t.data.data_ptr() for t in ts)
        ent = self._state.get(key)
        if ent is None:
            self.check_tables(ts.dtype)
            h = ctypes.c_void_p()
            ts.ctx.check(ts.ctx.lib.dlrm_sr_sgd_create(ts.ctx.bind(), ts.handle, _as_i64(self.seed), ctypes.byref(h)))
            ent = self._state[key] = (ts, [], h)  # (no state tensors: the handle holds the step)
        return ent

    def _destroy(self, lib, handle):
        lib.dlrm_sr_sgd_destroy(handle)

    def launch(self, ts, indexer, flags, idx, index_base, grad, grad_offset):
        ctx = ts.ctx
        return ctx.lib.dlrm_sr_sgd_update(ctx.bind(), ts.handle, self.handle_of(ts), indexer.handle, flags,
                                          ptr(idx.data), idx.itype, idx.stride, index_base, idx.B, idx.L, ptr(grad),
                                          dtype_code(grad.dtype), grad.stride(0), grad_offset, self.eta)

    def seek(self, tables, step):
        """The next update of `tables` uses `step` (asynchronous, in stream order)."""
        ts, _, h = self._entry(tables)
        if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < 2 ** 64:
            raise ValueError("StochasticDescent.seek: step is an integer in [0, 2^64)")
        ts.ctx.check(ts.ctx.lib.dlrm_sr_sgd_seek(ts.ctx.bind(), h, _as_i64(step)))

    def step_of(self, tables):
        """The step the next update of `tables` will use (synchronises)."""
        ts, _, h = self._entry(tables)
        out = ctypes.c_uint64()
        ts.ctx.check(ts.ctx.lib.dlrm_sr_sgd_step(ts.ctx.bind(), h, ctypes.byref(out)))
        return out.value

    def __repr__(self):
        return f"StochasticDescent({self.eta}, seed={self.seed})"


def _as_i64(u):
    """The 64 bits of an unsigned value as the int64 the C ABI passes them in."""
    return u - 2 ** 64 if u >= 2 ** 63 else u


def _tables_dtype(tables):
    """The element type of `tables` (a table set, HipTables, or a list of tables / tensors)."""
    first = next(iter(getattr(tables, "_ts", tables)))  # (HipTables: its table set, without a bounds check)
    return getattr(first, "data", first).dtype


class SparseEmbeddingUpdate:
    """SparseEmbeddingUpdate{Static{D}}(delta, indices): the gradient of one table.

    `delta` is a [B][D] view (column block of the interaction's dt); `grad`, `grad_offset`
    keep the parent matrix so that all tables can be updated in one launch."""

    def __init__(self, grad, grad_offset, featuresize, indices, table_index):
        self.grad = grad
        self.grad_offset = int(grad_offset)
        self.featuresize = int(featuresize)
        self.indices = indices  # PackedIndices of ALL tables (row `table_index` is this table's)
        self.table_index = int(table_index)

    @property
    def delta(self):
        return self.grad[:, self.grad_offset:self.grad_offset + self.featuresize]

    def uncompress(self, nrows, *, index_base=1):
        """uncompress(update, nrows) (test/train/backprop.jl:156): the dense [nrows][D] gradient,
        Σ of delta rows per index (pooled bags: a bag's row counts once per lookup).  It is
        update!(Descent(-1)) into a zero table -- the same deterministic HIP indexer + apply, so the
        sum per row runs in ascending position order, fp32."""
        if self.indices.data.device.type != "cuda":
            raise ValueError("uncompress runs on the GPU (the indices must be device tensors)")
        dev = self.indices.data.device
        out = torch.zeros((nrows, self.featuresize), dtype=torch.float32, device=dev)
        ts = EmbeddingTableSet([out])
        one = PackedIndices(self.indices.data[self.table_index:self.table_index + 1].reshape(
            1, self.indices.B, self.indices.L))
        g = self.grad
        if g.stride(1) != 1:
            raise ValueError("gradient rows must be contiguous")
        require_device(g, dev, "gradient")
        ix = SparseIndexer(1, one.B * one.L, dev)
        ctx = ts.ctx
        ctx.check(ctx.lib.dlrm_sgd_update(ctx.bind(), ts.handle, ix.handle, 0, ptr(one.data), one.itype, one.stride,
                                          index_base, one.B, one.L, ptr(g), dtype_code(g.dtype), g.stride(0),
                                          self.grad_offset, -1.0))
        ctx.check_bounds()
        return out


def maplookup_pullback(strategy_prealloc, tables, sparse, dy):
    """Pullback of maplookup(PreallocationStrategy(P), tables, sparse) given dy [B][P + D*T]
    (e.g. dt_reshaped from dot_back): views, no arithmetic (the rows 1:P belong to x).
    HipTables + the LazyGrad of the fused interaction's pullback: DeferredUpdate views (lazy.py)."""
    from .lazy import HipTables, LazyGrad, pullback_lazy
    if isinstance(tables, HipTables) and isinstance(dy, LazyGrad):
        return pullback_lazy(strategy_prealloc, tables, dy)
    if isinstance(tables, HipTables):
        tables = tables.ts
    ts = as_table_set(tables)
    idx = PackedIndices(sparse, device=ts.device)
    return [SparseEmbeddingUpdate(dy, strategy_prealloc + t * ts.D, ts.D, idx, t) for t in range(len(ts))]


class SparseIndexer:
    """SparseIndexer(): dedupe state for `update_`.  One object serves a whole table set (the
    reference keeps one per table); sized for `capacity` lookups per table."""

    def __init__(self, num_tables, capacity, device=None):
        self.ctx = context(device)
        self.num_tables = int(num_tables)
        self.capacity = int(capacity)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dlrm_indexer_create(self.ctx.bind(), self.num_tables, self.capacity,
                                                        ctypes.byref(h)))
        self.handle = h
        self._built_from = None

    def build(self, tables, indices, *, index_base=1):
        """Dedupes `indices` (asynchronous).  May run on a side stream during the forward pass;
        pass prebuilt=True to update_ afterwards."""
        ts = as_table_set(tables)
        idx = PackedIndices(indices, device=ts.device)
        require_device(idx.data, ts.device, "indices")
        if idx.B * idx.L > self.capacity or idx.T != self.num_tables:
            raise ValueError("SparseIndexer: indices exceed the capacity / table count it was created for")
        self.ctx.check(self.ctx.lib.dlrm_indexer_build(self.ctx.bind(), self.handle, ts.handle, ptr(idx.data),
                                                       idx.itype, idx.stride, index_base, idx.B, idx.L))
        self._built_from = idx
        return self

    def prepare(self, tables, indices, *, index_base=1):
        """The training step's split build of `indices` (one-hot, <= 32768 positions per table) as its
        own launch (dlrm_indexer_prepare: the wave build): a following dlrm_step_fwd of
        these indices only gathers, and update_ / dlrm_sgd_update(PREBUILT) take its once-hit
        positions as well.  Returns False where the wave build does not apply (use build())."""
        ts = as_table_set(tables)
        idx = PackedIndices(indices, device=ts.device)
        require_device(idx.data, ts.device, "indices")
        if idx.L != 1 or idx.B > self.capacity or idx.T != self.num_tables:
            return False
        rc = self.ctx.lib.dlrm_indexer_prepare(self.ctx.bind(), self.handle, ts.handle, ptr(idx.data), idx.itype,
                                               idx.stride, index_base, idx.B)
        if rc == _lib.E_UNSUPPORTED:
            return False
        self.ctx.check(rc)
        self._built_from = idx
        return True

    def reserve(self, batch):
        """dlrm_indexer_reserve: a no-op since round 6 (the wave builds' packed layout needs no
        re-carving before a graph capture); kept for round-5 callers."""
        self.ctx.check(self.ctx.lib.dlrm_indexer_reserve(self.ctx.bind(), self.handle, int(batch)))
        return self

    def set_chunk(self, max_positions):
        """The wave build's chunk limit for later builds (16 or 32; dlrm_indexer_set_chunk)."""
        self.ctx.check(self.ctx.lib.dlrm_indexer_set_chunk(self.ctx.bind(), self.handle, int(max_positions)))
        return self

    def set_parts(self, parts):
        """Parts per table of later wave builds of <= 2048 positions (0 / 16, 32 or 64;
        dlrm_indexer_set_parts): the same segments whatever the setting."""
        self.ctx.check(self.ctx.lib.dlrm_indexer_set_parts(self.ctx.bind(), self.handle, int(parts)))
        return self

    def nbytes(self):
        """Device bytes held (dlrm_indexer_bytes: all allocated at creation, never grown)."""
        b = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.dlrm_indexer_bytes(self.handle, ctypes.byref(b)))
        return b.value

    def state(self):
        """Host-side state of the last build: a mask of _lib.IX_* bits (no GPU call)."""
        st = ctypes.c_uint()
        self.ctx.check(self.ctx.lib.dlrm_indexer_state(self.handle, ctypes.byref(st)))
        return st.value

    def unique_rows(self, table):
        """0-based unique rows touched in `table` by the last build, in segment order (synchronises)."""
        n = ctypes.c_int64()
        cap = self.capacity
        rows = (ctypes.c_int64 * max(cap, 1))()
        self.ctx.check(self.ctx.lib.dlrm_indexer_read(self.ctx.bind(), self.handle, table, ctypes.byref(n), rows,
                                                      None, None, cap))
        return list(rows[: n.value])

    def segments(self, table):
        """(unique_rows, positions, seg_start) of `table`: positions grouped by row (one segment per
        row, segment order unspecified), ascending within a row."""
        n = ctypes.c_int64()
        cap = self.capacity
        rows = (ctypes.c_int64 * max(cap, 1))()
        pos = (ctypes.c_int64 * max(cap, 1))()
        seg = (ctypes.c_int64 * (cap + 1))()
        self.ctx.check(self.ctx.lib.dlrm_indexer_read(self.ctx.bind(), self.handle, table, ctypes.byref(n), rows, pos,
                                                      seg, cap))
        U = n.value
        segs = list(seg[: U + 1])
        nv = segs[U] if U >= 0 else 0
        return list(rows[:U]), list(pos[:nv]), segs

    def __del__(self):
        try:
            if self.handle:
                self.ctx.lib.dlrm_indexer_destroy(self.handle)
        except Exception:
            pass


def update_(opt, tables, grads, indexers=None, *, num_splits=8, nthreads=12, index_base=None, deterministic=True,
            prebuilt=False, check_bounds=None):
    """EmbeddingTables.update!(opt, tables, grads, indexers; num_splits, nthreads).

    `grads` are the SparseEmbeddingUpdates of maplookup_pullback (they share one gradient
    matrix and one PackedIndices, so all tables update in one launch).  num_splits/nthreads
    are accepted for signature parity; the GPU decomposition is chunk-based.
    index_base: 1 (Julia) unless given; HipTables carry their own (a different one raises).
    Tables are mutated in place.  check_bounds (not a reference keyword): None = the default --
    synchronise and raise BoundsError for plain tables; HipTables follow their own policy (a
    deferred apply whose bounds surface at the next maplookup, lazy.py)."""
    del num_splits, nthreads
    from .lazy import DeferredUpdate, HipTables, update_lazy
    if isinstance(tables, HipTables) and grads and isinstance(grads[0], DeferredUpdate):
        tables.check_index_base(index_base, "update_")
        if not deterministic:
            raise ValueError("update_ on HipTables is the deterministic step apply (deterministic=False is not "
                             "available on the fused path)")
        # (indexers: accepted for the reference's signature; the step carries its own SparseIndexer)
        return update_lazy(opt, tables, grads, check_bounds=check_bounds)
    index_base = 1 if index_base is None else int(index_base)
    if isinstance(tables, HipTables):
        tables = tables.ts
    if not isinstance(opt, (Descent, _StatefulOpt)):
        raise TypeError("update_ implements Descent (plain SGD, the optimizer DLRM.jl trains with), ADAGrad, "
                        "RowwiseADAGrad, SplitDescent and StochasticDescent")
    stateful = isinstance(opt, _StatefulOpt)
    if stateful:
        if not deterministic:
            raise ValueError(f"update_ with {type(opt).__name__} is deterministic only: {opt.no_atomic}")
        opt.check_tables(_tables_dtype(tables))
    ts = as_table_set(tables)
    if len(grads) != len(ts):
        raise ValueError(f"{len(grads)} gradients for {len(ts)} tables")
    g0 = grads[0]
    for t, g in enumerate(grads):
        if (g.grad.data_ptr() != g0.grad.data_ptr() or g.indices is not g0.indices or g.table_index != t or
                g.grad_offset != g0.grad_offset + t * ts.D):
            raise ValueError("update_ expects the per-table views produced by maplookup_pullback")
    grad = g0.grad
    if grad.stride(1) != 1:
        raise ValueError("gradient rows must be contiguous")
    require_device(grad, ts.device, "gradient")
    idx = g0.indices.on(ts.device)
    if grad.shape[0] != idx.B:
        raise ValueError(f"gradient has {grad.shape[0]} rows for a batch of {idx.B}")
    flags = 0
    ix = None
    if deterministic:
        if indexers is None:
            indexers = SparseIndexer(len(ts), idx.B * idx.L, ts.device)
        ix = indexers
        if ix.num_tables != len(ts) or ix.capacity < idx.B * idx.L:
            raise ValueError("SparseIndexer too small for this batch / table set")
        if prebuilt:
            flags |= _lib.UPDATE_PREBUILT
    else:
        flags |= _lib.UPDATE_ATOMIC
    ctx = ts.ctx
    if stateful:
        ctx.check(opt.launch(ts, ix, flags, idx, index_base, grad, g0.grad_offset))
    else:
        ctx.check(ctx.lib.dlrm_sgd_update(ctx.bind(), ts.handle, ix.handle if ix is not None else None, flags,
                                          ptr(idx.data), idx.itype, idx.stride, index_base, idx.B, idx.L, ptr(grad),
                                          dtype_code(grad.dtype), grad.stride(0), g0.grad_offset, opt.eta))
    if check_bounds or check_bounds is None:
        ctx.check_bounds()
    return tables
