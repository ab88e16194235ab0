"""int8 row-quantized embedding tables for inference and evaluation (include/dlrm_hip.h).

A quantized table is codes `q[N][D]` (uint8) and `sb[N]` = {scale, bias} (fp32 pairs), two device arrays:
the standard DLRM serving format (8-bit rows with a per-row scale and bias), half the bytes of bf16 rows and a
quarter of fp32 rows.  `quantize_rows` / `dequantize_rows` restate the arithmetic in numpy float32, element for
element and bit for bit (every operation separately rounded; the kernels never fuse the dequantizing multiply and
add); they play the role `sr_round` and `eval_reference` play for their features.

`QuantizedTableSet` owns the arrays and the library handle, `Q8Inference` is `HotPath.infer` over them, and
`DLRMModel.quantize()` / `predict(..., q8=)` / `test(..., q8=)` score a trained model on its quantized tables.
"""
import ctypes

import numpy as np

from . import _lib

_F = np.float32


def _as_f32_rows(w):
    w = np.asarray(w)
    if w.dtype != np.float32:
        raise TypeError("rows are float32 (bf16 rows: their values as float32)")
    if w.ndim != 2:
        raise ValueError("rows are [N][D]")
    return w


def quantize_rows(w):
    """[N][D] float32 rows (bf16 rows: their values, exactly, as float32) -> (q [N][D] uint8, scale [N], bias [N])
    by the library's arithmetic, each operation one float32 rounding:
    lo = min, hi = max, range = hi - lo, scale = range / 255, inv = 255 / range (0 for a constant row),
    q = min(255, max(0, rint((w - lo) * inv))) with ties to even, bias = lo."""
    w = _as_f32_rows(w)
    lo = w.min(axis=1)
    hi = w.max(axis=1)
    with np.errstate(all="ignore"):
        rng = (hi - lo).astype(_F)
        scale = (rng / _F(255.0)).astype(_F)
        inv = np.where(rng > 0, _F(255.0) / np.where(rng > 0, rng, _F(1.0)), _F(0.0)).astype(_F)
        t = ((w - lo[:, None]).astype(_F) * inv[:, None]).astype(_F)
        q = np.minimum(_F(255.0), np.maximum(_F(0.0), np.rint(t))).astype(np.uint8)
    return q, scale, lo.astype(_F)


def bf16_round(v):
    """float32 -> the nearest bf16 value (ties to even), as float32: the library's f32_to_bf16 for finite values."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def dequantize_rows(q, scale, bias, dtype=np.float32):
    """v = (q * scale) + bias in two float32 roundings (never an fma); dtype float32, or "bfloat16" /
    torch.bfloat16: v rounded once to bf16 (returned as float32 values)."""
    q = np.asarray(q)
    if q.dtype != np.uint8 or q.ndim != 2:
        raise TypeError("codes are [N][D] uint8")
    scale = np.asarray(scale, dtype=_F).reshape(-1, 1)
    bias = np.asarray(bias, dtype=_F).reshape(-1, 1)
    with np.errstate(all="ignore"):
        v = ((q.astype(_F) * scale).astype(_F) + bias).astype(_F)
    if str(dtype).endswith("bfloat16"):
        return bf16_round(v)
    if not str(dtype).endswith("float32") and np.dtype(dtype) != np.float32:
        raise TypeError("dequantize_rows: float32 or bfloat16")
    return v


def q8_bound(w, scale):
    """The derived error bound of a quantized row, per element: (0.5 + 2^-10) * scale + 2^-22 * max(|lo|, |hi|)
    -- (w - lo) * inv is two roundings on a value of at most 255 (under 2^-10 codes before the rint), and the two
    dequantizing roundings are relative 2^-24 each on magnitudes of at most max(|lo|, |hi|)."""
    w = _as_f32_rows(w).astype(np.float64)
    m = np.maximum(np.abs(w.min(axis=1)), np.abs(w.max(axis=1)))
    return (0.5 + 2.0 ** -10) * np.asarray(scale, dtype=np.float64) + 2.0 ** -22 * m


class QuantizedTableSet:
    """T quantized tables of one feature size registered with the library (one dlrm_q8_tables): `qs[t]` a
    [N_t][D] uint8 device tensor, `sbs[t]` a [N_t][2] float32 one ({scale, bias} per row)."""

    def __init__(self, qs, sbs):
        import torch
        from .runtime import context
        qs, sbs = list(qs), list(sbs)
        if not qs or len(qs) != len(sbs):
            raise ValueError("QuantizedTableSet needs as many code arrays as scale/bias arrays, at least one")
        D, dev = qs[0].shape[1], qs[0].device
        for q, sb in zip(qs, sbs):
            if q.dtype != torch.uint8 or q.dim() != 2 or q.shape[1] != D or not q.is_contiguous():
                raise ValueError("codes are contiguous [N][D] uint8 tensors of one D")
            if sb.dtype != torch.float32 or sb.shape != (q.shape[0], 2) or not sb.is_contiguous():
                raise ValueError("scale/bias arrays are contiguous [N][2] float32 tensors")
            if not q.is_cuda or q.device != dev or sb.device != dev:
                raise ValueError("quantized tables live on one GPU")
        self.qs, self.sbs = qs, sbs
        self.D, self.device = int(D), dev
        self.ctx = context(dev)
        T = len(qs)
        qp = (ctypes.c_void_p * T)(*[q.data_ptr() for q in qs])
        sp = (ctypes.c_void_p * T)(*[sb.data_ptr() for sb in sbs])
        nrows = (ctypes.c_int64 * T)(*[q.shape[0] for q in qs])
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.dlrm_q8_tables_create(self.ctx.bind(), T, self.D, qp, sp, nrows, ctypes.byref(h)))
        self.handle = h

    @classmethod
    def from_arrays(cls, qs, sbs):
        """Wraps given device tensors (codes [N_t][D] uint8, scale/bias [N_t][2] float32)."""
        return cls(qs, sbs)

    @classmethod
    def from_tables(cls, ts):
        """Allocates the codes and scale/bias arrays of `ts` (an EmbeddingTableSet, fp32 or bf16) and quantizes it
        (dlrm_q8_quantize: one launch over every table)."""
        import torch
        from .embedding import as_table_set
        ts = as_table_set(ts)
        qs = [torch.empty((len(t), ts.D), dtype=torch.uint8, device=ts.device) for t in ts]
        sbs = [torch.empty((len(t), 2), dtype=torch.float32, device=ts.device) for t in ts]
        return cls(qs, sbs).quantize_from(ts)

    def quantize_from(self, ts):
        """Quantizes `ts` (same table count, feature size and row counts) into this set's arrays."""
        self.ctx.check(self.ctx.lib.dlrm_q8_quantize(self.ctx.bind(), ts.handle, self.handle))
        return self

    def dequantize(self, dtype=None):
        """An EmbeddingTableSet of v (float32, the default) or bf16(v) (dlrm_q8_dequantize)."""
        import torch
        from .embedding import EmbeddingTableSet
        dtype = torch.float32 if dtype is None else dtype
        ts = EmbeddingTableSet([torch.empty((q.shape[0], self.D), dtype=dtype, device=self.device) for q in self.qs])
        self.ctx.check(self.ctx.lib.dlrm_q8_dequantize(self.ctx.bind(), self.handle, ts.handle))
        return ts

    def __len__(self):
        return len(self.qs)

    @property
    def dim(self):
        return self.D

    def nrows(self):
        return [q.shape[0] for q in self.qs]

    @property
    def nbytes(self):
        """Bytes of the codes plus the scale/bias arrays."""
        return sum(q.numel() + sb.numel() * 4 for q, sb in zip(self.qs, self.sbs))

    def __del__(self):
        try:
            if self.handle:
                self.ctx.lib.dlrm_q8_tables_destroy(self.handle)
        except Exception:
            pass


class Q8Inference:
    """`HotPath.infer` over quantized tables: lookup + interaction into `out` ([batch][width] of `dtype`, which is
    also x's).  One launch (dlrm_q8_lookup_interact_fwd) where the fused kernel exists; a shape without it takes
    dlrm_q8_maplookup + dlrm_interact_fwd through a `ys` allocated on its first call (allocate before a graph
    capture by one eager call), with the same bits.  `route` says which ran last: "fused" or "two-launch"."""

    def __init__(self, q8, batch, lookups=1, *, d=None, dtype=None, index_base=0, pad_to=1):
        import torch
        from .interact import interaction_sizes
        from .runtime import dtype_code
        if not isinstance(q8, QuantizedTableSet):
            raise TypeError("Q8Inference: q8 is a QuantizedTableSet")
        self.q8 = q8
        self.B, self.L = int(batch), int(lookups)
        self.T, self.D = len(q8), q8.D
        self.d = self.D if d is None else int(d)
        if self.d != self.D:
            raise ValueError(f"Q8Inference: the dense vector length {self.d} must equal the feature size {self.D}")
        self.F = self.T + 1
        self.dtype = torch.float32 if dtype is None else dtype
        self.dcode = dtype_code(self.dtype)
        self.index_base = int(index_base)
        _, self.width, self.padding = interaction_sizes(self.d, self.F, pad_to)
        self.out = torch.empty((self.B, self.width), dtype=self.dtype, device=q8.device)
        self.ys = None
        self.route = None
        self.ctx, self.lib = q8.ctx, q8.ctx.lib

    def _check(self, rc):
        if rc != _lib.OK:
            self.ctx.check(rc)

    def fused(self, x, idx, out=None):
        """The raw fused call's status: _lib.OK (launched) or _lib.E_UNSUPPORTED (nothing launched)."""
        from .runtime import ptr
        out = self.out if out is None else out
        rc = self.lib.dlrm_q8_lookup_interact_fwd(self.ctx.bind(), self.q8.handle, ptr(idx.data), idx.itype, idx.stride,
                                                  self.index_base, self.B, self.L, self.dcode, ptr(x), x.stride(0),
                                                  ptr(out), out.stride(0), self.padding)
        if rc != _lib.E_UNSUPPORTED:
            self._check(rc)
        return rc

    def two_launch(self, x, idx, out=None):
        """dlrm_q8_maplookup into `ys`, then dlrm_interact_fwd."""
        import torch
        from .runtime import ptr
        out = self.out if out is None else out
        if self.ys is None:
            self.ys = torch.empty((self.B, self.F * self.D), dtype=self.dtype, device=self.q8.device)
        h, ys = self.ctx.bind(), self.ys
        self._check(self.lib.dlrm_q8_maplookup(h, self.q8.handle, ptr(idx.data), idx.itype, idx.stride, self.index_base,
                                               self.B, self.L, self.dcode, ptr(ys), ys.stride(0), self.d))
        self._check(self.lib.dlrm_interact_fwd(h, self.dcode, self.d, self.F, self.B, ptr(x), x.stride(0), ptr(ys),
                                               ys.stride(0), ptr(out), out.stride(0), self.padding))
        self.route = "two-launch"
        return out

    def infer(self, x, idx, out=None):
        """x: [batch][d] of `dtype`; idx: PackedIndices.  `out`: another [batch][>= width] buffer of `dtype`."""
        if self.route != "two-launch":
            if self.fused(x, idx, out) == _lib.OK:
                self.route = "fused"
                return self.out if out is None else out
        return self.two_launch(x, idx, out)

    def check_bounds(self):
        self.ctx.check_bounds()
