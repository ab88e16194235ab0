"""Fused bf16 MLP inference: a whole Dense chain in one MFMA launch (csrc/mlp_bf16.hip).

`Bf16MLP(dense_mlp)` packs a `DenseMLP`'s fp32 weights as bf16 in MFMA operand order (one launch) and `infer` runs
the chain a_{l+1} = act_l(a_l W_l^T + b_l) in one launch: bf16 operands, fp32 accumulation and bias, hidden
activations rounded to bf16 and kept in LDS.  Scoring only; training keeps the fp32 GEMMs.  `mlp_bf16_reference`
restates the arithmetic in numpy float64: the yardstick of tests/test_mlp_bf16.py.
"""
import ctypes

import numpy as np

from . import _lib


def _bf16_round(a):
    """float64 / float32 array -> the nearest bf16 values (ties to even), as float64.  Finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def mlp_bf16_reference(x, Ws, bs, last_relu, acts=None):
    """The chain in float64 on bf16-rounded operands: x [B][K0] and every W_l [N][K] rounded to bf16, the bias fp32;
    every hidden activation relu'd and rounded to bf16; the last layer relu'd if `last_relu`, NOT rounded.  Returns
    (y, S): the last layer's values and S = sum_k |a_k w_k| + |b| of them (the error bound's scale).  acts: a list
    that receives every hidden activation."""
    a = _bf16_round(np.asarray(x, dtype=np.float64))
    n = len(Ws)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        Wr = _bf16_round(np.asarray(W, dtype=np.float64))
        b = np.asarray(b, dtype=np.float32).astype(np.float64)
        y = a @ Wr.T + b
        if i == n - 1:
            S = np.abs(a) @ np.abs(Wr).T + np.abs(b)
            return (np.maximum(y, 0.0) if last_relu else y), S
        a = _bf16_round(np.maximum(y, 0.0))
        if acts is not None:
            acts.append(a)


def mlp_bf16_plan(sizes, batch, x_dtype=_lib.F32, out_dtype=_lib.F32):
    """csrc/mlp_plan.hpp through dlrm_mlp_bf16_plan (pure host): dict(rc, mt, grid, lds_bytes, packed_bytes, kp, np)."""
    lib = _lib.load()
    layers = len(sizes) - 1
    arr = (ctypes.c_int * max(len(sizes), 1))(*sizes)
    mt, grid = ctypes.c_int(), ctypes.c_int()
    lds, packed = ctypes.c_int64(), ctypes.c_int64()
    kp, npad = (ctypes.c_int * max(layers, 1))(), (ctypes.c_int * max(layers, 1))()
    rc = lib.dlrm_mlp_bf16_plan(layers, arr, int(batch), x_dtype, out_dtype, ctypes.byref(mt), ctypes.byref(grid),
                                ctypes.byref(lds), ctypes.byref(packed), kp, npad)
    return dict(rc=rc, mt=mt.value, grid=grid.value, lds_bytes=lds.value, packed_bytes=packed.value,
                kp=list(kp)[:max(layers, 0)], np=list(npad)[:max(layers, 0)])


class Bf16MLP:
    """The packed bf16 form of a `DenseMLP` (create + pack).  The handle owns the packed weights; `mlp`'s own fp32
    weights are only read, by `repack()`.  A chain without a kernel (more than 8 layers, a width above 1024) raises
    DLRMError(E_UNSUPPORTED): there is no fall-back."""

    def __init__(self, mlp):
        from .runtime import context
        self.mlp = mlp
        self.sizes = [int(s) for s in mlp.sizes]
        self.device = mlp.W[0].device
        self.ctx = context(self.device)
        self.lib = self.ctx.lib
        self.handle = ctypes.c_void_p()
        arr = (ctypes.c_int * len(self.sizes))(*self.sizes)
        self.ctx.check(self.lib.dlrm_mlp_bf16_create(self.ctx.bind(), len(self.sizes) - 1, arr, ctypes.byref(self.handle)))
        self.repack()

    def repack(self):
        """Packs the DenseMLP's current weights and biases again (one launch, capturable): after training steps."""
        import torch
        n = len(self.sizes) - 1
        W, b = self.mlp.W, self.mlp.b
        for t in W + b:
            if t.dtype != torch.float32 or t.device != self.device or t.stride(-1) != 1:
                raise ValueError("Bf16MLP: weights and biases are float32 rows on the MLP's device")
        wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in W])
        bp = (ctypes.c_void_p * n)(*[v.data_ptr() for v in b])
        ld = (ctypes.c_int64 * n)(*[w.stride(0) for w in W])
        self.ctx.check(self.lib.dlrm_mlp_bf16_pack(self.ctx.bind(), self.handle, wp, ld, bp))
        return self

    def infer(self, x, out=None, out_dtype=None, last_relu=None):
        """x: [B][>= sizes[0]] float32 or bfloat16 rows (any leading dimension); returns out [B][sizes[-1]] of
        `out_dtype` (default float32; `out`: a buffer to write, its dtype and leading dimension are taken).
        last_relu: the last layer's activation (default: relu unless the MLP ends in the sigmoid, whose logits are
        returned)."""
        import torch
        from .runtime import dtype_code, ptr, require_device
        require_device(x, self.device, "x")
        if x.dim() != 2 or x.shape[1] != self.sizes[0] or x.stride(1) != 1:
            raise ValueError(f"x must be [B][{self.sizes[0]}] rows")
        B = x.shape[0]
        if out is None:
            out = torch.empty((B, self.sizes[-1]), dtype=out_dtype or torch.float32, device=self.device)
        else:
            require_device(out, self.device, "out")
            if out.dim() != 2 or out.shape != (B, self.sizes[-1]) or out.stride(1) != 1:
                raise ValueError(f"out must be [{B}][{self.sizes[-1]}] rows")
        if last_relu is None:
            last_relu = not self.mlp.sigmoid_last
        self.ctx.check(self.lib.dlrm_mlp_bf16_infer(self.ctx.bind(), self.handle, B, ptr(x), dtype_code(x.dtype),
                                                    x.stride(0), ptr(out), dtype_code(out.dtype), out.stride(0),
                                                    int(bool(last_relu))))
        return out

    def __del__(self):
        try:
            if self.handle:
                self.lib.dlrm_mlp_bf16_destroy(self.handle)
        except Exception:
            pass
