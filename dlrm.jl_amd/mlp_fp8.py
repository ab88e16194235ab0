"""Fused MXFP8 MLP inference: a whole Dense chain in one launch on the block-scaled fp8 MFMA (csrc/mlp_fp8.hip,
DESIGN.md section 31).

`Fp8MLP(dense_mlp)` quantises a `DenseMLP`'s fp32 weights to OCP MXFP8 in MFMA operand order (one launch) and `infer`
runs the chain a_{l+1} = act_l(a_l W_l^T + b_l) in one launch: e4m3 codes with one E8M0 scale per 32 consecutive k,
fp32 accumulation and bias, hidden activations re-quantised from fp32 and kept in LDS.  Scoring only.
`mx_quantize` and `mlp_fp8_reference` restate the arithmetic in numpy float64: the yardstick of tests/test_mlp_fp8.py.
"""
import ctypes

import numpy as np

from . import _lib


def _floor_log2(a):
    """floor(log2 a) of positive finite values, exactly (the binary exponent)."""
    return (np.frexp(a)[1] - 1).astype(np.float64)


def _e4m3_round(t):
    """float64 array -> the nearest OCP e4m3 values (ties to even, saturated to +-448), and their codes."""
    a = np.minimum(np.abs(t), 448.0)
    e = np.maximum(_floor_log2(np.maximum(a, 2.0 ** -20)), -6.0)  # below 2^-6 the subnormal step 2^-9
    step = 2.0 ** (e - 3)
    r = np.minimum(np.rint(a / step) * step, 448.0)  # (np.rint: ties to even; a value rounded up to 2^(e+1) is exact)
    er = _floor_log2(np.maximum(r, 2.0 ** -6))
    code = np.where(r < 2.0 ** -6, r * 2.0 ** 9, (er + 7) * 8 + (r / 2.0 ** er - 1) * 8)
    code = code.astype(np.uint8) | np.where(np.signbit(t) & (r > 0), 0x80, 0).astype(np.uint8)
    return np.copysign(r, t), code


def mx_quantize(a):
    """OCP MX v1.0 along the last axis in blocks of 32 (zero-padded to a multiple of 32): per block m = max |v|,
    X = clamp(floor(log2 m) - 8, -127, 127), the scale byte X + 127 (0 for a zero block), the codes
    RNE_e4m3(v 2^-X) saturated to +-448.  Returns (codes uint8 [..., Kp], scale bytes uint8 [..., Kp / 32], the
    dequantised values float64 [..., Kp]).  Finite inputs."""
    a = np.asarray(a, dtype=np.float64)
    K = a.shape[-1]
    Kp = (K + 31) // 32 * 32
    v = np.zeros(a.shape[:-1] + (Kp,), np.float64)
    v[..., :K] = a
    blk = v.reshape(a.shape[:-1] + (Kp // 32, 32))
    m = np.abs(blk).max(axis=-1)
    X = np.where(m > 0, np.clip(_floor_log2(np.where(m > 0, m, 1.0)) - 8, -127, 127), -127.0)
    r, codes = _e4m3_round(blk * 2.0 ** -X[..., None])
    vals = r * 2.0 ** X[..., None]
    return codes.reshape(v.shape), (X + 127).astype(np.uint8), vals.reshape(v.shape)


def mlp_fp8_reference(x, Ws, bs, last_relu, acts=None):
    """The chain in float64 on MXFP8 operands: x [B][K0] and every W_l [N][K] through `mx_quantize` along k, the bias
    fp32; every hidden activation relu'd, rounded to fp32 (what the kernel holds) and quantised once; the last layer
    relu'd if `last_relu`, NOT rounded.  Returns (y, S): the last layer's values and S = sum_k |a_k w_k| + |b| of
    them over the dequantised operands (the error bound's scale).  acts: a list that receives every hidden
    activation as the next layer reads it (dequantised, [B][N])."""
    a = mx_quantize(np.asarray(x, dtype=np.float64))[2]
    n = len(Ws)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        W = np.asarray(W, dtype=np.float64)
        N, K = W.shape
        Wq = mx_quantize(W)[2]
        b = np.asarray(b, dtype=np.float32).astype(np.float64)
        a = a[:, :Wq.shape[1]] if a.shape[1] >= Wq.shape[1] else np.pad(a, ((0, 0), (0, Wq.shape[1] - a.shape[1])))
        y = a @ Wq.T + b
        if i == n - 1:
            S = np.abs(a) @ np.abs(Wq).T + np.abs(b)
            return (np.maximum(y, 0.0) if last_relu else y), S
        a = mx_quantize(np.maximum(y, 0.0).astype(np.float32).astype(np.float64))[2][:, :N]
        if acts is not None:
            acts.append(a)


def mlp_fp8_plan(sizes, batch, x_dtype=_lib.F32, out_dtype=_lib.F32):
    """csrc/mlp_fp8_plan.hpp through dlrm_mlp_fp8_plan (pure host): dict(rc, mt, grid, lds_bytes, packed_bytes, kp,
    np, offsets), offsets a (codes, scales, bias) byte triple per layer."""
    lib = _lib.load()
    layers = len(sizes) - 1
    n = max(layers, 1)
    arr = (ctypes.c_int * max(len(sizes), 1))(*sizes)
    mt, grid = ctypes.c_int(), ctypes.c_int()
    lds, packed = ctypes.c_int64(), ctypes.c_int64()
    kp, npad, off = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int64 * (3 * n))()
    rc = lib.dlrm_mlp_fp8_plan(layers, arr, int(batch), x_dtype, out_dtype, ctypes.byref(mt), ctypes.byref(grid),
                               ctypes.byref(lds), ctypes.byref(packed), kp, npad, off)
    L = max(layers, 0)
    return dict(rc=rc, mt=mt.value, grid=grid.value, lds_bytes=lds.value, packed_bytes=packed.value,
                kp=list(kp)[:L], np=list(npad)[:L], offsets=[tuple(off[3 * l:3 * l + 3]) for l in range(L)])


class Fp8MLP:
    """The packed MXFP8 form of a `DenseMLP` (create + pack).  The handle owns the packed weights; `mlp`'s own fp32
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
        self.ctx.check(self.lib.dlrm_mlp_fp8_create(self.ctx.bind(), len(self.sizes) - 1, arr, ctypes.byref(self.handle)))
        self.repack()

    def repack(self):
        """Quantises the DenseMLP's current weights and biases again (one launch, capturable): after training steps."""
        import torch
        n = len(self.sizes) - 1
        W, b = self.mlp.W, self.mlp.b
        for t in W + b:
            if t.dtype != torch.float32 or t.device != self.device or t.stride(-1) != 1:
                raise ValueError("Fp8MLP: weights and biases are float32 rows on the MLP's device")
        wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in W])
        bp = (ctypes.c_void_p * n)(*[v.data_ptr() for v in b])
        ld = (ctypes.c_int64 * n)(*[w.stride(0) for w in W])
        self.ctx.check(self.lib.dlrm_mlp_fp8_pack(self.ctx.bind(), self.handle, wp, ld, bp))
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
        self.ctx.check(self.lib.dlrm_mlp_fp8_infer(self.ctx.bind(), self.handle, B, ptr(x), dtype_code(x.dtype),
                                                   x.stride(0), ptr(out), dtype_code(out.dtype), out.stride(0),
                                                   int(bool(last_relu))))
        return out

    def __del__(self):
        try:
            if self.handle:
                self.lib.dlrm_mlp_fp8_destroy(self.handle)
        except Exception:
            pass
