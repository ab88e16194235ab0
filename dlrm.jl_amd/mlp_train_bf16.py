"""Mixed-precision MLP training: forward, dgrad and wgrad of a Dense chain on bf16 MFMA (csrc/mlp_train.hip,
DESIGN.md section 28).

`Bf16TrainMLP(dense_mlp, max_batch)` owns the torch buffers the kernels read and write -- the bf16 weights, the saved
activations, the gradients g_l and the wgrad slab partials, at `mlp_train_plan`'s sizes -- so every saved tensor can be
read back.  fp32 masters (the `DenseMLP`'s own W, b, gW, gb), bf16 operands, fp32 accumulation.
`mlp_train_bf16_reference` restates the arithmetic in numpy float64: the yardstick of tests/test_mlp_train_bf16.py.
"""
import ctypes

import numpy as np

from . import _lib
from .mlp_bf16 import _bf16_round

_MAXL = 8


class Layout(ctypes.Structure):
    """include/dlrm_hip.h dlrm_mlp_train_layout."""
    _fields_ = ([("layers", ctypes.c_int), ("batch", ctypes.c_int), ("ldt", ctypes.c_int),
                 ("tile", ctypes.c_int * 3 * 3), ("ld", ctypes.c_int * (_MAXL + 1)), ("slabs", ctypes.c_int * _MAXL),
                 ("slab_rows", ctypes.c_int * _MAXL), ("grid", ctypes.c_int * 3 * 3 * _MAXL)] +
                [f for n in "wagp" for f in ((f"{n}_off", ctypes.c_int64 * _MAXL),
                                             (f"{n}{'b' if n == 'p' else 't'}_off", ctypes.c_int64 * _MAXL),
                                             (f"{n}_bytes", ctypes.c_int64))])


def mlp_train_plan(sizes, batch):
    """csrc/mlp_train_plan.hpp through dlrm_mlp_train_plan (pure host): dict(rc, ...) with the layout's fields as
    lists cut to the chain's layers (ld: layers + 1; grid[layer][role] = [x, y, z], roles forward, dgrad, wgrad)."""
    lib = _lib.load()
    n = len(sizes) - 1
    L = Layout()
    rc = lib.dlrm_mlp_train_plan(n, (ctypes.c_int * max(len(sizes), 1))(*sizes), int(batch), ctypes.byref(L))
    if rc != _lib.OK:
        return dict(rc=rc)
    d = dict(rc=rc, layers=L.layers, batch=L.batch, ldt=L.ldt, tile=[list(r) for r in L.tile], ld=list(L.ld)[:n + 1],
             slabs=list(L.slabs)[:n], slab_rows=list(L.slab_rows)[:n],
             grid=[[list(r) for r in L.grid[l]] for l in range(n)])
    for name, _ in Layout._fields_[8:]:
        v = getattr(L, name)
        d[name] = v if isinstance(v, int) else list(v)[:n]
    return d


def mlp_train_bf16_reference(x, Ws, bs, dy, last_relu, need_dx=True):
    """One forward and backward in float64 on bf16-rounded operands.  x [B][K0], W_l [N][K], b_l [N], dy [B][N_last].
    Forward: a_0 = bf16(x); z = a W16^T + b; hidden a_l = bf16(relu(z)); the last layer relu(z) if `last_relu` else z,
    NOT rounded.  Backward: g_n = bf16(dy), where out > 0 if `last_relu`; gW_l = g_l^T a_{l-1}, gb_l = sum_m g_l;
    g_{l-1} = bf16((g_l W16_l) * (a_{l-1} > 0)); dx = g_1 W16_1, NOT rounded and not masked.
    Returns dict(out, acts [a_0 ..], g [g_1 .. g_n], gW, gb, dx)."""
    n = len(Ws)
    W16 = [_bf16_round(np.asarray(W, dtype=np.float64)) for W in Ws]
    acts = [_bf16_round(np.asarray(x, dtype=np.float64))]
    for l in range(n):
        z = acts[-1] @ W16[l].T + np.asarray(bs[l], dtype=np.float32).astype(np.float64)
        if l == n - 1:
            out = np.maximum(z, 0.0) if last_relu else z
        else:
            acts.append(_bf16_round(np.maximum(z, 0.0)))
    g = _bf16_round(np.asarray(dy, dtype=np.float64))
    if last_relu:
        g = g * (out > 0)
    gs, gW, gb, dx = [None] * n, [None] * n, [None] * n, None
    for l in reversed(range(n)):
        gs[l] = g
        gW[l] = g.T @ acts[l]
        gb[l] = g.sum(0)
        if l > 0:
            g = _bf16_round((g @ W16[l]) * (acts[l] > 0))
        elif need_dx:
            dx = g @ W16[0]
    return dict(out=out, acts=acts, g=gs, gW=gW, gb=gb, dx=dx)


class Bf16TrainMLP:
    """The training state of a `DenseMLP` on the bf16 kernels, for batches up to `max_batch`.  Views of the buffers,
    per layer l (0-based: W[l] is [N][K], its input level l, its output level l + 1):
      W16[l] [N][ld K], W16T[l] [K][ld N]          bf16(W) as last refreshed
      a[l] [max_batch][ld K], aT[l] [K][ldt]       the layer's input as the last forward saved it
      g[l] [max_batch][ld N], gT[l] [N][ldt]       dLoss/d(the layer's output) of the last backward
    A chain without a kernel (more than 8 layers, a width above 8192) raises DLRMError(E_UNSUPPORTED)."""

    def __init__(self, mlp, max_batch):
        import torch
        from .runtime import context
        self.mlp = mlp
        self.sizes = [int(s) for s in mlp.sizes]
        self.max_batch = int(max_batch)
        self.device = mlp.W[0].device
        self.ctx = context(self.device)
        self.lib = self.ctx.lib
        n = self.n = len(self.sizes) - 1
        self.handle = ctypes.c_void_p()
        arr = (ctypes.c_int * len(self.sizes))(*self.sizes)
        self.ctx.check(self.lib.dlrm_mlp_train_create(self.ctx.bind(), n, arr, self.max_batch, ctypes.byref(self.handle)))
        p = self.plan = mlp_train_plan(self.sizes, self.max_batch)

        def buf(nbytes):
            return torch.zeros(nbytes // 2, dtype=torch.bfloat16, device=self.device)

        def view(b, off, rows, cols):
            return b[off // 2: off // 2 + rows * cols].view(rows, cols)

        self.w16, self.acts, self.grads = buf(p["w_bytes"]), buf(p["a_bytes"]), buf(p["g_bytes"])
        self.part = torch.zeros(p["p_bytes"] // 4, dtype=torch.float32, device=self.device)
        ld, ldt, S = p["ld"], p["ldt"], self.sizes
        self.W16 = [view(self.w16, p["w_off"][l], S[l + 1], ld[l]) for l in range(n)]
        self.W16T = [view(self.w16, p["wt_off"][l], S[l], ld[l + 1]) for l in range(n)]
        self.a = [view(self.acts, p["a_off"][l], self.max_batch, ld[l]) for l in range(n)]
        self.aT = [view(self.acts, p["at_off"][l], S[l], ldt) for l in range(n)]
        self.g = [view(self.grads, p["g_off"][l], self.max_batch, ld[l + 1]) for l in range(n)]
        self.gT = [view(self.grads, p["gt_off"][l], S[l + 1], ldt) for l in range(n)]
        self._out = None
        self._B = 0
        self.refresh()

    def _ptrs(self, ts):
        return (ctypes.c_void_p * self.n)(*[t.data_ptr() for t in ts])

    def refresh(self):
        """bf16(W) of the DenseMLP's current masters into W16 and W16T (one launch, capturable): after every Descent."""
        import torch
        W = self.mlp.W
        for t in W + self.mlp.b:
            if t.dtype != torch.float32 or t.device != self.device or t.stride(-1) != 1:
                raise ValueError("Bf16TrainMLP: weights and biases are float32 rows on the MLP's device")
        ld = (ctypes.c_int64 * self.n)(*[w.stride(0) for w in W])
        self.ctx.check(self.lib.dlrm_mlp_train_refresh(self.ctx.bind(), self.handle, self._ptrs(W), ld, self.w16.data_ptr()))
        return self

    def forward(self, x, out=None, out_dtype=None):
        """x: [B][sizes[0]] float32 or bfloat16 rows, B <= max_batch; returns out [B][sizes[-1]] (`out`: a buffer to
        write, float32 or bfloat16; default a new one of `out_dtype`, default float32): the logits of a sigmoid-last
        MLP, relu(z) otherwise.  Saves what `backward` reads."""
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
        self.ctx.check(self.lib.dlrm_mlp_train_forward(
            self.ctx.bind(), self.handle, B, ptr(x), dtype_code(x.dtype), x.stride(0), self._ptrs(self.mlp.b),
            self.w16.data_ptr(), self.acts.data_ptr(), ptr(out), dtype_code(out.dtype), out.stride(0),
            int(not self.mlp.sigmoid_last)))
        self._out, self._B = out, B
        return out

    def backward(self, dy, need_dx=True, dx_dtype=None, dx=None):
        """dy = dLoss/d(the last forward's result), [B][sizes[-1]] float32 or bfloat16 -> dx [B][sizes[0]] of
        `dx_dtype` (default float32; `dx`: a buffer to write), or None without `need_dx`.  Fills the DenseMLP's gW and
        gb; the last gb of a sigmoid-last MLP is left to its writer (dlrm_bce_head)."""
        import torch
        from .runtime import dtype_code, ptr, require_device
        require_device(dy, self.device, "dy")
        B = self._B
        if self._out is None or dy.shape != (B, self.sizes[-1]) or dy.stride(1) != 1:
            raise ValueError(f"dy must be [{B}][{self.sizes[-1]}] rows, after a forward")
        if need_dx and dx is None:
            dx = torch.empty((B, self.sizes[0]), dtype=dx_dtype or torch.float32, device=self.device)
        if not need_dx:
            dx = None
        elif dx.shape != (B, self.sizes[0]) or dx.stride(1) != 1:
            raise ValueError(f"dx must be [{B}][{self.sizes[0]}] rows")
        mlp, out = self.mlp, (None if self.mlp.sigmoid_last else self._out)
        ldw = (ctypes.c_int64 * self.n)(*[g.stride(0) for g in mlp.gW])
        self.ctx.check(self.lib.dlrm_mlp_train_backward(
            self.ctx.bind(), self.handle, B, ptr(dy), dtype_code(dy.dtype), dy.stride(0),
            None if out is None else ptr(out), 0 if out is None else dtype_code(out.dtype),
            0 if out is None else out.stride(0), self.w16.data_ptr(), self.acts.data_ptr(), self.grads.data_ptr(),
            self.part.data_ptr(), self._ptrs(mlp.gW), ldw, self._ptrs(mlp.gb), int(not mlp.sigmoid_last),
            None if dx is None else ptr(dx), 0 if dx is None else dtype_code(dx.dtype),
            0 if dx is None else dx.stride(0)))
        return dx

    def __del__(self):
        try:
            if self.handle:
                self.lib.dlrm_mlp_train_destroy(self.handle)
        except Exception:
            pass
