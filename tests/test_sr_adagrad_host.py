"""The Adagrad rules with the stochastic store on the host: the optimizer classes' seed handling, repr and table check,
the new C entry points' NULL-argument returns, and the walk of row-wise Adagrad steps below half a bf16 ulp restated
in numpy with sr_round against the closed form (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch


def _rules(pkg):
    return (pkg.ADAGrad, pkg.RowwiseADAGrad)


def test_entry_points_reject_null_arguments(pkg):
    """Argument validation runs on the host before any HIP call."""
    _lib = pkg._lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    for rowwise in (0, 1):
        assert lib.dlrm_adagrad_create_sr(None, None, rowwise, None, 0, ctypes.byref(out)) == _lib.E_ARG
        assert lib.dlrm_adagrad_create_sr(None, None, rowwise, None, 0, None) == _lib.E_ARG
        assert not out.value
    assert lib.dlrm_adagrad_seek(None, None, 0) == _lib.E_ARG
    step = ctypes.c_uint64(77)
    assert lib.dlrm_adagrad_step(None, None, ctypes.byref(step)) == _lib.E_ARG and step.value == 77
    assert lib.dlrm_adagrad_step(None, None, None) == _lib.E_ARG
    assert lib.dlrm_adagrad_destroy(None) == 0


def test_optimizer_classes(pkg):
    for rule in _rules(pkg):
        name = rule.__name__
        o = rule()
        assert o.seed is None and repr(o) == f"{name}(0.1, 1e-08)"
        assert o.step_keyword == "adagrad_step" and o.step_entry[0] == "dlrm_adagrad_step_bwd"
        o = rule(0.5, 1e-6, seed=0)
        assert o.seed == 0 and (o.eta, o.eps) == (0.5, 1e-6) and repr(o) == f"{name}(0.5, 1e-06, seed=0)"
        assert o.step_keyword is None and o.step_entry is None  # (no fused step: the operator route)
        o = rule(0.5, seed=2 ** 63 + 7)
        assert o.seed == 2 ** 63 + 7 and repr(o) == f"{name}(0.5, 1e-08, seed={2 ** 63 + 7})"
        assert rule().step_keyword == "adagrad_step"  # (a seeded instance leaves the class as it was)
        for bad in (1.0, "7", True):
            with pytest.raises(TypeError):
                rule(0.1, seed=bad)
        for bad in (-1, 2 ** 64):
            with pytest.raises(ValueError):
                rule(0.1, seed=bad)
        assert name in pkg.__all__


def test_check_tables(pkg):
    for rule in _rules(pkg):
        for dtype in (torch.float32, torch.bfloat16):
            rule().check_tables(dtype)  # (seedless: both, as before)
        rule(seed=1).check_tables(torch.bfloat16)
        with pytest.raises(ValueError, match="bfloat16"):
            rule(seed=1).check_tables(torch.float32)
        with pytest.raises(ValueError, match="bfloat16"):
            pkg.update_(rule(seed=1), [torch.zeros((4, 8), dtype=torch.float32)], [], index_base=0)
        with pytest.raises(ValueError, match="deterministic"):
            pkg.update_(rule(seed=1), [torch.zeros((4, 8), dtype=torch.bfloat16)], [], index_base=0, deterministic=False)
        # no seed: no step to set or read (refused before any table is looked at)
        for call in (lambda o: o.seek(None, 3), lambda o: o.step_of(None)):
            with pytest.raises(ValueError, match="seed"):
                call(rule())


def _walk(pkg, seed, steps=64, rows=64, D=128, eta=2.0 ** -9, eps=1e-8):
    """rows x D weights 1.5, every row hit once per step with G = 1, row-wise Adagrad in fp32 as the kernels compute
    it (m += (1/D) sum G^2; s = eta / (sqrt(m) + eps); W' = fmaf(-s, G, w)) with the restated store.  Returns (moved
    after step 0, the stochastic walk's mean, the fp32 walk's mean, round-to-nearest's weights)."""
    w = np.full((rows, D), 1.5, dtype=np.float32)
    exact = w.copy()
    near = torch.full((rows, D), 1.5, dtype=torch.bfloat16)
    m = np.float32(0.0)
    moved0 = None
    for k in range(steps):
        m = np.float32(m + np.float32(D) / np.float32(D))
        s = np.float32(np.float32(eta) / np.float32(np.sqrt(m, dtype=np.float32) + np.float32(eps)))
        wp = (w - s).astype(np.float32)  # (fmaf(-s, 1, w): one rounding)
        if k == 0:
            assert (wp.view(np.uint32) == 0x3FBFC000).all()  # a quarter of a bf16 ulp below 1.5
        w = (pkg.sr_round(wp, seed, k, 0).astype(np.uint32) << 16).view(np.float32)
        exact = (exact - s).astype(np.float32)
        near = (near.float() - float(s)).to(torch.bfloat16)
        if k == 0:
            moved0 = int((w != 1.5).sum())
    return moved0, float(w.astype(np.float64).mean()), float(exact.astype(np.float64).mean()), near


@pytest.mark.parametrize("seed", [12345, 7, 99])
def test_walk_is_unbiased_where_nearest_rounding_stalls(pkg, seed):
    """Step k of the walk is eta / (sqrt(k) + eps) <= 2^-9, under half a bf16 ulp of the weight (2^-8), so
    round-to-nearest leaves every element at 1.5 for all 64 steps.  With the stochastic store
      * moved after step 0: within 2048 +- 235 (W' is a quarter of an ulp below 1.5: an element moves with probability
        1/4; six binomial standard deviations, test_sr_sgd_host.py);
      * mean after 64 steps: within 2.1e-3 of the closed form 1.5 - sum_k eta / (sqrt(k) + eps) = 1.47148 (six standard
        deviations of the mean at a per-step variance of at most 1/4 ulp^2, as derived there; the steps here are
        smaller, so is the variance)."""
    eta, eps = 2.0 ** -9, 1e-8
    closed = 1.5 - sum(eta / (np.sqrt(k) + eps) for k in range(1, 65))
    moved0, mean, exact, near = _walk(pkg, seed)
    print(f"seed {seed}: moved after step 0 = {moved0}, mean after 64 steps = {mean:.5f}, fp32 {exact:.5f}, "
          f"closed form {closed:.5f}")
    assert abs(closed - 1.47148) <= 1e-5
    assert abs(exact - closed) <= 1e-5  # (fp32 accumulates 64 roundings of at most 2^-24 * 1.5 each)
    assert abs(moved0 - 2048) <= 235, moved0
    assert abs(mean - closed) <= 2.1e-3, mean
    assert (near.float() == 1.5).all()
