"""Sparse Adagrad: the host side of the three C entry points and the optimizer classes (no GPU)."""
import ctypes


def test_adagrad_entry_points_reject_null_arguments(pkg):
    """Argument validation runs on the host before any HIP call."""
    _lib = pkg._lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.dlrm_adagrad_create(None, None, 0, None, ctypes.byref(out)) == _lib.E_ARG
    assert lib.dlrm_adagrad_create(None, None, 1, None, None) == _lib.E_ARG
    assert not out.value
    assert lib.dlrm_adagrad_update(None, None, None, None, 0, None, 0, 0, 0, 1, 1, None, 0, 0, 0, 0.1,
                                   1e-8) == _lib.E_ARG
    assert lib.dlrm_adagrad_update(None, None, None, None, _lib.UPDATE_PREBUILT, None, 0, 0, 0, 1, 1, None, 0, 0, 0,
                                   0.1, 1e-8) == _lib.E_ARG


def test_adagrad_destroy_null_is_ok(pkg):
    assert pkg._lib.load().dlrm_adagrad_destroy(None) == 0


def test_optimizer_classes(pkg):
    a, r = pkg.ADAGrad(), pkg.RowwiseADAGrad()
    assert (a.eta, a.eps) == (0.1, 1e-8) and (r.eta, r.eps) == (0.1, 1e-8)
    assert repr(a) == "ADAGrad(0.1, 1e-08)" and repr(r) == "RowwiseADAGrad(0.1, 1e-08)"
    assert repr(pkg.ADAGrad(0.5, 1e-6)) == "ADAGrad(0.5, 1e-06)"
    assert not a.rowwise and r.rowwise
    assert "ADAGrad" in pkg.__all__ and "RowwiseADAGrad" in pkg.__all__
