"""dlrm_split_step_bwd / dlrm_split_step_bwd_prepare: argument validation on the host, before any HIP call
(CPU only; the arithmetic is tests/test_split_step.py's)."""
import pytest


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def test_entry_points_are_declared_bound_and_exported(pkg, lib):
    for name in ("dlrm_split_step_bwd", "dlrm_split_step_bwd_prepare"):
        assert name in pkg._lib.header_functions()
        assert name in pkg._lib.SIGNATURES and hasattr(lib, name)
    # the split pair = the Descent pair + the optimizer handle after the tables
    for split, plain in (("dlrm_split_step_bwd", "dlrm_step_bwd"), ("dlrm_split_step_bwd_prepare", "dlrm_step_bwd_prepare")):
        a, b = pkg._lib.SIGNATURES[split][1], pkg._lib.SIGNATURES[plain][1]
        assert a == b[:2] + [a[2]] + b[2:]
    assert pkg._lib.IX_SINGLES_SPLIT == 16


def test_null_arguments_are_rejected_without_touching_a_device(pkg, lib):
    E_ARG = pkg._lib.E_ARG
    assert lib.dlrm_split_step_bwd(None, None, None, None, None, 0, 0, 0, 1, None, 16, None, 17, 0, None, 16, None, 32,
                                   0.1, 0) == E_ARG
    assert lib.dlrm_split_step_bwd_prepare(None, None, None, None, None, 0, 0, 0, 1, None, 16, None, 17, 0, None, 16, None,
                                           32, 0.1, None, None, 0) == E_ARG


def test_indexer_state_bit_in_the_header(pkg):
    text = open(pkg._lib.HEADER).read()
    assert "DLRM_IX_SINGLES_SPLIT = 16" in text
