"""dlrm_adagrad_step_bwd / dlrm_adagrad_step_bwd_prepare: argument validation on the host, before any HIP call
(CPU only; the arithmetic is tests/test_adagrad_step.py's)."""
import re

import pytest


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _header_arity(pkg, name):
    text = re.sub(r"/\*.*?\*/", "", open(pkg._lib.HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_entry_points_are_declared_bound_and_exported(pkg, lib):
    for name in ("dlrm_adagrad_step_bwd", "dlrm_adagrad_step_bwd_prepare"):
        assert name in pkg._lib.header_functions()
        assert name in pkg._lib.SIGNATURES and hasattr(lib, name)
        assert len(pkg._lib.SIGNATURES[name][1]) == _header_arity(pkg, name)
    # the Adagrad pair = the split pair (an optimizer handle after the tables) + eps after the learning rate
    F = pkg._lib.SIGNATURES["dlrm_adagrad_step_bwd"][1][-2]
    for ada, split, tail in (("dlrm_adagrad_step_bwd", "dlrm_split_step_bwd", 1),
                             ("dlrm_adagrad_step_bwd_prepare", "dlrm_split_step_bwd_prepare", 3)):
        a, b = pkg._lib.SIGNATURES[ada][1], pkg._lib.SIGNATURES[split][1]
        assert a == b[:-tail] + [F] + b[-tail:]
        assert a[-tail - 2] == F  # (lr, then eps)


def test_null_arguments_are_rejected_without_touching_a_device(pkg, lib):
    E_ARG = pkg._lib.E_ARG
    assert lib.dlrm_adagrad_step_bwd(None, None, None, None, None, 0, 0, 0, 1, None, 16, None, 17, 0, None, 16, None, 32,
                                     0.1, 1e-8, 0) == E_ARG
    assert lib.dlrm_adagrad_step_bwd_prepare(None, None, None, None, None, 0, 0, 0, 1, None, 16, None, 17, 0, None, 16,
                                             None, 32, 0.1, 1e-8, None, None, 0) == E_ARG


def test_indexer_state_bits_equal_the_header(pkg):
    text = open(pkg._lib.HEADER).read()
    for name in ("BUILT", "SPLIT", "PREPARED", "SINGLES_DONE", "SINGLES_SPLIT", "SINGLES_ADAGRAD", "SINGLES_ROWWISE"):
        m = re.search(r"\bDLRM_IX_" + name + r"\s*=\s*(\d+)", text)
        assert m, name
        assert getattr(pkg._lib, "IX_" + name) == int(m.group(1)), name
    assert pkg._lib.IX_SINGLES_ADAGRAD == 32 and pkg._lib.IX_SINGLES_ROWWISE == 64
