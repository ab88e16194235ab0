"""The fused training step with the stochastic rule, on the host: dlrm_sr_step_bwd / dlrm_sr_step_bwd_prepare are
exported and bound with the header's signatures, reject NULL arguments before any HIP call, and the indexer
state bit DLRM_IX_SINGLES_STOCHASTIC has its value and collides with no other bit (no GPU)."""
import inspect
import re

NEW = ("dlrm_sr_step_bwd", "dlrm_sr_step_bwd_prepare")


def _header(pkg):
    return re.sub(r"/\*.*?\*/", "", open(pkg._lib.HEADER).read(), flags=re.S)


def _params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
    assert m, f"{name}: no prototype in the header"
    return [" ".join(q.split()) for q in m.group(1).split(",")]


def test_entry_points_are_exported_and_bound(pkg):
    lib = pkg._lib.load()
    for n in NEW:
        assert n in pkg._lib.header_functions()
        assert hasattr(lib, n), f"{n} declared in include/dlrm_hip.h but not exported"
        assert n in pkg._lib.SIGNATURES, f"{n} has no ctypes signature"
        assert getattr(lib, n).argtypes == pkg._lib.SIGNATURES[n][1]


def test_signatures_are_the_split_steps_with_the_stochastic_handle(pkg):
    """The header's prototypes: dlrm_split_step_bwd's and dlrm_split_step_bwd_prepare's parameter for parameter,
    the optimizer a dlrm_sr_sgd*; the ctypes signatures have the same kinds in the same places."""
    hdr = _header(pkg)
    for n, like in zip(NEW, ("dlrm_split_step_bwd", "dlrm_split_step_bwd_prepare")):
        mine, theirs = _params(hdr, n), _params(hdr, like)
        assert mine == [q.replace("dlrm_split_sgd*", "dlrm_sr_sgd*") for q in theirs], (n, mine)
        assert mine[2] == "dlrm_sr_sgd* opt"
        assert pkg._lib.SIGNATURES[n] == pkg._lib.SIGNATURES[like]
        assert len(pkg._lib.SIGNATURES[n][1]) == len(mine)


def test_null_arguments_are_rejected(pkg):
    _lib = pkg._lib
    lib = _lib.load()
    step = (None, 0, 0, 0, 1, None, 16, None, 32, 0, None, 16, None, 64, 0.1)
    for flags in (0, _lib.STEP_BWD_ONLY, _lib.STEP_APPLY_ONLY):
        assert lib.dlrm_sr_step_bwd(None, None, None, None, *step, flags) == _lib.E_ARG
        assert lib.dlrm_sr_step_bwd_prepare(None, None, None, None, *step, None, None, flags) == _lib.E_ARG


def test_state_bit(pkg):
    _lib = pkg._lib
    assert _lib.IX_SINGLES_STOCHASTIC == 128
    m = re.search(r"DLRM_IX_SINGLES_STOCHASTIC\s*=\s*(\d+)", _header(pkg))
    assert m and int(m.group(1)) == 128
    bits = {k: v for k, v in vars(_lib).items() if k.startswith("IX_")}
    assert len(set(bits.values())) == len(bits), bits
    for k, v in bits.items():
        assert v & (v - 1) == 0, (k, v)  # one bit each
    enum = dict(re.findall(r"DLRM_(IX_[A-Z_]+)\s*=\s*(\d+)", _header(pkg)))
    assert {k: int(v) for k, v in enum.items()} == bits


def test_keywords_exist_and_default_off(pkg):
    for cls in (pkg.HotPath, pkg.HipTables):
        p = inspect.signature(cls.__init__).parameters["stochastic_step"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
