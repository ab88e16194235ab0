"""The fused training step with the seeded Adagrad rules, on the host (no GPU): dlrm_sr_adagrad_step_bwd /
dlrm_sr_adagrad_step_bwd_prepare are exported and bound with dlrm_adagrad_step_bwd's signatures and reject NULL
arguments before any HIP call; the two indexer state bits have their values; a seeded optimizer describes its fused
step in sr_step_keyword / sr_step_entry and a seedless one in step_keyword / step_entry; and plan_interact
(tests/interact_plan_print.cpp, compiled as tests/test_interact_plan_host.py compiles it) gives rules 5 and 6 their
step backward forms: the parents' forms on bf16 tables but the two that DESIGN.md section 24 leaves out."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

import interact_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("dlrm_sr_adagrad_step_bwd", "dlrm_sr_adagrad_step_bwd_prepare")
LIKE = ("dlrm_adagrad_step_bwd", "dlrm_adagrad_step_bwd_prepare")
SR_ADAGRAD, SR_ROWWISE = 5, 6  # kRuleStochasticAdagrad, kRuleStochasticRowwise (csrc/build_plan.hpp)
SU = {SR_ADAGRAD: "dlrm::StochasticAdagradStepUpdate<false>", SR_ROWWISE: "dlrm::StochasticAdagradStepUpdate<true>"}


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


def test_signatures_are_the_adagrad_steps(pkg):
    hdr = _header(pkg)
    for n, like in zip(NEW, LIKE):
        mine = _params(hdr, n)
        assert mine == _params(hdr, like), (n, mine)
        assert mine[2] == "dlrm_adagrad* opt"
        assert pkg._lib.SIGNATURES[n] == pkg._lib.SIGNATURES[like]
        assert len(pkg._lib.SIGNATURES[n][1]) == len(mine)


def test_null_arguments_are_rejected(pkg):
    _lib = pkg._lib
    lib = _lib.load()
    step = (None, 0, 0, 0, 1, None, 16, None, 32, 0, None, 16, None, 64, 0.1, 1e-8)
    for flags in (0, _lib.STEP_BWD_ONLY, _lib.STEP_APPLY_ONLY):
        assert lib.dlrm_sr_adagrad_step_bwd(None, None, None, None, *step, flags) == _lib.E_ARG
        assert lib.dlrm_sr_adagrad_step_bwd_prepare(None, None, None, None, *step, None, None, flags) == _lib.E_ARG


def test_state_bits(pkg):
    _lib = pkg._lib
    assert (_lib.IX_SINGLES_SR_ADAGRAD, _lib.IX_SINGLES_SR_ROWWISE) == (256, 512)
    enum = {k: int(v) for k, v in re.findall(r"DLRM_(IX_[A-Z_]+)\s*=\s*(\d+)", _header(pkg))}
    assert enum["IX_SINGLES_SR_ADAGRAD"] == 256 and enum["IX_SINGLES_SR_ROWWISE"] == 512
    bits = {k: v for k, v in vars(_lib).items() if k.startswith("IX_")}
    assert enum == bits and len(set(bits.values())) == len(bits)


def test_optimizer_attributes(pkg):
    pair = ("dlrm_sr_adagrad_step_bwd", "dlrm_sr_adagrad_step_bwd_prepare")
    for cls in (pkg.ADAGrad, pkg.RowwiseADAGrad):
        seeded, plain = cls(0.1, 1e-8, seed=3), cls(0.1, 1e-8)
        assert seeded.step_keyword is None and seeded.step_entry is None
        assert seeded.sr_step_keyword == "sr_adagrad_step" and seeded.sr_step_entry == pair
        assert plain.step_keyword == "adagrad_step" and plain.step_entry == LIKE
        assert plain.sr_step_keyword is None and plain.sr_step_entry is None
        assert seeded.step_params() == (0.1, 1e-8) == plain.step_params()
    for other in (pkg.SplitDescent(0.1), pkg.StochasticDescent(0.1, seed=1)):
        assert other.sr_step_keyword is None and other.sr_step_entry is None


def test_keywords_exist_and_default_off(pkg):
    for cls in (pkg.HotPath, pkg.HipTables):
        p = inspect.signature(cls.__init__).parameters["sr_adagrad_step"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert isinstance(pkg.HotPath.sr_adagrad_step, property) and pkg.HotPath.sr_adagrad_step.fset is None


# ---- the plan of rules 5 and 6
def _split(NB, DC, SPB, WPS, rule, CPL=4):
    return f"interact_bwd_split_kernel<unsigned short, {NB}, {DC}, {SPB}, {WPS}, false, {CPL}, false, {SU[rule]}>"


NONE = ic.UNSUPPORTED
PLAN = [  # (name, rule, dtype, d, F, B, x's (address, ld) or None, expected)
    # the required form: two waves per sample at d = 128, 17 to 32 features
    ("two-wave", SR_ADAGRAD, ic.BF16, 128, 21, 8, None, _split(2, 128, 4, 2, SR_ADAGRAD)),
    ("two-wave-rw", SR_ROWWISE, ic.BF16, 128, 21, 8, None, _split(2, 128, 4, 2, SR_ROWWISE)),
    ("two-wave-F17", SR_ROWWISE, ic.BF16, 128, 17, 2048, None, _split(2, 128, 4, 2, SR_ROWWISE)),
    ("two-wave-F32", SR_ROWWISE, ic.BF16, 128, 32, 2048, None, _split(2, 128, 4, 2, SR_ROWWISE)),
    # up to 16 features: the element-wise rule's two-wave form; the row-wise rule has none (as its parent)
    ("nb1-d128", SR_ADAGRAD, ic.BF16, 128, 5, 8, None, _split(1, 128, 4, 2, SR_ADAGRAD)),
    ("nb1-d128-rw", SR_ROWWISE, ic.BF16, 128, 5, 8, None, NONE),
    ("nb1-F16-rw", SR_ROWWISE, ic.BF16, 128, 16, 8, None, NONE),
    ("nb1-d16-rw", SR_ROWWISE, ic.BF16, 16, 16, 8, None, NONE),
    # d <= 64, one wave per sample: NB = 2 for both rules; the element-wise NB = 1 form is left out (7 waves per SIMD
    # against the parent's 8)
    ("one-wave", SR_ADAGRAD, ic.BF16, 64, 21, 8, None, _split(2, 0, 8, 1, SR_ADAGRAD)),
    ("one-wave-rw", SR_ROWWISE, ic.BF16, 16, 21, 8, None, _split(2, 0, 8, 1, SR_ROWWISE)),
    ("one-wave-d8-rw", SR_ROWWISE, ic.BF16, 8, 21, 8, None, _split(2, 0, 8, 1, SR_ROWWISE)),
    ("one-wave-nb1", SR_ADAGRAD, ic.BF16, 16, 5, 8, None, NONE),
    ("one-wave-d48", SR_ADAGRAD, ic.BF16, 48, 21, 8, None, _split(2, 0, 8, 1, SR_ADAGRAD)),
    # row-wise: d a power of two >= 8
    ("d48-rw", SR_ROWWISE, ic.BF16, 48, 21, 8, None, NONE),
    ("d4-rw", SR_ROWWISE, ic.BF16, 4, 21, 8, None, NONE),
    # fp32 tables: nothing to round
    ("f32", SR_ADAGRAD, ic.F32, 128, 21, 8, None, NONE),
    ("f32-rw", SR_ROWWISE, ic.F32, 128, 21, 8, None, NONE),
    # B = 2049: 8 columns per lane for the element-wise rule; the row-wise 8-column form is left out (8 registers
    # spilt), so that rule keeps two waves per sample
    ("cpl8", SR_ADAGRAD, ic.BF16, 128, 21, 2049, None, _split(2, 128, 2, 1, SR_ADAGRAD, CPL=8)),
    ("cpl8-rw", SR_ROWWISE, ic.BF16, 128, 21, 2049, None, _split(2, 128, 4, 2, SR_ROWWISE)),
    ("cpl8-nb1", SR_ADAGRAD, ic.BF16, 128, 5, 2049, None, _split(1, 128, 4, 2, SR_ADAGRAD)),
    ("B2048", SR_ADAGRAD, ic.BF16, 128, 21, 2048, None, _split(2, 128, 4, 2, SR_ADAGRAD)),
    # the shapes without a split backward or a form
    ("d256", SR_ADAGRAD, ic.BF16, 256, 21, 8, None, NONE),
    ("F33", SR_ADAGRAD, ic.BF16, 16, 34, 8, None, NONE),
    ("x-unaligned", SR_ADAGRAD, ic.BF16, 128, 21, 8, (ic.A0 + 8, 128), NONE),
    ("x-ld", SR_ROWWISE, ic.BF16, 128, 21, 8, (ic.A0, 132), NONE),
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("sr_adagrad_plan")), "plan")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-o", exe,
                    os.path.join(HERE, "interact_plan_print.cpp")], check=True)
    lines = []
    for name, rule, dtype, d, F, B, x, _ in PLAN:
        c = ic.C(name, "step_bwd", "", dtype, d=d, F=F, B=B, ptr={"x": x} if x else None)
        lines.append(" ".join(ic.encode(c).split()[:-1] + [str(rule)]))  # (the rule's number in place of Descent's)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    out = out.splitlines()
    assert len(out) == len(PLAN)
    return [ln.split() for ln in out]


@pytest.mark.parametrize("k", range(len(PLAN)), ids=[p[0] for p in PLAN])
def test_plan_of_the_seeded_rules(plans, k):
    name, rule, want = PLAN[k][0], PLAN[k][1], PLAN[k][-1]
    f = plans[k]
    if f[0] == "bwd_split":  # (spelled with this rule's StepUpdate type)
        rc, f32, NB, DC, WPS, CPL, SPB = map(int, f[1:8])
        assert rc == 0 and not f32
        got = _split(NB, DC, SPB, WPS, rule, CPL)
    else:
        got = ic.spelled(f, "descent")[0]
    assert got == want, (name, got, want)
