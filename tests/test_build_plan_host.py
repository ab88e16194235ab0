"""csrc/build_plan.hpp alone, on the host: plan_build against the literal rows of tests/build_cases.py.

tests/build_plan_print.cpp (its own main, includes only build_plan.hpp) is compiled with the host C++ compiler --
which is also the proof that the header needs no HIP -- fed every case on stdin and must print each row's expected
(form, kind, vshift, split, has_map, bounds word, side stream, return code).  It also prints what
dlrm_indexer_create would carve for the capacity (carve_virtual_tables, carve_hash), held against the row's TV and
hash slots.  A second build with -fsanitize=address,undefined runs the same input.
"""
import os
import shutil
import subprocess

import pytest

import build_cases

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def _build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe,
                    os.path.join(HERE, "build_plan_print.cpp")], check=True)
    return exe


def _run(exe):
    text = "".join(build_cases.encode(c) + "\n" for c in build_cases.CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(build_cases.CASES)
    return [ln.split() for ln in out]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    return _run(_build(tmp_path_factory.mktemp("build_plan"), "plan", ["-O1"]))


@pytest.mark.parametrize("k", range(len(build_cases.CASES)), ids=[c.name for c in build_cases.CASES])
def test_plan_row(answers, k):
    c, f = build_cases.CASES[k], answers[k]
    got = (f[0], f[1], int(f[2]), int(f[3]), int(f[4]), f[5], int(f[6]), int(f[7]))
    assert got == c.expected, (c.name, got, c.expected)
    form, prepared, build_err = f[0], int(f[8]), int(f[9])
    # what the site's row says beyond the eight columns: a prepared result from the two sites that make one, and
    # IndexerDev::build_err from dlrm_indexer_prepare alone
    assert prepared == int(form == "wave")
    assert build_err == int(form == "wave" and c.site == "prepare")
    tv, hs = build_cases.carved(c.cap, c.T)
    assert (int(f[10]), int(f[11])) == (tv, int(hs != 0))


def test_cases_cover_what_the_table_needs():
    """Both sides of every threshold for the five sites that have sizes, and every value of every knob."""
    names = {c.name for c in build_cases.CASES}
    for site in ("build", "split", "prepare", "fwd", "apply"):
        for n in (2048, 4096, 8192, 16384, 32768, 1 << 20):
            assert {f"{site}-{n}", f"{site}-{n + 1}"} <= names
    seen = {(k, v) for c in build_cases.CASES for k, v in c.knobs.items()}
    want = ({("step_parts", v) for v in (1, 2, 4, 8, 16, 32)} | {("build_parts", v) for v in (2, 4, 8)} |
            {("bag_vs", v) for v in (1, 2, 8, 9)} | {("bag_hash", 1), ("bag_split", 0), ("wave_rounds", 1)})
    assert want <= seen
    assert {c.set_parts for c in build_cases.CASES} >= {0, 4, 5, 6}
    off = {k for c in build_cases.CASES for k, v in c.caps.items() if v != build_cases.CAP_DEFAULTS[k]}
    assert off >= {"prepared", "step_fwd", "step_split", "split_bwd", "bwd_only", "idx_vec32"}
    assert all(n in build_cases.BY_NAME for n in build_cases.GPU_CASES)


def test_plan_under_sanitizers(tmp_path, answers):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer (stand-alone host code): no report, the
    same answers."""
    exe = _build(tmp_path, "plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _run(exe) == answers
